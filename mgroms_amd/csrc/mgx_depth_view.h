// The depths in the model's own padded arrays (mgx_matrices_depths_device, mgx_update_depths_device of include/mgx.h): what strides a call
// may carry, as a pure host function after mgx_state_view.h.  The pointers name z_r(1,1,1) and z_w(1,1,0); element (i, j, k) lies
// (i-1) + (j-1) * sj + dk * sk elements further on, dk counted from the first level of the array (the i stride is 1).  Only i = 1..nx,
// j = 1..ny are ever addressed.  Nothing here calls HIP, keeps state or reads the environment: mgx_api.cpp answers mgx_depth_strides_check
// with it and the depth entries call it before anything is launched; tests/test_depths_host.py pins its answers.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdio>

#include "../../include/mgx.h"

// the logical shape of one depth array: elements of a row (along i), rows of a level (along j), levels (along k)
struct DepthArrayShape { const char *name; long long len, rows, levels; };
static inline void depth_array_shapes(int nx, int ny, int nz, DepthArrayShape out[2]) {
  out[0] = {"zr", (long long)nx, (long long)ny, (long long)nz};
  out[1] = {"zw", (long long)nx, (long long)ny, (long long)nz + 1};
}

// 0 = the strides serve the depths of an nx x ny x nz level 1; 1 = refused, with the array, the field and the offending value in msg.
// The refusals of state_strides_refusal (mgx_state_view.h), in its words: a stride that is not positive; sj below the row length; sk below
// sj x rows; an extent whose last element lies further from the first than 63 bits hold, counted in bytes of a double.
static inline int depth_strides_refusal(int nx, int ny, int nz, const mgx_depth_strides *s, char *msg, size_t n) {
  if (nx < 1 || ny < 1 || nz < 1) { snprintf(msg, n, "nx, ny, nz = %d, %d, %d: need positive sizes", nx, ny, nz); return 1; }
  if (!s) { snprintf(msg, n, "the strides are NULL"); return 1; }
  DepthArrayShape a[2];
  depth_array_shapes(nx, ny, nz, a);
  const long long sj[2] = {s->zr_sj, s->zw_sj}, sk[2] = {s->zr_sk, s->zw_sk};
  for (int q = 0; q < 2; q++) {
    const char *nm = a[q].name;
    if (sj[q] <= 0) { snprintf(msg, n, "%s_sj = %lld: the row stride of %s is not positive", nm, sj[q], nm); return 1; }
    if (sk[q] <= 0) { snprintf(msg, n, "%s_sk = %lld: the level stride of %s is not positive", nm, sk[q], nm); return 1; }
    if (sj[q] < a[q].len) { snprintf(msg, n, "%s_sj = %lld is below the row length of %s, %lld: rows would overlap", nm, sj[q], nm, a[q].len); return 1; }
    long long level, top, side, last;
    const bool fits = !__builtin_mul_overflow(sj[q], a[q].rows, &level);
    if (fits && sk[q] < level) {
      snprintf(msg, n, "%s_sk = %lld is below %s_sj x rows of %s = %lld x %lld: levels would overlap", nm, sk[q], nm, nm, sj[q], a[q].rows);
      return 1;
    }
    // offset of the last logical element: (levels - 1) sk + (rows - 1) sj + (len - 1)
    const bool over = !fits || __builtin_mul_overflow(sk[q], a[q].levels - 1, &top) || __builtin_mul_overflow(sj[q], a[q].rows - 1, &side) ||
                      __builtin_add_overflow(top, side, &last) || __builtin_add_overflow(last, a[q].len - 1, &last) || last > LLONG_MAX / 8;
    if (over) {
      snprintf(msg, n, "%s_sj = %lld, %s_sk = %lld: the extent of %s does not fit in 63 bits", nm, sj[q], nm, sk[q], nm);
      return 1;
    }
  }
  return 0;
}
