// The model state in the model's own padded arrays (the *_view entries of include/mgx.h): what strides a call may carry, as a pure host
// function.  The pointer of an array names its first logical element, u(1,0,1), v(0,1,1), w(0,0,0); element (i, j, k) of it lies
// di + dj * sj + dk * sk elements further on, with di, dj, dk counted from that first element (the i stride is 1).  Nothing here calls
// HIP, keeps state or reads the environment: mgx_api.cpp answers mgx_state_strides_check with it and the view entries call it before
// anything is launched; tests/test_state_view_host.py pins its answers.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdio>

#include "../../include/mgx.h"

// the logical shape of one state array: elements of a row (along i), rows of a level (along j), levels (along k)
struct StateArrayShape { const char *name; long long len, rows, levels; };
static inline void state_array_shapes(int nx, int ny, int nz, StateArrayShape out[3]) {
  out[0] = {"u", (long long)nx + 1, (long long)ny + 2, (long long)nz};
  out[1] = {"v", (long long)nx + 2, (long long)ny + 1, (long long)nz};
  out[2] = {"w", (long long)nx + 2, (long long)ny + 2, (long long)nz + 1};
}
// the strides of the densely packed arrays of mgx_solve_device
static inline mgx_state_strides state_dense_strides(int nx, int ny, int nz) {
  StateArrayShape a[3];
  state_array_shapes(nx, ny, nz, a);
  return {a[0].len, a[0].len * a[0].rows, a[1].len, a[1].len * a[1].rows, a[2].len, a[2].len * a[2].rows};
}

// 0 = the strides serve an nx x ny x nz state; 1 = refused, with the array, the field and the offending value in msg.  Refused: a stride
// that is not positive; sj below the row length (rows would overlap); sk below sj x rows (levels would overlap); an extent whose last
// element lies further from the first than 63 bits hold, counted in bytes of the wider state type (8), so that no address wraps either.
static inline int state_strides_refusal(int nx, int ny, int nz, const mgx_state_strides *s, char *msg, size_t n) {
  if (nx < 1 || ny < 1 || nz < 1) { snprintf(msg, n, "nx, ny, nz = %d, %d, %d: need positive sizes", nx, ny, nz); return 1; }
  if (!s) { snprintf(msg, n, "the strides are NULL"); return 1; }
  StateArrayShape a[3];
  state_array_shapes(nx, ny, nz, a);
  const long long sj[3] = {s->u_sj, s->v_sj, s->w_sj}, sk[3] = {s->u_sk, s->v_sk, s->w_sk};
  for (int q = 0; q < 3; q++) {
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
