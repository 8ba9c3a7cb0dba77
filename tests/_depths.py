"""The depths a caller hands to nhydro_matrices_depths, and the rule by which the library coarsens them, in pure numpy (tests/test_depths_host.py,
tests/test_gpu_depths.py).

Arrays are numpy arrays in the library's index order: zr[i, j, k], zw[i, j, k] with k fastest -- the INTERIOR columns, shapes (nx, ny, nz)
and (nx, ny, nz+1), unless a function says otherwise; dense() puts an interior into the library's dense layout (nx+4, ny+4, .), whose halo
the library never reads and the tests therefore fill with NaN."""
import numpy as np


def interior(a):
    """the interior columns of an array in the library's dense layout of zr / zw (two halo cells per side)"""
    return a[2:-2, 2:-2]


def dense(a, fill=np.nan):
    """an interior (nx, ny, n) in the library's dense layout (nx+4, ny+4, n), the halo set to `fill`"""
    out = np.full((a.shape[0] + 4, a.shape[1] + 4, a.shape[2]), fill)
    out[2:-2, 2:-2] = a
    return out


def _avg(x):
    """0.25 * (x(fj,fi) + x(fj+1,fi) + x(fj,fi+1) + x(fj+1,fi+1)), summed in that order (numpy adds left to right; index [i, j])"""
    return 0.25 * (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2])


def coarsen_depths(zr, zw, held):
    """(zr_C, zw_C) of the next coarser level from the interiors of a level.  A pair that halves nz: zw_C(kc) = avg zw_F(2kc-1),
    kc = 1..nz_C+1, zr_C(kc) = avg zw_F(2kc), kc = 1..nz_C (only zw_F is read); a held pair: zw_C(k) = avg zw_F(k), zr_C(k) = avg zr_F(k)."""
    nz = zr.shape[2]
    assert zw.shape == zr.shape[:2] + (nz + 1,) and zr.shape[0] % 2 == 0 and zr.shape[1] % 2 == 0
    if held:
        return _avg(zr), _avg(zw)
    assert nz % 2 == 0, "halving from an odd nz has no top interface"
    return _avg(zw[:, :, 1::2]), _avg(zw[:, :, 0::2])


def hierarchy(zr, zw, nzs):
    """[(zr, zw)] of every level of a one-rank hierarchy whose levels have nzs[l] rows (level 1 first), from the level-1 interiors"""
    out = [(zr, zw)]
    for nzf, nzc in zip(nzs[:-1], nzs[1:]):
        assert nzc in (nzf, nzf // 2), (nzf, nzc)
        zr, zw = coarsen_depths(zr, zw, held=nzc == nzf)
        assert zr.shape[2] == nzc
        out.append((zr, zw))
    return out


def old_s_depths(h, zeta, nz, hc=50.0, theta_s=5.0, theta_b=0.4):
    """ROMS Vtransform = 1 with the stretching of Song and Haidvogel (1994), a grid no (hc, theta_b, theta_s) of the library produces:
        z0 = hc s + (h - hc) C(s),   z = z0 + zeta (1 + z0 / h)
        C(s) = (1 - theta_b) sinh(theta_s s) / sinh(theta_s) + theta_b [tanh(theta_s (s + 1/2)) / (2 tanh(theta_s / 2)) - 1/2]
        s_w(k) = (k - 1 - nz) / nz, k = 1..nz+1;   s_r(k) = (k - nz - 1/2) / nz, k = 1..nz
    h, zeta: 2-D arrays of one shape (the interior columns) -> (zr, zw) of shapes h.shape + (nz,), h.shape + (nz+1,)."""
    h = np.asarray(h, dtype=np.float64); zeta = np.asarray(zeta, dtype=np.float64)
    assert h.shape == zeta.shape and h.ndim == 2 and hc <= h.min()

    def C(s):
        return (1.0 - theta_b) * np.sinh(theta_s * s) / np.sinh(theta_s) + theta_b * (np.tanh(theta_s * (s + 0.5)) / (2.0 * np.tanh(0.5 * theta_s)) - 0.5)

    def z(s):
        z0 = hc * s + (h[..., None] - hc) * C(s)
        return z0 + zeta[..., None] * (1.0 + z0 / h[..., None])

    zw = z((np.arange(1, nz + 2) - 1.0 - nz) / nz)
    zr = z((np.arange(1, nz + 1) - nz - 0.5) / nz)
    assert_monotone(zr, zw)
    return zr, zw


def assert_monotone(zr, zw):
    """zw strictly increasing in k and zw(k) < zr(k) < zw(k+1): the caller's duty towards nhydro_matrices_depths"""
    assert np.all(np.diff(zw, axis=-1) > 0.0)
    assert np.all(zw[..., :-1] < zr) and np.all(zr < zw[..., 1:])


def model_arrays(zr, zw, ghost, pad, fill=np.nan):
    """The interiors as a model keeps them: i fastest, arrays Z_R (nz, ny + 2g, nx + 2g + pad), Z_W (nz+1, ...) with g ghost cells per
    side and a padded pitch, ghost cells and padding set to `fill` -> (Z_R, Z_W, the slices that select the interior)."""
    nx, ny, nz = zr.shape
    sl = (slice(None), slice(ghost, ghost + ny), slice(ghost, ghost + nx))
    out = []
    for a in (zr, zw):
        A = np.full((a.shape[2], ny + 2 * ghost, nx + 2 * ghost + pad), fill)
        A[sl] = a.transpose(2, 1, 0)
        out.append(A)
    return out[0], out[1], sl
