"""Host-side mirror of the reference's model-facing API (src/nhydro.f90) and of the solver-level entry points
the reference's tests drive (src/mg_solvers.f90, mg_relax.f90, mg_intergrids.f90), same names and argument
meaning.  Arrays follow the reference's Fortran shapes; pass numpy arrays whose C-order index is the reversed
Fortran index, i.e. a field p(nz,0:ny+1,0:nx+1) is a numpy array of shape (nx+2, ny+2, nz).
"""
import ctypes as C
import threading
import warnings

import numpy as np

from ._lib import Params, MgxError, StateStrides, DepthStrides, lib, check  # noqa: F401

FIELD = {"p": 0, "b": 1, "r": 2, "cA": 3, "dx": 4, "dy": 5, "zeta": 6, "h": 7, "zr": 8, "zw": 9, "cw": 10, "rmask": 14}
_DP = C.POINTER(C.c_double)
_FP = C.POINTER(C.c_float)


class _PerThread(threading.local):
    """dims of the instance the calling thread drives (include/mgx.h: the instance selection is per thread as well)"""
    dims = None


_state = _PerThread()


def _dp(a):
    return a.ctypes.data_as(_DP)


def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


def default_params(**kw):
    p = Params()
    check(lib().mgx_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(f"{k} is not a member of namelist /nhparam/")
        setattr(p, k, v.encode() if isinstance(v, str) else v)
    return p


def read_nhnamelist(filename="nh_namelist", **overrides):
    """read_nhnamelist (mg_namelist.f90:55): defaults, then the file if it exists, then keyword overrides."""
    p = default_params()
    check(lib().mgx_read_namelist(filename.encode(), C.byref(p)))
    for k, v in overrides.items():
        setattr(p, k, v.encode() if isinstance(v, str) else v)
    return p


def set_option(name, value):
    """warm_start / tictoc / exact_halos / verbose (include/mgx.h: mgx_set_option)."""
    check(lib().mgx_set_option(name.encode(), int(value)))


def synchronize():
    """wait for the solver's stream and raise what the device flagged (counterpart of set_option("async", 1))"""
    check(lib().mgx_synchronize())


def get_option(name):
    """read back an option or an integer / logical member of /nhparam/ (include/mgx.h: mgx_get_option)"""
    v = C.c_int()
    check(lib().mgx_get_option(name.encode(), C.byref(v)))
    return v.value


def print_tictoc(path="fort.10"):
    """print_tictoc (mg_tictoc.f90:114): per-level timer table of relax / residual / Fcycle / solve / compute_rhs."""
    check(lib().mgx_print_tictoc(path.encode()))


def set_verbose(level):
    check(lib().mgx_set_verbose(int(level)))


def nhydro_init(nx, ny, nz, npxg=1, npyg=1, rank=0, params=None, comm=None):
    """nhydro_init(nx,ny,nz,npxg,npyg) (nhydro.f90:18).  `params=None` reads ./nh_namelist like the reference.
    `comm`: an mgroms_amd.parallel.Comm when npxg*npyg > 1 (one process per GPU)."""
    if comm is not None:
        comm.install()
    check(lib().mgx_init(nx, ny, nz, npxg, npyg, rank, None if params is None else C.byref(params)))
    _state.dims = (nx, ny, nz)
    if comm is not None and npxg * npyg > 1:
        comm.after_init()


def nhydro_matrices(dx, dy, zeta, h, rmask=None, hc=0.0, theta_b=0.0, theta_s=0.0):
    """nhydro_matrices (nhydro.f90:36): 2-D arrays are (0:ny+1,0:nx+1) in Fortran = numpy shape (nx+2, ny+2)."""
    nx, ny, _ = _state.dims
    sh = (nx + 2, ny + 2)
    dx, dy, zeta, h = (_f64(a, sh, n) for a, n in ((dx, "dx"), (dy, "dy"), (zeta, "zeta"), (h, "h")))
    rm = None if rmask is None else _f64(rmask, sh, "rmask")
    check(lib().mgx_matrices(_dp(dx), _dp(dy), _dp(zeta), _dp(h), None if rm is None else _dp(rm), hc, theta_b, theta_s))


def _uvw_shapes():
    nx, ny, nz = _state.dims
    return ((nz, ny + 2, nx + 1), "u"), ((nz, ny + 1, nx + 2), "v"), ((nz + 1, ny + 2, nx + 2), "w")


def _one_dtype(dtypes, both, what):
    """the scalar type of the model state: "" when u, v, w are all float64, "_f32" (the suffix of the library's float entries, include/mgx.h:
    the float state) when they are all float32; anything else, a mix included, is refused"""
    if len(set(dtypes)) != 1 or dtypes[0] not in both:
        raise ValueError(f"u, v, w: need three {what} of one dtype, float64 or float32; got {', '.join(str(d) for d in dtypes)}")
    return "" if dtypes[0] == both[0] else "_f32"


def _uvw(u, v, w):
    """host u, v, w: C-contiguous numpy arrays of the model's shapes, all float64 or all float32 -> (entry suffix, the three pointers)"""
    sfx = _one_dtype([getattr(a, "dtype", type(a)) for a in (u, v, w)], (np.dtype(np.float64), np.dtype(np.float32)), "arrays")
    for a, (sh, n) in zip((u, v, w), _uvw_shapes()):
        if not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.shape == sh):
            raise ValueError(f"{n}: need a C-contiguous float64 or float32 array of shape {sh} (updated in place)")
    return sfx, [a.ctypes.data_as(_FP if sfx else _DP) for a in (u, v, w)]


def _uvw_dev(u, v, w):
    """device u, v, w: contiguous torch CUDA tensors of the model's shapes, all float64 or all float32 -> (entry suffix, the three pointers)"""
    sfx = _one_dtype([str(getattr(a, "dtype", type(a))) for a in (u, v, w)], ("torch.float64", "torch.float32"), "tensors")
    for a, (sh, n) in zip((u, v, w), _uvw_shapes()):
        if not (hasattr(a, "is_cuda") and a.is_cuda and a.is_contiguous() and tuple(a.shape) == sh):
            raise ValueError(f"{n}: need a contiguous float64 or float32 CUDA tensor of shape {sh}")
    return sfx, [C.c_void_p(a.data_ptr()) for a in (u, v, w)]


def _mask(rmask):
    """rmaska of the call, (0:ny+1,0:nx+1) in Fortran = numpy (nx+2, ny+2); None = the mask of nhydro_matrices / all ones."""
    if rmask is None:
        return None, None
    nx, ny, _ = _state.dims
    rm = _f64(rmask, (nx + 2, ny + 2), "rmask")
    return rm, _dp(rm)


def nhydro_solve(u, v, w, rmask=None):
    """nhydro_solve (nhydro.f90:53): u(1:nx+1,0:ny+1,1:nz) = numpy (nz, ny+2, nx+1) etc.; corrected in place.  u, v, w all float64, or all
    float32: then each element comes back as the float64 result rounded once (include/mgx.h: the float state)."""
    sfx, ptrs = _uvw(u, v, w)
    rm, prm = _mask(rmask)
    check(getattr(lib(), "mgx_solve" + sfx)(*ptrs, prm))


def nhydro_solve_device(u, v, w, rmask=None):
    """nhydro_solve on torch CUDA tensors (all float64 or all float32, contiguous, shapes as nhydro_solve; rmask float64 (nx+2, ny+2)): no host
    round trip.  A float32 state comes back as the float64 result rounded once (include/mgx.h: the float state)."""
    sfx, ptrs = _uvw_dev(u, v, w)
    nx, ny, nz = _state.dims
    prm = None if rmask is None else _dev(rmask, (nx + 2, ny + 2), "rmask")
    _wait_for_caller()
    check(getattr(lib(), "mgx_solve_device" + sfx)(*ptrs, prm))


def _dev(a, shape, name):
    """data pointer of a torch CUDA tensor after the checks of nhydro_solve_device (float64, contiguous, exact shape, on the device)"""
    ok = hasattr(a, "is_cuda") and a.is_cuda and a.is_contiguous() and tuple(a.shape) == tuple(shape) and str(a.dtype) == "torch.float64"
    if not ok:
        raise ValueError(f"{name}: need a contiguous float64 CUDA tensor of shape {tuple(shape)}")
    return C.c_void_p(a.data_ptr())


def _wait_for_caller():
    import torch
    torch.cuda.current_stream().synchronize()


def nhydro_matrices_device(dx, dy, zeta, h, rmask=None, hc=0.0, theta_b=0.0, theta_s=0.0):
    """nhydro_matrices on torch CUDA tensors of shape (nx+2, ny+2): no host round trip (include/mgx.h: mgx_matrices_device)."""
    nx, ny, _ = _state.dims
    sh = (nx + 2, ny + 2)
    ptrs = [_dev(a, sh, n) for a, n in ((dx, "dx"), (dy, "dy"), (zeta, "zeta"), (h, "h"))]
    prm = None if rmask is None else _dev(rmask, sh, "rmask")
    _wait_for_caller()
    check(lib().mgx_matrices_device(*ptrs, prm, hc, theta_b, theta_s))


def nhydro_update_zeta_device(zeta):
    """the per-step call of a resident model: a new zeta (torch CUDA tensor, (nx+2, ny+2)) under the dx, dy, h, rmask of the last
    nhydro_matrices / nhydro_matrices_device; everything that depends on zeta is rebuilt (include/mgx.h: mgx_update_zeta_device)."""
    if _state.dims is None:
        check(lib().mgx_update_zeta_device(None))   # the library's refusal (no mgx_init), in its words
    nx, ny, _ = _state.dims
    p = _dev(zeta, (nx + 2, ny + 2), "zeta")
    _wait_for_caller()
    check(lib().mgx_update_zeta_device(p))


def nhydro_check_nondivergence_device(u, v, w, rmask=None):
    """nhydro_check_nondivergence on torch CUDA tensors (shapes as nhydro_solve_device): the divergence is left in grid(1).b"""
    sfx, ptrs = _uvw_dev(u, v, w)
    nx, ny, nz = _state.dims
    prm = None if rmask is None else _dev(rmask, (nx + 2, ny + 2), "rmask")
    _wait_for_caller()
    check(getattr(lib(), "mgx_check_nondivergence_device" + sfx)(*ptrs, prm))


# ---- the state in the model's own padded arrays (include/mgx.h: the *_view entries) ----
def state_strides_check(nx, ny, nz, strides):
    """mgx_state_strides_check: strides = (u_sj, u_sk, v_sj, v_sk, w_sj, w_sk) in elements; raises MgxError, in the library's words, for
    strides that cannot hold an nx x ny x nz state.  Host only: needs neither a GPU nor nhydro_init."""
    s = StateStrides(*(int(x) for x in strides))
    check(lib().mgx_state_strides_check(int(nx), int(ny), int(nz), C.byref(s)))


def _uvw_view(u, v, w, entry):
    """device u, v, w that may be views: torch CUDA tensors of the model's shapes with unit stride along i, all float64 or all float32
    -> (f32, the three pointers, the strides as the tensors have them: the library judges them)"""
    if _state.dims is None:
        check(getattr(lib(), entry)(None, None, None, C.byref(StateStrides()), 0, None))   # the library's refusal (no mgx_init), in its words
    sfx = _one_dtype([str(getattr(a, "dtype", type(a))) for a in (u, v, w)], ("torch.float64", "torch.float32"), "tensors")
    strides = []
    for a, (sh, n) in zip((u, v, w), _uvw_shapes()):
        if not (hasattr(a, "is_cuda") and a.is_cuda and tuple(a.shape) == sh):
            raise ValueError(f"{n}: need a float64 or float32 CUDA tensor of shape {sh} (it may be a view)")
        if a.stride(-1) != 1:
            raise ValueError(f"{n}: need stride 1 along i (the last dimension), got {a.stride(-1)}")
        strides += [a.stride(1), a.stride(0)]
    return 1 if sfx else 0, [C.c_void_p(a.data_ptr()) for a in (u, v, w)], StateStrides(*strides)


def _call_view(entry, u, v, w, rmask):
    f32, ptrs, s = _uvw_view(u, v, w, entry)
    nx, ny, nz = _state.dims
    prm = None if rmask is None else _dev(rmask, (nx + 2, ny + 2), "rmask")
    _wait_for_caller()
    check(getattr(lib(), entry)(*ptrs, C.byref(s), f32, prm))


def nhydro_solve_view(u, v, w, rmask=None):
    """nhydro_solve_device on the model's own padded arrays: u, v, w are torch CUDA tensors of the shapes of nhydro_solve that may be views
    -- e.g. U[:, 2:-2, 3:-2] of a tensor with ghost cells -- with unit stride along i; the other strides go to the library as they are
    (include/mgx.h: mgx_solve_device_view).  Only the elements of the views are read or written.  rmask: dense, as in nhydro_solve_device."""
    _call_view("mgx_solve_device_view", u, v, w, rmask)


def nhydro_check_nondivergence_view(u, v, w, rmask=None):
    """nhydro_check_nondivergence_device on views (as nhydro_solve_view): u, v, w are only read, the divergence is left in grid(1).b"""
    _call_view("mgx_check_nondivergence_device_view", u, v, w, rmask)


def nhydro_update_zeta_view(zeta):
    """nhydro_update_zeta_device from the model's own zeta: a float64 torch CUDA tensor of shape (ny+2, nx+2) -- i fastest -- that may be a
    view with unit stride along i; its row pitch goes to the library (include/mgx.h: mgx_update_zeta_device_view)."""
    if _state.dims is None:
        check(lib().mgx_update_zeta_device_view(None, 0))   # the library's refusal (no mgx_init), in its words
    nx, ny, _ = _state.dims
    ok = hasattr(zeta, "is_cuda") and zeta.is_cuda and tuple(zeta.shape) == (ny + 2, nx + 2) and str(zeta.dtype) == "torch.float64"
    if not ok:
        raise ValueError(f"zeta: need a float64 CUDA tensor of shape {(ny + 2, nx + 2)} (it may be a view)")
    if zeta.stride(-1) != 1:
        raise ValueError(f"zeta: need stride 1 along i (the last dimension), got {zeta.stride(-1)}")
    _wait_for_caller()
    check(lib().mgx_update_zeta_device_view(C.c_void_p(zeta.data_ptr()), zeta.stride(0)))


# ---- the matrices from the model's own vertical grid (include/mgx.h: mgx_matrices_depths*) ----
def depth_strides_check(nx, ny, nz, strides):
    """mgx_depth_strides_check: strides = (zr_sj, zr_sk, zw_sj, zw_sk) in elements; raises MgxError, in the library's words, for strides
    that cannot hold the depths of an nx x ny x nz level 1.  Host only: needs neither a GPU nor nhydro_init."""
    s = DepthStrides(*(int(x) for x in strides))
    check(lib().mgx_depth_strides_check(int(nx), int(ny), int(nz), C.byref(s)))


def depths_launch(nx, ny, nz):
    """the launches of the depth kernels for a level 1 of nx x ny x nz as a dict (include/mgx.h: mgx_depths_launch).  Pure host logic."""
    out = (C.c_int * 17)()
    check(lib().mgx_depths_launch(int(nx), int(ny), int(nz), out))
    keys = ("in_i_tiles", "in_k_tiles_zr", "in_k_tiles_zw", "in_grid_x", "in_grid_y", "in_block_x", "in_block_y", "in_lds",
            "copy_grid", "copy_block", "coarsen_grid", "coarsen_block", "hz_grid_x", "hz_grid_y", "hz_block_x", "hz_block_y", "pass_stored")
    return dict(zip(keys, list(out)))


def nhydro_matrices_depths(dx, dy, zr, zw, rmask=None):
    """nhydro_matrices from the caller's own depths: dx, dy (and rmask) as in nhydro_matrices; zr, zw numpy arrays in the library's dense
    layout, what grid(1).zr / grid(1).zw return -- shapes (nx+4, ny+4, nz) and (nx+4, ny+4, nz+1).  Only the interior columns are read."""
    if _state.dims is None:
        check(lib().mgx_matrices_depths(None, None, None, None, None))   # the library's refusal (no mgx_init), in its words
    nx, ny, nz = _state.dims
    sh = (nx + 2, ny + 2)
    dx, dy = _f64(dx, sh, "dx"), _f64(dy, sh, "dy")
    zr, zw = _f64(zr, (nx + 4, ny + 4, nz), "zr"), _f64(zw, (nx + 4, ny + 4, nz + 1), "zw")
    rm = None if rmask is None else _f64(rmask, sh, "rmask")
    check(lib().mgx_matrices_depths(_dp(dx), _dp(dy), _dp(zr), _dp(zw), None if rm is None else _dp(rm)))


def _depths_dev(zr, zw):
    """device zr, zw -> (the two pointers, the strides or None): a contiguous float64 CUDA tensor of the library's shape, (nx+4, ny+4, nz) /
    (nx+4, ny+4, nz+1), goes dense; tensors of shape (nz, ny, nx) / (nz+1, ny, nx) with unit stride along i -- views of the model's padded
    arrays -- go through their strides, which the library judges (as nhydro_solve_view derives them)"""
    nx, ny, nz = _state.dims
    for a, n in ((zr, "zr"), (zw, "zw")):
        if not (hasattr(a, "is_cuda") and a.is_cuda and str(a.dtype) == "torch.float64"):
            raise ValueError(f"{n}: need a float64 CUDA tensor")
    dense = ((nx + 4, ny + 4, nz), (nx + 4, ny + 4, nz + 1))
    view = ((nz, ny, nx), (nz + 1, ny, nx))
    if tuple(zr.shape) == dense[0] and tuple(zw.shape) == dense[1] and zr.is_contiguous() and zw.is_contiguous():
        return [C.c_void_p(zr.data_ptr()), C.c_void_p(zw.data_ptr())], None
    if tuple(zr.shape) == view[0] and tuple(zw.shape) == view[1]:
        for a, n in ((zr, "zr"), (zw, "zw")):
            if a.stride(-1) != 1:
                raise ValueError(f"{n}: need stride 1 along i (the last dimension), got {a.stride(-1)}")
        s = DepthStrides(zr.stride(1), zr.stride(0), zw.stride(1), zw.stride(0))
        return [C.c_void_p(zr.data_ptr()), C.c_void_p(zw.data_ptr())], s
    raise ValueError(f"zr, zw: need contiguous tensors of shapes {dense[0]}, {dense[1]} (the library's layout) or i-fastest tensors, "
                     f"which may be views, of shapes {view[0]}, {view[1]}; got {tuple(zr.shape)}, {tuple(zw.shape)}")


def nhydro_matrices_depths_device(dx, dy, zr, zw, rmask=None):
    """nhydro_matrices_depths on torch CUDA tensors: dx, dy, rmask dense (nx+2, ny+2) as in nhydro_matrices_device; zr, zw in the library's
    layout or as i-fastest views of the model's own padded arrays, zr[k-1, j-1, i-1] = z_r(i,j,k), zw[k, j-1, i-1] = z_w(i,j,k) -- e.g.
    Z_R[:, 2:-2, 2:-2] (include/mgx.h: mgx_matrices_depths_device).  Only the elements of the views are read; nothing of them is written."""
    if _state.dims is None:
        check(lib().mgx_matrices_depths_device(None, None, None, None, None, None))   # the library's refusal (no mgx_init), in its words
    nx, ny, _ = _state.dims
    sh = (nx + 2, ny + 2)
    pxy = [_dev(a, sh, n) for a, n in ((dx, "dx"), (dy, "dy"))]
    ptrs, s = _depths_dev(zr, zw)
    prm = None if rmask is None else _dev(rmask, sh, "rmask")
    _wait_for_caller()
    check(lib().mgx_matrices_depths_device(*pxy, *ptrs, None if s is None else C.byref(s), prm))


def nhydro_update_depths_device(zr, zw):
    """the per-step call of a resident model that owns its vertical grid: new depths (as in nhydro_matrices_depths_device) under the dx, dy,
    rmask of the last set-up; every level's operator is rebuilt (include/mgx.h: mgx_update_depths_device)."""
    if _state.dims is None:
        check(lib().mgx_update_depths_device(None, None, None))   # the library's refusal (no mgx_init), in its words
    ptrs, s = _depths_dev(zr, zw)
    _wait_for_caller()
    check(lib().mgx_update_depths_device(*ptrs, None if s is None else C.byref(s)))


def nhydro_check_nondivergence(u, v, w, rmask=None):
    sfx, ptrs = _uvw(u, v, w)
    rm, prm = _mask(rmask)
    check(getattr(lib(), "mgx_check_nondivergence" + sfx)(*ptrs, prm))


def compute_rhs(u, v, w, rmask=None):
    sfx, ptrs = _uvw(u, v, w)
    rm, prm = _mask(rmask)
    check(getattr(lib(), "mgx_compute_rhs" + sfx)(*ptrs, prm))


def nhydro_clean():
    lib().mgx_clean()
    _state.dims = None


# ---- mg_solvers / mg_relax / mg_intergrids ------------------------------------------------------
def solve_p(tol, maxite):
    """solve_p(tol,maxite) (mg_solvers.f90:17).  Returns (nite, history) with history[0] the initial ||r||/||b||."""
    n = C.c_int()
    res = C.c_double()
    hist = (C.c_double * (maxite + 1))()
    check(lib().mgx_solve_p(tol, maxite, C.byref(n), C.byref(res), hist))
    return n.value, np.array(hist[:n.value + 1])


def Fcycle():
    check(lib().mgx_fcycle())


def Vcycle(lev=1):
    check(lib().mgx_vcycle(lev))


def Vcycle2(lev1, lev2):
    check(lib().mgx_vcycle2(lev1, lev2))


def relax(lev, nsweeps):
    check(lib().mgx_relax(lev, nsweeps))


def compute_residual(lev):
    """compute_residual(lev,res) (mg_relax.f90:337): returns the global L2 norm of r."""
    r = C.c_double()
    check(lib().mgx_residual(lev, C.byref(r)))
    return r.value


def fine2coarse(lev):
    check(lib().mgx_fine2coarse(lev))


def coarse2fine(lev):
    check(lib().mgx_coarse2fine(lev))


def fill_halo(lev, name):
    check(lib().mgx_fill_halo(lev, FIELD[name]))


def testgalerkin(lev):
    """testgalerkin(lev) (mg_solvers.f90:203): returns (norm_c, norm_f) for the coarse field found in grid(lev).p."""
    a, b = C.c_double(), C.c_double()
    check(lib().mgx_testgalerkin(lev, C.byref(a), C.byref(b)))
    return a.value, b.value


def nlevs():
    return lib().mgx_nlevs()


# ---- the level matrices as torch sparse CSR tensors on the device (include/mgx.h: mgx_operator_csr, mgx_transfer_csr) ----
def _csr(size_call, fill_call):
    """allocate from the *_size call, fill, wrap: float64 values, int32 indices, on the solver's device"""
    import torch
    nrows, ncols, nnz = size_call()
    dev = torch.device("cuda", torch.cuda.current_device())
    rowptr = torch.empty(nrows + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)   # (never an empty allocation: the library refuses a null pointer)
    val = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
    _wait_for_caller()
    fill_call(C.c_void_p(rowptr.data_ptr()), C.c_void_p(col.data_ptr()), C.c_void_p(val.data_ptr()))
    with warnings.catch_warnings():   # (torch announces once per process that its CSR support is in beta)
        warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta")
        return torch.sparse_csr_tensor(rowptr, col[:nnz], val[:nnz], size=(nrows, ncols))


def operator_csr(lev):
    """A of level lev with the sign of compute_residual (r = b - A p), the level's halo rule folded in, as a torch.sparse_csr_tensor on the
    device.  Unknown (k, j, i) has index ((i-1)*ny + (j-1))*nz + (k-1): for a field f of grid(lev), f[1:-1, 1:-1, :].reshape(-1)."""
    def size():
        n, nnz = C.c_longlong(), C.c_longlong()
        check(lib().mgx_operator_csr_size(int(lev), C.byref(n), C.byref(nnz)))
        return n.value, n.value, nnz.value
    return _csr(size, lambda r, c, v: check(lib().mgx_operator_csr(int(lev), r, c, v)))


def _transfer_csr(lev, which):
    def size():
        n, m, nnz = C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(lib().mgx_transfer_csr_size(int(lev), which, C.byref(n), C.byref(m), C.byref(nnz)))
        return n.value, m.value, nnz.value
    return _csr(size, lambda r, c, v: check(lib().mgx_transfer_csr(int(lev), which, r, c, v)))


def restriction_csr(lev):
    """R from level lev to lev + 1, what fine2coarse(lev) does to grid(lev).r to produce grid(lev+1).b: (unknowns of lev+1) x (unknowns of lev)"""
    return _transfer_csr(lev, 0)


def prolongation_csr(lev):
    """P from level lev + 1 to lev under the live interp_type, what coarse2fine(lev) adds to grid(lev).p from grid(lev+1).p with its halo
    filled: (unknowns of lev) x (unknowns of lev+1)"""
    return _transfer_csr(lev, 1)


def mixed_op(op, lev, n=1):
    """one fp32 operator of the mixed-precision cycle (option "cycle_precision" = 32) on level lev's fp64 fields, converted in and
    back: "relax" (n sweeps), "coarsest" (the coarsest solve of a cycle, lev = nlevs), "residual", "fine2coarse", "coarse2fine", "resrest", "vcycle" (include/mgx.h: mgx_mixed_op)."""
    check(lib().mgx_mixed_op(op.encode(), int(lev), int(n)))


def mixed_tail_first(nx, ny, nz):
    """first level of the tail of an fp32 cycle on the one-rank hierarchy of nx x ny x nz (option "mixed_tail"): from there down every level has
    at most 32768 cells and nz <= 32; 0 = no level is that small.  Pure host logic (include/mgx.h: mgx_mixed_tail_first)."""
    first = C.c_int()
    check(lib().mgx_mixed_tail_first(int(nx), int(ny), int(nz), C.byref(first)))
    return first.value


def mixed_ring_levels(nx, ny, nz):
    """the levels of the one-rank hierarchy of nx x ny x nz whose fp32 colour passes option "mixed_ring" hands to the pipelined kernel: bit
    lev-1 set = level lev served (nz one of 16, 20, 24, 32, 40, 48, 64 and more than 32768 cells, or nz > 32).  Pure host logic
    (include/mgx.h: mgx_mixed_ring_levels)."""
    mask = C.c_int()
    check(lib().mgx_mixed_ring_levels(int(nx), int(ny), int(nz), C.byref(mask)))
    return mask.value


def mixed_ring_choice(nx, ny, nz, nplanes):
    """the launch option "mixed_ring" = 1 makes for a colour pass of nplanes planes of a level of nx x ny x nz, as a dict: served, depth,
    planes_per_workgroup, stream (the non-temporal instance), workgroups, instance_nz.  Pure host logic (include/mgx.h: mgx_mixed_ring_choice)."""
    out = (C.c_int * 6)()
    check(lib().mgx_mixed_ring_choice(int(nx), int(ny), int(nz), int(nplanes), out))
    return dict(zip(("served", "depth", "planes_per_workgroup", "stream", "workgroups", "instance_nz"), out))


def mixed_direct_cells(nx, ny, nz, small_any_nz=0):
    """cells of the coarsest level of the one-rank hierarchy of nx x ny x nz where option "mixed_direct" serves the coarsest solve of an fp32
    cycle as one product (nz = 2 or 4, or 3 with small_any_nz; even nx, ny; at most 2048 cells; at least two levels), 0 = the sweeps.  Pure
    host logic (include/mgx.h: mgx_mixed_direct_cells)."""
    cells = C.c_int()
    check(lib().mgx_mixed_direct_cells(int(nx), int(ny), int(nz), int(small_any_nz), C.byref(cells)))
    return cells.value


def krylov_op(op, fields, nd=0, slot=None, sin=(), nout=2):
    """one pass of option "krylov" on level 1 (include/mgx.h: mgx_krylov_op).  fields: the pass's level-1 arrays (nx+2, ny+2, nz) in the
    header's order, C-contiguous float64; the ones the pass writes are rewritten in place.  -> (sout[:nout], path), path = the launch taken
    as a dict (mf, real, stream, gx, gy).  "apply32" / "update32": the two passes of option "krylov_precision" = 32."""
    nx, ny, nz = _state.dims
    for a in fields:
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (nx + 2, ny + 2, nz)):
            raise ValueError(f"krylov_op: need C-contiguous float64 arrays of shape {(nx + 2, ny + 2, nz)}")
    want = {"apply": 2 + nd, "ortho": 3 + 2 * nd, "update": 4, "apply32": 3 + nd, "update32": 5}.get(op)
    if want is not None and 0 <= nd <= 8 and len(fields) != want:   # (an unknown op or nd is the library's to refuse)
        raise ValueError(f"krylov_op({op}, nd = {nd}): {want} fields expected, got {len(fields)}")
    ptrs = (_DP * max(len(fields), 1))(*[_dp(a) for a in fields])
    sl = None if slot is None else (C.c_int * max(len(slot), 1))(*[int(s) for s in slot])
    si = (C.c_double * 17)(*[float(v) for v in sin])
    so = (C.c_double * 8)()
    path = (C.c_int * 5)()
    check(lib().mgx_krylov_op(op.encode(), int(nd), ptrs, sl, si, so, path))
    return np.array(so[:nout]), dict(zip(("mf", "real", "stream", "gx", "gy"), list(path)))


def rbseq_window_info(lev):
    """(rho, planes): the contraction bound of the level's red-black walk and the planes of warm-up of the windowed walk
    (option "rbseq_window", include/mgx.h); planes = 0: the walk over the whole level stays."""
    rho, m = C.c_double(), C.c_int()
    check(lib().mgx_rbseq_window_info(lev, C.byref(rho), C.byref(m)))
    return rho.value, m.value


def rbseq_window_rows(lev):
    """rows (from the bottom) the windowed walk's correction reaches on the level (option "rbseq_rowcut"); nz = every row."""
    r = C.c_int()
    check(lib().mgx_rbseq_window_rows(lev, C.byref(r)))
    return r.value


class _Level:
    """grid(lev) (mg_grids.f90:24-65): dims, decomposition info and host copies of the level's arrays."""

    def __init__(self, lev):
        self.lev = lev
        nx, ny, nz = C.c_int(), C.c_int(), C.c_int()
        check(lib().mgx_level_dims(lev, C.byref(nx), C.byref(ny), C.byref(nz)))
        self.nx, self.ny, self.nz = nx.value, ny.value, nz.value
        info = (C.c_int * 18)()
        check(lib().mgx_level_info(lev, info))
        (self.npx, self.npy, self.incx, self.incy, self.gather, self.ngx, self.ngy, self.key, self.color) = list(info[:9])
        self.neighb = list(info[10:18])

    def _shape(self, name):
        nx, ny, nz = self.nx, self.ny, self.nz
        return {"p": (nx + 2, ny + 2, nz), "b": (nx + 2, ny + 2, nz), "r": (nx + 2, ny + 2, nz),
                "cA": (nx + 2, ny + 2, nz, 8), "dx": (nx + 2, ny + 2), "dy": (nx + 2, ny + 2),
                "zeta": (nx + 2, ny + 2), "h": (nx + 2, ny + 2), "rmask": (nx + 2, ny + 2), "zr": (nx + 4, ny + 4, nz),
                "zw": (nx + 4, ny + 4, nz + 1), "cw": (nx + 2, ny + 2, nz + 1)}[name]

    def get(self, name):
        a = np.empty(self._shape(name), dtype=np.float64)
        check(lib().mgx_get_field(self.lev, FIELD[name], _dp(a)))
        return a

    def set(self, name, a):
        a = _f64(a, self._shape(name), name)
        check(lib().mgx_set_field(self.lev, FIELD[name], _dp(a)))

    def __getattr__(self, name):
        if name in FIELD:
            return self.get(name)
        raise AttributeError(name)


def grid(lev):
    return _Level(lev)


def _table(nl, out, what):
    if nl < 0:
        raise MgxError(f"{what}: invalid arguments")
    keys = ["nx", "ny", "nz", "npx", "npy", "incx", "incy", "gather", "ngx", "ngy", "key", "color"]
    res = []
    for l in range(nl):
        d = dict(zip(keys, list(out[20 * l:20 * l + 12])))
        d["neighb"] = list(out[20 * l + 12:20 * l + 20])
        res.append(d)
    return res


def level_table(nx, ny, nz, npx=1, npy=1, rank=0, nsmall=8, hold_odd_nz=0, hold_z_levels=0):
    """Level hierarchy of `rank` (mg_grids.f90:468-738) as a list of dicts; pure host logic, no GPU needed.
    hold_odd_nz=1: the table mgx_init builds under option "hold_odd_nz" -- an odd nz is handed on to the coarser levels, which go on
    coarsening in x and y down to the horizontal bound (include/mgx.h: mgx_level_table_hold).
    hold_z_levels=m: the table under option "hold_z_levels" -- the first m coarsenings keep nz (mgx_level_table_semi)."""
    out = (C.c_int * (20 * 32))()
    if hold_z_levels:
        return _table(lib().mgx_level_table_semi(nx, ny, nz, npx, npy, rank, nsmall, 0, int(hold_odd_nz), int(hold_z_levels), 32, out), out, "level_table")
    if hold_odd_nz:
        return _table(lib().mgx_level_table_hold(nx, ny, nz, npx, npy, rank, nsmall, 0, int(hold_odd_nz), 32, out), out, "level_table")
    return _table(lib().mgx_level_table(nx, ny, nz, npx, npy, rank, nsmall, 32, out), out, "level_table")


def level_table_periodic(nx, ny, nz, npx=1, npy=1, rank=0, nsmall=8, periodic=0, hold_odd_nz=0, hold_z_levels=0):
    """level_table with option "periodic" (bit 1: i, bit 2: j): the neighbour past the end of a periodic row or column of ranks is the rank
    at its other end, the rank itself on a level with one rank along the direction; pure host logic.  hold_odd_nz, hold_z_levels: as in
    level_table."""
    out = (C.c_int * (20 * 32))()
    if hold_z_levels:
        return _table(lib().mgx_level_table_semi(nx, ny, nz, npx, npy, rank, nsmall, periodic, int(hold_odd_nz), int(hold_z_levels), 32, out), out, "level_table_periodic")
    if hold_odd_nz:
        return _table(lib().mgx_level_table_hold(nx, ny, nz, npx, npy, rank, nsmall, periodic, int(hold_odd_nz), 32, out), out, "level_table_periodic")
    return _table(lib().mgx_level_table_periodic(nx, ny, nz, npx, npy, rank, nsmall, periodic, 32, out), out, "level_table_periodic")


def hold_z_hint(dx, dy, h, nz):
    """The m of option "hold_z_levels" that makes the cells of this block no taller than wide: the smallest m in 0..8 with
    2^m * min(dx, dy) >= max(h) / nz over the interior.  dx, dy, h: (nx+2, ny+2) arrays as handed to nhydro_matrices.  Pure host logic; on a
    process grid every rank must set the same option: take the maximum over the ranks (include/mgx.h: mgx_hold_z_hint)."""
    dx = np.ascontiguousarray(dx, dtype=np.float64); dy = np.ascontiguousarray(dy, dtype=np.float64); h = np.ascontiguousarray(h, dtype=np.float64)
    if dx.ndim != 2 or dx.shape != dy.shape or dx.shape != h.shape:
        raise MgxError(f"hold_z_hint: dx, dy, h must be 2-D arrays of one shape, got {dx.shape}, {dy.shape}, {h.shape}")
    m = C.c_int()
    check(lib().mgx_hold_z_hint(_dp(dx), _dp(dy), _dp(h), dx.shape[0] - 2, dx.shape[1] - 2, int(nz), C.byref(m)))
    return m.value


def exchange_plan(neighb, rank):
    """(entries, self_dirs) of one halo exchange of a rank with the neighbour table `neighb` (S, E, N, W, SW, SE, NE, NW; -1 = none): entries =
    [(peer, send direction, receive direction)] in the order handed to the exchange hook, self_dirs = the directions whose neighbour is the
    rank itself (served by device copies, never in the list).  include/mgx.h: mgx_exchange_plan; pure host logic."""
    nb = (C.c_int * 8)(*[int(v) for v in neighb])
    out = (C.c_int * 24)()
    mask = C.c_int()
    n = lib().mgx_exchange_plan(nb, rank, out, C.byref(mask))
    if n < 0:
        raise MgxError("exchange_plan: no decomposition produces this neighbour table")
    return [tuple(out[3 * t:3 * t + 3]) for t in range(n)], [d for d in range(8) if mask.value >> d & 1]


# ---- measurement helpers (bench.py) -------------------------------------------------------------
def time_relax(lev, reps):
    ms = C.c_float()
    check(lib().mgx_time_relax(lev, reps, C.byref(ms)))
    return ms.value


def time_residual(lev, reps):
    ms = C.c_float()
    check(lib().mgx_time_residual(lev, reps, C.byref(ms)))
    return ms.value


def counters():
    out = (C.c_longlong * 4)()
    check(lib().mgx_counters(out))
    d = dict(zip(("launches", "halo_fills", "exchanges", "allreduces"), list(out)))
    d["p2p_exchanges"] = int(lib().mgx_p2p_exchanges())
    return d
