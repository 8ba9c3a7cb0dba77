"""The padded storage of tests/test_gpu_state_view.py and its rank worker: a model's arrays with ghost cells, filled with a NaN sentinel of a
known bit pattern, and the views of the logical state inside them."""
import numpy as np

SENTINEL = {8: 0x7FF80000DEADBEEF, 4: 0x7FC0BEEF}   # quiet NaNs with a payload no computation produces
GHOST_K, GHOST_J, GHOST_I = (1, 0), (2, 3), (3, 2)  # ghost cells below / above the logical range, per direction


def _int_dtype(torch, esz):
    return torch.int64 if esz == 8 else torch.int32


def padded(torch, a):
    """(storage, view): storage holds the sentinel everywhere but in view, which is `a` (a float64 or float32 numpy array of a logical
    shape (nk, nj, ni)) inside ghost widths 3/2 in i, 2/3 in j, 1/0 in k, with the row pitch made odd by one more column where it is not"""
    nk, nj, ni = a.shape
    esz = a.dtype.itemsize
    pitch = ni + sum(GHOST_I)
    pitch += 1 - pitch % 2
    store = torch.full((nk + sum(GHOST_K), nj + sum(GHOST_J), pitch), SENTINEL[esz], dtype=_int_dtype(torch, esz), device="cuda")
    store = store.view(torch.float64 if esz == 8 else torch.float32)
    view = store[GHOST_K[0]:GHOST_K[0] + nk, GHOST_J[0]:GHOST_J[0] + nj, GHOST_I[0]:GHOST_I[0] + ni]
    view.copy_(torch.from_numpy(a).cuda())
    assert view.stride(2) == 1 and view.stride(1) % 2 == 1 and not view.is_contiguous()
    return store, view


def bits(torch, t):
    """a tensor's elements as integers (a contiguous copy)"""
    t = t.contiguous()
    return t.view(_int_dtype(torch, t.element_size()))


def padding_untouched(torch, store, view):
    """every element of the storage outside the view still holds the sentinel's bits"""
    esz = store.element_size()
    b = store.view(_int_dtype(torch, esz)).clone()
    off = view.storage_offset() - store.storage_offset()
    k0, r = divmod(off, store.stride(0))
    j0, i0 = divmod(r, store.stride(1))
    nk, nj, ni = view.shape
    inside = b[k0:k0 + nk, j0:j0 + nj, i0:i0 + ni]
    n_inside_sentinel = int((inside == SENTINEL[esz]).sum())
    inside.fill_(SENTINEL[esz])
    return bool((b == SENTINEL[esz]).all()), n_inside_sentinel


def state(dims, seed, dtype):
    """u, v, w of tests/_problem.uvw(dims, seed) as `dtype`, with no zero element"""
    from _problem import uvw
    s = tuple(np.ascontiguousarray(a.astype(dtype)) for a in uvw(dims, seed))
    assert all(np.all(a != 0) for a in s)
    return s
