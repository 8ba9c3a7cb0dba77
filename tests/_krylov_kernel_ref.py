"""Plain references of the three passes of option "krylov" (mgx_krylov.hip), for tests/test_gpu_krylov_kernels.py and the CPU tests of
tests/test_krylov_reference.py: numpy on host arrays of shape (nx+2, ny+2, nz) (index [i][j][k], halo included) plus the CPU oracle's
residual.  Nothing here touches the GPU.

Exactness by construction (ortho, update): the fields hold small integers, the betas are small integers, t / s is a power of two, so every
intermediate is an integer (or a multiple of `unit`, a power of two) and every sum stays below 2^53 units: then EVERY summation order gives
the same bits, and a kernel must return the numpy result exactly.  `check_exact` asserts that bound case by case."""
import math

import numpy as np

HALO = 2.0 ** 40   # magnitude of the halo cells of r, q, q_i: one of them leaking into a sum changes it by >= 2^40, still exactly

# Level-1 shapes (nx, ny, nz) and the launch paths of mgx_krylov.hip they take.  gx = ceil(ny/2 / 64), gy = ceil(nx / 4) are the block map of
# pass 1; stream = nx*ny*nz*72 > 256e6 (the non-temporal variant of all three passes).
#   (4, 4, 2)       nz = 2: the stored-slot operator although the matrix is the library's own; gx = 1, gy = 1 (second branch of kr_block_map)
#   (6, 10, 4)      nx not a multiple of 4: plane group cut by i <= nx, gy = 2; ny/2 = 5 odd: a 16-byte pair ends mid-way in both half-rows
#   (30, 6, 6)      the same cuts with gy = 8 (first branch of kr_block_map), matrix-free.  (30, 18, 6), the size first thought of, is refused by
#                   mgx_init: its second level would be 15 x 9; a single-level shape is the nearest one that is accepted
#   (30, 18, 2)     the same cuts, nz = 2 -> stored slots (one level: nz = 2 does not coarsen)
#   (24, 40, 8)     gy = 6: gy & 7 != 0 with several plane groups
#   (4, 130, 4)     ny/2 = 65: gx = 2, the second j-chunk has ONE live lane; ny/2 odd
#   (32, 32, 24)    nz not a power of two, gy = 8
#   (16, 16, 128)   tall columns (nz per lane in the column walk of pass 1)
#   (64, 64, 16)    the size of the solver-level comparisons
#   (256, 256, 64)  stream = 1, gx = 2 with two full chunks, gy = 64
#   (512, 512, 64)  stream = 1 at the size of the benchmark, gx = 4, gy = 128
SMALL_SHAPES = [(4, 4, 2), (6, 10, 4), (30, 6, 6), (30, 18, 2), (24, 40, 8), (4, 130, 4), (32, 32, 24), (16, 16, 128), (64, 64, 16)]
BIG_SHAPES = [(256, 256, 64), (512, 512, 64)]
SHAPES = SMALL_SHAPES + BIG_SHAPES
NDS = (0, 1, 3, 8)


def interior(a):
    return a[1:-1, 1:-1, :]


def expected_path(nx, ny, nz):
    """what the shape list above claims, from the dimensions alone: (stream, gx, gy)"""
    return int(nx * ny * nz * 72.0 > 256e6), (ny // 2 + 63) // 64, (nx + 3) // 4


# ---- sums --------------------------------------------------------------------------------------------------------------------
def dot_plain(x, y):
    return float((interior(x) * interior(y)).sum())


def dot_reversed(x, y):
    return float((interior(x) * interior(y)).ravel()[::-1].sum())


def dot_fsum(x, y):
    return math.fsum((interior(x) * interior(y)).ravel())


def abs_dot(x, y):
    """sum |x y| over the interior (the weight of a summation bound)"""
    return math.fsum(np.abs(interior(x) * interior(y)).ravel())


# ---- the three passes ----------------------------------------------------------------------------------------------------------
def ref_apply(o, z):
    """q = A z by the oracle: the negative of the r its residual(1) leaves for b = 0 (interior cells; the halo of q is not defined).
    z: halos as given, physical ones refreshed by the oracle's fill_halo as the issue of the operator asks."""
    o.field("b")[...] = 0.0
    o.field("p")[...] = z
    o.fill_halo(1, "p")
    o.residual(1)
    return -o.field("r").copy()


def ref_ortho(z, q, r, zi, qi, sc, qq, slot, dot=dot_plain):
    """-> (z', q', (q', q'), (r, q')): beta_n = sc[n] / qq[slot[n]], whole arrays updated, sums over the interior"""
    z, q = z.copy(), q.copy()
    for n in range(len(qi)):
        be = sc[n] / qq[slot[n]]
        q -= be * qi[n]
        z -= be * zi[n]
    return z, q, dot(q, q), dot(r, q)


def step_ok(s, t):
    return s > 0.0 and math.isfinite(s) and math.isfinite(t)


def ref_update(p, r, z, q, s, t, dot=dot_plain):
    """-> (p', r', ||r'||^2 or -1, qq_new): no step with unusable scalars"""
    if not step_ok(s, t):
        return p.copy(), r.copy(), -1.0, s
    al = t / s
    p, r = p + al * z, r - al * q
    return p, r, dot(r, r), s


# ---- integer cases --------------------------------------------------------------------------------------------------------------
def int_field(rng, shape, halo=None):
    """integers of [-8, 8] everywhere; halo: the halo cells (i = 0, nx+1, j = 0, ny+1) get +-halo instead"""
    nx, ny, nz = shape
    a = rng.integers(-8, 9, size=(nx + 2, ny + 2, nz), dtype=np.int8).astype(np.float64)
    if halo is not None:
        sg = np.where(rng.integers(0, 2, size=a.shape, dtype=np.int8) > 0, halo, -halo)
        keep = interior(a).copy()
        a[...] = sg
        interior(a)[...] = keep
    return a


def rotated_slots(nd, shift=None):
    """the slots of the nd retained pairs in a ring of nd + 1 after its head has wrapped: oldest first, head = (last + 1) mod (nd + 1)"""
    if nd == 0:
        return []
    shift = (nd // 2 + 1) if shift is None else shift
    return [(shift + n) % (nd + 1) for n in range(nd)]


def ortho_case(shape, nd, seed, slot=None):
    """integer inputs of pass 2: |fields| <= 8 inside, 2^40 in the halos of r, q, q_i; qq[slot] distinct powers of two, sc[n] = b_n qq[slot[n]]
    with integer 1 <= |b_n| <= 4"""
    rng = np.random.default_rng(seed)
    slot = list(range(nd)) if slot is None else list(slot)
    z, q, r = int_field(rng, shape), int_field(rng, shape, HALO), int_field(rng, shape, HALO)
    zi = [int_field(rng, shape) for _ in range(nd)]
    qi = [int_field(rng, shape, HALO) for _ in range(nd)]
    qq = [2.0 ** (3 + s) for s in range(9)]                      # every ring slot another value: a wrong slot gives another (integer) beta
    b = [float(((n % 4) + 1) * (-1) ** n) for n in range(nd)]
    sc = [b[n] * qq[slot[n]] for n in range(nd)] + [0.0] * (8 - nd)
    return dict(z=z, q=q, r=r, zi=zi, qi=qi, sc=sc, qq=qq, slot=slot, b=b)


def update_case(shape, seed, s=4.0, t=2.0):
    rng = np.random.default_rng(seed)
    return dict(p=int_field(rng, shape), r=int_field(rng, shape, HALO), z=int_field(rng, shape), q=int_field(rng, shape, HALO), s=s, t=t)


def check_exact(arrays, products, unit=1.0):
    """the condition under which every summation order gives the same bits: every listed array holds multiples of `unit` (a power of two)
    and for every listed pair sum |x y| over the interior, in units of unit^2, stays below 2^53 (as does every element)"""
    for a in arrays:
        assert np.array_equal(np.round(a / unit) * unit, a), "a field is not a multiple of the unit"
        assert np.abs(a).max() / unit < 2.0 ** 53
    for x, y in products:
        w = float(np.abs(interior(x) * interior(y)).sum(dtype=np.float64)) / (unit * unit)
        assert w < 2.0 ** 53, w


# ---- one-hot probes of the inner products of pass 1 ----------------------------------------------------------------------------------
def onehot_cells(nx, ny, nz):
    """interior cells (i, j, k) where pass 1's reduction goes wrong first.  A lane of pass 1 is a column: lane = jh % 64 with j = 2 jh + 1
    (odd half-row) or 2 jh + 2 (even), wave = (i - 1) % 4, workgroup = (j-chunk of 64, plane group of 4, parity)."""
    cells = [(i, j, k) for i in (1, nx) for j in (1, ny) for k in (1, nz)]                 # the eight corners (k = 1 and k = nz)
    mid = (nx + 1) // 2
    cells += [(mid, j, 1) for j in (1, ny - 1, 2, ny)]                                     # first and last cell of either half-row
    if ny // 2 > 64:
        cells += [(1, 127, nz), (1, 129, nz), (1, 128, 1), (1, 130, 1)]                    # lane 63 of a full wave, lane 0 of the next j-chunk
    if nx >= 2:
        cells += [(1, ny - 1, nz), (2, 1, 1)]                                              # last live lane of wave 0, first lane of wave 1
    if nx >= 5:
        cells += [(4, ny, 1), (5, 2, nz)]                                                  # last wave of a plane group, first of the next
    cells += [(nx, 2, nz), (nx, ny - 1, 1)]                                                # the last plane (of a cut plane group when nx % 4)
    out = []
    for c in cells:
        if c not in out:
            out.append(c)
    return out


def halo_probes(nx, ny, nz):
    """halo cells: a one-hot there must give exactly 0"""
    mid, mjd = (nx + 1) // 2, (ny + 1) // 2
    return [(0, mjd, 1), (nx + 1, mjd, nz), (mid, 0, 1), (mid, ny + 1, nz), (0, 0, 1), (nx + 1, ny + 1, nz), (0, ny + 1, 1), (nx + 1, 0, nz)]


def is_interior(c, nx, ny, nz):
    i, j, k = c
    return 1 <= i <= nx and 1 <= j <= ny and 1 <= k <= nz


def onehot_fields(cells, shape):
    """one field per cell with 2^n at cell n (k is 1-based) -> (fields, weights)"""
    nx, ny, nz = shape
    fs, ws = [], []
    for n, (i, j, k) in enumerate(cells):
        a = np.zeros((nx + 2, ny + 2, nz))
        a[i, j, k - 1] = 2.0 ** n
        fs.append(a); ws.append(2.0 ** n)
    return fs, ws


# ---- summation bounds ------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative bound (against sum |x_i y_i|) of an inner product whose longest chain of
    additions, plus one for the rounding of the product, is n"""
    return n * U / (1.0 - n * U)


def apply_chain(nx, ny, nz):
    """longest chain of additions of one (q, q_i) of pass 1, read off mgx_krylov.hip: a lane adds its column's nz products one after the
    other (PUT_ROW), kr_block_sums folds the wave in 6 shuffle steps and adds the 4 waves in 3 additions, k_kr_reduce lets each of 256
    threads add ceil(nblk / 256) partial sums sequentially and folds them in 8 tree steps; nblk = 2 gx gy workgroups"""
    gx, gy = (ny // 2 + 63) // 64, (nx + 3) // 4
    return nz + 6 + 3 + -(-(2 * gx * gy) // 256) + 8


def stream_chain(nx, ny, nz):
    """the same for a sum of passes 2 and 3: a lane takes pairs of a chunk of 2048 elements 512 apart, 4 pairs = 8 additions; then as above
    with nblk = ceil(plane / 2048) (nx + 2) workgroups, plane = nz RS, RS = the padded row of the solver's layout"""
    up = lambda a, m: (a + m - 1) // m * m
    ho = up(16 + ny // 2, 16)
    rs = up(ho + ny // 2 + 1, 16)
    nblk = -(-(nz * rs) // 2048) * (nx + 2)
    return 8 + 6 + 3 + -(-nblk // 256) + 8


# ---- one GCR built from the three reference passes (the CPU test that ties them to tests/_krylov_ref.gcr) -----------------------------------
def gcr_from_passes(o, m, tol, maxite):
    """the loop of tests/_krylov_ref.gcr without restarts, every step taken through ref_apply / ref_ortho / ref_update and the ring of
    m + 1 slots of solve_p_krylov -> (iterations, history)"""
    p, b, r = o.field("p"), o.field("b"), o.field("r")
    b0 = b.copy()
    bn = math.sqrt(dot_plain(b0, b0))
    x = np.zeros_like(p)
    b[...] = b0; p[...] = x; o.residual(1)
    res = r.copy()
    hist = [math.sqrt(dot_plain(res, res)) / bn]
    Z, Q, qq = [None] * (m + 1), [None] * (m + 1), [0.0] * (m + 1)
    kept = head = n = 0
    while n < maxite and hist[-1] > tol:
        b[...] = res; p[...] = 0.0; o.residual(1); o.fcycle()
        z = p.copy()
        q = ref_apply(o, z)
        slot = [(head + m + 1 - kept + k) % (m + 1) for k in range(kept)]
        sc = [dot_plain(q, Q[s]) for s in slot]
        z, q, s, t = ref_ortho(z, q, res, [Z[s] for s in slot], [Q[s] for s in slot], sc, qq, slot)
        x, res, rr, qq[head] = ref_update(x, res, z, q, s, t)
        if rr < 0:
            break
        Z[head], Q[head] = z, q
        kept = min(kept + 1, m); head = (head + 1) % (m + 1)
        n += 1
        hist.append(math.sqrt(rr) / bn)
    return n, np.array(hist)
