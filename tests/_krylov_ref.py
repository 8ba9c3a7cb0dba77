"""Reference for option "krylov": right-preconditioned truncated GCR (Orthomin(m)) in numpy over the CPU oracle.  Preconditioner = the
oracle's F-cycle from p = 0 on the right-hand side r, operator = the oracle's residual with b = 0 (sign turned), inner products over
interior cells.  Convergence is only reported on the true residual b - A p: where that is not below tol it replaces r, the retained
pairs are dropped (a restart) and the loop goes on.  `dot` lets a test sum the inner products in another order."""
import math

import numpy as np


def dot_plain(x, y):
    return float((x * y).sum())


def dot_reversed(x, y):
    return float((x * y).ravel()[::-1].sum())


def dot_fsum(x, y):
    return math.fsum((x * y).ravel())


def gcr(o, m, tol, maxite, dot=dot_plain, cold=True):
    """-> (iterations, history, restarts); o.field("p") holds the iterate and o.field("r") its true residual afterwards"""
    nx, ny = o.field("p").shape[0] - 2, o.field("p").shape[1] - 2
    I = (slice(1, nx + 1), slice(1, ny + 1), slice(None))
    p, b, r = o.field("p"), o.field("b"), o.field("r")
    b0 = b.copy()
    x = np.zeros_like(p) if cold else p.copy()
    bn = math.sqrt(dot(b0[I], b0[I]))

    def true_res():
        b[...] = b0; p[...] = x; o.residual(1)
        return r.copy()

    def prec(rr):   # z = M rr, halo of z valid
        b[...] = rr; p[...] = 0.0; o.residual(1); o.fcycle()
        return p.copy()

    def aop(z):     # q = A z
        b[...] = 0.0; p[...] = z; o.residual(1)
        return -r

    res = true_res()
    hist = [math.sqrt(dot(res[I], res[I])) / bn]
    Z, Q, S, n, restarts, fresh = [], [], [], 0, 0, True
    while True:
        while n < maxite and hist[-1] > tol:
            z = prec(res); q = aop(z)
            for zi, qi, si in zip(Z, Q, S):
                be = dot(q[I], qi[I]) / si
                q -= be * qi; z -= be * zi
            s, t = dot(q[I], q[I]), dot(res[I], q[I])
            fresh = False
            if not (s > 0.0 and math.isfinite(s) and math.isfinite(t)):
                break
            x += (t / s) * z; res -= (t / s) * q
            Z.append(z); Q.append(q); S.append(s)
            if len(Z) > m:
                Z.pop(0); Q.pop(0); S.pop(0)
            n += 1
            hist.append(math.sqrt(dot(res[I], res[I])) / bn)
        if fresh:
            break
        res = true_res(); fresh = True
        hist[-1] = math.sqrt(dot(res[I], res[I])) / bn
        if n >= maxite or not hist[-1] > tol or not (s > 0.0 and math.isfinite(s) and math.isfinite(t)):
            break
        restarts += 1; Z, Q, S = [], [], []
    true_res()
    return n, np.array(hist), restarts


def history_noise(h1, h2, floor):
    """largest relative difference of two histories, entry by entry, over the entries both hold above `floor`"""
    k = min(len(h1), len(h2))
    a, c = np.asarray(h1[:k]), np.asarray(h2[:k])
    use = (a > floor) & (c > floor)
    return float((np.abs(a - c)[use] / c[use]).max())


def eps_ref(make, m, tol, maxite=50):
    """the reference's own sensitivity to the order of its sums on one case: make() -> a fresh oracle with its right-hand side set.
    -> (eps_ref, iterations, history of the plain order).  The largest of plain-vs-reversed and plain-vs-fsum."""
    n0, h0, _ = gcr(make(), m, tol, maxite)
    e = 0.0
    for d in (dot_reversed, dot_fsum):
        _, h, _ = gcr(make(), m, tol, maxite, dot=d)
        e = max(e, history_noise(h, h0, tol))
    return e, n0, h0
