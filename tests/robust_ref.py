"""fp64 restatement of rti_fit_shared_robust's semantics (include/rti.h): a plain NumPy per-pixel loop that
imports nothing from the package.  The tests compare the kernels with it and check their input conditions
with the pivots it reports."""
import numpy as np

PIVOT_TOL = 1e-10


def solve(A, y, w):
    """Weighted normal equations by Cholesky -> (coef or None, pivot): the solve fails at a pivot
    d_j <= PIVOT_TOL·max diag G; pivot = the failing d_j, or the smallest one, over max diag G."""
    G = (A * w[:, None]).T @ A
    b = A.T @ (w * y)
    k = G.shape[0]
    dmax = G.diagonal().max()
    L = np.zeros((k, k))
    piv = np.inf
    for j in range(k):
        d = G[j, j] - L[j, :j] @ L[j, :j]
        if not d > PIVOT_TOL * dmax:
            return None, d / dmax
        piv = min(piv, d / dmax)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return np.linalg.solve(L.T, np.linalg.solve(L, b)), piv


def fit_robust_ref(A, I, lo=-np.inf, hi=np.inf, min_lights=None, iters=0, delta=0.0):
    """A fp64 [N, k], I [N, P] -> dict(coef [P, k], res [P], kept [P], fallback_px, min_pivot [P] (smallest
    pivot of the pixel's successful solves), fail_pivot [P] (the window solve's failing pivot, NaN if none))."""
    N, k = A.shape
    P = I.shape[1]
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    min_lights = k if min_lights is None else min_lights
    coef, res, kept = np.full((P, k), np.nan), np.full(P, np.nan), np.zeros(P, np.int32)
    min_pivot, fail_pivot, fallback_px = np.full(P, np.inf), np.full(P, np.nan), 0
    for p in range(P):
        y = I[:, p].astype(np.float64)
        win = ((y >= lo) & (y <= hi)).astype(np.float64)
        c, piv = solve(A, y, win) if win.sum() >= min_lights else (None, np.nan)
        if c is None:
            fail_pivot[p] = piv
            fallback_px += 1
            win = np.ones(N)
            c, piv = solve(A, y, win)
        kept[p] = int(win.sum())
        if c is None:
            continue
        min_pivot[p] = piv
        for _ in range(iters):
            r = np.abs(y - A @ c)
            c2, piv = solve(A, y, win * np.where(r <= delta, 1.0, delta / np.maximum(r, 1e-300)))
            if c2 is None:
                break
            c, min_pivot[p] = c2, min(min_pivot[p], piv)
        coef[p] = c
        res[p] = np.sqrt((win * (y - A @ c) ** 2).sum() / kept[p])
    return dict(coef=coef, res=res, kept=kept, fallback_px=fallback_px, min_pivot=min_pivot, fail_pivot=fail_pivot)


def check_inputs(ref, I, lo=-np.inf, hi=np.inf, rank_fallback=()):
    """The condition under which a rounding difference cannot flip a decision of the fit: every successful solve
    keeps its pivots >= 1e-6·max diag G, the pixels meant to fall back on rank (and only they) fail at a pivot
    <= 1e-13·max diag G, and no sample lies within 1e-3 of a bound."""
    assert (ref["min_pivot"][np.isfinite(ref["coef"]).all(-1)] >= 1e-6).all(), ref["min_pivot"].min()
    failed = np.flatnonzero(~np.isnan(ref["fail_pivot"]))
    assert sorted(failed) == sorted(rank_fallback), failed
    assert (ref["fail_pivot"][failed] <= 1e-13).all(), ref["fail_pivot"][failed]
    y = np.asarray(I, np.float64)
    for bound in (lo, hi):
        if np.isfinite(bound):
            assert np.abs(y - bound).min() > 1e-3
