"""NumPy restatement of the HSH peak search of include/rti.h (rti_hsh_normals.hip): the grid, the luminance map, and
from the fp32 grid values V[E] the argmax with the smallest-index tie, the fp64 parabolic refinement, the kinds, the
normal and the peak.  What it does not restate is V itself: a test takes that from rti.relight (whose bits the
kernel must reproduce) or, on the CPU, from the oracle's fp64 basis."""
import functools

import numpy as np

LUMA = (0.299, 0.587, 0.114)


@functools.lru_cache(maxsize=None)
def grid_points(G):
    """The masked integer pairs ((i, j), ...) in the kernel's order: j ascending, then i ascending."""
    return tuple((i, j) for j in range(-G, G + 1) for i in range(-G, G + 1) if i * i + j * j <= G * G)


@functools.lru_cache(maxsize=None)
def _grid_index(G):
    return {p: e for e, p in enumerate(grid_points(G))}


def grid_dirs(G):
    """(u [E], v [E]) in fp64: i / G and j / G."""
    pts = np.array(grid_points(G), np.float64)
    return pts[:, 0] / np.float64(G), pts[:, 1] / np.float64(G)


def luminance(maps, weights=None):
    """maps fp32 [3, P, k] -> fp32 [P, k]: (wR·r + wG·g) + wB·b, two products and two sums, each rounded."""
    w = np.asarray(LUMA if weights is None else weights, np.float32)
    m = np.asarray(maps, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        rg = (w[0] * m[0]).astype(np.float32) + (w[1] * m[1]).astype(np.float32)
        return (rg.astype(np.float32) + (w[2] * m[2]).astype(np.float32)).astype(np.float32)


def _step(has, vm, v0, vp):
    if not has:
        return 0.0
    vm, v0, vp = np.float64(vm), np.float64(v0), np.float64(vp)
    d = (vm - 2.0 * v0) + vp
    if not d < 0.0:
        return 0.0
    t = 0.5 * (vm - vp) / d
    t = -0.5 if t < -0.5 else t
    return 0.5 if t > 0.5 else float(t)


def peak_normal(V, G, finite=True):
    """One pixel: V fp32 [E] (the grid values), finite: every luminance coefficient is finite ->
    (normal fp32 [3], kind, peak fp32)."""
    pts, index = grid_points(G), _grid_index(G)
    V = np.asarray(V, np.float32)
    assert V.shape == (len(pts),)
    if not finite:
        return np.full(3, np.nan, np.float32), 4, np.float32(np.nan)
    e = int(np.argmax(V))  # the first of equal maxima
    v0 = V[e]
    if V.max() == V.min():
        return np.float32([0.0, 0.0, 1.0]), 2, v0
    i, j = pts[e]

    def at(p):
        return V[index[p]] if p in index else v0

    du = _step((i - 1, j) in index and (i + 1, j) in index, at((i - 1, j)), v0, at((i + 1, j)))
    dv = _step((i, j - 1) in index and (i, j + 1) in index, at((i, j - 1)), v0, at((i, j + 1)))
    u0 = (np.float64(i) + du) / np.float64(G)
    w0 = (np.float64(j) + dv) / np.float64(G)
    r2 = u0 * u0 + w0 * w0
    if r2 <= 1.0:
        return np.float32([u0, w0, np.sqrt(1.0 - r2)]), 0, v0
    s = np.sqrt(r2)
    return np.float32([u0 / s, w0 / s, 0.0]), 1, v0


def peak_normals(V, G, lum=None):
    """V fp32 [E, P] (rti.relight's eval-major output), lum fp32 [P, k] or None (all finite) ->
    (normals fp32 [P, 3], kind uint8 [P], peak fp32 [P])."""
    V = np.asarray(V, np.float32)
    P = V.shape[1]
    finite = np.ones(P, bool) if lum is None else np.isfinite(np.asarray(lum)).all(axis=-1)
    n, kind, peak = np.empty((P, 3), np.float32), np.empty(P, np.uint8), np.empty(P, np.float32)
    for p in range(P):
        n[p], kind[p], peak[p] = peak_normal(V[:, p], G, bool(finite[p]))
    return n, kind, peak
