"""NumPy fp64 restatement of rti_height_from_normals (include/rti.h) and the shared inputs of
tests/test_height_abi.py and tests/test_gpu_height.py.

The problem: mask (with the isolated-pixel rule), gradients p and q, the right-hand side b in the stated order, the
graph Laplacian (dense), its exact minimum-norm solution and smallest non-zero eigenvalue (one eigendecomposition,
A⁺ = V Λ⁺ Vᵀ), component labels by a flood fill.  The preconditioner: the 2×2 aggregation hierarchy with summed
integer weights, the prolongations as matrices, and the V-cycle as a matrix for small shapes."""
import functools

import numpy as np

OMEGA, OVER, COARSEST_SWEEPS, COARSEST_MAX = 0.8, 2.0, 8, 4
NZ_MIN = 0.1


# ---- the problem ---------------------------------------------------------------------------------------------------

def raw_valid(n, nz_min=NZ_MIN):
    """n fp32 [H, W, 3]: finite components and n_z >= nz_min."""
    n = np.asarray(n, np.float32)
    return np.isfinite(n).all(-1) & (np.where(np.isfinite(n[..., 2]), n[..., 2], -1.0).astype(np.float64) >= nz_min)


def edge_weights(valid):
    """wR[y, x] = 1 for an edge (y, x)-(y, x+1), wD[y, x] = 1 for (y, x)-(y+1, x), between valid pixels."""
    wR = np.zeros(valid.shape, np.int64)
    wD = np.zeros(valid.shape, np.int64)
    wR[:, :-1] = valid[:, :-1] & valid[:, 1:]
    wD[:-1, :] = valid[:-1, :] & valid[1:, :]
    return wR, wD


def degree(wR, wD):
    d = wR + wD
    d[:, 1:] += wR[:, :-1]
    d[1:, :] += wD[:-1, :]
    return d


def mask(n, nz_min=NZ_MIN):
    """The valid pixels: raw-valid with at least one raw-valid 4-neighbour (the degree of the edge graph)."""
    return degree(*edge_weights(raw_valid(n, nz_min))) > 0


def gradients(n, nz_min=NZ_MIN, flip_y=False):
    """p = −n_x/n_z, q = ∓n_y/n_z in fp64 from the fp32 components at raw-valid pixels, 0 elsewhere."""
    n = np.asarray(n, np.float32).astype(np.float64)
    v = raw_valid(n.astype(np.float32), nz_min)
    nz = np.where(v, n[..., 2], 1.0)
    px = np.where(v, n[..., 0], 0.0) / nz
    qy = np.where(v, n[..., 1], 0.0) / nz
    return -px, (qy if flip_y else -qy)


def rhs(p, q, wR, wD):
    """b_i = Σ −g_ij with the edge oriented from i, in the order left, right, up, down."""
    H, W = p.shape
    b = np.zeros((H, W))
    gx = 0.5 * (p[:, :-1] + p[:, 1:])  # the edge (y, x)-(y, x+1)
    gy = 0.5 * (q[:-1, :] + q[1:, :])
    b[:, 1:] += np.where(wR[:, :-1] > 0, gx, 0.0)   # left neighbour
    b[:, :-1] -= np.where(wR[:, :-1] > 0, gx, 0.0)  # right
    b[1:, :] += np.where(wD[:-1, :] > 0, gy, 0.0)   # up
    b[:-1, :] -= np.where(wD[:-1, :] > 0, gy, 0.0)  # down
    return b


def laplacian(wR, wD):
    """The dense weighted graph Laplacian [h·w, h·w] of a grid's edge weights."""
    h, w = wR.shape
    n = h * w
    A = np.zeros((n, n))
    idx = np.arange(n).reshape(h, w)
    for wt, i, j in ((wR[:, :-1], idx[:, :-1], idx[:, 1:]), (wD[:-1, :], idx[:-1, :], idx[1:, :])):
        wt, i, j = wt.ravel().astype(np.float64), i.ravel(), j.ravel()
        np.add.at(A, (i, j), -wt)
        np.add.at(A, (j, i), -wt)
        np.add.at(A, (i, i), wt)
        np.add.at(A, (j, j), wt)
    return A


def components(valid):
    """Labels 1, 2, ... of the 4-connected components of the valid pixels (0 = invalid), by a flood fill."""
    H, W = valid.shape
    lab = np.zeros((H, W), np.int64)
    cur = 0
    for y0 in range(H):
        for x0 in range(W):
            if not valid[y0, x0] or lab[y0, x0]:
                continue
            cur += 1
            lab[y0, x0] = cur
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= yy < H and 0 <= xx < W and valid[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = cur
                        stack.append((yy, xx))
    return lab


class Problem:
    """Everything the checks need of one normal map, computed once."""

    def __init__(self, n, nz_min=NZ_MIN, flip_y=False):
        self.n = np.ascontiguousarray(n, np.float32)
        self.H, self.W = self.n.shape[:2]
        rv = raw_valid(self.n, nz_min)
        self.wR, self.wD = edge_weights(rv)
        self.deg = degree(self.wR, self.wD)
        self.valid = self.deg > 0
        self.p, self.q = gradients(self.n, nz_min, flip_y)
        self.b = rhs(self.p, self.q, self.wR, self.wD)
        self.norm_b = float(np.sqrt((self.b ** 2).sum()))
        self.labels = components(self.valid)

    @functools.cached_property
    def A(self):
        return laplacian(self.wR, self.wD)

    @functools.cached_property
    def _eig(self):
        if not self.valid.any():
            return np.zeros(0), np.zeros((self.H * self.W, 0))
        lam, V = np.linalg.eigh(self.A)
        keep = lam > 1e-9 * max(lam[-1], 1.0)  # the null space: one constant per component, and the invalid pixels
        return lam[keep], V[:, keep]

    @property
    def lambda2(self):
        """The smallest non-zero eigenvalue of the Laplacian."""
        return float(self._eig[0][0])

    @functools.cached_property
    def z(self):
        """The exact least-squares surface [H, W]: A⁺ b, zero mean on every component, NaN at invalid pixels."""
        lam, V = self._eig
        z = (V @ ((V.T @ self.b.ravel()) / lam)).reshape(self.H, self.W)
        return np.where(self.valid, z, np.nan)

    def align(self, got):
        """got with each component's mean difference to the reference removed (the components float)."""
        out = np.array(got, np.float64)
        for c in range(1, int(self.labels.max()) + 1):
            m = self.labels == c
            out[m] -= (out[m] - self.z[m]).mean()
        return out


# ---- the preconditioner --------------------------------------------------------------------------------------------

def levels(H, W):
    """Grids of the hierarchy: halve (rounding up) until max(H_l, W_l) <= 4."""
    L = 1
    while max(H, W) > COARSEST_MAX:
        H, W, L = (H + 1) // 2, (W + 1) // 2, L + 1
    return L


def coarsen(wR, wD):
    """The next level's weights: a coarse edge sums the fine weights crossing between the two 2×2 aggregates."""
    h, w = wR.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    cR = np.zeros((ch, cw), np.int64)
    cD = np.zeros((ch, cw), np.int64)
    for y in range(h):
        for x in range(w):
            if x + 1 < w and (x + 1) // 2 != x // 2:
                cR[y // 2, x // 2] += wR[y, x]
            if y + 1 < h and (y + 1) // 2 != y // 2:
                cD[y // 2, x // 2] += wD[y, x]
    return cR, cD


def hierarchy(wR, wD):
    """[(wR_l, wD_l)] for l = 0 .. levels − 1."""
    out = [(np.asarray(wR, np.int64), np.asarray(wD, np.int64))]
    while max(out[-1][0].shape) > COARSEST_MAX:
        out.append(coarsen(*out[-1]))
    return out


def prolongation(wR, wD):
    """P [n_l, n_{l+1}]: 1 from a cell that has a row (degree > 0) to its aggregate, piecewise constant."""
    h, w = wR.shape
    cw = (w + 1) // 2
    d = degree(wR, wD)
    P = np.zeros((h * w, ((h + 1) // 2) * cw))
    for y in range(h):
        for x in range(w):
            if d[y, x] > 0:
                P[y * w + x, (y // 2) * cw + x // 2] = 1.0
    return P


def _sweeps(A, dinv, F, X, count):
    for _ in range(count):
        X = X + OMEGA * dinv[:, None] * (F - A @ X)
    return X


def vcycle_apply(levels_, F, l=0):
    """The V-cycle of level l applied to the columns of F."""
    wR, wD = levels_[l]
    A = laplacian(wR, wD)
    d = degree(wR, wD).ravel().astype(np.float64)
    dinv = np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0)
    X = np.zeros_like(F)
    if l == len(levels_) - 1:
        return _sweeps(A, dinv, F, X, COARSEST_SWEEPS)
    X = _sweeps(A, dinv, F, X, 2)
    P = prolongation(wR, wD)
    X = X + OVER * (P @ vcycle_apply(levels_, P.T @ (F - A @ X), l + 1))
    return _sweeps(A, dinv, F, X, 2)


def vcycle_matrix(wR, wD):
    """M⁻¹ [n, n] of the multigrid preconditioner on the grid of these weights."""
    n = wR.size
    return vcycle_apply(hierarchy(wR, wD), np.eye(n))


def pcg(A, b, apply_m, rtol, max_iters):
    """Preconditioned conjugate gradients from 0 -> (z, iterations, met)."""
    z = np.zeros_like(b)
    r = b.copy()
    nb = np.linalg.norm(b)
    if nb == 0.0:
        return z, 0, True
    s = apply_m(r)
    p = s.copy()
    rho = r @ s
    for k in range(1, max_iters + 1):
        q = A @ p
        pq = p @ q
        alpha = rho / pq if pq > 0 else 0.0
        z += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= rtol * nb:
            return z, k, True
        s = apply_m(r)
        rho, old = r @ s, rho
        p = s + (rho / old if old > 0 else 0.0) * p
    return z, max_iters, False


# ---- inputs --------------------------------------------------------------------------------------------------------

def normals_of(zx, zy):
    """Unit normals (−z_x, −z_y, 1)/‖·‖ rounded to fp32, [H, W, 3]."""
    n = np.stack([-zx, -zy, np.ones_like(zx)], -1)
    return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)


def relief(H, W, seed=0):
    """A smooth synthetic relief's normals: a few low-frequency waves with slopes below 1."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    zx, zy = np.zeros((H, W)), np.zeros((H, W))
    for _ in range(4):
        fx, fy = rng.uniform(0.02, 0.25, 2)
        a, ph = rng.uniform(0.3, 1.0), rng.uniform(0, 2 * np.pi)
        c = a * np.cos(fx * x + fy * y + ph) / 4.0
        zx += c * fx / max(fx, fy)
        zy += c * fy / max(fx, fy)
    return normals_of(zx, zy)


def steep(nz=0.05):
    """A unit normal with n_z below the default nz_min."""
    return np.array([np.sqrt(1.0 - nz * nz), 0.0, nz], np.float32)


def holed(H, W, seed=0):
    """The relief with the four kinds of invalidity: a rectangular hole (with one isolated valid pixel in it),
    scattered NaN pixels, pixels with n_z below nz_min, and a wall column with a second component behind it."""
    n = relief(H, W, seed)
    rng = np.random.default_rng(seed + 1)
    keep = n[H // 3 + 2, W // 4 + 2].copy()
    n[H // 3:H // 3 + 5, W // 4:W // 4 + 6] = np.nan
    n[H // 3 + 2, W // 4 + 2] = keep                 # valid, no valid neighbour: invalid by the isolated rule
    for _ in range(max(3, H * W // 40)):
        n[rng.integers(H), rng.integers(W)] = np.nan
    for _ in range(max(3, H * W // 60)):
        n[rng.integers(H), rng.integers(W)] = steep()
    n[:, W - 6] = np.nan                             # the wall: columns W−5 .. W−1 are a second component
    n[0, W - 6, :] = (0.0, 0.0, np.inf)              # a non-finite component other than NaN
    return n


@functools.lru_cache(maxsize=None)
def case(name):
    """The shapes of tests/test_gpu_height.py -> a Problem (cached: the eigendecomposition is shared)."""
    if name == "1x1":
        return Problem(relief(1, 1))
    if name == "nan5x5":
        return Problem(np.full((5, 5, 3), np.nan, np.float32))
    if name == "37x41":
        return Problem(holed(37, 41, 3))
    H, W = (int(v) for v in name.split("x"))
    return Problem(relief(H, W, H * 1000 + W))


CASES = ["1x1", "nan5x5", "1x7", "7x1", "2x2", "4x4", "5x4", "37x41", "64x64", "33x130"]
