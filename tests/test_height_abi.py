"""rti_height_* without a GPU: the symbols are bound, every argument check answers before any HIP call (the pointers
below are never dereferenced) with a message that names the function, the host queries follow their rules, and the
NumPy restatement (tests/height_ref.py) has the properties the GPU tests lean on: it integrates a quadratic surface
exactly, its hierarchy is the Galerkin one, and its V-cycle is a symmetric positive operator."""
import ctypes

import numpy as np
import pytest

import height_ref as hr
import rti
from rti import _lib as L

NRM, WS, OUT = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 40)  # far apart, aligned
NAN, INF = float("nan"), float("inf")
ENTRY = b"rti_height_from_normals"


def height_call(n=NRM, nl=0, H=16, W=16, nz_min=0.1, flip_y=0, z0=None, rtol=1e-6, max_iters=100, check_every=8,
                precond=0, ws=WS, height=OUT, valid=None, stats=None):
    return rti.load().rti_height_from_normals(n, nl, H, W, nz_min, flip_y, z0, rtol, max_iters, check_every, precond,
                                              ws, height, valid, stats, None)


def test_symbols_and_constants():
    lib = rti.load()
    for name in ("rti_height_levels", "rti_height_workspace_bytes", "rti_height_from_normals"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert (L.RTI_HEIGHT_MULTIGRID, L.RTI_HEIGHT_JACOBI) == (0, 1)
    for fn in ("height_from_normals", "height_from_normals_into", "height_workspace", "height_levels"):
        assert callable(getattr(rti, fn)) and getattr(rti.api, fn) is getattr(rti, fn)
    assert rti.api.HEIGHT_PRECONDS == {"multigrid": 0, "jacobi": 1}


BAD = {
    "null normals": dict(n=None), "null workspace": dict(ws=None), "null height": dict(height=None),
    "H = 0": dict(H=0), "W = 0": dict(W=0), "H < 0": dict(H=-3), "W < 0": dict(W=-1),
    "H*W = 2^31": dict(H=1 << 16, W=1 << 15), "H*W > 2^31": dict(H=1 << 20, W=1 << 20),
    "layout 2": dict(nl=2), "layout -1": dict(nl=-1), "precond 2": dict(precond=2), "precond -1": dict(precond=-1),
    "nz_min 0": dict(nz_min=0.0), "nz_min < 0": dict(nz_min=-0.5), "nz_min > 1": dict(nz_min=1.0000001),
    "nz_min NaN": dict(nz_min=NAN), "nz_min inf": dict(nz_min=INF),
    "rtol NaN": dict(rtol=NAN), "rtol inf": dict(rtol=INF), "rtol < 0": dict(rtol=-1e-9),
    "max_iters < 0": dict(max_iters=-1), "max_iters 100001": dict(max_iters=100001),
    "check_every 0": dict(check_every=0), "check_every 1025": dict(check_every=1025), "check_every < 0": dict(check_every=-8),
    "workspace off 256": dict(ws=ctypes.c_void_p((1 << 30) + 128)), "workspace off 8": dict(ws=ctypes.c_void_p((1 << 30) + 8)),
    "in place": dict(height=NRM), "height inside normals": dict(height=ctypes.c_void_p((1 << 20) + 16 * 16 * 12 - 4)),
    "normals inside height": dict(n=ctypes.c_void_p((1 << 40) + 16 * 16 * 4 - 4)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments(case):
    assert height_call(**BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert ENTRY in rti.load().rti_last_error()


def test_limits_are_inclusive_where_stated():
    """nz_min = 1, rtol = 0, max_iters = 0 / 100000 and check_every = 1 / 1024 are inside: the next check (the
    misaligned workspace, placed last on purpose) is the one that answers."""
    off = ctypes.c_void_p((1 << 30) + 64)
    for kw in (dict(nz_min=1.0), dict(rtol=0.0), dict(max_iters=0), dict(max_iters=100000), dict(check_every=1),
               dict(check_every=1024), dict(precond=1), dict(nl=1), dict(H=1, W=1)):
        assert height_call(ws=off, **kw) == L.RTI_ERR_BAD_ARG
        assert b"workspace" in rti.load().rti_last_error(), kw


@pytest.mark.parametrize("H,W", [(1, 1), (4, 4), (5, 4), (37, 41), (3840, 2160), (1, 9), (4, 5), (8, 8), (9, 8)])
def test_levels_follow_the_rule(H, W):
    assert rti.load().rti_height_levels(H, W) == hr.levels(H, W) == rti.height_levels(H, W)


def test_levels_at_the_named_sizes():
    lib = rti.load()
    assert [lib.rti_height_levels(*s) for s in ((1, 1), (4, 4), (5, 4), (37, 41), (3840, 2160))] == [1, 1, 2, 5, 11]
    for H, W in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
        assert lib.rti_height_levels(H, W) == -1
        with pytest.raises(ValueError):
            rti.height_levels(H, W)


def test_workspace_bytes():
    """Monotone in H·W (equal products give equal sizes whatever the aspect), 0 on bad sizes or preconditioner, the
    multigrid workspace above the Jacobi one, and enough for the vectors the solver names."""
    lib = rti.load()
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (4, 4), (5, 3), (1, 16), (5, 4), (37, 41), (41, 37), (1, 1517), (64, 64),
              (33, 130), (1080, 1920), (2160, 3840), (1, (1 << 31) - 1)]
    for pc in (L.RTI_HEIGHT_MULTIGRID, L.RTI_HEIGHT_JACOBI):
        sizes = sorted((H * W, lib.rti_height_workspace_bytes(H, W, pc)) for H, W in shapes)
        assert all(b > 0 and b % 256 == 0 for _, b in sizes)
        for (p0, b0), (p1, b1) in zip(sizes, sizes[1:]):
            assert b0 <= b1 and (p0 != p1 or b0 == b1), (p0, b0, p1, b1)
        for H, W in ((0, 4), (4, 0), (-2, 4), (1 << 16, 1 << 15)):
            assert lib.rti_height_workspace_bytes(H, W, pc) == 0
    for H, W in shapes:
        mg, ja = (lib.rti_height_workspace_bytes(H, W, pc) for pc in (0, 1))
        assert mg > ja >= H * W * (6 * 8 + 3 * 4)  # z, r, p, Ap, M⁻¹r, b in fp64; two weights and the degree
    assert lib.rti_height_workspace_bytes(8, 8, 2) == 0 and lib.rti_height_workspace_bytes(8, 8, -1) == 0


def test_python_layer_rejects_what_it_cannot_launch():
    import torch

    with pytest.raises(ValueError, match="CUDA"):
        rti.height_from_normals(torch.zeros((8, 8, 3)))
    with pytest.raises(ValueError, match="float32"):
        rti.height_from_normals(torch.zeros((8, 8, 3), dtype=torch.float64))
    for shape, layout in (((8, 8, 4), "pixel"), ((8, 8, 3), "planar"), ((8, 8), "pixel")):
        with pytest.raises(ValueError, match="normal map"):
            rti.height_from_normals(torch.zeros(shape), layout=layout)
    with pytest.raises(ValueError, match="layout"):
        rti.height_from_normals(torch.zeros((8, 8, 3)), layout="rows")
    with pytest.raises(ValueError, match="preconditioner"):
        rti.height_workspace(8, 8, "ilu", "cpu")
    with pytest.raises(ValueError):
        rti.height_workspace(0, 8, "jacobi", "cpu")
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    with pytest.raises(ValueError, match="CUDA"):
        torch.ops.rti.height_from_normals(torch.zeros((8, 8, 3)))


# ---- the reference itself ------------------------------------------------------------------------------------------

def quadratic_normals(H, W, a, b, c, d, e):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = a * x * x + b * x * y + c * y * y + d * x + e * y
    zx, zy = 2 * a * x + b * y + d, b * x + 2 * c * y + e
    exact = np.stack([-zx, -zy, np.ones_like(zx)], -1)
    exact /= np.linalg.norm(exact, axis=-1, keepdims=True)
    return z, exact, exact.astype(np.float32)


def test_reference_is_exact_on_a_quadratic_surface():
    """z = ax² + bxy + cy² + dx + ey with analytic normals rounded to fp32, two components and a hole: the midpoint
    functional is exact for quadratics, so with the exact fp64 normals the solution is the surface up to a constant
    per component, and with the fp32 ones it moves by at most ‖A⁺‖·‖Δb‖ = ‖Δb‖₂/λ₂ in the 2-norm, hence per
    pixel.  Δb is formed here from the two right-hand sides; λ₂ from eigvalsh of the test's Laplacian."""
    H, W = 13, 17
    z, exact, n32 = quadratic_normals(H, W, 0.004, -0.003, 0.005, 0.11, -0.07)
    hole = np.zeros((H, W), bool)
    hole[4:7, 3:6] = True
    hole[:, 11] = True  # a wall: two components
    n32[hole] = np.nan
    pr = hr.Problem(n32)
    assert pr.labels.max() == 2 and np.array_equal(pr.valid, ~hole)
    lam = np.linalg.eigvalsh(pr.A)
    lam2 = lam[lam > 1e-9][0]
    assert abs(lam2 - pr.lambda2) <= 1e-12
    # b of the exact (fp64) normals on the same graph
    p64 = np.where(pr.valid, -exact[..., 0] / exact[..., 2], 0.0)
    q64 = np.where(pr.valid, -exact[..., 1] / exact[..., 2], 0.0)
    b64 = hr.rhs(p64, q64, pr.wR, pr.wD)
    V = np.linalg.eigh(pr.A)
    keep = V[0] > 1e-9
    z64 = (V[1][:, keep] @ ((V[1][:, keep].T @ b64.ravel()) / V[0][keep])).reshape(H, W)
    for cmp in (1, 2):
        m = pr.labels == cmp
        d = (z64[m] - z[m]) - (z64[m] - z[m]).mean()
        assert np.abs(d).max() <= 1e-11 * np.abs(z).max(), "the functional is not exact on a quadratic"
    db = float(np.linalg.norm(pr.b - b64))
    assert 0.0 < db <= 2.0 ** -22 * 4 * np.sqrt(H * W)  # fp32 rounding of the normals, not something larger
    bound = db / lam2 + 1e-11 * np.abs(z).max()
    got = pr.align(np.where(pr.valid, pr.z, 0.0))
    for cmp in (1, 2):
        m = pr.labels == cmp
        d = (got[m] - z[m]) - (got[m] - z[m]).mean()
        assert np.abs(d).max() <= bound, (cmp, np.abs(d).max(), bound)


def test_mask_rules():
    n = np.zeros((5, 6, 3), np.float32)
    n[..., 2] = 1.0
    n[0, 0] = NAN
    n[1, 1] = (0.0, INF, 1.0)
    n[2, 2] = hr.steep()               # n_z = 0.05 < 0.1
    n[4, 5] = (0.0, 0.0, 0.0)          # a kind-1 edge normal
    n[3, 0] = (0.6, 0.0, 0.8)
    n[[2, 4, 3], [0, 0, 1]] = NAN      # (3, 0) keeps no valid neighbour
    m = hr.mask(n)
    assert not m[0, 0] and not m[1, 1] and not m[2, 2] and not m[4, 5] and not m[3, 0]
    assert not m[1, 0] and not m[2, 1]  # these two lost their last valid neighbour as well
    assert m.sum() == 30 - 10
    assert hr.mask(n, 0.04)[2, 2]
    assert np.array_equal(hr.Problem(n).valid, m)
    assert not hr.mask(np.ones((1, 1, 3), np.float32)).any()  # a single pixel has no neighbour


def test_rhs_sums_to_zero_and_flip_y():
    pr, fl = hr.Problem(hr.holed(9, 11, 5)), hr.Problem(hr.holed(9, 11, 5), flip_y=True)
    for c in range(1, int(pr.labels.max()) + 1):
        assert abs(pr.b[pr.labels == c].sum()) <= 1e-13
    neg = hr.holed(9, 11, 5)
    neg[..., 1] = -neg[..., 1]
    assert np.array_equal(hr.Problem(neg).b, fl.b) and not np.array_equal(pr.b, fl.b)
    assert np.abs(pr.A @ np.where(pr.valid, pr.z, 0.0).ravel() - pr.b.ravel()).max() <= 1e-12


def test_hierarchy_is_galerkin():
    """9×11 with holes: PᵀAP equals the summed-weight Laplacian on every level, and the level count is the rule's."""
    pr = hr.Problem(hr.holed(9, 11, 5))
    assert not pr.valid.all() and pr.labels.max() >= 2
    lv = hr.hierarchy(pr.wR, pr.wD)
    assert len(lv) == hr.levels(9, 11) == 3
    assert [l[0].shape for l in lv] == [(9, 11), (5, 6), (3, 3)]
    for l in range(len(lv) - 1):
        A, P = hr.laplacian(*lv[l]), hr.prolongation(*lv[l])
        assert np.array_equal(P.T @ A @ P, hr.laplacian(*lv[l + 1])), l  # integers: exact


def test_vcycle_is_symmetric_and_positive():
    """The V-cycle matrix at 9×11 with holes: symmetric to rounding, and positive on the complement of the null
    space (the range of A), where PCG works."""
    pr = hr.Problem(hr.holed(9, 11, 5))
    M = hr.vcycle_matrix(pr.wR, pr.wD)
    assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max()
    lam, V = np.linalg.eigh(pr.A)
    Q = V[:, lam > 1e-9]
    assert Q.shape[1] == pr.valid.sum() - pr.labels.max()
    ev = np.linalg.eigvalsh(Q.T @ (0.5 * (M + M.T)) @ Q)
    assert ev.min() > 1e-3, ev.min()
    assert not M[~pr.valid.ravel()].any() and not M[:, ~pr.valid.ravel()].any()  # degree 0: a zero correction
    z, k, met = hr.pcg(pr.A, pr.b.ravel(), lambda r: M @ r, 1e-10, 100)
    assert met and k <= 40
    assert np.abs(pr.align(z.reshape(9, 11)) - pr.z)[pr.valid].max() <= 1e-10 * pr.norm_b / pr.lambda2 + 1e-13
