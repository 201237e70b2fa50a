"""rti.fit_robust / rti_fit_shared_robust on the GPU against the fp64 restatement of its semantics
(tests/robust_ref.py): the intensity window, the m = k and fallback pixels, Huber IRLS, the resident and the
streaming form, dtypes, layouts, channels and the torch op.

Synthetic stacks of P = 549 pixels (two full 256-pixel tiles plus 37 pixels).  Light directions: radius² uniform
in [0.02, 0.8], angle uniform, seeded (cond(A) ≈ 8–19).  Clean stacks are I = A·c_true rounded to fp32 with
c_true drawn so that I stays in about [60, 170].  Every case first checks, on the CPU, the condition under which
a rounding difference cannot flip a decision of the fit (robust_ref.check_inputs).  Coefficients are compared
through conftest.coef_close at the project criterion (1e-4), kept exactly, res at rtol 1e-4 + atol 1e-3."""
import functools

import numpy as np
import pytest
import torch

import rti
from conftest import coef_close
from rti import _lib as L
from robust_ref import check_inputs, fit_robust_ref

pytestmark = pytest.mark.gpu

P0 = 549
STREAM = L.RTI_KERNEL_ONE_LAUNCH


def dirs(N, seed=0):
    rng = np.random.default_rng(1000 + seed)
    r, a = np.sqrt(rng.uniform(0.02, 0.8, N)), rng.uniform(0.0, 2.0 * np.pi, N)
    return (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clean(N, P=P0, basis="ptm", seed=0):
    """(lu, lv, A fp64 [N, k], c_true [P, k], I fp32 [N, P])"""
    lu, lv = dirs(N, seed)
    A = rti.design_matrix(lu, lv, basis)
    rng = np.random.default_rng(2000 + seed)
    c = rng.uniform(-15.0, 15.0, (P, A.shape[1]))
    const = 5 if basis == "ptm" else 0  # the basis' constant term
    c[:, const] = rng.uniform(105.0, 125.0, P) / A[0, const]
    return lu, lv, A, c, (A @ c.T).astype(np.float32)


def bad_mask(N, P, n_bad, seed):
    """exactly n_bad samples of every pixel"""
    return np.random.default_rng(3000 + seed).random((N, P)).argsort(0) < n_bad


@functools.lru_cache(maxsize=None)
def clipped(N, P=P0, basis="ptm", integer=False):
    """Case 1's stack: 30 % of each pixel's samples set to 255 or 0."""
    lu, lv, A, c, I = clean(N, P, basis)
    I = np.rint(I) if integer else I.copy()
    bad = bad_mask(N, P, round(0.3 * N), N)
    high = np.random.default_rng(4000 + N).random((N, P)) < 0.5
    I[bad & high], I[bad & ~high] = 255.0, 0.0
    return lu, lv, A, c, I, N - bad.sum(0)


@functools.lru_cache(maxsize=None)
def noisy(N):
    """Case 4's stack: noise of σ = 1 plus 60 added to N // 10 samples of every pixel."""
    lu, lv, A, c, I = clean(N)
    rng = np.random.default_rng(5000 + N)
    I = I + rng.normal(0.0, 1.0, I.shape).astype(np.float32)
    I[bad_mask(N, P0, N // 10, 7 * N)] += 60.0
    return lu, lv, A, c, I


@functools.lru_cache(maxsize=None)
def ref_clipped(N, P=P0, basis="ptm", integer=False, iters=0):
    lu, lv, A, c, I, good = clipped(N, P, basis, integer)
    r = fit_robust_ref(A, I, 1.0, 254.0, iters=iters, delta=5.0)
    check_inputs(r, I, 1.0, 254.0)
    return r


@functools.lru_cache(maxsize=None)
def ref_noisy(N, iters):
    lu, lv, A, c, I = noisy(N)
    r = fit_robust_ref(A, I, iters=iters, delta=5.0)
    check_inputs(r, I)
    return r


def run(cuda, I, lu, lv, dtype=torch.float32, **kw):
    stats = {}
    out = rti.fit_robust(torch.as_tensor(I, device=cuda).to(dtype), lu, lv, stats=stats, **kw)
    return [t.cpu().numpy() for t in out] + [stats["fallback_px"]]


def check(got, ref):
    coef, res, kept, fallback_px = got
    err, ok = coef_close(coef, ref["coef"])
    assert ok, err
    assert np.array_equal(kept, ref["kept"])
    assert np.allclose(res, ref["res"], rtol=1e-4, atol=1e-3), np.abs(res - ref["res"]).max()
    assert fallback_px == ref["fallback_px"]


def median_err(coef, c_true):
    return float(np.median((np.abs(coef - c_true) / np.abs(c_true).max(-1, keepdims=True)).max(-1)))


@pytest.mark.parametrize("N", [24, 100])
def test_window_recovers_the_truth(cuda, N):
    lu, lv, A, c_true, I, good = clipped(N)
    ref = ref_clipped(N)
    got = run(cuda, I, lu, lv, lo=1, hi=254)
    check(got, ref)
    err, ok = coef_close(got[0], c_true)
    assert ok, err
    assert np.array_equal(got[2], good) and got[3] == 0
    plain = rti.fit(torch.as_tensor(I, device=cuda), lu, lv).cpu().numpy()
    assert median_err(plain, c_true) > 1e-2  # the fit the window replaces: 0.93 at N = 24, 0.41 at N = 100


@pytest.mark.parametrize("N", [24, 100])
def test_no_bounds_no_iterations_is_the_plain_fit(cuda, N):
    lu, lv, A, c_true, I = noisy(N)
    It = torch.as_tensor(I, device=cuda)
    coef, res, kept = (t.cpu().numpy() for t in rti.fit_robust(It, lu, lv))
    c0, r0, _ = (t.cpu().numpy() for t in rti.fit_with_residual(It, lu, lv))
    err, ok = coef_close(coef, c0, rtol=1e-5)
    assert ok, err
    assert np.allclose(res, r0, rtol=1e-5, atol=1e-5), np.abs(res - r0).max()
    assert (kept == N).all()
    check([coef, res, kept, 0], ref_noisy(N, 0))


def test_m_equals_k_and_fallback(cuda):
    N = 7
    lu, lv, A, c_true, I = clean(N)
    I = I.copy()
    I[3, 10] = 255.0  # pixel 10 keeps exactly k = 6 lights
    I[:, 20] = 255.0  # pixel 20 keeps none: every light, the plain fit of the clipped samples
    ref = fit_robust_ref(A, I, 1.0, 254.0)
    check_inputs(ref, I, 1.0, 254.0)
    assert ref["fallback_px"] == 1 and ref["kept"][10] == 6 and ref["kept"][20] == N
    got = run(cuda, I, lu, lv, lo=1, hi=254)
    check(got, ref)
    assert got[2][10] == 6 and got[2][20] == N and got[3] == 1
    plain = rti.fit(torch.as_tensor(I, device=cuda), lu, lv).cpu().numpy()
    err, ok = coef_close(got[0][20], plain[20])
    assert ok, err


@pytest.mark.parametrize("iters", [0, 2])
def test_rank_deficient_window_falls_back(cuda, iters):
    """Lights 6-8 and 9-11 repeat two directions; pixel 300 keeps only those six (m = 6 >= min_lights), an
    exactly rank-2 system: its windowed solve fails at a pivot and the pixel falls back to every light."""
    N = 12
    lu, lv = dirs(N)
    lu[6:9], lv[6:9], lu[9:12], lv[9:12] = lu[6], lv[6], lu[9], lv[9]
    A = rti.design_matrix(lu, lv)
    c = clean(N)[3]
    I = (A @ c.T).astype(np.float32)
    I[:6, 300] = 255.0
    ref = fit_robust_ref(A, I, 1.0, 254.0, iters=iters, delta=5.0)
    check_inputs(ref, I, 1.0, 254.0, rank_fallback=[300])
    assert ref["fallback_px"] == 1 and ref["kept"][300] == N
    got = run(cuda, I, lu, lv, lo=1, hi=254, iters=iters, delta=5.0)
    check(got, ref)
    assert got[3] == 1 and got[2][300] == N


@pytest.mark.parametrize("N", [24, 100])
def test_huber(cuda, N):
    lu, lv, A, c_true, I = noisy(N)
    errs = {}
    for iters in (0, 1, 3):
        got = run(cuda, I, lu, lv, iters=iters, delta=5.0)
        check(got, ref_noisy(N, iters))
        errs[iters] = median_err(got[0], c_true)
    assert errs[3] < 0.5 * errs[0], errs  # fp64 restatement: 0.033 vs 0.23 at N = 24, 0.013 vs 0.107 at N = 100


@pytest.mark.parametrize("N", [24, 100])
def test_streaming_form_agrees_with_auto(cuda, N):
    lib = rti.load()
    assert lib.rti_fit_shared_robust_plan(6, N, L.RTI_F32, 3, 0) == 256
    assert lib.rti_fit_shared_robust_plan(6, N, L.RTI_F32, 3, STREAM) == 0
    lu, lv, A, c_true, I, good = clipped(N)
    lu2, lv2, _, _, I2 = noisy(N)
    for stack, l_u, l_v, kw in ((I, lu, lv, dict(lo=1, hi=254)), (I2, lu2, lv2, dict(iters=3, delta=5.0)),
                                (I, lu, lv, dict(lo=1, hi=254, iters=2, delta=5.0))):
        auto = run(cuda, stack, l_u, l_v, **kw)
        forced = run(cuda, stack, l_u, l_v, kernel=STREAM, **kw)
        assert np.abs(auto[0] - forced[0]).max() <= 1e-6 * np.abs(auto[0]).max()
        assert np.array_equal(auto[2], forced[2]) and auto[3] == forced[3]
        assert np.allclose(auto[1], forced[1], rtol=1e-4, atol=1e-3)
    check(run(cuda, I, lu, lv, lo=1, hi=254, iters=2, delta=5.0, kernel=STREAM), ref_clipped(N, iters=2))


def test_no_tile_fits(cuda):
    N, P = 700, 300
    assert rti.load().rti_fit_shared_robust_plan(6, N, L.RTI_F32, 1, 0) == 0
    lu, lv, A, c_true, I, good = clipped(N, P)
    got = run(cuda, I, lu, lv, lo=1, hi=254, iters=1, delta=5.0)
    check(got, ref_clipped(N, P, iters=1))
    assert np.array_equal(got[2], good)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32])
@pytest.mark.parametrize("iters", [0, 2])
def test_integer_stacks(cuda, dtype, iters):
    lu, lv, A, c_true, I, good = clipped(24, integer=True)
    kw = {} if dtype == torch.uint8 and iters == 0 else dict(lo=1, hi=254)  # uint8 defaults to the 1..254 window
    got = run(cuda, I, lu, lv, dtype=dtype, iters=iters, delta=5.0, **kw)
    check(got, ref_clipped(24, integer=True, iters=iters))
    assert np.array_equal(got[2], good)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_aligned_planes_take_the_vector_loads(cuda, dtype):
    """P = 576: 16-byte aligned planes, two full tiles (16-byte tile loads) and a 64-pixel tail tile."""
    P = 576
    lu, lv, A, c_true, I, good = clipped(24, P, integer=True)
    got = run(cuda, I, lu, lv, dtype=dtype, lo=1, hi=254, iters=2, delta=5.0)
    check(got, ref_clipped(24, P, integer=True, iters=2))


def test_planar_channels_and_single_pixel(cuda):
    lu, lv, A, c_true, I, good = clipped(24)
    ref = ref_clipped(24, iters=2)
    kw = dict(lo=1, hi=254, iters=2, delta=5.0)
    coef, res, kept, fb = run(cuda, I, lu, lv, layout="planar", **kw)
    assert coef.shape == (6, P0)
    check([coef.T, res, kept, fb], ref)
    # C = 3 as [C, N, H, W] with H·W = 549: the stack, its pixel-reversed copy and the stack again
    I4 = np.stack([I, I[:, ::-1], I]).reshape(3, 24, 9, 61)
    coef, res, kept, fb = run(cuda, I4, lu, lv, **kw)
    assert coef.shape == (3, 9, 61, 6) and res.shape == (3, 9, 61) and kept.shape == (3, 9, 61) and kept.dtype == np.int32
    for c, flip in enumerate((False, True, False)):
        cc, rr, kk = coef[c].reshape(P0, 6), res[c].reshape(P0), kept[c].reshape(P0)
        if flip:
            cc, rr, kk = cc[::-1], rr[::-1], kk[::-1]
        check([cc, rr, kk, 0], ref)
    one = run(cuda, I[:, 5:6], lu, lv, **kw)
    check([one[0], one[1], one[2], 0], {k: (v[5:6] if isinstance(v, np.ndarray) else 0) for k, v in ref.items()})


@pytest.mark.parametrize("iters", [0, 2])
def test_hsh9(cuda, iters):
    lu, lv, A, c_true, I, good = clipped(24, basis="hsh9")
    got = run(cuda, I, lu, lv, basis="hsh9", lo=1, hi=254, iters=iters, delta=5.0)
    check(got, ref_clipped(24, basis="hsh9", iters=iters))
    assert got[0].shape == (P0, 9)
    if iters == 0:
        err, ok = coef_close(got[0], c_true)
        assert ok, err


def test_arguments_raise(cuda):
    lu, lv, A, c_true, I = clean(24)
    It = torch.as_tensor(I, device=cuda)
    with pytest.raises(ValueError):
        rti.fit_robust(It, lu, lv, lo=200, hi=100)
    with pytest.raises(ValueError):
        rti.fit_robust(It, lu, lv, iters=2)  # no delta
    with pytest.raises(ValueError):
        rti.fit_robust(It, lu, lv, min_lights=25)
    with pytest.raises(NotImplementedError):
        rti.fit_robust(It, lu, lv, basis="hsh")
    with pytest.raises(ValueError, match="CUDA"):
        rti.fit_robust(torch.as_tensor(I), lu, lv)


@pytest.mark.parametrize("planar", [False, True])
def test_torch_op_fit_robust(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    lu, lv, A, c_true, I, good = clipped(24)
    It = torch.as_tensor(I, device=cuda)
    Ad = torch.as_tensor(A, device=cuda)
    coef, res, kept, fb = torch.ops.rti.fit_robust(Ad, It, 1.0, 254.0, 6, 2, 5.0, planar)
    stats = {}
    c2, r2, k2 = rti.fit_robust(It, lu, lv, lo=1, hi=254, iters=2, delta=5.0, layout="planar" if planar else "pixel",
                                stats=stats)
    assert torch.equal(coef, c2) and torch.equal(res, r2) and torch.equal(kept, k2)
    assert fb.dtype == torch.int32 and fb.shape == (1,) and int(fb) == stats["fallback_px"] == 0
    I3 = torch.stack([It, It.flip(1)])
    coef3, res3, kept3, _ = torch.ops.rti.fit_robust(Ad, I3, 1.0, 254.0, 6, 2, 5.0, planar)
    assert torch.equal(coef3[0], coef) and torch.equal(res3[0], res) and torch.equal(kept3[0], kept)
    torch.library.opcheck(torch.ops.rti.fit_robust.default, (Ad, I3, 1.0, 254.0, 6, 2, 5.0, planar, 0),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.rti.fit_robust.default, (Ad, It, -float("inf"), float("inf"), 6, 0, 0.0, planar, 0),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.fit_robust(Ad.float(), It, 1.0, 254.0, 6, 2, 5.0, planar)
