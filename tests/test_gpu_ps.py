"""rti.photometric_stereo / rti_photometric_stereo on the GPU against the fp64 restatement of its semantics
(tests/ps_ref.py) on the synthetic Lambertian scene: 24 lights on a golden-angle spiral, tilt 0..60°, albedo 150..400,
samples clipped to [0, 255] (attached shadow at 0, highlights at 255), window 0.5..254.5.

Every case first checks, on the CPU, the conditions under which a rounding difference cannot flip a decision of the
fit or a kind (ps_ref.check_ps_inputs).  Tolerances, from the project's criterion (coefficients to 1e-4 of the
pixel's largest, conftest.coef_close):
  g_c ≈ albedo_c·n recombined   coef_close at 1e-4, as test_gpu_robust.py holds its coefficients
  normal                        angle <= 0.01° (sin θ <= ‖Δg‖/‖g‖ <= √3·1e-4 = 0.0099°), |‖n‖ − 1| <= 2⁻²² (three
                                fp32 roundings of 2⁻²⁴ relative each)
  albedo                        4e-4·‖g_c‖: √3·1e-4 from g_c plus the same from n, for channels that share a normal
  res                           rtol 1e-4 + atol 1e-3;  kept, kind, fallback_px exact."""
import functools

import numpy as np
import pytest
import torch

import rti
from conftest import coef_close, relight_close
from ps_ref import FP32_MARGIN, check_ps_inputs, ps_ref, scene
from rti import _lib as L

pytestmark = pytest.mark.gpu

STREAM = L.RTI_KERNEL_ONE_LAUNCH
LO, HI = 0.5, 254.5
DTYPES = {"f32": torch.float32, "u8": torch.uint8, "i32": torch.int32}


@functools.lru_cache(maxsize=None)
def stack(P, C, N=24, integer=False):
    lu, lv, A, n_true, alb_true, I = scene(P, N, rgb=C == 3)
    return lu, lv, A, (np.rint(I) if integer else I)


@functools.lru_cache(maxsize=None)
def reference(P, C, iters, N=24, integer=False, margin=1e-3):
    lu, lv, A, I = stack(P, C, N, integer)
    # an integer stack's window 1..254 keeps the samples 0.5..254.5 keeps: the bounds the conditions are checked at
    lo, hi = (1.0, 254.0) if integer else (LO, HI)
    ref = ps_ref(A, I, lo, hi, 3, iters, 5.0)
    check_ps_inputs(ref, I, LO, HI, margin=margin)
    return ref


def run(cuda, I, lu, lv, dtype=torch.float32, **kw):
    """rti.photometric_stereo on [N, P] or, as [3, N, 1, P], on an RGB stack [3, N, P] -> normals [P, 3] (or [3, P]),
    albedo [P] or [P, 3], kind [P], res and kept [P] or [3, P] on the host, and fallback_px"""
    stats = {}
    It = torch.as_tensor(I, device=cuda).to(dtype)
    P = It.shape[-1]
    out = rti.photometric_stereo(It.unsqueeze(2) if It.dim() == 3 else It, lu, lv, return_kind=True, return_res=True,
                                 return_kept=True, stats=stats, **kw)
    n, albedo, kind, res, kept = (t.cpu().numpy() for t in out)
    if It.dim() == 3:
        n = n.reshape((3, P) if kw.get("normal_layout") == "planar" else (P, 3))
        albedo, kind, res, kept = albedo.reshape(P, 3), kind.reshape(P), res.reshape(3, P), kept.reshape(3, P)
    return [n, albedo, kind, res, kept, stats["fallback_px"]]


def check(got, ref, planar=False):
    """got: normals [P, 3] ([3, P] if planar), albedo [P] or [P, 3], kind [P], res and kept [P] or [3, P], count"""
    n, albedo, kind, res, kept, fallback_px = got
    n = n.T if planar else n
    P = n.shape[0]
    albedo = albedo.reshape(P, -1).T.astype(np.float64)  # [C, P]
    res, kept = res.reshape(-1, P), kept.reshape(-1, P)
    assert np.array_equal(kind, ref["kind"]), np.flatnonzero(kind != ref["kind"])
    assert np.array_equal(kept, ref["kept"])
    assert fallback_px == ref["fallback_px"]
    assert np.allclose(res, ref["res"], rtol=1e-4, atol=1e-3, equal_nan=True), np.nanmax(np.abs(res - ref["res"]))
    bad, flat = ref["kind"] == 4, ref["kind"] == 2
    assert np.isnan(n[bad]).all() and np.isnan(albedo[:, bad]).all()
    assert (n[flat] == (0.0, 0.0, 1.0)).all()
    ok = ~bad
    n64 = n[ok].astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1.0).max(initial=0.0) <= 2.0 ** -22
    fitted = ok & ~flat
    chord = np.linalg.norm(n[fitted] - ref["normals"][fitted], axis=-1)
    angle = np.degrees(2.0 * np.arcsin(0.5 * chord))
    assert angle.max(initial=0.0) <= 0.01, angle.max()
    for c in range(albedo.shape[0]):
        assert (np.abs(albedo[c][ok] - ref["albedo"][c][ok]) <= 4e-4 * np.linalg.norm(ref["g"][c][ok], axis=1)).all()
        # recombined: albedo_c·n is the channel's fitted vector (its part along the shared normal for RGB)
        err, close = coef_close(albedo[c][fitted, None] * n[fitted].astype(np.float64),
                                ref["albedo"][c][fitted, None] * ref["normals"][fitted])
        assert close, err


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("P", [1, 255, 260, 1027])
def test_against_reference(cuda, P, C, iters):
    """P: a lone pixel, a partial unaligned tile, a full tile plus a tail, odd with several tiles."""
    lu, lv, A, I = stack(P, C)
    ref = reference(P, C, iters)
    kw = dict(lo=LO, hi=HI, iters=iters, delta=5.0)
    got = run(cuda, I, lu, lv, **kw)
    assert got[0].shape == (P, 3) and got[1].shape == ((P, 3) if C == 3 else (P,)) and got[2].shape == (P,)
    assert got[3].shape == got[4].shape == ((3, P) if C == 3 else (P,)) and got[4].dtype == np.int32
    check(got, ref)
    planar = run(cuda, I, lu, lv, normal_layout="planar", **kw)
    assert planar[0].shape == (3, P) and np.array_equal(planar[0].T, got[0], equal_nan=True)
    check(planar, ref, planar=True)


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("dtype", ["u8", "i32"])
def test_integer_stacks(cuda, dtype, C, iters):
    """The scene rounded, window 1..254: a uint8 stack given neither bound uses it by default."""
    P = 260
    lu, lv, A, I = stack(P, C, integer=True)
    kw = {} if dtype == "u8" else dict(lo=1, hi=254)
    check(run(cuda, I, lu, lv, dtype=DTYPES[dtype], iters=iters, delta=5.0, **kw), reference(P, C, iters, integer=True))


def into(cuda, A, I3, *, iters, kernel=0, pad=0, weights=None, planar=False, lo=LO, hi=HI, dtype=torch.float32):
    """The _into entry on a [C, N, P] stack, optionally a view of planes padded by `pad` elements -> the device
    tensors (normals, albedo, kind, res, kept, fallback)."""
    C, N, P = I3.shape
    buf = torch.full((C, N, P + pad), 7.0, device=cuda).to(dtype)
    buf[:, :, :P] = torch.as_tensor(I3, device=cuda).to(dtype)
    view = buf[:, :, :P]
    outs = (torch.empty((3, P) if planar else (P, 3), device=cuda), torch.empty((C, P), device=cuda),
            torch.empty(P, dtype=torch.uint8, device=cuda), torch.empty((C, P), device=cuda),
            torch.empty((C, P), dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda))
    rti.photometric_stereo_into(torch.as_tensor(A, device=cuda), view if pad else view.contiguous(), *outs, lo=lo,
                                hi=hi, min_lights=3, iters=iters, delta=5.0, weights=weights, kernel=kernel,
                                normal_layout="planar" if planar else "pixel",
                                light_stride=P + pad if pad else None)
    return outs


def as_got(outs, C):
    n, albedo, kind, res, kept, fb = (t.cpu().numpy() for t in outs)
    return [n, albedo.T if C == 3 else albedo[0], kind, res if C == 3 else res[0], kept if C == 3 else kept[0], int(fb[0])]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("C", [1, 3])
def test_padded_light_stride(cuda, C, iters):
    """Planes of P + 4 elements (and channels of N such planes) through the _into entry: no 16-byte plane loads at
    P = 255, and the padding is never read as a pixel."""
    for P in (255, 260):
        lu, lv, A, I = stack(P, C)
        outs = into(cuda, A, I.reshape(C, 24, P), iters=iters, pad=4)
        check(as_got(outs, C), reference(P, C, iters))
        assert same_bits(outs, into(cuda, A, I.reshape(C, 24, P), iters=iters))


@pytest.mark.parametrize("N,tp", [(54, 128), (107, 64), (214, 0), (3, 256)])
def test_tile_sizes_and_forms_agree(cuda, N, tp):
    """C = 3 fp32 at P = 300: every resident tile size, no tile at all, and the minimum of three lights; the
    resident form and RTI_KERNEL_ONE_LAUNCH give identical bits in every output.  At N = 54, 214 and 3 a sample of
    this scene lies 3e-4 to 9e-4 from a bound: those cases state ps_ref.FP32_MARGIN."""
    P, C = 300, 3
    assert rti.load().rti_photometric_stereo_plan(N, L.RTI_F32, C, 2, 0) == tp
    assert rti.load().rti_photometric_stereo_plan(N, L.RTI_F32, C, 2, STREAM) == 0
    lu, lv, A, I = stack(P, C, N)
    ref = reference(P, C, 2, N, margin=1e-3 if N == 107 else FP32_MARGIN)
    auto = into(cuda, A, I, iters=2)
    check(as_got(auto, C), ref)
    assert same_bits(auto, into(cuda, A, I, iters=2, kernel=STREAM))
    assert same_bits(auto, into(cuda, A, I, iters=2, pad=1))  # planes off 16 bytes: the tile copied by elements


@pytest.mark.parametrize("dtype,C,tp", [("f32", 1, 256), ("u8", 1, 256), ("u8", 3, 256), ("i32", 3, 256)])
def test_forms_agree_at_the_full_tile(cuda, dtype, C, tp):
    """N = 24: TP = 256 in every dtype; P = 1027 has full tiles (16-byte tile loads) and a tail tile."""
    P = 1027 if dtype == "f32" else 260
    integer = dtype != "f32"
    assert rti.load().rti_photometric_stereo_plan(24, getattr(L, "RTI_" + dtype.upper()), C, 2, 0) == tp
    lu, lv, A, I = stack(P, C, integer=integer)
    kw = dict(iters=2, dtype=DTYPES[dtype], lo=1.0 if integer else LO, hi=254.0 if integer else HI)
    auto = into(cuda, A, I.reshape(C, 24, P), **kw)
    check(as_got(auto, C), reference(P, C, 2, integer=integer))
    assert same_bits(auto, into(cuda, A, I.reshape(C, 24, P), kernel=STREAM, **kw))


@pytest.mark.parametrize("iters", [0, 2])
def test_kinds_and_fallbacks(cuda, iters):
    P = 260
    lu, lv, A, I = stack(P, 1)
    I = I.copy()
    I[:, 10] = 0.0                                  # no sample in the window: every light, g = 0 -> kind 2
    I[:22, 20] = np.nan                             # two finite samples: falls back, and the NaN reach g -> kind 4
    I[:, 30] = np.where(np.arange(24) < 2, 100.0 + np.arange(24), 255.0)  # two samples inside the window
    ref = ps_ref(A, I, LO, HI, 3, iters, 5.0)
    check_ps_inputs(ref, I, LO, HI)
    assert ref["fallback_px"] == 3 and list(ref["kind"][[10, 20, 30]]) == [2, 4, 0]
    assert list(ref["kept"][0][[10, 20, 30]]) == [24, 24, 24]
    got = run(cuda, I, lu, lv, lo=LO, hi=HI, iters=iters, delta=5.0)
    check(got, ref)
    n, albedo, kind, res, kept, fb = got
    assert fb == 3 and list(kind[[10, 20, 30]]) == [2, 4, 0] and list(kept[[10, 20, 30]]) == [24, 24, 24]
    assert tuple(n[10]) == (0.0, 0.0, 1.0) and albedo[10] == 0.0 and res[10] == 0.0
    assert np.isnan(n[20]).all() and np.isnan(albedo[20])
    # a signed stack of a surface turned away (n_z < 0), nothing clipped and no window: the normal as fitted
    n_back = np.array([[0.3, -0.2, -np.sqrt(1 - 0.13)], [0.0, 0.0, -1.0], [0.6, 0.0, 0.8]])
    Ib = (200.0 * (A @ n_back.T)).astype(np.float32)
    refb = ps_ref(A, Ib, iters=iters, delta=5.0)
    check_ps_inputs(refb, Ib)
    assert list(refb["kind"]) == [1, 1, 0]
    gotb = run(cuda, Ib, lu, lv, iters=iters, delta=5.0)
    check(gotb, refb)
    assert list(gotb[2]) == [1, 1, 0] and gotb[5] == 0 and (gotb[0][:2, 2] < 0).all()
    assert np.abs(gotb[0] - n_back).max() <= 1e-6 and np.abs(gotb[1] - 200.0).max() <= 1e-3


@pytest.mark.parametrize("iters", [0, 2])
def test_rgb_shares_one_normal(cuda, iters):
    P = 260
    lu, lv, A, I = stack(P, 3)
    grey = into(cuda, A, I[:1], iters=iters)
    red = into(cuda, A, I, iters=iters, weights=(1.0, 0.0, 0.0))
    assert torch.equal(red[0], grey[0]) and torch.equal(red[1][0], grey[1][0]) and torch.equal(red[2], grey[2])
    assert torch.equal(red[3][0], grey[3][0]) and torch.equal(red[4][0], grey[4][0])
    same = into(cuda, A, np.stack([I[1]] * 3), iters=iters)
    assert torch.equal(same[1][0], same[1][1]) and torch.equal(same[1][0], same[1][2])
    assert torch.equal(same[3][0], same[3][2]) and torch.equal(same[4][0], same[4][1])
    ref = ps_ref(A, I, LO, HI, 3, iters, 5.0, weights=(0.2, 0.3, 0.5))
    check_ps_inputs(ref, I, LO, HI)
    check(as_got(into(cuda, A, I, iters=iters, weights=(0.2, 0.3, 0.5)), 3), ref)


def test_shaded_normals_reproduce_the_samples(cuda):
    """End to end: the normals and albedo render, through rti.shade_normals at light i, every unclipped and
    unshadowed sample of plane i."""
    H, W = 20, 13
    lu, lv, A, I = stack(H * W, 1)
    n, albedo = rti.photometric_stereo(torch.as_tensor(I.reshape(24, H, W), device=cuda), lu, lv, lo=LO, hi=HI)
    assert n.shape == (H, W, 3) and albedo.shape == (H, W)
    for i in range(24):
        img = rti.shade_normals(n, float(lu[i]), float(lv[i]), albedo=albedo).cpu().numpy().reshape(-1)
        inside = (I[i] > LO) & (I[i] < HI)
        assert inside.any()
        err, ok = relight_close(img[inside], I[i][inside])
        assert ok, (i, err)


def test_shapes_and_arguments(cuda):
    H, W = 20, 13
    lu, lv, A, I = stack(H * W, 3)
    It = torch.as_tensor(I.reshape(3, 24, H, W), device=cuda)
    n, albedo, kind, res, kept = rti.photometric_stereo(It, lu, lv, lo=LO, hi=HI, normal_layout="planar",
                                                        return_kind=True, return_res=True, return_kept=True)
    assert n.shape == (3, H, W) and albedo.shape == (H, W, 3) and albedo.is_contiguous() and kind.shape == (H, W)
    assert res.shape == kept.shape == (3, H, W) and kind.dtype == torch.uint8 and kept.dtype == torch.int32
    nz, az = rti.photometric_stereo(It[0], lu, lv, A[:, 2], lo=LO, hi=HI)  # a measured third component
    assert torch.equal(nz, rti.photometric_stereo(It[0], lu, lv, lo=LO, hi=HI)[0])
    with pytest.raises(ValueError):
        rti.photometric_stereo(It[0], lu, lv, lo=200, hi=100)
    with pytest.raises(ValueError):
        rti.photometric_stereo(It[0], lu, lv, iters=2)  # no delta
    with pytest.raises(ValueError):
        rti.photometric_stereo(It[0], lu, lv, min_lights=25)
    with pytest.raises(ValueError):
        rti.photometric_stereo(It[:2], lu, lv)  # two channels
    with pytest.raises(ValueError):
        rti.photometric_stereo(It[0], lu[:5], lv[:5])
    with pytest.raises(ValueError, match="CUDA"):
        rti.photometric_stereo(torch.as_tensor(I[0]), lu, lv)


@pytest.mark.parametrize("planar", [False, True])
def test_torch_op(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P = 260
    lu, lv, A, I = stack(P, 3)
    It, Ad = torch.as_tensor(I, device=cuda), torch.as_tensor(A, device=cuda)
    nl = "planar" if planar else "pixel"
    for stack_t in (It, It[0]):
        n, albedo, kind, res, kept, fb = torch.ops.rti.photometric_stereo(Ad, stack_t, LO, HI, 3, 2, 5.0, None, planar)
        stats = {}
        I4 = stack_t.reshape(3, 24, 1, P) if stack_t.dim() == 3 else stack_t
        n2, a2, k2, r2, m2 = rti.photometric_stereo(I4, lu, lv, lo=LO, hi=HI, iters=2, delta=5.0, normal_layout=nl,
                                                    return_kind=True, return_res=True, return_kept=True, stats=stats)
        if stack_t.dim() == 3:
            n2, a2, k2 = n2.reshape(n.shape), a2.reshape(P, 3).T, k2.reshape(P)
            r2, m2 = r2.reshape(3, P), m2.reshape(3, P)
        assert torch.equal(n, n2) and torch.equal(albedo, a2) and torch.equal(kind, k2)
        assert torch.equal(res, r2) and torch.equal(kept, m2)
        assert fb.dtype == torch.int32 and fb.shape == (1,) and int(fb) == stats["fallback_px"]
    torch.library.opcheck(torch.ops.rti.photometric_stereo.default, (Ad, It, LO, HI, 3, 2, 5.0, [0.2, 0.3, 0.5], planar, 0),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.rti.photometric_stereo.default,
                          (Ad, It[0], -float("inf"), float("inf"), 3, 0, 0.0, None, planar, 0),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.photometric_stereo(Ad.float(), It, LO, HI, 3, 2, 5.0, None, planar)


def test_graph_capture_replays_the_launch(cuda):
    P, C = 260, 3
    lu, lv, A, I = stack(P, C)
    Ad = torch.as_tensor(A, device=cuda)
    Id = torch.as_tensor(I[:, :, ::-1].copy(), device=cuda)
    outs = (torch.empty((P, 3), device=cuda), torch.empty((C, P), device=cuda),
            torch.empty(P, dtype=torch.uint8, device=cuda), torch.empty((C, P), device=cuda),
            torch.empty((C, P), dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda))

    def call():
        rti.photometric_stereo_into(Ad, Id, *outs, lo=LO, hi=HI, min_lights=3, iters=2, delta=5.0)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        call()  # loads the kernel before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    Id.copy_(torch.as_tensor(I, device=cuda))
    outs[5].zero_()
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = [t.clone() for t in outs]
    assert same_bits(replayed, into(cuda, A, I, iters=2)) and bool(replayed[1].any())
    check(as_got(replayed, C), reference(P, C, 2))
