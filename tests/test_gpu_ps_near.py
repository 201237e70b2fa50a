"""rti.photometric_stereo_near / rti_photometric_stereo_near on the GPU against the fp64 restatement of its semantics
(tests/ps_near_ref.py) on the near-light scene: lights at 2·W from the image centre, a Gaussian bump, albedo 150..400,
inverse-square fall-off, samples clipped to [0, 255], window 0.5..254.5, origin (3.5, −2.25).

Every case first checks, on the CPU, the conditions under which a rounding difference cannot flip a decision of the
fit or a kind (ps_near_ref.check_ps_near_inputs).  The tolerances are test_gpu_ps.py's, through its own check(): they
derive from the project's 1e-4 coefficient criterion, and the rows add only fp64 roundings (at most 8 ulps a
component, include/rti.h) to a design the far entry reads as given."""
import functools

import numpy as np
import pytest
import torch

import rti
from ps_near_ref import check_ps_near_inputs, ps_near_ref, refine_ref, scene
from ps_ref import angle_deg, ps_design
from rti import _lib as L
from test_gpu_ps import check, same_bits

pytestmark = pytest.mark.gpu

STREAM = L.RTI_KERNEL_ONE_LAUNCH
LO, HI = 0.5, 254.5
ORIGIN = (3.5, -2.25)
DTYPES = {"f32": torch.float32, "u8": torch.uint8, "i32": torch.int32}
OUT_KW = dict(return_kind=True, return_res=True, return_kept=True)


def stack(H, W, C, N=24, falloff=1, integer=False):
    sc = scene(H, W, N, C == 3, ORIGIN, 0.0, falloff)
    return sc, (np.rint(sc["I"]) if integer else sc["I"].copy())


@functools.lru_cache(maxsize=None)
def reference(H, W, C, iters, N=24, falloff=1, with_height=False, integer=False, margin=1e-3):
    sc, I = stack(H, W, C, N, falloff, integer)
    # an integer stack's window 1..254 keeps the samples 0.5..254.5 keeps: the bounds the conditions are checked at
    lo, hi = (1.0, 254.0) if integer else (LO, HI)
    ref = ps_near_ref(sc["lights"], I, H, W, ORIGIN, sc["h"] if with_height else None, 0.0, falloff, sc["r0"], lo, hi,
                      3, iters, 5.0)
    check_ps_near_inputs(ref, I, LO, HI, margin=margin)
    return ref


def near_kw(sc, falloff=1, with_height=False, cuda=None):
    kw = dict(origin=ORIGIN, falloff=bool(falloff), r0=sc["r0"])
    if with_height:
        kw["height"] = torch.tensor(sc["h"], device=cuda).float()
    return kw


def run(cuda, I, H, W, lights, dtype=torch.float32, **kw):
    """rti.photometric_stereo_near on [N, H, W] or [3, N, H, W] -> what test_gpu_ps.check takes: normals [P, 3] (or
    [3, P]), albedo [P] or [P, 3], kind [P], res and kept [P] or [3, P] on the host, and fallback_px"""
    stats = {}
    It = torch.as_tensor(I, device=cuda).to(dtype)
    P = H * W
    out = rti.photometric_stereo_near(It.reshape(It.shape[:-1] + (H, W)), lights[:, :3], light_scale=lights[:, 3],
                                      stats=stats, **OUT_KW, **kw)
    n, albedo, kind, res, kept = (t.cpu().numpy() for t in out)
    rgb = It.dim() == 3
    assert n.shape == ((3, H, W) if kw.get("normal_layout") == "planar" else (H, W, 3))
    assert albedo.shape == ((H, W, 3) if rgb else (H, W)) and kind.shape == (H, W)
    assert res.shape == kept.shape == ((3, H, W) if rgb else (H, W)) and kept.dtype == np.int32
    n = n.reshape((3, P) if kw.get("normal_layout") == "planar" else (P, 3))
    albedo, kind = albedo.reshape((P, 3) if rgb else (P,)), kind.reshape(P)
    res, kept = res.reshape((3, P) if rgb else (P,)), kept.reshape((3, P) if rgb else (P,))
    return [n, albedo, kind, res, kept, stats["fallback_px"]]


@pytest.mark.parametrize("with_height", [False, True])
@pytest.mark.parametrize("falloff", [0, 1])
@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (15, 17), (13, 20), (13, 79)])
def test_against_reference(cuda, H, W, C, iters, falloff, with_height):
    """H×W: a lone pixel, a partial tile, a tile plus a tail, several tiles with row ends inside every tile and every
    wave.  The scene is lit with or without fall-off and fitted with the same; without the height map the fit's
    model is off by the bump, so the Huber passes have residuals to weigh."""
    sc, I = stack(H, W, C, falloff=falloff)
    ref = reference(H, W, C, iters, falloff=falloff, with_height=with_height)
    kw = dict(lo=LO, hi=HI, iters=iters, delta=5.0, **near_kw(sc, falloff, with_height, cuda))
    got = run(cuda, I, H, W, sc["lights"], **kw)
    check(got, ref)
    planar = run(cuda, I, H, W, sc["lights"], normal_layout="planar", **kw)
    assert np.array_equal(planar[0].T, got[0], equal_nan=True)
    check(planar, ref, planar=True)


MARGIN_N = {}  # N -> ps_ref.FP32_MARGIN where a sample of that scene lies within 1e-3 of a bound


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("N", [3, 24, 25])
def test_light_counts(cuda, N, iters):
    """The minimum of three lights, an even count, and the odd tail of the loop unrolled by two."""
    H, W, C = 13, 20, 3
    sc, I = stack(H, W, C, N)
    ref = reference(H, W, C, iters, N, with_height=True, margin=MARGIN_N.get(N, 1e-3))
    check(run(cuda, I, H, W, sc["lights"], lo=LO, hi=HI, iters=iters, delta=5.0, **near_kw(sc, 1, True, cuda)), ref)


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("dtype", ["u8", "i32"])
def test_integer_stacks(cuda, dtype, C, iters):
    """The scene rounded, window 1..254: a uint8 stack given neither bound uses it by default."""
    H, W = 13, 20
    sc, I = stack(H, W, C, integer=True)
    kw = {} if dtype == "u8" else dict(lo=1, hi=254)
    got = run(cuda, I, H, W, sc["lights"], dtype=DTYPES[dtype], iters=iters, delta=5.0, **near_kw(sc, 1, True, cuda), **kw)
    check(got, reference(H, W, C, iters, with_height=True, integer=True))


def into(cuda, sc, I3, H, W, *, iters, kernel=0, pad=0, planar=False, dtype=torch.float32, height=None, z_offset=0.0,
         scale=True, lo=LO, hi=HI, lights=None):
    """The _into entry on a [C, N, P] stack, optionally a view of planes padded by `pad` elements -> the device
    tensors (normals, albedo, kind, res, kept, fallback)."""
    C, N, P = I3.shape
    buf = torch.full((C, N, P + pad), 7.0, device=cuda).to(dtype)
    buf[:, :, :P] = torch.as_tensor(I3, device=cuda).to(dtype)
    view = buf[:, :, :P]
    outs = (torch.empty((3, P) if planar else (P, 3), device=cuda), torch.empty((C, P), device=cuda),
            torch.empty(P, dtype=torch.uint8, device=cuda), torch.empty((C, P), device=cuda),
            torch.empty((C, P), dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda))
    lights = sc["lights"] if lights is None else lights
    table = rti.ps_near_lights(lights[:, :3], lights[:, 3] if scale else None)
    rti.photometric_stereo_near_into(torch.as_tensor(table, device=cuda), view if pad else view.contiguous(), H, W,
                                     *outs, lo=lo, hi=hi, min_lights=3, origin=ORIGIN, height=height, z_offset=z_offset,
                                     r0=sc["r0"], iters=iters, delta=5.0, kernel=kernel,
                                     normal_layout="planar" if planar else "pixel",
                                     light_stride=P + pad if pad else None)
    return outs


def as_got(outs, C):
    n, albedo, kind, res, kept, fb = (t.cpu().numpy() for t in outs)
    return [n, albedo.T if C == 3 else albedo[0], kind, res if C == 3 else res[0], kept if C == 3 else kept[0], int(fb[0])]


@pytest.mark.parametrize("N,tp", [(54, 128), (107, 64), (3, 256)])
def test_tile_sizes_and_forms_agree(cuda, N, tp):
    """C = 3 fp32 at 13×23 = 299 pixels: every resident tile size the plan returns at a small N; the resident form
    and RTI_KERNEL_ONE_LAUNCH give identical bits in every output, with 16-byte tile loads and without."""
    H, W, C = 13, 23, 3
    plan = rti.load().rti_photometric_stereo_near_plan
    assert plan(N, L.RTI_F32, C, 2, 0) == tp == rti.load().rti_photometric_stereo_plan(N, L.RTI_F32, C, 2, 0)
    assert plan(N, L.RTI_F32, C, 2, STREAM) == 0
    sc, I = stack(H, W, C, N)
    h = torch.tensor(sc["h"], device=cuda).float()
    auto = into(cuda, sc, I, H, W, iters=2, height=h)
    assert same_bits(auto, into(cuda, sc, I, H, W, iters=2, height=h, kernel=STREAM))
    assert same_bits(auto, into(cuda, sc, I, H, W, iters=2, height=h, pad=1))  # planes off 16 bytes
    assert bool(torch.isfinite(auto[0]).all()) and bool(auto[1].any())


@pytest.mark.parametrize("dtype,C", [("f32", 1), ("u8", 1), ("u8", 3), ("i32", 3)])
def test_forms_agree_at_the_full_tile(cuda, dtype, C):
    """N = 24: TP = 256 in every dtype; 13×79 has full tiles (16-byte tile loads where 1027 elements allow) and a tail
    tile, and a row end in every wave."""
    H, W = 13, 79
    integer = dtype != "f32"
    assert rti.load().rti_photometric_stereo_near_plan(24, getattr(L, "RTI_" + dtype.upper()), C, 2, 0) == 256
    sc, I = stack(H, W, C, integer=integer)
    h = torch.tensor(sc["h"], device=cuda).float()
    kw = dict(iters=2, dtype=DTYPES[dtype], lo=1.0 if integer else LO, hi=254.0 if integer else HI, height=h)
    auto = into(cuda, sc, I.reshape(C, 24, H * W), H, W, **kw)
    check(as_got(auto, C), reference(H, W, C, 2, with_height=True, integer=integer))
    assert same_bits(auto, into(cuda, sc, I.reshape(C, 24, H * W), H, W, kernel=STREAM, **kw))


@pytest.mark.parametrize("iters", [0, 2])
def test_plumbing_identities(cuda, iters):
    H, W, C = 13, 20, 1
    P = H * W
    sc, I = stack(H, W, C)
    I3 = I.reshape(C, 24, P)
    base = into(cuda, sc, I3, H, W, iters=iters)
    assert same_bits(base, into(cuda, sc, I3, H, W, iters=iters, height=torch.zeros(P, device=cuda)))
    c = 2.75  # exact in fp32
    lifted = into(cuda, sc, I3, H, W, iters=iters, z_offset=c)
    assert same_bits(lifted, into(cuda, sc, I3, H, W, iters=iters, height=torch.full((P,), c, device=cuda)))
    assert not torch.equal(lifted[0], base[0])
    h = torch.tensor(sc["h"], device=cuda).float().reshape(P)
    holes = h.clone()
    holes[::7] = float("nan")
    holes[3] = float("inf")
    zeroed = torch.where(torch.isfinite(holes), h, torch.zeros_like(h))
    assert same_bits(into(cuda, sc, I3, H, W, iters=iters, height=holes), into(cuda, sc, I3, H, W, iters=iters, height=zeroed))
    assert same_bits(base, into(cuda, sc, I3, H, W, iters=iters, scale=False))  # the scene's scales are ones


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("C", [1, 3])
def test_padded_light_stride(cuda, C, iters):
    """Planes of P + 5 elements (and channels of N such planes) through the _into entry: the padding is never read as
    a pixel, and the outputs are those of the contiguous stack bit for bit."""
    for H, W in ((15, 17), (13, 20)):
        sc, I = stack(H, W, C)
        I3 = I.reshape(C, 24, H * W)
        outs = into(cuda, sc, I3, H, W, iters=iters, pad=5)
        check(as_got(outs, C), reference(H, W, C, iters))
        assert same_bits(outs, into(cuda, sc, I3, H, W, iters=iters))


@pytest.mark.parametrize("form", ["resident", "streaming"])
def test_far_light_stride(cuda, form):
    """A light_stride of 2^29 + 3 elements at N = 5 (plane 4 starts 2^33 bytes in: only a 64-bit offset reaches it),
    13×20 pixels of fp32, in the manner of tests/test_gpu_far_strides.py: the planes are views into one sparse
    allocation filled with NaN, so a truncated offset reads NaN.  The outputs equal the dense stack's bit for bit."""
    H, W, N = 13, 20, 5
    P = H * W
    sc, I = stack(H, W, 1, N)
    ls = (1 << 29) + 3
    buf = torch.full(((N - 1) * ls + P,), float("nan"), dtype=torch.float32, device=cuda)
    view = torch.as_strided(buf, (1, N, P), (N * ls, ls, 1))
    view.copy_(torch.as_tensor(I.reshape(1, N, P), device=cuda))
    iters = 2 if form == "resident" else 0
    outs = (torch.empty((P, 3), device=cuda), torch.empty((1, P), device=cuda),
            torch.empty(P, dtype=torch.uint8, device=cuda), torch.empty((1, P), device=cuda),
            torch.empty((1, P), dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda))
    rti.photometric_stereo_near_into(torch.as_tensor(sc["lights"], device=cuda), view, H, W, *outs, lo=LO, hi=HI,
                                     min_lights=3, origin=ORIGIN, r0=sc["r0"], iters=iters, delta=5.0, light_stride=ls)
    assert same_bits(outs, into(cuda, sc, I.reshape(1, N, P), H, W, iters=iters))
    del view, buf
    torch.cuda.empty_cache()


def test_light_on_a_pixel(cuda):
    """Light 5 sits exactly on pixel (4, 7) of the plane: its row there is NaN, the pixel ends as kind 4 with NaN
    normal and albedo through the fit's own failure path, and every other pixel still matches the reference.  For
    the degenerate pixel only kind, normals and albedo are compared.  Without fall-off: under the inverse square a
    light one pixel away outweighs the other 23 by (2·W)² and the neighbours' systems miss the pivot condition."""
    H, W, C = 13, 20, 1
    sc, I = stack(H, W, C, falloff=0)
    lights = sc["lights"].copy()
    lights[5, :3] = (ORIGIN[0] + 7.0, ORIGIN[1] + 4.0, 0.0)
    bad = 4 * W + 7
    ref = ps_near_ref(lights, I, H, W, ORIGIN, None, 0.0, 0, sc["r0"], LO, HI, 3, 2, 5.0)
    assert np.isnan(ref["rows"][bad, 5]).all() and ref["kind"][bad] == 4 and (np.delete(ref["kind"], bad) != 4).all()
    check_ps_near_inputs(ref, I, LO, HI)
    got = run(cuda, I, H, W, lights, lo=LO, hi=HI, iters=2, delta=5.0, origin=ORIGIN, falloff=False)
    assert got[2][bad] == 4 and np.isnan(got[0][bad]).all() and np.isnan(got[1][bad])
    got[3][bad], got[4][bad] = ref["res"][0][bad], ref["kept"][0][bad]
    got[5] = ref["fallback_px"]
    check(got, ref)


def test_far_limit_is_the_shared_design(cuda):
    """Without fall-off and with the lights at D = 1e7·W along the directions l_n, the rows are the far design to
    first order: the direction from a pixel δ off the centre is l − (δ − (δ·l)l)/D + O(|δ|²/D²), |Δl| <= |δ|/D <=
    W/(1e7·W) = 1e-7 for every pixel of a W×W or flatter image.  The least-squares g = A⁺y then moves by at most
    κ(A)·‖ΔA‖/‖A‖·‖g‖ (first order; ‖ΔA‖_F <= 1e-7·√N, ‖A‖_2 >= ‖A‖_F/√3 = √(N/3), so ‖ΔA‖/‖A‖ <= √3·1e-7), and a
    windowed pixel's sub-design of the kept rows is held by the same bound with its own κ, which the test takes from
    the worst pixel's kept rows.  Two fp32 roundings of the unit normals add 2·√3·2⁻²⁴.  So the angle between the two
    normals is at most 2·κ·√3·1e-7 + 2·√3·2⁻²⁴ rad, the factor 2 covering the second-order terms and the
    normalisation."""
    H, W, C = 13, 20, 1
    sc, I = stack(H, W, C, falloff=0)
    A = ps_design(sc["lu"], sc["lv"])
    centre = np.array([ORIGIN[0] + 0.5 * (W - 1), ORIGIN[1] + 0.5 * (H - 1), 0.0])
    pos = centre + 1e7 * W * A
    It = torch.as_tensor(I.reshape(24, H, W), device=cuda)
    far = rti.photometric_stereo(It, sc["lu"], sc["lv"], A[:, 2], lo=LO, hi=HI, **OUT_KW)
    near = rti.photometric_stereo_near(It, pos, origin=ORIGIN, falloff=False, lo=LO, hi=HI, **OUT_KW)
    assert torch.equal(far[2], near[2]) and torch.equal(far[4], near[4]) and bool((far[2] == 0).all())
    inside = (I >= LO) & (I <= HI)
    kappa = max(np.linalg.cond(A[inside[:, p]]) for p in range(H * W))
    bound = np.degrees(2.0 * kappa * np.sqrt(3.0) * 1e-7 + 2.0 * np.sqrt(3.0) * 2.0 ** -24)
    angle = angle_deg(far[0].cpu().numpy().astype(np.float64), near[0].cpu().numpy().astype(np.float64))
    assert angle.max() <= bound, (angle.max(), bound)
    assert np.abs(far[1].cpu().numpy() - near[1].cpu().numpy()).max() <= 400.0 * np.radians(bound)


@functools.lru_cache(maxsize=None)
def refinement_reference():
    """The alternation on the CPU (ps_near_ref and height_ref): the maximum normal error of rounds 0, 1 and 2."""
    sc = scene(64, 64)
    return [angle_deg(r["normals"], sc["n"]).max() for r in refine_ref(sc, 64, 64, 2, LO, HI)]


def test_refinement(cuda):
    """The 64×64 grey scene with z_offset at the scene's gauge (0: the bump has zero mean).  refine=2 returns a height
    of the right shape; its maximum normal error is below refine=0's and at most 1.5× the CPU alternation's round-2
    error: the GPU solver stops at rtol = 1e-6 of ‖b‖ where the reference solves its system directly, and that
    margin covers the difference."""
    sc = scene(64, 64)
    ref_err = refinement_reference()
    assert ref_err[2] < ref_err[0]
    It = torch.as_tensor(sc["I"].reshape(24, 64, 64), device=cuda)
    n0, a0 = rti.photometric_stereo_near(It, sc["lights"][:, :3], r0=sc["r0"], lo=LO, hi=HI)
    n2, a2, h2 = rti.photometric_stereo_near(It, sc["lights"][:, :3], r0=sc["r0"], lo=LO, hi=HI, refine=2,
                                             return_height=True)
    assert h2.shape == (64, 64) and h2.dtype == torch.float32 and n2.shape == (64, 64, 3) and a2.shape == (64, 64)
    err0 = angle_deg(n0.cpu().numpy().reshape(-1, 3).astype(np.float64), sc["n"]).max()
    err2 = angle_deg(n2.cpu().numpy().reshape(-1, 3).astype(np.float64), sc["n"]).max()
    print(f"max normal error: GPU round 0 {err0:.4g}°, round 2 {err2:.4g}°; CPU rounds {ref_err}")
    assert err2 < err0
    assert err2 <= 1.5 * ref_err[2], (err2, ref_err)
    # the loop composed by hand gives the same bits: the height fed back is the one returned
    h = rti.height_from_normals(n0)
    n1, _ = rti.photometric_stereo_near(It, sc["lights"][:, :3], r0=sc["r0"], lo=LO, hi=HI, height=h)
    h = rti.height_from_normals(n1)
    n2b, a2b = rti.photometric_stereo_near(It, sc["lights"][:, :3], r0=sc["r0"], lo=LO, hi=HI, height=h)
    assert torch.equal(h, h2) and torch.equal(n2b, n2) and torch.equal(a2b, a2)
    # the default r0: the lights' mean distance from the ROI centre at z_offset
    nd, _ = rti.photometric_stereo_near(It, sc["lights"][:, :3], lo=LO, hi=HI)
    centre = np.array([31.5, 31.5, 0.0])
    r0 = float(np.linalg.norm(sc["lights"][:, :3] - centre, axis=1).mean())
    assert torch.equal(nd, rti.photometric_stereo_near(It, sc["lights"][:, :3], r0=r0, lo=LO, hi=HI)[0])


@pytest.mark.parametrize("planar", [False, True])
def test_torch_op(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    H, W = 13, 20
    P = H * W
    sc, I = stack(H, W, 3)
    It = torch.as_tensor(I, device=cuda)
    Ld = torch.as_tensor(sc["lights"], device=cuda)
    h = torch.tensor(sc["h"], device=cuda).float().reshape(P)
    nl = "planar" if planar else "pixel"
    for stack_t in (It, It[0]):
        n, albedo, kind, res, kept, fb = torch.ops.rti.photometric_stereo_near(
            Ld, stack_t, H, W, LO, HI, 3, 2, 5.0, None, planar, 0, ORIGIN[0], ORIGIN[1], h, 0.0, True, sc["r0"])
        stats = {}
        I4 = stack_t.reshape(3, 24, H, W) if stack_t.dim() == 3 else stack_t.reshape(24, H, W)
        n2, a2, k2, r2, m2 = rti.photometric_stereo_near(I4, sc["lights"][:, :3], origin=ORIGIN, height=h.reshape(H, W),
                                                         r0=sc["r0"], lo=LO, hi=HI, iters=2, delta=5.0,
                                                         normal_layout=nl, stats=stats, **OUT_KW)
        n2, k2 = n2.reshape(n.shape), k2.reshape(P)
        if stack_t.dim() == 3:
            a2, r2, m2 = a2.reshape(P, 3).T, r2.reshape(3, P), m2.reshape(3, P)
        else:
            a2, r2, m2 = a2.reshape(P), r2.reshape(P), m2.reshape(P)
        assert torch.equal(n, n2) and torch.equal(albedo, a2) and torch.equal(kind, k2)
        assert torch.equal(res, r2) and torch.equal(kept, m2)
        assert fb.dtype == torch.int32 and fb.shape == (1,) and int(fb) == stats["fallback_px"]
    args = (Ld, It, H, W, LO, HI, 3, 2, 5.0, [0.2, 0.3, 0.5], planar, 0, ORIGIN[0], ORIGIN[1], h, 0.0, True, sc["r0"])
    torch.library.opcheck(torch.ops.rti.photometric_stereo_near.default, args,
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.rti.photometric_stereo_near.default,
                          (Ld, It[0], H, W, -float("inf"), float("inf"), 3, 0, 0.0, None, planar, 0),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.photometric_stereo_near(Ld.float(), It, H, W, LO, HI, 3, 2, 5.0, None, planar)


def test_into_entry_and_graph_capture(cuda):
    """The _into entry gives the public function's bits, and under graph capture (one branch: the one launch) replays
    to the same bits on new data."""
    H, W, C = 13, 20, 3
    P = H * W
    sc, I = stack(H, W, C)
    h = torch.tensor(sc["h"], device=cuda).float().reshape(P)
    want = into(cuda, sc, I, H, W, iters=2, height=h)
    pub = rti.photometric_stereo_near(torch.as_tensor(I.reshape(3, 24, H, W), device=cuda), sc["lights"][:, :3],
                                      origin=ORIGIN, height=h, r0=sc["r0"], lo=LO, hi=HI, iters=2, delta=5.0, **OUT_KW)
    assert torch.equal(pub[0].reshape(P, 3), want[0]) and torch.equal(pub[1].reshape(P, 3).T, want[1])
    assert torch.equal(pub[2].reshape(P), want[2]) and torch.equal(pub[3].reshape(3, P), want[3])
    assert torch.equal(pub[4].reshape(3, P), want[4])
    Ld = torch.as_tensor(sc["lights"], device=cuda)
    Id = torch.as_tensor(I[:, :, ::-1].copy(), device=cuda)
    outs = (torch.empty((P, 3), device=cuda), torch.empty((C, P), device=cuda),
            torch.empty(P, dtype=torch.uint8, device=cuda), torch.empty((C, P), device=cuda),
            torch.empty((C, P), dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda))

    def call():
        rti.photometric_stereo_near_into(Ld, Id, H, W, *outs, lo=LO, hi=HI, min_lights=3, origin=ORIGIN, height=h,
                                         r0=sc["r0"], iters=2, delta=5.0)

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
    assert same_bits(replayed, want) and bool(replayed[1].any())
    check(as_got(replayed, C), reference(H, W, C, 2, with_height=True))
