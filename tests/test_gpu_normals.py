"""rti_ptm_normals / rti_relight_enhanced on the GPU against their fp64 NumPy restatement (tests/normals_ref.py).

The coefficient maps mix every class of pixel (interior maxima, maxima outside the disc, saddles, minima, all-zero
rows, NaN / inf rows), each far from every branch threshold (normals_ref.mixed_coef), so no pixel is left out of
the normal and kind comparisons.  Sizes: the scalar path (1, 3), one lane (4), one pixel short of a wave (255), a
wave (256), a wave plus one lane (260), a block (1024), a block plus a partial wave plus 3 (1279), odd (2313)."""
import functools

import numpy as np
import pytest
import torch

import rti
from conftest import golden, relight_close
from normals_ref import mixed_coef, normals_ref, relight_enhanced_ref, to_int32, to_uint8

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 255, 256, 260, 1024, 1279, 2313]
DIRS = [(0.0, 0.0), (0.3, -0.45), (0.8, 0.75)]  # the last has lu² + lv² > 1
GAINS = [0.5, 1.0, 3.0]
SPECULAR = [(1.0, 0.0, 1), (0.4, 150.0, 1), (0.4, 150.0, 75), (0.4, 150.0, 255)]
NP_DT = {torch.float32: np.float32, torch.float64: np.float64}


@functools.lru_cache(maxsize=None)
def case(P, dtype=torch.float32):
    """(coef [P, 6] host array, its reference) -- computed once, shared and never written."""
    coef = mixed_coef(P, 1000 + P, NP_DT[dtype])
    coef.setflags(write=False)
    return coef, normals_ref(coef)


@functools.lru_cache(maxsize=None)
def enhanced_ref(P, dtype, lu, lv, mode, kw):
    """The fp64 reference image of case(P, dtype) for one parameter set (kw: sorted items) -- computed once."""
    want = relight_enhanced_ref(case(P, dtype)[0], lu, lv, mode, **dict(kw))
    want.setflags(write=False)
    return want


def on_device(cuda, coef, layout, offset):
    """The map on the device in `layout`, contiguous; offset: it starts 8 bytes into a 16-byte aligned buffer."""
    t = torch.as_tensor(np.array(coef.T if layout == "planar" else coef, order="C"), device=cuda)
    if not offset:
        return t
    pad = 8 // t.element_size()
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=cuda)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def check_normals(ref, n, kind, peak, nl):
    n = n.cpu().numpy().astype(np.float64)
    n = n.T if nl == "planar" else n
    assert np.array_equal(kind.cpu().numpy(), ref["kind"])
    bad = ref["kind"] == 4
    assert np.isnan(n[bad]).all() and not np.isnan(n[~bad]).any()
    err = np.abs(n[~bad] - ref["n"][~bad]).max() if (~bad).any() else 0.0
    pk = peak.cpu().numpy().astype(np.float64)
    assert np.isnan(pk[bad]).all() and not np.isnan(pk[~bad]).any()
    perr = (np.abs(pk - ref["peak"]) / np.maximum(np.abs(ref["peak"]), 255.0))[~bad].max() if (~bad).any() else 0.0
    print(f"normal err {err:.3g}, peak err {perr:.3g}")
    assert err <= 1e-6 and perr <= 1e-6


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("nl", ["pixel", "planar"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_normals_kind_and_peak(cuda, P, layout, dtype, nl, offset):
    coef, ref = case(P, dtype)
    c = on_device(cuda, coef, layout, offset)
    # outputs with guard pixels on both sides: a store outside the map would show
    nb = torch.full((3 * (P + 8),), -7.0, dtype=torch.float32, device=cuda)
    kb = torch.full((P + 8,), 99, dtype=torch.uint8, device=cuda)
    pb = torch.full((P + 8,), -7.0, dtype=torch.float32, device=cuda)
    n = nb[12:12 + 3 * P].view((3, P) if nl == "planar" else (P, 3))
    rti.ptm_normals_into(c, n, kb[4:4 + P], pb[4:4 + P], layout=layout, normal_layout=nl)
    check_normals(ref, n, kb[4:4 + P], pb[4:4 + P], nl)
    assert (nb[:12] == -7).all() and (nb[12 + 3 * P:] == -7).all()
    assert (kb[:4] == 99).all() and (kb[4 + P:] == 99).all() and (pb[:4] == -7).all() and (pb[4 + P:] == -7).all()


@pytest.mark.parametrize("nl", ["pixel", "planar"])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", [256, 1280, 2316])
def test_vector_and_scalar_paths_agree_to_the_bit(cuda, P, layout, nl):
    """The same pixels through the vector path (aligned map) and one pixel per lane (the map 8 bytes off; the
    outputs of the last partial chunk go that way in both), normals, kind, peak and every enhanced output."""
    coef, _ = case(P)
    a, b = on_device(cuda, coef, layout, False), on_device(cuda, coef, layout, True)
    outs = []
    for c in (a, b):
        o = rti.normals(c.view((6, P) if layout == "planar" else (P, 6)), layout=layout, normal_layout=nl,
                        return_kind=True, return_peak=True)
        o += tuple(rti.relight_enhanced(c, 0.3, -0.45, mode, gain=3.0, kd=0.4, ks=150.0, exp=75, layout=layout,
                                        out_dtype=dt)
                   for mode in ("diffuse_gain", "specular") for dt in (torch.float32, torch.int32, torch.uint8))
        outs.append(o)
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.uint8 else x.view(torch.int32),
                           y.view(torch.uint8) if y.dtype == torch.uint8 else y.view(torch.int32))


@pytest.mark.parametrize("nl", ["pixel", "planar"])
@pytest.mark.parametrize("P", [260, 2313])
def test_optional_outputs(cuda, P, nl):
    coef, ref = case(P)
    c = on_device(cuda, coef, "pixel", False)
    n, kind, peak = rti.normals(c, normal_layout=nl, return_kind=True, return_peak=True)
    assert n.shape == ((3, P) if nl == "planar" else (P, 3)) and kind.shape == (P,) and peak.shape == (P,)
    assert n.dtype == torch.float32 and kind.dtype == torch.uint8 and peak.dtype == torch.float32
    only = rti.normals(c, normal_layout=nl)
    assert torch.is_tensor(only) and torch.equal(only.view(torch.int32), n.view(torch.int32))
    n2, k2 = rti.normals(c, normal_layout=nl, return_kind=True)
    n3, p3 = rti.normals(c, normal_layout=nl, return_peak=True)
    assert torch.equal(n2.view(torch.int32), n.view(torch.int32)) and torch.equal(k2, kind)
    assert torch.equal(n3.view(torch.int32), n.view(torch.int32)) and torch.equal(p3.view(torch.int32), peak.view(torch.int32))


def test_nan_pixels_leave_their_neighbours(cuda):
    """NaN rows between finite rows (first and last of a wave and of the block): only their own outputs are NaN."""
    coef = case(1024)[0].copy()
    coef[[0, 5, 511, 1023]] = np.nan
    ref = normals_ref(coef)
    n, kind, peak = rti.normals(torch.as_tensor(coef, device=cuda), return_kind=True, return_peak=True)
    check_normals(ref, n, kind, peak, "pixel")


def enhanced_params():
    for g in GAINS:
        yield "diffuse_gain", dict(gain=g)
    for kd, ks, e in SPECULAR:
        yield "specular", dict(kd=kd, ks=ks, exp=e)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_enhanced_float(cuda, P, layout, dtype, offset):
    coef, ref = case(P, dtype)
    c = on_device(cuda, coef, layout, offset)
    bad = ref["kind"] == 4
    worst = 0.0
    for mode, kw in enhanced_params():
        for lu, lv in DIRS:
            want = enhanced_ref(P, dtype, lu, lv, mode, tuple(sorted(kw.items())))
            got = rti.relight_enhanced(c, lu, lv, mode, layout=layout, **kw).cpu().numpy().astype(np.float64)
            assert got.shape == (P,) and np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any()
            if (~bad).any():
                err = (np.abs(got - want) / np.maximum(np.abs(want), 255.0))[~bad].max()
                worst = max(worst, err)
                assert err <= 1e-6, (mode, kw, lu, lv, err)
    print(f"enhanced fp32 worst err {worst:.3g}")


def check_integer_outputs(cuda, P, layout, offset, share_bound):
    """int32 / uint8 outputs equal the converted fp64 reference except where the reference lies within 1e-4 of an
    integer (an exact integer is compared all the same: an all-zero row under diffuse gain, where nothing rounds);
    returns the share of the pixels within 1e-4 of an integer, exact ones included."""
    coef, _ = case(P)
    c = on_device(cuda, coef, layout, offset)
    worst = 0.0
    for mode, kw in enhanced_params():
        for lu, lv in DIRS:
            want = enhanced_ref(P, torch.float32, lu, lv, mode, tuple(sorted(kw.items())))
            with np.errstate(invalid="ignore"):
                dist = np.abs(want - np.rint(want))
                near = (dist < 1e-4) & (dist > 0.0)
            for dt, conv in ((torch.int32, to_int32), (torch.uint8, to_uint8)):
                got = rti.relight_enhanced(c, lu, lv, mode, layout=layout, out_dtype=dt, **kw)
                assert got.dtype == dt and got.shape == (P,)
                assert np.array_equal(got.cpu().numpy()[~near], conv(want)[~near]), (mode, kw, lu, lv, dt)
            share = (dist < 1e-4).mean()
            worst = max(worst, share)
            if share_bound is not None:
                assert share <= share_bound, (mode, kw, lu, lv, share)
    return worst


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_enhanced_integer_outputs(cuda, P, layout, offset):
    check_integer_outputs(cuda, P, layout, offset, None)


def test_enhanced_integer_outputs_near_integer_share(cuda):
    """On a map large enough for a share to mean something (40 003 pixels: a uniform fractional part puts 0.02 %
    within 1e-4 of an integer and the 11 all-zero rows add 0.03 %; the reference's worst parameter set has
    0.057 %), the pixels within 1e-4 of an integer are at most 0.1 % of the map."""
    share = check_integer_outputs(cuda, 40003, "pixel", False, 1e-3)
    print(f"near-integer share {share:.4%}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
def test_identities_against_relight(cuda, layout, dtype):
    coef, ref = case(2313, dtype)
    c = on_device(cuda, coef, layout, False)
    fin = ref["kind"] != 4
    for lu, lv in DIRS:
        plain = rti.relight(c, lu, lv, layout=layout).cpu().numpy()
        for mode, kw in (("diffuse_gain", dict(gain=1.0)), ("specular", dict(kd=1.0, ks=0.0, exp=75))):
            got = rti.relight_enhanced(c, lu, lv, mode, layout=layout, **kw).cpu().numpy()
            err, ok = relight_close(got[fin], plain[fin])
            assert ok, (mode, lu, lv, err)


def test_end_to_end_golden_fit(cuda):
    """rti.fit of the 256² golden stack -> rti.normals equals the reference of the SAME GPU coefficients; a pixel
    is left out only if the reference's D/S is within 1e-9 of the threshold or its r² within 1e-9 of 1 (at most
    0.1 % of the pixels).  relight_enhanced(int32) -> relight_frame equals relight_frame of the reference's image."""
    d = golden("ptm_shared_256x256_N20.npz")
    I = torch.as_tensor(d["I"], device=cuda)
    coef = rti.fit(I, d["lu"], d["lv"])
    assert coef.shape == (256, 256, 6)
    ref = normals_ref(coef.cpu().numpy().reshape(-1, 6))
    n, kind, peak = rti.normals(coef, return_kind=True, return_peak=True)
    assert n.shape == (256, 256, 3) and kind.shape == (256, 256) and peak.shape == (256, 256)
    with np.errstate(all="ignore"):
        edge = (np.abs(ref["D"] / ref["S"] - 1e-6) <= 1e-9) | (ref["has_max"] & (np.abs(ref["r2"] - 1.0) <= 1e-9))
    assert edge.mean() <= 1e-3
    keep = ~edge
    assert np.array_equal(kind.cpu().numpy().ravel()[keep], ref["kind"][keep])
    assert (ref["kind"] != 4).all()
    assert np.abs(n.cpu().numpy().reshape(-1, 3)[keep] - ref["n"][keep]).max() <= 1e-6
    perr = np.abs(peak.cpu().numpy().ravel() - ref["peak"]) / np.maximum(np.abs(ref["peak"]), 255.0)
    assert perr[keep].max() <= 1e-6
    npl = rti.normals(coef.permute(2, 0, 1).contiguous(), layout="planar", normal_layout="planar")
    assert npl.shape == (3, 256, 256) and torch.equal(npl.permute(1, 2, 0).contiguous().view(torch.int32), n.view(torch.int32))
    # an enhanced BGR frame
    hsv = torch.as_tensor(np.random.default_rng(4).integers(0, 256, (256, 256, 3), dtype=np.uint8), device=cuda)
    for mode, kw in (("diffuse_gain", dict(gain=3.0)), ("specular", dict(kd=0.4, ks=150.0, exp=75))):
        want = relight_enhanced_ref(coef.cpu().numpy().reshape(-1, 6), 0.3, -0.45, mode, **kw)
        with np.errstate(invalid="ignore"):
            dist = np.abs(want - np.rint(want))
            assert ((dist < 1e-4) | edge).mean() <= 1e-3
        near = ((dist < 1e-4) & (dist > 0.0)) | edge
        src = rti.relight_enhanced(coef, 0.3, -0.45, mode, out_dtype=torch.int32, **kw)
        assert src.shape == (256, 256) and src.dtype == torch.int32
        assert np.array_equal(src.cpu().numpy().ravel()[~near], to_int32(want)[~near])
        frame = rti.relight_frame(src, hsv)
        ref_src = torch.as_tensor(to_int32(want).reshape(256, 256), device=cuda)
        ref_frame = rti.relight_frame(ref_src, hsv)
        same = (frame == ref_frame).all(-1).cpu().numpy().ravel()
        assert same[~near].all()


def test_python_layer_validation(cuda):
    c = on_device(cuda, case(260)[0], "pixel", False)
    with pytest.raises(ValueError, match="terms"):
        rti.normals(c[:, :5])
    with pytest.raises(ValueError, match="terms"):
        rti.relight_enhanced(c, 0.1, 0.2, "specular", layout="planar")
    with pytest.raises(ValueError):
        rti.normals(c, normal_layout="rows")
    with pytest.raises(ValueError):
        rti.normals(c, layout="rows")
    with pytest.raises(ValueError):
        rti.relight_enhanced(c, 0.1, 0.2, "glossy")
    with pytest.raises(ValueError):
        rti.relight_enhanced(c, 0.1, 0.2, "diffuse_gain", gain=-1.0)
    with pytest.raises(ValueError):
        rti.relight_enhanced(c, 0.1, 0.2, "specular", exp=0)
    with pytest.raises(ValueError):
        rti.relight_enhanced(c, float("nan"), 0.2, "specular")
    with pytest.raises(ValueError):
        rti.relight_enhanced(c, 0.1, 0.2, "specular", out_dtype=torch.float64)
    with pytest.raises(ValueError):
        rti.normals(c.half())
    with pytest.raises(NotImplementedError, match="PTM-6"):
        rti.normals(torch.zeros((8, 16), device=cuda), basis="hsh")
    with pytest.raises(NotImplementedError, match="PTM-6"):
        rti.relight_enhanced(torch.zeros((8, 9), device=cuda), 0.1, 0.2, "diffuse_gain", basis="hsh9")
    with pytest.raises(ValueError):
        rti.ptm_normals_into(c, torch.empty((259, 3), device=cuda))
    with pytest.raises(ValueError):
        rti.ptm_normals_into(c, torch.empty((260, 3), device=cuda), kind=torch.empty(260, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError):
        rti.relight_enhanced_into(c, 0.1, 0.2, "specular", torch.empty(261, device=cuda))
    with pytest.raises(ValueError):
        rti.relight_enhanced_into(c.t(), 0.1, 0.2, "specular", torch.empty(260, device=cuda))


@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    coef, _ = case(1279)
    layout = "planar" if planar else "pixel"
    c = on_device(cuda, coef, layout, False)
    for nplanar in (False, True):
        n, kind, peak = torch.ops.rti.ptm_normals(c, planar, nplanar)
        want = rti.normals(c, layout=layout, normal_layout="planar" if nplanar else "pixel", return_kind=True,
                           return_peak=True)
        for x, y in zip((n, kind, peak), want):
            assert x.shape == y.shape and x.dtype == y.dtype
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.uint8 else x.view(torch.int32),
                               y.view(torch.uint8) if y.dtype == torch.uint8 else y.view(torch.int32))
        torch.library.opcheck(torch.ops.rti.ptm_normals.default, (c, planar, nplanar),
                              test_utils=("test_schema", "test_faketensor"))
    for mode, kw in (("diffuse_gain", dict(gain=3.0)), ("specular", dict(kd=0.4, ks=150.0, exp=75))):
        for dt in (torch.float32, torch.int32, torch.uint8):
            args = (c, 0.3, -0.45, rti.api.ENHANCE_MODES[mode], kw.get("gain", 1.0), kw.get("kd", 1.0), kw.get("ks", 0.0),
                    kw.get("exp", 1), planar, dt)
            got = torch.ops.rti.relight_enhanced(*args)
            want = rti.relight_enhanced(c, 0.3, -0.45, mode, layout=layout, out_dtype=dt, **kw)
            assert got.shape == want.shape and got.dtype == dt
            assert torch.equal(got.view(torch.uint8) if dt == torch.uint8 else got.view(torch.int32),
                               want.view(torch.uint8) if dt == torch.uint8 else want.view(torch.int32))
            torch.library.opcheck(torch.ops.rti.relight_enhanced.default, args,
                                  test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.ptm_normals(c.t().contiguous(), planar, False)
