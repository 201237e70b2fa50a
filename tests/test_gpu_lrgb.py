"""rti_lrgb_from_rgb / rti_relight_lrgb on the GPU against their fp64 NumPy restatement (tests/lrgb_ref.py).

Sizes: the scalar path (1), P % 4 != 0 one pixel short of a wave (255), exactly one wave chunk (256), the vector path
with four chunks and a 52-pixel tail (1076), and the scalar path with a tail (1073).  Every size runs in both layouts
on each side and with the maps starting 8 bytes into a 16-byte aligned buffer; outputs sit between guard elements.
The maps mix every class of biquadratic with planted black pixels (chroma 1) and NaN pixels (lrgb_ref.mixed_*).

Margin: 1e-6·max(1, |v|) for an fp32 result of fp64 arithmetic, the project's standing one (tests/test_gpu_normals.py);
integer outputs are compared exactly except where the fp64 reference lies within that margin of an integer."""
import functools

import numpy as np
import pytest
import torch

import rti
from lrgb_ref import (INT32_MIN, lrgb_ref, mixed_lrgb, mixed_rgb_coef, relight_lrgb_ref, synth_dirs, to_int32,
                      to_uint8)

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 1076, 1073]
LUMA = (0.299, 0.587, 0.114)
ES = [1, 2, 65]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]


@functools.lru_cache(maxsize=None)
def gram():
    g = rti.gram(*synth_dirs(12, 7))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def dirs(E):
    """E directions: (0.3, -0.45), then (0.8, 0.75) with lu² + lv² > 1, then seeded ones in [-0.9, 0.9]²."""
    rng = np.random.default_rng(65)
    lu = np.concatenate([[0.3, 0.8], rng.uniform(-0.9, 0.9, 63)])[:E]
    lv = np.concatenate([[-0.45, 0.75], rng.uniform(-0.9, 0.9, 63)])[:E]
    return lu, lv


@functools.lru_cache(maxsize=None)
def compress_case(P, weights=None):
    """(coef [3, P, 6] fp32, its reference [P, 9] fp64) -- computed once, shared and never written."""
    coef = mixed_rgb_coef(P, 2000 + P)
    ref = lrgb_ref(coef, gram(), weights)
    coef.setflags(write=False)
    ref.setflags(write=False)
    return coef, ref


@functools.lru_cache(maxsize=None)
def relight_case(P):
    """(lrgb [P, 9] fp32, the fp64 reference images [65, P, 3]) -- computed once, shared and never written."""
    m = mixed_lrgb(P, 3000 + P)
    ref = relight_lrgb_ref(m, *dirs(65))
    m.setflags(write=False)
    ref.setflags(write=False)
    return m, ref


def on_device(cuda, a, offset):
    """The host array on the device as it is laid out; offset: it starts 8 bytes into a 16-byte aligned buffer."""
    t = torch.as_tensor(np.array(a, order="C"), device=cuda)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    pad = 8 // t.element_size()
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=cuda)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def guarded(cuda, n, dtype, offset):
    """(buffer, view of n elements) with at least 12 guard elements on both sides; the view is 16-byte aligned, or
    8 bytes off with offset (uint8: 1 byte off a dword)."""
    fill = 77 if dtype == torch.uint8 else -7
    buf = torch.full((n + 48,), fill, dtype=dtype, device=cuda)
    lead = 16 + ((1 if dtype == torch.uint8 else 2) if offset else 0)
    return buf, buf[lead:lead + n], lead, fill


def guards_untouched(buf, lead, n, fill):
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + n:] == fill).all())


def close32(got, want):
    """NaN and ±inf positions equal, the rest within 1e-6·max(1, |want|); returns the worst ratio to that margin."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / (1e-6 * np.maximum(1.0, np.abs(want[ok])))).max())


def planar_of(a, planar):
    """[..., P, k] -> [..., k, P] when planar."""
    return np.swapaxes(a, -1, -2) if planar else a


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


# ---- rti_lrgb_from_rgb -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("lrgb_layout", ["pixel", "planar"])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_lrgb_from_rgb(cuda, P, layout, lrgb_layout, offset):
    for weights in (None, LUMA):
        coef, ref = compress_case(P, weights)
        c = on_device(cuda, planar_of(coef, layout == "planar"), offset)
        buf, view, lead, fill = guarded(cuda, 9 * P, torch.float32, offset)
        out = view.view((9, P) if lrgb_layout == "planar" else (P, 9))
        rti.lrgb_from_rgb_into(c, gram(), out, weights=weights, layout=layout, lrgb_layout=lrgb_layout)
        got = out.cpu().numpy()
        got = got.T if lrgb_layout == "planar" else got
        worst = close32(got, ref)
        print(f"P={P} weights={weights}: {worst:.3g} of the margin")
        assert worst <= 1.0
        assert guards_untouched(buf, lead, 9 * P, fill)
        nan = np.isnan(ref[:, 0])
        assert np.isnan(got[nan]).all() and np.isfinite(got[~nan]).all()
        if P >= 8:  # the planted pixels: black -> zero luminance and chroma 1; NaN -> nine NaNs
            assert np.array_equal(got[0], [0, 0, 0, 0, 0, 0, 1, 1, 1]) and np.array_equal(got[P - 1], got[0])
            assert np.isnan(got[1]).all() and np.isnan(got[P - 2]).all()
        w = np.full(3, 1.0 / 3.0) if weights is None else np.asarray(weights)
        # Σ w·chroma = 1 whenever d > 0: three fp32 roundings of chroma weigh in with Σ w·|chroma|·2^-24
        chroma = got[~nan, 6:].astype(np.float64)
        excess = np.abs(chroma @ w - 1.0) / np.maximum(1.0, np.abs(chroma) @ w)
        assert (excess <= 1e-6).all()


@pytest.mark.parametrize("lrgb_layout", ["pixel", "planar"])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", [256, 1076])
def test_lrgb_from_rgb_paths_agree_to_the_bit(cuda, P, layout, lrgb_layout):
    """The same pixels through the vector path (aligned maps) and one pixel per lane (the maps 8 bytes off)."""
    coef, _ = compress_case(P)
    outs = []
    for offset in (False, True):
        c = on_device(cuda, planar_of(coef, layout == "planar"), offset)
        _, view, _, _ = guarded(cuda, 9 * P, torch.float32, offset)
        out = view.view((9, P) if lrgb_layout == "planar" else (P, 9))
        outs.append(bits(rti.lrgb_from_rgb_into(c, gram(), out, weights=LUMA, layout=layout, lrgb_layout=lrgb_layout)))
    assert torch.equal(*outs)


def test_lrgb_from_rgb_shapes_and_strides(cuda):
    """rti.lrgb_from_rgb on [3, H, W, 6] / [3, 6, H, W]; a channel stride above the dense one through the C entry."""
    from rti import _lib as L
    from rti import api

    H, W = 12, 21  # P = 252
    P = H * W
    coef = mixed_rgb_coef(P, 77)
    ref = lrgb_ref(coef, gram())
    for layout in ("pixel", "planar"):
        c = on_device(cuda, planar_of(coef, layout == "planar"), False)
        c = c.view((3, 6, H, W) if layout == "planar" else (3, H, W, 6))
        for ol in ("pixel", "planar"):
            m = rti.lrgb_from_rgb(c, gram(), layout=layout, lrgb_layout=ol)
            assert m.shape == ((9, H, W) if ol == "planar" else (H, W, 9)) and m.dtype == torch.float32
            got = m.reshape(9, P).t() if ol == "planar" else m.reshape(P, 9)
            assert close32(got.cpu().numpy(), ref) <= 1.0
    pad = 6 * P + 20  # elements between channels
    buf = torch.full((3 * pad,), float("nan"), dtype=torch.float32, device=cuda)
    for ch in range(3):
        buf[ch * pad:ch * pad + 6 * P] = torch.as_tensor(coef[ch].ravel(), device=cuda)
    out = torch.empty((P, 9), dtype=torch.float32, device=cuda)
    g = np.ascontiguousarray(gram())
    st = rti.load().rti_lrgb_from_rgb(api._vp(buf), L.RTI_COEF_PIXEL_MAJOR, pad, P, api._dptr(g), None, api._vp(out),
                                      L.RTI_COEF_PIXEL_MAJOR, api._stream_of(buf))
    assert st == L.RTI_OK
    assert close32(out.cpu().numpy(), ref) <= 1.0


# ---- rti_relight_lrgb ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_relight_lrgb(cuda, P, layout, offset):
    m, ref65 = relight_case(P)
    md = on_device(cuda, planar_of(m, layout == "planar"), offset)
    nan_px = np.isnan(m).all(1)
    for E in ES:
        ref = ref65[:E]
        luv = torch.as_tensor(np.stack(dirs(E), -1), device=cuda)
        with np.errstate(invalid="ignore"):
            dist = np.abs(ref - np.rint(ref))
            near = dist <= 1e-6 * np.maximum(1.0, np.abs(ref))
        for dt, conv in zip(OUT_DTYPES, (None, to_int32, to_uint8)):
            n = E * P * 3
            buf, view, lead, fill = guarded(cuda, n, dt, offset)
            out = rti.relight_lrgb_into(md, luv, view.view(E, P, 3), layout=layout)
            got = out.cpu().numpy()
            assert guards_untouched(buf, lead, n, fill), (E, dt)
            if conv is None:
                worst = close32(got, ref)
                print(f"P={P} E={E}: {worst:.3g} of the margin")
                assert worst <= 1.0
                assert np.isnan(got[:, nan_px]).all()
            else:
                assert np.array_equal(got[~near], conv(ref)[~near]), (E, dt)
                assert (got[:, nan_px] == (INT32_MIN if dt == torch.int32 else 0)).all()


@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", [256, 1076])
def test_relight_lrgb_paths_agree_to_the_bit(cuda, P, layout):
    m, _ = relight_case(P)
    luv = torch.as_tensor(np.stack(dirs(65), -1), device=cuda)
    for dt in OUT_DTYPES:
        outs = []
        for offset in (False, True):
            md = on_device(cuda, planar_of(m, layout == "planar"), offset)
            _, view, _, _ = guarded(cuda, 65 * P * 3, dt, offset)
            outs.append(bits(rti.relight_lrgb_into(md, luv, view.view(65, P, 3), layout=layout)))
        assert torch.equal(*outs), dt


@pytest.mark.parametrize("layout", ["pixel", "planar"])
def test_unit_chroma_is_relight_to_the_bit(cuda, layout):
    """With chroma = 1 every channel of the fp32 output is rti.relight of the fp64 coefficients, bit for bit."""
    P = 1076
    m = relight_case(P)[0].copy()
    m[:, 6:] = 1.0
    lu, lv = dirs(65)
    got = rti.relight_lrgb(on_device(cuda, planar_of(m, layout == "planar"), False), lu, lv, layout=layout)
    coef6 = torch.as_tensor(m[:, :6], device=cuda).double()
    want = rti.relight(coef6, lu, lv, out_dtype=torch.float32).cpu().numpy()
    assert got.shape == (65, P, 3) and want.shape == (65, P)
    got = got.cpu().numpy()
    assert np.isfinite(want).sum() > 0.9 * want.size
    for c in range(3):
        assert np.array_equal(got[..., c], want, equal_nan=True), c


def test_relight_lrgb_shapes(cuda):
    H, W = 12, 21
    m = mixed_lrgb(H * W, 5)
    ref = relight_lrgb_ref(m, *dirs(2))
    pix = torch.as_tensor(m.reshape(H, W, 9), device=cuda)
    pla = pix.permute(2, 0, 1).contiguous()
    for lrgb, layout in ((pix, "pixel"), (pla, "planar")):
        out = rti.relight_lrgb(lrgb, *dirs(2), layout=layout)
        assert out.shape == (2, H, W, 3) and out.dtype == torch.float32
        assert close32(out.reshape(2, H * W, 3).cpu().numpy(), ref) <= 1.0
        one = rti.relight_lrgb(lrgb, 0.3, -0.45, layout=layout, out_dtype=torch.uint8)
        assert one.shape == (H, W, 3) and one.dtype == torch.uint8
        with np.errstate(invalid="ignore"):
            near = np.abs(ref[0] - np.rint(ref[0])) <= 1e-6 * np.maximum(1.0, np.abs(ref[0]))
        assert np.array_equal(one.reshape(-1, 3).cpu().numpy()[~near], to_uint8(ref[0])[~near])
    with pytest.raises(ValueError, match="terms"):
        rti.relight_lrgb(pix, 0.1, 0.2, layout="planar")
    with pytest.raises(ValueError):
        rti.relight_lrgb(pix, 0.1, 0.2, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        rti.relight_lrgb(pix.half(), 0.1, 0.2)
    with pytest.raises(ValueError):
        rti.relight_lrgb_into(pix, torch.zeros((1, 2), device=cuda), torch.empty((1, H * W, 3), device=cuda))
    with pytest.raises(ValueError):
        rti.relight_lrgb_into(pix, torch.zeros((1, 2), dtype=torch.float64, device=cuda),
                              torch.empty((1, H * W, 2), device=cuda))
    with pytest.raises(ValueError):
        rti.lrgb_from_rgb(torch.zeros((2, H, W, 6), device=cuda), gram())
    with pytest.raises(ValueError):
        rti.lrgb_from_rgb(torch.zeros((3, H, W, 6), device=cuda), np.eye(5))
    with pytest.raises(ValueError, match="weight"):
        rti.lrgb_from_rgb(torch.zeros((3, H, W, 6), device=cuda), gram(), weights=(0.5, -0.5, 1.0))
    with pytest.raises(NotImplementedError, match="PTM-6"):
        rti.fit_lrgb(torch.zeros((3, 20, H, W), device=cuda), np.zeros(20), np.zeros(20), basis="hsh")


# ---- end to end ------------------------------------------------------------------------------------------------

# ten directions on the quarter grid: the PTM monomials are multiples of 1/16
LU10 = np.array([0, .5, -.5, 0, 0, .5, .5, -.5, -.5, .25], np.float32)
LV10 = np.array([0, 0, 0, .5, -.5, .5, -.5, .5, -.5, .25], np.float32)


@functools.lru_cache(maxsize=None)
def known_object(H=24, W=20):
    """A known LRGB map [H, W, 9] and the stack [3, 10, H, W] it renders to, with every product exact: coefficients
    in multiples of 32 make the luminance at each light an even integer in [8, 152], chroma is a permutation of
    (1.5, 1, 0.5) (mean 1, as the fit normalises it), so every sample is an integer in [4, 228]."""
    rng = np.random.default_rng(24)
    a = np.concatenate([rng.choice([-32.0, 0.0, 32.0], (H, W, 5)), rng.choice([64.0, 96.0], (H, W, 1))], -1)
    chroma = rng.permuted(np.tile([1.5, 1.0, 0.5], (H, W, 1)), axis=-1)
    A = np.stack([LU10 * LU10, LV10 * LV10, LU10 * LV10, LU10, LV10, np.ones(10, np.float32)], -1).astype(np.float64)
    lum = np.einsum("nk,hwk->nhw", A, a)
    I = chroma.transpose(2, 0, 1)[:, None] * lum[None]
    assert np.array_equal(I, np.rint(I)) and I.min() >= 4 and I.max() <= 228 and np.linalg.matrix_rank(A) == 6
    m = np.concatenate([a, chroma], -1)
    m.setflags(write=False)
    I.setflags(write=False)
    return m, I


@pytest.mark.parametrize("lrgb_layout", ["pixel", "planar"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_fit_lrgb_end_to_end(cuda, dtype, lrgb_layout):
    """rti.fit_lrgb recovers the known map and rti.relight_lrgb at the capture directions reproduces the stack, to
    test_gpu_fit.py's tolerance for exact recovery: 1e-4 of the per-coefficient scale max(max|true|, 1)."""
    m, I = known_object()
    H, W = m.shape[:2]
    Id = torch.as_tensor(np.array(I), device=cuda).to(dtype)
    got = rti.fit_lrgb(Id, LU10, LV10, lrgb_layout=lrgb_layout)
    assert got.shape == ((9, H, W) if lrgb_layout == "planar" else (H, W, 9)) and got.dtype == torch.float32
    g = (got.permute(1, 2, 0) if lrgb_layout == "planar" else got).cpu().numpy().astype(np.float64)
    scale = np.maximum(np.abs(m).max((0, 1)), 1.0)
    err = (np.abs(g - m) / scale).max((0, 1))
    print("recovery error / scale per channel:", np.array2string(err, precision=2))
    assert err.max() < 1e-4
    out = rti.relight_lrgb(got, LU10, LV10, layout=lrgb_layout)
    assert out.shape == (10, H, W, 3)
    want = I.transpose(1, 2, 3, 0)
    rerr = np.abs(out.cpu().numpy() - want).max() / max(np.abs(want).max(), 1.0)
    print(f"relight error / scale: {rerr:.3g}")
    assert rerr < 1e-4
    # weights: the luma weighting scales luminance and chroma reciprocally, the rendering stays
    lum = rti.fit_lrgb(Id, LU10, LV10, weights=LUMA, lrgb_layout=lrgb_layout)
    out2 = rti.relight_lrgb(lum, LU10, LV10, layout=lrgb_layout)
    assert np.abs(out2.cpu().numpy() - want).max() / max(np.abs(want).max(), 1.0) < 1e-4
    ch = (lum[6:].permute(1, 2, 0) if lrgb_layout == "planar" else lum[..., 6:]).cpu().numpy().astype(np.float64)
    assert np.abs(ch @ np.asarray(LUMA) - 1.0).max() <= 1e-6


def test_luminance_planes_feed_the_ptm_entries(cuda):
    """The luminance view of a planar LRGB map is a dense planar PTM-6 map: rti.normals of it equals rti.normals of
    a copy of those planes to the bit, and relight_enhanced / unsharp / relight take it too."""
    m, I = known_object()
    lrgb = rti.fit_lrgb(torch.as_tensor(np.array(I), device=cuda).float(), LU10, LV10, lrgb_layout="planar")
    lum = rti.lrgb_luminance(lrgb)
    assert lum.shape == (6, 24, 20) and lum.data_ptr() == lrgb.data_ptr()
    copy = lrgb[:6].clone()
    for x, y in zip(rti.normals(lum, layout="planar", return_kind=True, return_peak=True),
                    rti.normals(copy, layout="planar", return_kind=True, return_peak=True)):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(bits(rti.relight_enhanced(lum, 0.3, -0.2, "diffuse_gain", gain=2.0, layout="planar")),
                       bits(rti.relight_enhanced(copy, 0.3, -0.2, "diffuse_gain", gain=2.0, layout="planar")))
    assert torch.equal(bits(rti.unsharp(lum, 1.0, 1.5, layout="planar")), bits(rti.unsharp(copy, 1.0, 1.5, layout="planar")))
    # grey image · chroma = the colour image
    grey = rti.relight(lum, 0.25, 0.25, layout="planar")
    rgb = rti.relight_lrgb(lrgb, 0.25, 0.25, layout="planar")
    want = grey[..., None].double() * lrgb[6:].permute(1, 2, 0).double()
    assert (rgb.double() - want).abs().max().item() <= 1e-4 * 255
    with pytest.raises(ValueError, match="planar"):
        rti.lrgb_luminance(lrgb.permute(1, 2, 0).contiguous(), layout="pixel")


@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P = 1076
    layout = "planar" if planar else "pixel"
    coef, _ = compress_case(P)
    c = on_device(cuda, planar_of(coef, planar), False)
    g = torch.as_tensor(np.array(gram()))
    for lrgb_planar in (False, True):
        for weights in (None, list(LUMA)):
            got = torch.ops.rti.lrgb_from_rgb(c, g, weights, planar, lrgb_planar)
            want = rti.lrgb_from_rgb_into(c, gram(), torch.empty((9, P) if lrgb_planar else (P, 9), device=cuda),
                                          weights=weights, layout=layout,
                                          lrgb_layout="planar" if lrgb_planar else "pixel")
            assert got.shape == want.shape and got.dtype == torch.float32 and torch.equal(bits(got), bits(want))
            torch.library.opcheck(torch.ops.rti.lrgb_from_rgb.default, (c, g, weights, planar, lrgb_planar),
                                  test_utils=("test_schema", "test_faketensor"))
    m, _ = relight_case(P)
    md = on_device(cuda, planar_of(m, planar), False)
    lu, lv = dirs(2)
    luv = torch.as_tensor(np.stack([lu, lv], -1))
    for dt in OUT_DTYPES:
        got = torch.ops.rti.relight_lrgb(md, luv, planar, dt)
        want = rti.relight_lrgb(md, lu, lv, layout=layout, out_dtype=dt)
        assert got.shape == want.shape == (2, P, 3) and got.dtype == dt and torch.equal(bits(got), bits(want))
        torch.library.opcheck(torch.ops.rti.relight_lrgb.default, (md, luv, planar, dt),
                              test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.lrgb_from_rgb(c.transpose(1, 2).contiguous(), g, None, planar, False)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_lrgb(md.t().contiguous(), luv, planar, torch.float32)
