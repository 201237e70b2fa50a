"""8-bit LRGB PTMs on the GPU (rti_lrgb8.hip) against what the project already has: the host quantiser of rti/io.py
(write_ptm, _ptm_quantise) for the bytes and the 13 header values, and rti.relight_lrgb of the dequantised fp32 map
for the images.  Every comparison is exact: bytes, and bit patterns of fp64 / fp32 / int32 values.

Sizes: the scalar path (1, 7), one pixel short of a wave (255), one wave chunk (256), the scalar path with a tail
(1073), the vector path with four chunks and a 52-pixel tail (1076), more than one workgroup (3077), and 787532 =
768·1024 + 1024 + 76 pixels: the extremes' grid is capped at 768 workgroups of 1024 pixels, so two workgroups fold a
second chunk there and the tail kernel folds 768 partials, three per lane.  Maps run in both layouts, aligned and 8
bytes into a 16-byte aligned buffer; the byte blocks aligned and 1 byte off a dword; outputs between guard elements.

One thing the files add: write_ptm prints the scales with nine significant digits, so the scales a
file carries are roundings of the fp64 scales the bytes were made with.  Tests that go through a file therefore
compare with QuantisedLRGB.with_file_scales(), which is the object a round trip yields; the count of fp32 values
that differ without it is printed."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import rti
from lrgb_ref import mixed_lrgb
from rti.io import _ptm_quantise

pytestmark = pytest.mark.gpu

BIG = 768 * 1024 + 1024 + 76
SIZES = [1, 7, 255, 256, 1073, 1076, 3077, BIG]
ES = [1, 2, 65]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]


@functools.lru_cache(maxsize=None)
def dirs(E):
    """test_gpu_lrgb.py's directions: (0.3, -0.45), then (0.8, 0.75) with lu² + lv² > 1, then seeded ones."""
    rng = np.random.default_rng(65)
    lu = np.concatenate([[0.3, 0.8], rng.uniform(-0.9, 0.9, 63)])[:E]
    lv = np.concatenate([[-0.45, 0.75], rng.uniform(-0.9, 0.9, 63)])[:E]
    return lu, lv


def host_quantise(m):
    """An fp32 LRGB map [P, 9] -> what the host writes: (raw uint8 [P, 6], rgb uint8 [P, 3], qparams fp64 [13]).
    The bytes are read back from the file write_ptm writes (one row of P pixels); the full-precision scales, the
    biases and s are those write_ptm computes on the way (_ptm_quantise of the luminance times s)."""
    P = m.shape[0]
    m64 = m.astype(np.float64)
    fin = m64[:, 6:][np.isfinite(m64[:, 6:])]
    s = float(fin.max()) if fin.size and fin.max() > 0 else 1.0
    with np.errstate(all="ignore"):
        raw, scale, bias = _ptm_quantise(m64[:, :6] * s)
    with tempfile.TemporaryDirectory() as d:
        with np.errstate(all="ignore"):
            path = rti.write_ptm(os.path.join(d, "ref.ptm"), m.reshape(1, P, 9))
        q = rti.read_ptm(path, quantised=True)[1]
    file_raw, rgb = q.coef.numpy().reshape(P, 6), q.rgb.numpy().reshape(P, 3)
    assert np.array_equal(file_raw, raw) and np.array_equal(q.bias, bias)
    qparams = np.concatenate([scale, bias.astype(np.float64), [s]])
    for a in (raw, rgb, qparams):
        a.setflags(write=False)
    return raw, rgb, qparams


@functools.lru_cache(maxsize=None)
def case(P):
    """(map [P, 9] fp32, raw, rgb, qparams of the host) -- computed once, shared and never written."""
    m = mixed_lrgb(P, 5000 + P)
    m.setflags(write=False)
    return (m,) + host_quantise(m)


def on_device(cuda, a, offset):
    """The host array on the device as it is laid out; offset: it starts 8 bytes (uint8: 1 byte) into a 16-byte
    aligned buffer."""
    t = torch.as_tensor(np.array(a, order="C"), device=cuda)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    pad = 1 if t.dtype == torch.uint8 else 8 // t.element_size()
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=cuda)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == pad * t.element_size() and v.is_contiguous()
    return v


def guarded(cuda, n, dtype, offset):
    """(buffer, view of n elements) with at least 12 guard elements on both sides; the view is 16-byte aligned, or
    8 bytes off with offset (uint8: 1 byte off a dword; fp64: 16 bytes on, it must stay 8-byte aligned)."""
    fill = 77 if dtype == torch.uint8 else -7
    buf = torch.full((n + 48,), fill, dtype=dtype, device=cuda)
    lead = 16 + ((1 if dtype == torch.uint8 else 2) if offset else 0)
    return buf, buf[lead:lead + n], lead, fill


def guards_untouched(buf, lead, n, fill):
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + n:] == fill).all())


def planar_of(a, planar):
    return np.ascontiguousarray(a.T) if planar else a


def bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def run_quantiser(cuda, m, layout, offset):
    """rti_lrgb_qparams + rti_lrgb_quantise through the _into forms, everything between guards, the workspace
    holding NaN bit patterns -> (qparams fp64 [13], coef8 [P, 6], rgb8 [P, 3]) on the host, guards checked."""
    P = m.shape[0]
    md = on_device(cuda, planar_of(m, layout == "planar"), offset)
    ws = torch.full((rti.lrgb_qparams_workspace(P),), 0xFF, dtype=torch.uint8, device=cuda)
    qbuf, qp, qlead, qfill = guarded(cuda, 13, torch.float64, offset)
    cbuf, c8, clead, cfill = guarded(cuda, 6 * P, torch.uint8, offset)
    rbuf, r8, rlead, rfill = guarded(cuda, 3 * P, torch.uint8, offset)
    rti.lrgb_qparams_into(md, ws, qp, layout=layout)
    rti.lrgb_quantise_into(md, qp, c8, r8, layout=layout)
    assert guards_untouched(qbuf, qlead, 13, qfill)
    assert guards_untouched(cbuf, clead, 6 * P, cfill) and guards_untouched(rbuf, rlead, 3 * P, rfill)
    return qp.cpu().numpy(), c8.cpu().numpy().reshape(P, 6), r8.cpu().numpy().reshape(P, 3)


def same_f64_bits(got, want):
    return np.array_equal(np.asarray(got, np.float64).view(np.int64), np.asarray(want, np.float64).view(np.int64))


# ---- rti_lrgb_qparams, rti_lrgb_quantise -------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_qparams_are_the_hosts(cuda, P, layout, offset):
    m, _, _, want = case(P)
    got, _, _ = run_quantiser(cuda, m, layout, offset)
    print("scale", got[:6], "bias", got[6:12], "s", got[12])
    assert same_f64_bits(got, want)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_bytes_are_the_hosts(cuda, P, layout, offset):
    m, raw, rgb, _ = case(P)
    _, c8, r8 = run_quantiser(cuda, m, layout, offset)
    if P >= 255:  # the comparison is of bytes inside the range, not of saturated planes
        inside = float(((raw > 0) & (raw < 255)).mean())
        print(f"P={P}: {inside:.3f} of the luminance bytes strictly inside 1..254")
        assert inside > 0.9
    assert np.array_equal(c8, raw)
    assert np.array_equal(r8, rgb)
    if P >= 8:  # the planted NaN pixels: bias and 0
        _, _, _, qp = case(P)
        assert np.array_equal(c8[2], qp[6:12]) and np.array_equal(c8[P - 3], qp[6:12])
        assert not r8[2].any() and not r8[P - 3].any()


def planted(name):
    """A 2100-pixel map (two workgroups and a 52-pixel tail; P % 4 == 0) with one planted feature."""
    P = 2100
    m = mixed_lrgb(P, 77).copy()
    if name.startswith("extremes at "):
        lo_px, hi_px = {"0 and P-1": (0, P - 1), "P-1 and 0": (P - 1, 0), "255 and 256": (255, 256),
                        "256 and 255": (256, 255), "1023 and 1024": (1023, 1024),
                        "1024 and 1023": (1024, 1023)}[name[len("extremes at "):]]
        m[[lo_px, hi_px]] = 1.0
        for j in range(6):  # outside every other finite value of the plane
            plane = m[np.isfinite(m[:, j]), j]
            m[lo_px, j] = plane.min() - 100.0 - 7 * j
            m[hi_px, j] = plane.max() + 100.0 + 11 * j
        m[hi_px, 6 + (hi_px % 3)] = 2.75  # the chroma maximum (the map's chroma is below 1.8) sits there too
    elif name == "constant plane":
        m[:, 3] = 12.5
    elif name == "all-NaN plane":
        m[:, 1] = np.nan
    elif name == "inf and NaN plane":
        m[:, 4] = np.where(np.arange(P) % 3 == 0, np.nan, np.where(np.arange(P) % 3 == 1, np.inf, -np.inf))
    elif name == "plane above zero":  # a5 in [20, 250]: the bias clips to 0 and the bytes saturate
        m[:, 5] = np.linspace(20.0, 250.0, P, dtype=np.float32)
    elif name == "plane below zero":
        m[:, 0] = np.linspace(-250.0, -20.0, P, dtype=np.float32)
    elif name == "chroma all <= 0":
        m[:, 6:] = -np.abs(m[:, 6:])
        m[5, 6] = 0.0
    elif name == "chroma with inf":
        m[10, 6], m[11, 7], m[1500, 8] = np.inf, -np.inf, np.inf
    elif name == "all NaN":
        m[:] = np.nan
    else:
        raise KeyError(name)
    return m


PLANTED = ["extremes at 0 and P-1", "extremes at P-1 and 0", "extremes at 255 and 256", "extremes at 256 and 255",
           "extremes at 1023 and 1024", "extremes at 1024 and 1023", "constant plane", "all-NaN plane",
           "inf and NaN plane", "plane above zero", "plane below zero", "chroma all <= 0", "chroma with inf", "all NaN"]


@pytest.mark.parametrize("name", PLANTED)
def test_planted_cases(cuda, name):
    m = planted(name)
    raw, rgb, want = host_quantise(m)
    if name == "constant plane":
        assert want[3] == 1.0
    elif name == "all-NaN plane":
        assert want[1] == 1.0 and want[6 + 1] == 0.0
    elif name == "inf and NaN plane":
        assert want[4] == 1.0 and want[6 + 4] == 0.0 and set(np.unique(raw[:, 4])) == {0, 255}
    elif name == "plane above zero":
        assert want[6 + 5] == 0.0 and (raw[:, 5] == 255).sum() > 10
    elif name == "chroma all <= 0":
        assert want[12] == 1.0 and not rgb.any()
    elif name == "chroma with inf":
        assert np.isfinite(want[12]) and rgb[10, 0] == 255 and rgb[11, 1] == 0
    elif name == "all NaN":
        assert np.array_equal(want, [1.0] * 6 + [0.0] * 6 + [1.0])
    for layout in ("pixel", "planar"):
        for offset in (False, True):  # the vector path and one pixel per lane
            got, c8, r8 = run_quantiser(cuda, m, layout, offset)
            assert same_f64_bits(got, want), (layout, offset, got, want)
            assert np.array_equal(c8, raw) and np.array_equal(r8, rgb), (layout, offset)


@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", [256, 1076])
def test_quantiser_paths_agree_to_the_bit(cuda, P, layout):
    """The same pixels through the vector path (aligned) and one pixel per lane (map 8 bytes, blocks 1 byte off)."""
    m = case(P)[0]
    a, b = run_quantiser(cuda, m, layout, False), run_quantiser(cuda, m, layout, True)
    assert same_f64_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- rti_relight_lrgb8 -------------------------------------------------------------------------------------------

def device_q(cuda, P, offset):
    """The host's quantised map of case(P) on the device (so these tests do not lean on the device quantiser)."""
    _, raw, rgb, qp = case(P)
    return on_device(cuda, raw, offset), on_device(cuda, rgb, offset), on_device(cuda, qp, False)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("P", SIZES)
def test_relight_lrgb8_is_relight_lrgb_of_the_dequantised_map(cuda, P, offset):
    m = case(P)[0]
    c8, r8, qp = device_q(cuda, P, offset)
    fp32 = rti.dequantise_lrgb(rti.QuantisedLRGB(c8.clone(), r8.clone(), qp))
    assert fp32.shape == (P, 9) and fp32.dtype == torch.float32 and bool(torch.isfinite(fp32).all())
    nan_px = torch.as_tensor(np.isnan(m).all(1), device=cuda)
    for E in (ES if P < BIG else [2]):
        lu, lv = dirs(E)
        luv = torch.as_tensor(np.stack([lu, lv], -1), device=cuda)
        for dt in OUT_DTYPES:
            n = E * P * 3
            buf, view, lead, fill = guarded(cuda, n, dt, offset)
            got = rti.relight_lrgb8_into(c8, r8, qp, luv, view.view(E, P, 3))
            want = rti.relight_lrgb(fp32, lu, lv, out_dtype=dt)
            assert guards_untouched(buf, lead, n, fill), (E, dt)
            assert torch.equal(bits(got), bits(want)), (E, dt)
            if P >= 8:  # a NaN pixel is stored as (bias, 0): it renders finite, and black
                assert bool(nan_px.any()) and bool((got[:, nan_px] == 0).all()), (E, dt)


@pytest.mark.parametrize("P", [256, 1076])
def test_relight_lrgb8_paths_agree_to_the_bit(cuda, P):
    luv = torch.as_tensor(np.stack(dirs(65), -1), device=cuda)
    for dt in OUT_DTYPES:
        outs = []
        for offset in (False, True):
            c8, r8, qp = device_q(cuda, P, offset)
            _, view, _, _ = guarded(cuda, 65 * P * 3, dt, offset)
            outs.append(bits(rti.relight_lrgb8_into(c8, r8, qp, luv, view.view(65, P, 3))))
        assert torch.equal(*outs), dt


def test_api_shapes_and_refusals(cuda):
    H, W = 12, 21
    m = torch.as_tensor(mixed_lrgb(H * W, 5).reshape(H, W, 9), device=cuda)
    q = rti.quantise_lrgb(m)
    assert isinstance(q, rti.QuantisedLRGB) and q.shape == (H, W) and q.device == m.device
    assert q.coef.shape == (H, W, 6) and q.rgb.shape == (H, W, 3) and q.qparams.shape == (13,)
    qp = rti.quantise_lrgb(m.permute(2, 0, 1).contiguous(), layout="planar")
    assert torch.equal(qp.coef, q.coef) and torch.equal(qp.rgb, q.rgb) and torch.equal(bits(qp.qparams), bits(q.qparams))
    flat = rti.quantise_lrgb(m.reshape(H * W, 9))
    assert flat.shape == (H * W,) and torch.equal(flat.coef, q.coef.reshape(-1, 6))
    assert q.scale.shape == (6,) and q.bias.shape == (6,) and q.s > 0
    out = rti.relight_lrgb8(q, *dirs(2))
    assert out.shape == (2, H, W, 3) and out.dtype == torch.float32
    one = rti.relight_lrgb8(q, 0.3, -0.45, out_dtype=torch.uint8)
    assert one.shape == (H, W, 3) and one.dtype == torch.uint8
    assert rti.relight_lrgb8(flat, 0.3, -0.45).shape == (H * W, 3)
    d = rti.dequantise_lrgb(q)
    assert d.shape == (H, W, 9) and d.dtype == torch.float32 and d.device == m.device
    host = q.to("cpu")
    assert host.device.type == "cpu" and torch.equal(host.coef, q.coef.cpu())
    assert torch.equal(bits(rti.dequantise_lrgb(host)), bits(d.cpu()))  # the same arithmetic on either device
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_lrgb8(host, 0.1, 0.2)
    with pytest.raises(ValueError, match="terms"):
        rti.quantise_lrgb(m, layout="planar")
    with pytest.raises(ValueError):
        rti.quantise_lrgb(m.half())
    with pytest.raises(ValueError):
        rti.relight_lrgb8(q, 0.1, 0.2, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="workspace"):
        rti.lrgb_qparams_into(m, torch.empty(8, dtype=torch.uint8, device=cuda), q.qparams)
    with pytest.raises(ValueError, match="qparams"):
        rti.lrgb_quantise_into(m, q.qparams.float(), q.coef, q.rgb)
    with pytest.raises(ValueError, match="rgb8"):
        rti.lrgb_quantise_into(m, q.qparams, q.coef, q.rgb[:-1].contiguous())
    with pytest.raises(ValueError):
        rti.relight_lrgb8_into(q.coef, q.rgb, q.qparams, torch.zeros((1, 2), device=cuda),
                               torch.empty((1, H * W, 3), device=cuda))


# ---- files -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(24, 20), (5, 7)])
def test_file_identity_and_dequantise(cuda, tmp_path, H, W):
    """write_ptm of the device-quantised map and today's host path write byte-identical files; dequantise_lrgb
    equals read_ptm of that file bit for bit with the scales the file carries."""
    m = mixed_lrgb(H * W, 300 + H).reshape(H, W, 9)
    q = rti.quantise_lrgb(torch.as_tensor(m, device=cuda))
    with np.errstate(all="ignore"):
        host_path = rti.write_ptm(str(tmp_path / "host.ptm"), m)
    dev_path = rti.write_ptm(str(tmp_path / "device.ptm"), q)
    assert open(dev_path, "rb").read() == open(host_path, "rb").read()
    fmt, back = rti.read_ptm(dev_path)
    assert fmt == "lrgb"
    want = torch.as_tensor(back).view(torch.int32)
    fresh = bits(rti.dequantise_lrgb(q)).cpu()
    print(f"{H}x{W}: {int((fresh != want).sum())} of {want.numel()} fp32 values differ with the full fp64 scales")
    assert torch.equal(bits(rti.dequantise_lrgb(q.with_file_scales())).cpu(), want)
    loaded = rti.read_ptm(dev_path, quantised=True)[1].to(cuda)
    assert torch.equal(loaded.coef, q.coef) and torch.equal(loaded.rgb, q.rgb)
    assert torch.equal(bits(loaded.qparams), bits(q.with_file_scales().qparams))
    assert torch.equal(bits(rti.dequantise_lrgb(loaded)).cpu(), want)


LU10 = np.array([0, .5, -.5, 0, 0, .5, .5, -.5, -.5, .25], np.float32)
LV10 = np.array([0, 0, 0, .5, -.5, .5, -.5, .5, -.5, .25], np.float32)


def known_stack(H=24, W=20):
    """test_gpu_lrgb.py's known_object stack [3, 10, H, W]: every sample an integer in [4, 228]."""
    rng = np.random.default_rng(24)
    a = np.concatenate([rng.choice([-32.0, 0.0, 32.0], (H, W, 5)), rng.choice([64.0, 96.0], (H, W, 1))], -1)
    chroma = rng.permuted(np.tile([1.5, 1.0, 0.5], (H, W, 1)), axis=-1)
    A = np.stack([LU10 * LU10, LV10 * LV10, LU10 * LV10, LU10, LV10, np.ones(10, np.float32)], -1).astype(np.float64)
    I = chroma.transpose(2, 0, 1)[:, None] * np.einsum("nk,hwk->nhw", A, a)[None]
    assert np.array_equal(I, np.rint(I)) and I.min() >= 4 and I.max() <= 228
    return I


def test_end_to_end(cuda, tmp_path):
    """fit_lrgb -> quantise_lrgb -> relight_lrgb8 (uint8) equals relight_lrgb of the map read back from the file
    the host writes: a viewer that keeps the 9 bytes shows what one that expands them to fp32 shows."""
    m = rti.fit_lrgb(torch.as_tensor(known_stack(), device=cuda).float(), LU10, LV10)
    q = rti.quantise_lrgb(m)
    path = rti.write_ptm(str(tmp_path / "object.ptm"), m)  # today's host path
    back = torch.as_tensor(rti.read_ptm(path)[1], device=cuda)
    want = rti.relight_lrgb(back, LU10, LV10, out_dtype=torch.uint8)
    got = rti.relight_lrgb8(q.with_file_scales(), LU10, LV10, out_dtype=torch.uint8)
    fresh = rti.relight_lrgb8(q, LU10, LV10, out_dtype=torch.uint8)
    print(f"{int((fresh != want).sum())} of {want.numel()} bytes differ with the full fp64 scales")
    assert got.shape == (10, 24, 20, 3) and torch.equal(got, want)
    assert torch.equal(fresh, want)  # on this object the ninth digit of the scales moves no byte either
    assert int(want.max()) > 100  # an image, not a black frame


# ---- torch ops ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P = 1076
    m = case(P)[0]
    md = on_device(cuda, planar_of(m, planar), False)
    q = rti.quantise_lrgb(md, layout="planar" if planar else "pixel")
    c8, r8, qp = torch.ops.rti.lrgb_quantise(md, planar)
    assert c8.shape == (P, 6) and r8.shape == (P, 3) and qp.shape == (13,)
    assert c8.dtype == r8.dtype == torch.uint8 and qp.dtype == torch.float64
    assert torch.equal(c8, q.coef) and torch.equal(r8, q.rgb) and torch.equal(bits(qp), bits(q.qparams))
    torch.library.opcheck(torch.ops.rti.lrgb_quantise.default, (md, planar), test_utils=("test_schema", "test_faketensor"))
    lu, lv = dirs(2)
    luv = torch.as_tensor(np.stack([lu, lv], -1))
    for dt in OUT_DTYPES:
        got = torch.ops.rti.relight_lrgb8(c8, r8, qp, luv, dt)
        want = rti.relight_lrgb8(q, lu, lv, out_dtype=dt)
        assert got.shape == want.shape == (2, P, 3) and got.dtype == dt and torch.equal(bits(got), bits(want))
        torch.library.opcheck(torch.ops.rti.relight_lrgb8.default, (c8, r8, qp, luv, dt),
                              test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.lrgb_quantise(md.t().contiguous(), planar)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_lrgb8(c8, r8[:-1], qp, luv, torch.float32)


def test_graph_capture_replays_the_eager_bytes(cuda):
    """Quantise then relight from the bytes, captured once (a single chain) and replayed on other data."""
    from rti import ops  # noqa: F401

    P = 3077
    first, second = case(P)[0], mixed_lrgb(P, 9)
    md = on_device(cuda, first, False)
    luv = torch.as_tensor(np.stack(dirs(2), -1), device=cuda)

    def chain():
        c8, r8, qp = torch.ops.rti.lrgb_quantise(md, False)
        return c8, r8, qp, torch.ops.rti.relight_lrgb8(c8, r8, qp, luv, torch.uint8)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = chain()
    for data in (first, second):
        md.copy_(torch.as_tensor(np.array(data), device=cuda))
        graph.replay()
        torch.cuda.synchronize(cuda)
        replayed = [t.clone() for t in captured]
        for got, want in zip(replayed, chain()):
            assert torch.equal(bits(got), bits(want))
    assert bool(replayed[3].any())
