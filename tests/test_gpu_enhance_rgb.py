"""Diffuse gain and specular rendering of the colour forms on the GPU (rti_relight_lrgb_enhanced,
rti_relight_lrgb8_enhanced, rti_relight_rgb8_enhanced) against tests/enhance_rgb_ref.py (the header's
arithmetic op by op in NumPy) and against the entries the project already has.  Every comparison is exact: bytes, and
bit patterns of fp32 / int32 values.  The header fixes the fp64 value before conversion to the bit, so the integer
outputs are compared at every pixel.  One thing it does not fix is the payload of a NaN: against NumPy the NaN
positions must agree and every other element's bits; between two GPU results the raw bits are compared.

Sizes (test_gpu_rgb8.py's, for its reasons): a lane owns 4 pixels, a wave 256, a workgroup 1024, so 1 and 7 are a
partial wave on the one-pixel path (P % 4 != 0), 255 is one pixel short of a wave, 256 one full wave, 1023 and 1024
the workgroup seam, 1028 a second workgroup whose only wave holds 4 pixels (P % 4 == 0: full waves on the vector path
and a partial one), 3077 four workgroups with P % 4 != 0.  Inputs run 16-byte aligned and 4 bytes off (the byte blocks
1 byte off), LRGB maps in both layouts, every output between guard elements."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import rti
from enhance_rgb_ref import (convert, kinds_of, lrgb8_enhanced_ref, lrgb_enhanced_ref, peaked_rgb8, rgb8_enhanced_ref,
                             dequantise_lrgb_ref)
from lrgb_ref import mixed_lrgb
from rgb8_ref import LUMA, luminance

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 255, 256, 1023, 1024, 1028, 3077]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]
DIRS = [(0.3, -0.45), (0.8, 0.75), (0.0, 0.0)]  # inside the disc, outside it (lw = 0), the pole
SETTINGS = ([("diffuse_gain", dict(gain=g)) for g in (0.0, 1.0, 3.5)]
            + [("specular", dict(kd=0.4, ks=150.0, exp=e)) for e in (1, 75, 255)])
RUNS = [(lu, lv, mode, kw) for lu, lv in DIRS for mode, kw in SETTINGS]
UNIT_WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
L_SPEC = rti._lib.RTI_ENHANCE_SPECULAR  # a mode as its RTI_ENHANCE_* value


def name_of(dt):
    return str(dt).replace("torch.", "")


def on_device(cuda, a, offset=0):
    """The host array on the device as it is laid out, starting `offset` bytes into a 16-byte aligned buffer."""
    t = torch.as_tensor(np.array(a, order="C"), device=cuda)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    pad = offset // t.element_size()
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=cuda)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset and v.is_contiguous()
    return v


def guarded(cuda, n, dtype, offset=0):
    """(buffer, view of n elements, lead, fill) with at least 16 guard elements on both sides; the view starts
    `offset` bytes past a 16-byte boundary."""
    fill = 77 if dtype == torch.uint8 else -7
    buf = torch.full((n + 48,), fill, dtype=dtype, device=cuda)
    lead = 16 + offset // buf.element_size()
    assert buf[lead:].data_ptr() % 16 == offset
    return buf, buf[lead:lead + n], lead, fill


def guards_untouched(buf, lead, n, fill):
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + n:] == fill).all())


def bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def render(cuda, launch, P, dt, out_offset=0):
    """launch(out [P, 3]) between guards -> a clone of the image, the guards checked."""
    buf, view, lead, fill = guarded(cuda, 3 * P, dt, out_offset)
    launch(view.view(P, 3))
    assert guards_untouched(buf, lead, 3 * P, fill), dt
    return view.view(P, 3).clone()


def is_the_reference(got, ref64, dt):
    """got [P, 3] on the device against the fp64 reference image converted as the header converts it."""
    got, want = got.cpu().numpy(), convert(ref64, name_of(dt))
    if dt != torch.float32:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def has_every_kind(kinds, P):
    """The luminance kinds of a case, from the reference alone: interior maxima, maxima outside the disc and pixels
    without a maximum whenever the map has 7 pixels or more."""
    return P < 7 or {0, 1, 2} <= set(kinds.tolist())


# ---- the cases: computed once, shared and never written ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lrgb_case(P):
    m = mixed_lrgb(P, 1000 + P)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def lrgb_refs(P):
    m = lrgb_case(P)
    return [lrgb_enhanced_ref(m, lu, lv, mode, **kw) for lu, lv, mode, kw in RUNS]


@functools.lru_cache(maxsize=None)
def lrgb8_case(P):
    """mixed_lrgb(P, 5000 + P) as the host writer quantises it: the bytes and the header values of the .ptm file
    write_ptm writes -> (raw [P, 6], rgb [P, 3], qparams fp64 [13])."""
    m = mixed_lrgb(P, 5000 + P)
    with tempfile.TemporaryDirectory() as d:
        with np.errstate(all="ignore"):
            path = rti.write_ptm(os.path.join(d, "ref.ptm"), m.reshape(1, P, 9))
        q = rti.read_ptm(path, quantised=True)[1]
    out = (q.coef.numpy().reshape(P, 6).copy(), q.rgb.numpy().reshape(P, 3).copy(), q.qparams.numpy().copy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lrgb8_refs(P):
    return [lrgb8_enhanced_ref(*lrgb8_case(P), lu, lv, mode, **kw) for lu, lv, mode, kw in RUNS]


@functools.lru_cache(maxsize=None)
def rgb8_refs(P, weights):
    raw, qp, _ = peaked_rgb8(P)
    return [rgb8_enhanced_ref(raw, qp, lu, lv, mode, weights=weights, **kw) for lu, lv, mode, kw in RUNS]


# ---- rti_relight_lrgb_enhanced -----------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_lrgb_is_the_reference(cuda, P, layout, offset):
    m = lrgb_case(P)
    kinds = kinds_of(m[:, :6])
    assert has_every_kind(kinds, P)
    if P >= 255:  # the fp32 map also has non-finite luminance rows and NaN chroma
        assert 4 in kinds and np.isnan(m[:, 6:]).any()
    md = on_device(cuda, np.ascontiguousarray(m.T) if layout == "planar" else m, offset)
    for (lu, lv, mode, kw), ref in zip(RUNS, lrgb_refs(P)):
        for dt in OUT_DTYPES:
            got = render(cuda, lambda o: rti.relight_lrgb_enhanced_into(md, lu, lv, mode, o, layout=layout, **kw), P, dt)
            assert is_the_reference(got, ref, dt), (lu, lv, mode, kw, dt)
        assert np.isnan(ref[kinds == 4]).all() and (P < 255 or np.isfinite(ref).any())


@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_lrgb_with_unit_chroma_is_relight_enhanced_of_the_luminance(cuda, P, layout):
    m = lrgb_case(P).copy()
    m[:, 6:] = 1.0
    assert has_every_kind(kinds_of(m[:, :6]), P)
    planar = layout == "planar"
    md = on_device(cuda, np.ascontiguousarray(m.T) if planar else m)
    lum = md[:6] if planar else md[:, :6].contiguous()
    for lu, lv, mode, kw in RUNS:
        for dt in OUT_DTYPES:
            got = rti.relight_lrgb_enhanced(md, lu, lv, mode, layout=layout, out_dtype=dt, **kw)
            want = rti.relight_enhanced(lum, lu, lv, mode, layout=layout, out_dtype=dt, **kw)
            assert got.shape == (P, 3) and want.shape == (P,)
            for c in range(3):
                assert torch.equal(bits(got[:, c]), bits(want)), (lu, lv, mode, kw, dt, c)


# ---- rti_relight_lrgb8_enhanced ----------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("P", SIZES)
def test_lrgb8_is_the_reference_and_the_fp32_entry_of_the_dequantised_map(cuda, P, offset):
    raw, rgb, qp = lrgb8_case(P)
    deq = dequantise_lrgb_ref(raw, rgb, qp)
    assert has_every_kind(kinds_of(deq[:, :6]), P) and np.isfinite(deq).all()
    c8, r8, qpd = on_device(cuda, raw, offset), on_device(cuda, rgb, offset), on_device(cuda, qp)
    q = rti.QuantisedLRGB(c8.clone(), r8.clone(), qpd)
    fp32 = rti.dequantise_lrgb(q)
    assert np.array_equal(fp32.cpu().numpy().view(np.uint32), deq.view(np.uint32))
    for (lu, lv, mode, kw), ref in zip(RUNS, lrgb8_refs(P)):
        for dt in OUT_DTYPES:
            got = render(cuda, lambda o: rti.relight_lrgb8_enhanced_into(c8, r8, qpd, lu, lv, mode, o, **kw), P, dt)
            assert is_the_reference(got, ref, dt), (lu, lv, mode, kw, dt)
            want = rti.relight_lrgb_enhanced(fp32, lu, lv, mode, out_dtype=dt, **kw)
            assert torch.equal(bits(got), bits(want)), (lu, lv, mode, kw, dt)
        assert P < 255 or bool(got.any())  # images, not black frames


# ---- rti_relight_rgb8_enhanced -----------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, (0.2, 0.5, 0.3)])
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("P", SIZES)
def test_rgb8_is_the_reference(cuda, P, offset, weights):
    raw, qp, deq = peaked_rgb8(P)
    kinds = kinds_of(luminance(deq, LUMA if weights is None else weights))
    assert has_every_kind(kinds, P) and 4 not in kinds
    c8, qpd = on_device(cuda, raw, offset), on_device(cuda, qp)
    for (lu, lv, mode, kw), ref in zip(RUNS, rgb8_refs(P, weights)):
        for dt in OUT_DTYPES:
            got = render(cuda, lambda o: rti.relight_rgb8_enhanced_into(c8, qpd, lu, lv, mode, o, weights=weights, **kw),
                         P, dt)
            assert is_the_reference(got, ref, dt), (lu, lv, mode, kw, dt)
        assert np.isfinite(ref).all()


@pytest.mark.parametrize("ch", [0, 1, 2])
@pytest.mark.parametrize("P", SIZES)
def test_rgb8_with_a_unit_weight_is_relight_enhanced_of_that_channel(cuda, P, ch):
    raw, qp, deq = peaked_rgb8(P)
    w = UNIT_WEIGHTS[ch]
    assert has_every_kind(kinds_of(luminance(deq, w)), P)
    q = rti.QuantisedRGB(on_device(cuda, raw), on_device(cuda, qp))
    chan = rti.dequantise_rgb(q)[ch].contiguous()
    for (lu, lv, mode, kw), ref in zip(RUNS, rgb8_refs(P, w)):
        for dt in OUT_DTYPES:
            got = rti.relight_rgb8_enhanced(q, lu, lv, mode, weights=w, out_dtype=dt, **kw)
            assert is_the_reference(got, ref, dt), (lu, lv, mode, kw, dt)
            want = rti.relight_enhanced(chan, lu, lv, mode, out_dtype=dt, **kw)
            assert torch.equal(bits(got[:, ch]), bits(want)), (lu, lv, mode, kw, dt)


# ---- the two paths -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [256, 1028])
def test_paths_agree_to_the_bit(cuda, P):
    """The same pixels through the vector path (everything aligned) and one pixel per lane (the input 4 bytes off,
    or the output off a lane's store)."""
    m = lrgb_case(P)
    raw, rgb, qp = lrgb8_case(P)
    praw, pqp, _ = peaked_rgb8(P)
    qpd, pqpd = on_device(cuda, qp), on_device(cuda, pqp)
    for dt in OUT_DTYPES:
        out_offs = (4, 8) if dt != torch.uint8 else (1, 2)
        for lu, lv, mode, kw in RUNS[:len(SETTINGS)]:
            for layout in ("pixel", "planar"):
                laid = np.ascontiguousarray(m.T) if layout == "planar" else m

                def lrgb(in_off, out_off):
                    md = on_device(cuda, laid, in_off)
                    return bits(render(cuda, lambda o: rti.relight_lrgb_enhanced_into(md, lu, lv, mode, o, layout=layout,
                                                                                      **kw), P, dt, out_off))
                ref = lrgb(0, 0)
                for in_off, out_off in ((4, 0), (8, 0), (0, out_offs[0]), (0, out_offs[1])):
                    assert torch.equal(lrgb(in_off, out_off), ref), (layout, dt, mode, in_off, out_off)

            def lrgb8(c_off, r_off, out_off):
                c8, r8 = on_device(cuda, raw, c_off), on_device(cuda, rgb, r_off)
                return bits(render(cuda, lambda o: rti.relight_lrgb8_enhanced_into(c8, r8, qpd, lu, lv, mode, o, **kw),
                                   P, dt, out_off))
            ref = lrgb8(0, 0, 0)
            for offs in ((4, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, out_offs[0]), (0, 0, out_offs[1])):
                assert torch.equal(lrgb8(*offs), ref), (dt, mode, offs)

            def rgb8(in_off, out_off):
                c8 = on_device(cuda, praw, in_off)
                return bits(render(cuda, lambda o: rti.relight_rgb8_enhanced_into(c8, pqpd, lu, lv, mode, o, **kw), P, dt,
                                   out_off))
            ref = rgb8(0, 0)
            for in_off, out_off in ((1, 0), (4, 0), (0, out_offs[0]), (0, out_offs[1])):
                assert torch.equal(rgb8(in_off, out_off), ref), (dt, mode, in_off, out_off)


# ---- the Python layer, ops, graphs -------------------------------------------------------------------------------

def test_api_shapes_and_refusals(cuda):
    H, W = 12, 21
    m = torch.as_tensor(mixed_lrgb(H * W, 5).reshape(H, W, 9), device=cuda)
    ql = rti.quantise_lrgb(m)
    raw, qp, _ = peaked_rgb8(H * W)
    qr = rti.QuantisedRGB(on_device(cuda, raw.reshape(3, H, W, 6)), on_device(cuda, qp))
    for dt in OUT_DTYPES:
        for out in (rti.relight_lrgb_enhanced(m, 0.3, -0.45, "specular", kd=0.4, ks=150, exp=75, out_dtype=dt),
                    rti.relight_lrgb_enhanced(m.permute(2, 0, 1).contiguous(), 0.3, -0.45, "diffuse_gain", gain=3.5,
                                              layout="planar", out_dtype=dt),
                    rti.relight_lrgb8_enhanced(ql, 0.3, -0.45, "diffuse_gain", gain=3.5, out_dtype=dt),
                    rti.relight_rgb8_enhanced(qr, 0.3, -0.45, L_SPEC, kd=0.4, ks=150, exp=75, out_dtype=dt,
                                              weights=(0.2, 0.5, 0.3))):
            assert out.shape == (H, W, 3) and out.dtype == dt and out.device == m.device
    assert rti.relight_lrgb_enhanced(m.reshape(H * W, 9), 0.3, -0.45, "specular").shape == (H * W, 3)
    pl = rti.relight_lrgb_enhanced(m.permute(2, 0, 1).contiguous(), 0.3, -0.45, "specular", ks=9.0, exp=3, layout="planar")
    px = rti.relight_lrgb_enhanced(m, 0.3, -0.45, "specular", ks=9.0, exp=3)
    assert torch.equal(bits(pl), bits(px))
    with pytest.raises(ValueError, match="mode"):
        rti.relight_lrgb_enhanced(m, 0.1, 0.2, "glossy")
    with pytest.raises(ValueError, match="gain"):
        rti.relight_lrgb8_enhanced(ql, 0.1, 0.2, "diffuse_gain", gain=-1.0)
    with pytest.raises(ValueError, match="spec_exp"):
        rti.relight_rgb8_enhanced(qr, 0.1, 0.2, "specular", exp=256)
    with pytest.raises(ValueError, match="light"):
        rti.relight_rgb8_enhanced(qr, float("nan"), 0.2, "specular")
    with pytest.raises(ValueError, match="weights"):
        rti.relight_rgb8_enhanced(qr, 0.1, 0.2, "specular", weights=(1.0, 2.0))
    with pytest.raises(ValueError, match="weight"):
        rti.relight_rgb8_enhanced(qr, 0.1, 0.2, "specular", weights=(1.0, float("inf"), 0.0))
    for call in (lambda dt: rti.relight_lrgb_enhanced(m, 0.1, 0.2, "specular", out_dtype=dt),
                 lambda dt: rti.relight_lrgb8_enhanced(ql, 0.1, 0.2, "specular", out_dtype=dt),
                 lambda dt: rti.relight_rgb8_enhanced(qr, 0.1, 0.2, "specular", out_dtype=dt)):
        with pytest.raises(ValueError, match="out_dtype"):
            call(torch.float64)
    with pytest.raises(ValueError, match="terms"):
        rti.relight_lrgb_enhanced(m[..., :8].contiguous(), 0.1, 0.2, "specular")
    with pytest.raises(ValueError):
        rti.relight_lrgb_enhanced(m.half(), 0.1, 0.2, "specular")
    with pytest.raises(ValueError, match="QuantisedLRGB"):
        rti.relight_lrgb8_enhanced(m, 0.1, 0.2, "specular")
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb8_enhanced(qr.to("cpu"), 0.1, 0.2, "specular")
    out = torch.empty((H * W, 3), device=cuda)
    with pytest.raises(ValueError, match="lrgb"):
        rti.relight_lrgb_enhanced_into(m[:, ::2], 0.1, 0.2, "specular", out)  # not dense
    with pytest.raises(ValueError, match="out"):
        rti.relight_lrgb_enhanced_into(m, 0.1, 0.2, "specular", out[:-1])
    with pytest.raises(ValueError, match="out"):
        rti.relight_lrgb8_enhanced_into(ql.coef, ql.rgb, ql.qparams, 0.1, 0.2, "specular", out.double())
    with pytest.raises(ValueError, match="rgb8"):
        rti.relight_lrgb8_enhanced_into(ql.coef, ql.rgb[:-1].contiguous(), ql.qparams, 0.1, 0.2, "specular", out)
    with pytest.raises(ValueError, match="qparams"):
        rti.relight_rgb8_enhanced_into(qr.coef, ql.qparams, 0.1, 0.2, "specular", out)
    with pytest.raises(ValueError, match="coef8"):
        rti.relight_rgb8_enhanced_into(qr.coef[:, :, ::2], qr.qparams, 0.1, 0.2, "specular", out)  # not dense



@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P = 1028
    m = lrgb_case(P)
    md = on_device(cuda, np.ascontiguousarray(m.T) if planar else m)
    raw, rgb, qp = lrgb8_case(P)
    c8, r8, qpd = on_device(cuda, raw), on_device(cuda, rgb), on_device(cuda, qp)
    praw, pqp, _ = peaked_rgb8(P)
    pc8, pqpd = on_device(cuda, praw), on_device(cuda, pqp)
    ql, qr = rti.QuantisedLRGB(c8, r8, qpd), rti.QuantisedRGB(pc8, pqpd)
    layout = "planar" if planar else "pixel"
    checks = ("test_schema", "test_faketensor")
    modes = {"diffuse_gain": rti._lib.RTI_ENHANCE_DIFFUSE_GAIN, "specular": L_SPEC}
    for lu, lv, mode, kw in (RUNS[2], RUNS[4]):
        mid, g, kd, ks, e = modes[mode], kw.get("gain", 1.0), kw.get("kd", 1.0), kw.get("ks", 0.0), kw.get("exp", 1)
        for dt in OUT_DTYPES:
            pairs = ((torch.ops.rti.relight_lrgb_enhanced, (md, lu, lv, mid, g, kd, ks, e, planar, dt),
                      rti.relight_lrgb_enhanced(md, lu, lv, mode, layout=layout, out_dtype=dt, **kw)),
                     (torch.ops.rti.relight_lrgb8_enhanced, (c8, r8, qpd, lu, lv, mid, g, kd, ks, e, dt),
                      rti.relight_lrgb8_enhanced(ql, lu, lv, mode, out_dtype=dt, **kw)),
                     (torch.ops.rti.relight_rgb8_enhanced, (pc8, pqpd, lu, lv, mid, g, kd, ks, e, [0.2, 0.5, 0.3], dt),
                      rti.relight_rgb8_enhanced(qr, lu, lv, mode, out_dtype=dt, weights=(0.2, 0.5, 0.3), **kw)))
            for op, args, want in pairs:
                got = op(*args)
                assert got.shape == want.shape == (P, 3) and got.dtype == dt and torch.equal(bits(got), bits(want))
                if not planar:
                    torch.library.opcheck(op.default, args, test_utils=checks)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_lrgb_enhanced(md, 0.1, 0.2, L_SPEC, 1.0, 1.0, 0.0, 1, not planar, torch.float32)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_lrgb8_enhanced(c8, r8[:-1], qpd, 0.1, 0.2, L_SPEC, 1.0, 1.0, 0.0, 1, torch.float32)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_rgb8_enhanced(pc8[:2], pqpd, 0.1, 0.2, L_SPEC, 1.0, 1.0, 0.0, 1, None, torch.float32)


def test_graph_capture_replays_the_eager_bits(cuda):
    """The three entries on one stream, captured once (a single chain, no parallel branches) and replayed once on
    other data: everything travels as kernel arguments."""
    P = 1028
    first, second = lrgb_case(P), mixed_lrgb(P, 77)
    md = on_device(cuda, first)
    ql = rti.quantise_lrgb(on_device(cuda, mixed_lrgb(P, 5000 + P)))
    praw, pqp, _ = peaked_rgb8(P)
    qr = rti.QuantisedRGB(on_device(cuda, praw), on_device(cuda, pqp))
    outs = [torch.empty((P, 3), dtype=dt, device=cuda) for dt in OUT_DTYPES]

    def chain():
        rti.relight_lrgb_enhanced_into(md, 0.3, -0.45, "specular", outs[0], kd=0.4, ks=150.0, exp=75)
        rti.relight_lrgb8_enhanced_into(ql.coef, ql.rgb, ql.qparams, 0.3, -0.45, "diffuse_gain", outs[1], gain=3.5)
        rti.relight_rgb8_enhanced_into(qr.coef, qr.qparams, 0.3, -0.45, "specular", outs[2], kd=0.4, ks=150.0, exp=75)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    md.copy_(torch.as_tensor(second, device=cuda))
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = [o.clone() for o in outs]
    eager = [rti.relight_lrgb_enhanced(md, 0.3, -0.45, "specular", kd=0.4, ks=150.0, exp=75, out_dtype=OUT_DTYPES[0]),
             rti.relight_lrgb8_enhanced(ql, 0.3, -0.45, "diffuse_gain", gain=3.5, out_dtype=OUT_DTYPES[1]),
             rti.relight_rgb8_enhanced(qr, 0.3, -0.45, "specular", kd=0.4, ks=150.0, exp=75, out_dtype=OUT_DTYPES[2])]
    for r, e in zip(replayed, eager):
        assert torch.equal(bits(r), bits(e)) and bool(r.any())
    assert is_the_reference(replayed[0], lrgb_enhanced_ref(second, 0.3, -0.45, "specular", kd=0.4, ks=150.0, exp=75),
                            OUT_DTYPES[0])
