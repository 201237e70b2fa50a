"""8-bit RGB PTMs on the GPU (rti_rgb8.hip) against tests/rgb8_ref.py (the header's arithmetic op by op in NumPy) for
the 12 header doubles, the bytes and the dequantised maps, against rti.relight of the dequantised maps for the
images and against rti.normals of their fp32 luminance for the normals.  Every comparison but the accuracy bound is
exact: bytes, and bit patterns of fp32 / fp64 / int32 values.

Sizes: a lane owns 4 pixels, a wave 256, a workgroup 1024, so 1 and 7 are a partial wave on the one-pixel path
(P % 4 != 0), 255 is one pixel short of a wave, 256 one full wave, 1023 and 1024 the workgroup seam, 1028 a second
workgroup whose only wave holds 4 pixels (P % 4 == 0: a full wave on the vector path and a partial one), 3077 four
workgroups with P % 4 != 0.  The quantiser also runs BIG = 768·1024 + 1024 + 76 = 787532 pixels: the extremes' grid
is capped at 768 workgroups of 1024 pixels, so two workgroups fold a second chunk there and the tail kernel folds
768 partials, three per lane.  Maps run in both layouts, dense and with a padded channel stride, 16-byte aligned and
4 bytes off; the bytes 8-byte aligned and off it; every output between guard elements."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rti
from normals_ref import peaked_coef
from rgb8_ref import (LUMA, finite_rgb, host_dequantise, host_qparams, host_quantise, mixed_rgb, straddling_rgb)
from rti import _lib as L
from rti import api

pytestmark = pytest.mark.gpu

BIG = 768 * 1024 + 1024 + 76
SIZES = [1, 7, 255, 256, 1023, 1024, 1028, 3077]
ES = [1, 3]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]


@functools.lru_cache(maxsize=None)
def dirs(E):
    """(0.3, -0.45), then (0.8, 0.75) with lu² + lv² > 1, then the pole, then seeded ones."""
    rng = np.random.default_rng(65)
    lu = np.concatenate([[0.3, 0.8, 0.0], rng.uniform(-0.7, 0.7, 5)])[:E]
    lv = np.concatenate([[-0.45, 0.75, 0.0], rng.uniform(-0.7, 0.7, 5)])[:E]
    return lu, lv


@functools.lru_cache(maxsize=None)
def case(P):
    """(maps [3, P, 6] fp32, qparams fp64 [12], raw [3, P, 6], dequantised [3, P, 6]) of the host -- computed once,
    shared and never written."""
    m = mixed_rgb(P, 7000 + P)
    qp = host_qparams(m)
    raw = host_quantise(m, qp)
    deq = host_dequantise(raw, qp)
    for a in (m, qp, raw, deq):
        a.setflags(write=False)
    return m, qp, raw, deq


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
    return t if t.dtype == torch.uint8 else t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def run_quantiser(cuda, m, layout="pixel", pad=0, offset=0, byte_offset=0):
    """rti_rgb8_qparams + rti_rgb8_quantise through the C ABI (the channel stride is an argument only there):
    the three maps `pad` elements apart beyond dense and `offset` bytes off 16, outputs between guards (the bytes
    `byte_offset` off 16), the workspace holding NaN bit patterns -> (qparams [12], coef8 [3, P, 6]) on the host."""
    P = m.shape[1]
    laid = np.ascontiguousarray(m.transpose(0, 2, 1)) if layout == "planar" else m
    stride = 6 * P + pad
    host = np.full((3, stride), -1e30, np.float32)  # the padding would wreck the extremes if it were read
    host[:, :6 * P] = laid.reshape(3, -1)
    md = on_device(cuda, host, offset)
    ws = torch.full((rti.rgb8_qparams_workspace(P),), 0xFF, dtype=torch.uint8, device=cuda)
    qbuf, qp, qlead, qfill = guarded(cuda, 12, torch.float64)
    cbuf, c8, clead, cfill = guarded(cuda, 18 * P, torch.uint8, byte_offset)
    lib, cl, sp = rti.load(), api._layout_id(layout), api._stream_of(md)
    L.check(lib.rti_rgb8_qparams(api._vp(md), cl, stride if pad else 0, P, api._vp(ws), api._vp(qp), sp), "qparams")
    L.check(lib.rti_rgb8_quantise(api._vp(md), cl, stride if pad else 0, P, api._vp(qp), api._vp(c8), sp), "quantise")
    assert guards_untouched(qbuf, qlead, 12, qfill) and guards_untouched(cbuf, clead, 18 * P, cfill)
    return qp.cpu().numpy(), c8.cpu().numpy().reshape(3, P, 6)


VARIANTS = {"dense": dict(), "padded": dict(pad=8), "padded off the vector": dict(pad=6),
            "offset": dict(offset=4, byte_offset=4)}


# ---- rti_rgb8_qparams, rti_rgb8_quantise, dequantise_rgb ---------------------------------------------------------

@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES + [BIG])
def test_quantiser_is_the_hosts(cuda, P, layout, variant):
    m, want_qp, want_raw, want_deq = case(P)
    qp, c8 = run_quantiser(cuda, m, layout, **VARIANTS[variant])
    print(f"P={P}: scale {qp[:6]} bias {qp[6:]}")
    assert same_bits(qp, want_qp)
    assert np.array_equal(c8, want_raw)
    assert want_qp[5] == 1.0 and want_qp[11] == 0.0 and (c8[..., 5] == 12).all()  # the constant plane
    if P >= 256:
        assert want_qp[4] == 1.0 and want_qp[10] == 0.0 and not c8[..., 4].any()    # the all-NaN plane
        live = [2, 3]  # the planes that straddle zero: the one-sided ones are clipped by the format
        inside = float(((want_raw[..., live] > 0) & (want_raw[..., live] < 255)).mean())
        print(f"P={P}: {inside:.3f} of the live planes' bytes strictly inside 1..254")
        assert inside > 0.9
    if P >= 8:  # the planted values: NaN -> bias, +inf -> 255, -inf -> 0
        assert c8[0, 2, 1] == qp[7] and c8[1, 3, 2] == 255 and c8[2, 4, 3] == 0
    q = rti.QuantisedRGB(torch.as_tensor(c8, device=cuda), torch.as_tensor(qp, device=cuda))
    deq = rti.dequantise_rgb(q)
    assert deq.shape == (3, P, 6) and deq.dtype == torch.float32
    assert same_bits(deq.cpu().numpy(), want_deq)


SEAMS = [(0, -1), (3, 4), (255, 256), (1023, 1024)]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("seam", SEAMS)
def test_extremes_at_the_seams(cuda, seam, swap):
    """A 2100-pixel map (two full workgroups and a 52-pixel tail) with the extremes of every plane at chosen
    pixels, each in another channel."""
    P = 2100
    m = finite_rgb(P, 77).copy()
    lo_px, hi_px = (seam[1], seam[0]) if swap else seam
    for j in range(6):
        plane = m[..., j]
        m[j % 3, lo_px, j] = plane.min() - 100.0 - 7 * j
        m[(j + 1) % 3, hi_px, j] = plane.max() + 100.0 + 11 * j
    want_qp = host_qparams(m)
    want_raw = host_quantise(m, want_qp)
    for layout in ("pixel", "planar"):
        for variant in ("dense", "offset"):  # the vector path and the one-pixel one
            qp, c8 = run_quantiser(cuda, m, layout, **VARIANTS[variant])
            assert same_bits(qp, want_qp), (layout, variant, qp, want_qp)
            assert np.array_equal(c8, want_raw), (layout, variant)


def test_all_nan_maps(cuda):
    m = np.full((3, 1300, 6), np.nan, np.float32)
    for layout in ("pixel", "planar"):
        qp, c8 = run_quantiser(cuda, m, layout)
        assert same_bits(qp, np.float64([1.0] * 6 + [0.0] * 6)) and not c8.any()


# ---- rti_relight_rgb8 --------------------------------------------------------------------------------------------

def device_q(cuda, P, offset=0):
    """The host's quantised map of case(P) on the device (these tests do not lean on the device quantiser)."""
    _, qp, raw, _ = case(P)
    return on_device(cuda, raw, offset), on_device(cuda, qp)


def relight_into(cuda, c8, qp, E, dt, offset=0):
    P = c8.numel() // 18
    luv = torch.as_tensor(np.stack(dirs(E), -1), device=cuda)
    n = E * P * 3
    buf, view, lead, fill = guarded(cuda, n, dt, offset)
    got = rti.relight_rgb8_into(c8, qp, luv, view.view(E, P, 3))
    assert guards_untouched(buf, lead, n, fill), (E, dt)
    return got


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("P", SIZES)
def test_relight_rgb8_is_relight_of_the_dequantised_maps(cuda, P, offset):
    c8, qp = device_q(cuda, P, offset)
    fp32 = rti.dequantise_rgb(rti.QuantisedRGB(c8.clone(), qp))
    assert fp32.shape == (3, P, 6) and bool(torch.isfinite(fp32).all())  # NaN and inf were stored as finite bytes
    for E in ES:
        lu, lv = dirs(E)
        for dt in OUT_DTYPES:
            got = relight_into(cuda, c8, qp, E, dt, offset)
            want = torch.stack([rti.relight(fp32[c], lu, lv, out_dtype=dt) for c in range(3)], -1)
            assert got.shape == want.shape == (E, P, 3)
            assert torch.equal(bits(got), bits(want)), (E, dt)
            assert P < 255 or bool(got.any()), (E, dt)  # images, not black frames


@pytest.mark.parametrize("P", [256, 1028])
def test_paths_agree_to_the_bit(cuda, P):
    """The same pixels through the vector path (aligned) and one pixel per lane (maps 4 bytes off or a channel
    stride that is no multiple of 4; bytes 1 or 4 bytes off 8; outputs 4 or 1 bytes off)."""
    m = case(P)[0]
    for layout in ("pixel", "planar"):
        a = run_quantiser(cuda, m, layout)
        for kw in (dict(offset=4), dict(pad=6), dict(byte_offset=1), dict(byte_offset=4)):
            b = run_quantiser(cuda, m, layout, **kw)
            assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]), (layout, kw)
    w = torch.tensor([0.2, 0.5, 0.3], dtype=torch.float32)
    for dt in OUT_DTYPES:
        c8, qp = device_q(cuda, P)
        ref = bits(relight_into(cuda, c8, qp, 3, dt))
        for in_off, out_off in ((1, 0), (4, 0), (0, 4 if dt != torch.uint8 else 1), (0, 8 if dt != torch.uint8 else 2)):
            c8o, _ = device_q(cuda, P, in_off)
            assert torch.equal(bits(relight_into(cuda, c8o, qp, 3, dt, out_off)), ref), (dt, in_off, out_off)
    c8, qp = device_q(cuda, P)
    for nl in ("pixel", "planar"):
        outs = []
        for in_off, out_off in ((0, 0), (1, 0), (0, 4)):
            c8o, _ = device_q(cuda, P, in_off)
            nbuf, n, nlead, nfill = guarded(cuda, 3 * P, torch.float32, out_off)
            kbuf, kind, klead, kfill = guarded(cuda, P, torch.uint8, out_off // 4)
            pbuf, peak, plead, pfill = guarded(cuda, P, torch.float32, out_off)
            rti.rgb8_normals_into(c8o, qp, n, kind, peak, normal_layout=nl, weights=w.tolist())
            assert guards_untouched(nbuf, nlead, 3 * P, nfill) and guards_untouched(kbuf, klead, P, kfill)
            assert guards_untouched(pbuf, plead, P, pfill)
            outs.append((bits(n).clone(), kind.clone(), bits(peak).clone()))
        for o in outs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(o, outs[0])), nl


# ---- rti_rgb8_normals --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def peaked_rgb(P):
    """Three channels of one surface: interior maxima, maxima outside the disc and minima in equal parts, the
    channels 0.8, 1.0 and 1.15 times the biquadratic plus a little noise -> fp32 [3, P, 6]."""
    rng = np.random.default_rng(900 + P)
    n = [P - 2 * (P // 3), P // 3, P // 3]
    a = np.concatenate([peaked_coef(rng, n[0], 0.0, 0.9)[0], peaked_coef(rng, n[1], 1.1, 2.0)[0],
                        peaked_coef(rng, n[2], 0.0, 0.9, sign=1.0)[0]])
    a = a[rng.permutation(P)]
    m = np.stack([g * a for g in (0.8, 1.0, 1.15)]) + rng.normal(0, 0.05, (3, P, 6))
    m = m.astype(np.float32)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("weights", [None, (0.2, 0.5, 0.3)])
@pytest.mark.parametrize("nl", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
def test_normals_from_the_bytes_are_normals_of_the_luminance(cuda, P, nl, weights):
    m = peaked_rgb(P)
    qp = host_qparams(m)
    q = rti.QuantisedRGB(torch.as_tensor(host_quantise(m, qp), device=cuda), torch.as_tensor(qp, device=cuda))
    n, kind, peak = rti.rgb8_normals(q, normal_layout=nl, weights=weights, return_kind=True, return_peak=True)
    d = rti.dequantise_rgb(q)
    w = torch.tensor(LUMA if weights is None else weights, dtype=torch.float32, device=cuda)
    t0 = d[0] * w[0]
    t1 = d[1] * w[1]
    rg = t0 + t1
    t2 = d[2] * w[2]
    lum = rg + t2  # (w0·r + w1·g) + w2·b, every operation a separate fp32 kernel
    wn, wkind, wpeak = rti.normals(lum, normal_layout=nl, return_kind=True, return_peak=True)
    assert n.shape == wn.shape == ((P, 3) if nl == "pixel" else (3, P)) and kind.shape == peak.shape == (P,)
    assert torch.equal(bits(n), bits(wn)) and torch.equal(kind, wkind) and torch.equal(bits(peak), bits(wpeak))
    only = rti.rgb8_normals(q, normal_layout=nl, weights=weights)
    assert torch.equal(bits(only), bits(n))
    kinds = set(kind.cpu().numpy().tolist())
    print(f"P={P}: kinds {sorted(kinds)}")
    assert 4 not in kinds and bool(torch.isfinite(n).all())
    if P >= 255:
        assert kinds == {0, 1, 2}


# ---- accuracy ----------------------------------------------------------------------------------------------------

def test_accuracy_against_the_unquantised_maps(cuda):
    """Every plane straddles zero, so the format clips nothing: a dequantised coefficient lies within 1.0·scale_j
    of the original (half a step from rounding the value, at most half a step from rounding the bias), and the
    image within Σ_j scale_j·|b_j(lu, lv)| + 1e-4·max(|L_ref|, 255) of rti.relight of the original maps."""
    P = 3077
    m = straddling_rgb(P, 31)
    md = torch.as_tensor(m, device=cuda)
    q = rti.quantise_rgb(md)
    scale = q.scale
    assert ((m.min(axis=(0, 1)) < 0) & (m.max(axis=(0, 1)) > 0)).all()
    steps = np.abs(rti.dequantise_rgb(q).cpu().numpy().astype(np.float64) - m.astype(np.float64)) / scale
    print(f"max |dequantised - original| in steps per plane: {steps.max(axis=(0, 1))}")
    assert (steps <= 1.0).all()
    lu, lv = dirs(8)
    got = rti.relight_rgb8(q, lu, lv).double()
    want = torch.stack([rti.relight(md[c], lu, lv) for c in range(3)], -1).double()
    b = np.abs(rti.basis_eval(lu, lv, "ptm"))  # [E, 6] fp64
    bound = torch.as_tensor(b @ scale, device=cuda)[:, None, None] + 1e-4 * want.abs().clamp(min=255.0)
    err = (got - want).abs()
    print(f"max error / bound per direction {(err / bound).amax(dim=(1, 2)).cpu().numpy()}")
    assert bool((err <= bound).all())
    assert bool((err.amax(dim=(1, 2)) > 0).all())  # the comparison is of a quantised map


# ---- the Python layer, files, ops, graphs ------------------------------------------------------------------------

def test_api_shapes_and_refusals(cuda):
    H, W = 12, 21
    m = torch.as_tensor(mixed_rgb(H * W, 5).reshape(3, H, W, 6), device=cuda)
    q = rti.quantise_rgb(m)
    assert isinstance(q, rti.QuantisedRGB) and q.shape == (H, W) and q.device == m.device
    assert q.coef.shape == (3, H, W, 6) and q.qparams.shape == (12,) and q.qparams.dtype == torch.float64
    qp = rti.quantise_rgb(m.permute(0, 3, 1, 2).contiguous(), layout="planar")
    assert torch.equal(qp.coef, q.coef) and torch.equal(bits(qp.qparams), bits(q.qparams))
    flat = rti.quantise_rgb(m.reshape(3, H * W, 6))
    assert flat.shape == (H * W,) and torch.equal(flat.coef, q.coef.reshape(3, -1, 6))
    out = rti.relight_rgb8(q, *dirs(2))
    assert out.shape == (2, H, W, 3) and out.dtype == torch.float32
    one = rti.relight_rgb8(q, 0.3, -0.45, out_dtype=torch.uint8)
    assert one.shape == (H, W, 3) and one.dtype == torch.uint8
    assert rti.relight_rgb8(flat, 0.3, -0.45).shape == (H * W, 3)
    n, kind = rti.rgb8_normals(q, return_kind=True)
    assert n.shape == (H, W, 3) and kind.shape == (H, W) and kind.dtype == torch.uint8
    assert rti.rgb8_normals(q, normal_layout="planar").shape == (3, H, W)
    assert rti.rgb8_normals(flat, return_peak=True)[1].shape == (H * W,)
    d = rti.dequantise_rgb(q)
    assert d.shape == (3, H, W, 6) and d.dtype == torch.float32 and d.device == m.device
    host = q.to("cpu")
    assert host.device.type == "cpu" and torch.equal(host.coef, q.coef.cpu())
    assert torch.equal(bits(rti.dequantise_rgb(host)), bits(d.cpu()))  # the same arithmetic on either device
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb8(host, 0.1, 0.2)
    with pytest.raises(ValueError, match="terms"):
        rti.quantise_rgb(m[..., :5].contiguous())
    with pytest.raises(ValueError):
        rti.quantise_rgb(m[:2])
    with pytest.raises(ValueError):
        rti.quantise_rgb(m.half())
    with pytest.raises(ValueError):
        rti.relight_rgb8(q, 0.1, 0.2, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="layout"):
        rti.rgb8_normals(q, normal_layout="rows")
    with pytest.raises(ValueError, match="weights"):
        rti.rgb8_normals(q, weights=(1.0, 2.0))
    with pytest.raises(ValueError, match="weight"):
        rti.rgb8_normals(q, weights=(1.0, float("nan"), 0.0))
    with pytest.raises(ValueError, match="workspace"):
        rti.rgb8_qparams_into(m, torch.empty(8, dtype=torch.uint8, device=cuda), q.qparams)
    with pytest.raises(ValueError, match="qparams"):
        rti.rgb8_quantise_into(m, q.qparams.float(), q.coef)
    with pytest.raises(ValueError, match="coef8"):
        rti.rgb8_quantise_into(m, q.qparams, q.coef[:, :-1].contiguous())
    with pytest.raises(ValueError, match="coef8"):
        rti.relight_rgb8_into(q.coef[:, :, ::2], q.qparams, torch.zeros((1, 2), dtype=torch.float64, device=cuda),
                              torch.empty((1, H * ((W + 1) // 2), 3), device=cuda))  # not dense
    with pytest.raises(ValueError):
        rti.relight_rgb8_into(q.coef, q.qparams, torch.zeros((1, 2), device=cuda),
                              torch.empty((1, H * W, 3), device=cuda))
    with pytest.raises(ValueError, match="normals"):
        rti.rgb8_normals_into(q.coef, q.qparams, torch.empty((H * W, 2), device=cuda))


@pytest.mark.parametrize("H,W", [(24, 20), (5, 7)])
def test_device_and_host_write_the_same_file(cuda, tmp_path, H, W):
    m = mixed_rgb(H * W, 300 + H).reshape(3, H, W, 6)
    md = torch.as_tensor(m, device=cuda)
    q = rti.quantise_rgb(md)
    host_path = rti.write_ptm(str(tmp_path / "host.ptm"), md.cpu(), format="rgb")
    dev_path = rti.write_ptm(str(tmp_path / "device.ptm"), q)
    assert open(dev_path, "rb").read() == open(host_path, "rb").read()
    fmt, back = rti.read_ptm(dev_path)
    assert fmt == "rgb" and same_bits(rti.dequantise_rgb(q.with_file_scales()).cpu().numpy(), back)
    loaded = rti.read_ptm8(dev_path)[1].to(cuda)
    assert torch.equal(loaded.coef, q.coef) and torch.equal(bits(loaded.qparams), bits(q.with_file_scales().qparams))


def test_end_to_end_from_a_fit(cuda, tmp_path):
    """fit (colour stack) -> quantise_rgb -> file -> read_ptm8 -> the GPU: images and normals of the loaded object
    are those of the in-memory one with the header's nine-digit scales, to the bit."""
    from rti_oracle import synth_dirs, synth_intensities

    lu, lv = synth_dirs(12, 0)
    I = np.stack([synth_intensities(24, 20, lu, lv, seed=s) for s in range(3)])
    coef = rti.fit(torch.as_tensor(I, device=cuda).float(), lu, lv)
    assert coef.shape == (3, 24, 20, 6) and bool(torch.isfinite(coef).all())
    q = rti.quantise_rgb(coef)
    path = rti.write_ptm(str(tmp_path / "object.ptm"), q)
    fmt, loaded = rti.read_ptm8(path)
    loaded, mem = loaded.to(cuda), q.with_file_scales()
    assert fmt == "rgb" and loaded.shape == (24, 20) and torch.equal(loaded.coef, q.coef)
    for dt in OUT_DTYPES:
        a, b = rti.relight_rgb8(loaded, *dirs(3), out_dtype=dt), rti.relight_rgb8(mem, *dirs(3), out_dtype=dt)
        assert a.shape == (3, 24, 20, 3) and torch.equal(bits(a), bits(b)) and bool(a.any())
    a = rti.rgb8_normals(loaded, return_kind=True, return_peak=True)
    b = rti.rgb8_normals(mem, return_kind=True, return_peak=True)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    assert same_bits(rti.dequantise_rgb(loaded).cpu().numpy(), rti.read_ptm(path)[1])


@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P = 1028
    m = case(P)[0]
    md = on_device(cuda, np.ascontiguousarray(m.transpose(0, 2, 1)) if planar else m)
    q = rti.quantise_rgb(md, layout="planar" if planar else "pixel")
    c8, qp = torch.ops.rti.rgb8_quantise(md, planar)
    assert c8.shape == (3, P, 6) and qp.shape == (12,) and c8.dtype == torch.uint8 and qp.dtype == torch.float64
    assert torch.equal(c8, q.coef) and torch.equal(bits(qp), bits(q.qparams))
    checks = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.rti.rgb8_quantise.default, (md, planar), test_utils=checks)
    lu, lv = dirs(2)
    luv = torch.as_tensor(np.stack([lu, lv], -1))
    for dt in OUT_DTYPES:
        got = torch.ops.rti.relight_rgb8(c8, qp, luv, dt)
        want = rti.relight_rgb8(q, lu, lv, out_dtype=dt)
        assert got.shape == want.shape == (2, P, 3) and got.dtype == dt and torch.equal(bits(got), bits(want))
        torch.library.opcheck(torch.ops.rti.relight_rgb8.default, (c8, qp, luv, dt), test_utils=checks)
    for nplanar in (False, True):
        n, kind, peak = torch.ops.rti.rgb8_normals(c8, qp, nplanar, [0.2, 0.5, 0.3])
        want = rti.rgb8_normals(q, normal_layout="planar" if nplanar else "pixel", weights=(0.2, 0.5, 0.3),
                                return_kind=True, return_peak=True)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip((n, kind, peak), want))
        torch.library.opcheck(torch.ops.rti.rgb8_normals.default, (c8, qp, nplanar, None), test_utils=checks)
    with pytest.raises(ValueError):
        torch.ops.rti.rgb8_quantise(md.transpose(1, 2).contiguous(), planar)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_rgb8(c8[:2], qp, luv, torch.float32)
    with pytest.raises(ValueError):
        torch.ops.rti.rgb8_normals(c8[..., :5], qp, False, None)


def test_graph_capture_replays_the_eager_bytes(cuda):
    """rgb8_qparams_into, rgb8_quantise_into, relight_rgb8_into and rgb8_normals_into on one stream, captured once
    (a single chain, no parallel branches) and replayed once on other data."""
    P = 3076
    first, second = mixed_rgb(P, 3), mixed_rgb(P, 9)
    md = on_device(cuda, first)
    luv = torch.as_tensor(np.stack(dirs(2), -1), device=cuda)
    ws = torch.empty(rti.rgb8_qparams_workspace(P), dtype=torch.uint8, device=cuda)
    qp = torch.empty(12, dtype=torch.float64, device=cuda)
    c8 = torch.empty((3, P, 6), dtype=torch.uint8, device=cuda)
    out = torch.empty((2, P, 3), dtype=torch.uint8, device=cuda)
    n = torch.empty((P, 3), dtype=torch.float32, device=cuda)
    kind = torch.empty(P, dtype=torch.uint8, device=cuda)

    def chain():
        rti.rgb8_qparams_into(md, ws, qp)
        rti.rgb8_quantise_into(md, qp, c8)
        rti.relight_rgb8_into(c8, qp, luv, out)
        rti.rgb8_normals_into(c8, qp, n, kind)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    md.copy_(torch.as_tensor(second, device=cuda))
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = [t.clone() for t in (qp, c8, out, n, kind)]
    q = rti.quantise_rgb(md)
    assert torch.equal(bits(replayed[0]), bits(q.qparams)) and torch.equal(replayed[1], q.coef)
    assert torch.equal(replayed[2], rti.relight_rgb8(q, *dirs(2), out_dtype=torch.uint8)) and bool(replayed[2].any())
    wn, wkind = rti.rgb8_normals(q, return_kind=True)
    assert torch.equal(bits(replayed[3]), bits(wn)) and torch.equal(replayed[4], wkind)
