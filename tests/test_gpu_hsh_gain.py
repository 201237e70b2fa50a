"""Diffuse gain for HSH maps under a normal map on the GPU (rti_hsh_gain.hip) against tests/hsh_gain_ref.py (the
header's arithmetic line by line in NumPy), and bit for bit against the entries that already exist: relight_hsh8 /
relight_rgb / relight and dequantise_hsh.

Sizes: one pixel per lane, 64 per wave, 256 per workgroup.  1 and 63 are a partial wave, 64 a full one, 65 a full wave
and one pixel, 255 / 256 / 257 the workgroup seam, 260 a second workgroup with P % 4 == 0 (uint8 rows leave as dwords),
1279 five workgroups less a pixel.  Every size runs with 16-byte aligned tensors (the staged paths) and with tensors
offset by one element (coefficients, bytes, normals and uint8 output then go per lane); every output lies between
guard elements.  The helpers are tests/test_gpu_hsh_specular.py's, restated."""
import numpy as np
import pytest
import torch

import rti
from hsh_gain_ref import (DIRS, GAINS, KS, NEAR_INTEGER_CAP, SIZES, convert, excluded, gain_ref, maps, normals,
                          reference)

pytestmark = pytest.mark.gpu

OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]
LAYOUTS = ["pixel", "planar"]
LU, LV = (list(x) for x in zip(*DIRS))
FORMS = [("bytes", "pixel"), ("rgb", "pixel"), ("rgb", "planar"), ("grey", "pixel"), ("grey", "planar")]
REF_OF = {"bytes": "bytes", "rgb": "fp32", "grey": "grey"}
F32_BOUND = 1e-6  # of max(|ref|, 1): tests/test_gpu_hsh_specular.py's


def on_device(cuda, a, offset):
    """The host array on the device as it is laid out; offset: it starts one element into a 16-byte aligned buffer."""
    t = torch.as_tensor(np.array(a, order="C"), device=cuda)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def guarded(cuda, n, dtype, offset):
    """(buffer, view of n elements, lead, fill) with at least 16 guard elements on both sides; the view is 16-byte
    aligned, or with offset one element off."""
    fill = 77 if dtype == torch.uint8 else -7
    buf = torch.full((n + 48,), fill, dtype=dtype, device=cuda)
    lead = 16 + (1 if offset else 0)
    return buf, buf[lead:lead + n], lead, fill


def guards_untouched(buf, lead, n, fill):
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + n:] == fill).all())


def bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def prepare(cuda, P, k, offset, source="fp32", n=None):
    """The device tensors of a case: {("rgb" | "grey", layout), ("n", layout), "bytes": (coef8, qparams)}."""
    m = maps(P, k, source)
    d = {}
    for cl in LAYOUTS:
        arr = m if cl == "pixel" else m.transpose(0, 2, 1)
        d["rgb", cl] = on_device(cuda, arr, offset)
        d["grey", cl] = on_device(cuda, arr[0], offset)
    n = normals(P) if n is None else n
    d["n", "pixel"], d["n", "planar"] = on_device(cuda, n, offset), on_device(cuda, n.T, offset)
    if source == "fp32":
        raw, qp, _ = maps(P, k, "bytes")
        d["bytes"] = (on_device(cuda, raw, offset), on_device(cuda, qp, False))
    return d


def launch(cuda, d, P, k, form, nl, gain, dt, offset, lu=LU, lv=LV):
    """One launch through the _into forms into a guarded output -> the device image [E, P, C]."""
    source, cl = form
    C, E = (1 if source == "grey" else 3), len(lu)
    buf, view, lead, fill = guarded(cuda, E * P * C, dt, offset)
    kw = dict(basis=f"hsh{k}", gain=gain, normal_layout=nl)
    if source == "bytes":
        rti.relight_hsh8_gain_into(*d["bytes"], d["n", nl], lu, lv, view, **kw)
    else:
        rti.relight_hsh_gain_into(d[source, cl], d["n", nl], lu, lv, view, layout=cl, **kw)
    assert guards_untouched(buf, lead, E * P * C, fill), (form, nl, gain, dt, offset)
    return view.view(E, P, C)


def check_against_reference(got, ref, dt, what):
    """got [E, P, C] of the device against the fp64 reference: item 1 of the module's contract."""
    got = got.cpu().numpy()
    assert got.shape == ref.shape, what
    if dt == torch.float32:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what
        ok = np.isfinite(ref)
        assert np.array_equal(got[~ok & ~np.isnan(ref)], ref[~ok & ~np.isnan(ref)]), what  # ±inf as they are
        err = np.abs(got.astype(np.float64)[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1.0)
        worst = float(err.max()) if err.size else 0.0
        assert worst <= F32_BOUND, (what, worst)
        return worst
    for e in range(ref.shape[0]):
        skip, share = excluded(ref[e])
        assert share <= NEAR_INTEGER_CAP, (what, e, share)
        want = convert(ref[e], str(dt).replace("torch.", ""))
        assert np.array_equal(got[e][~skip], want[~skip]), (what, e)
    return 0.0


# ---- 1. against the NumPy reference ----------------------------------------------------------------------------------

@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_against_the_reference(cuda, k, P):
    """Bytes, three fp32 maps and one, both coefficient and normal layouts, aligned and offset, the three directions in
    one launch, every gain and output type."""
    worst = 0.0
    for offset in (False, True):
        d = prepare(cuda, P, k, offset)
        for form in FORMS:
            for nl in LAYOUTS:
                for gain in GAINS:
                    ref = reference(P, k, REF_OF[form[0]], gain)
                    for dt in OUT_DTYPES:
                        got = launch(cuda, d, P, k, form, nl, gain, dt, offset)
                        worst = max(worst, check_against_reference(got, ref, dt, (form, nl, gain, dt, offset)))
    print(f"k={k} P={P}: worst |got - ref| / max(|ref|, 1) of the fp32 images {worst:.3g}")


# ---- 2. bit identities against entries that already exist ------------------------------------------------------------

@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_paths_layouts_and_the_bytes_agree_to_the_bit(cuda, k, P):
    """Aligned and offset tensors, planar and pixel-major inputs give the same bits, and the image from the bytes is
    that of the dequantised maps, every output type."""
    gain = 2.5
    d = {off: prepare(cuda, P, k, off) for off in (False, True)}
    raw, qp = d[False]["bytes"]
    deq = rti.dequantise_hsh(rti.QuantisedHSH(raw.clone(), qp, f"hsh{k}"))  # [3, P, k]
    dd = dict(d[False])
    dd["rgb", "pixel"] = deq
    for dt in OUT_DTYPES:
        for source in ("bytes", "rgb", "grey"):
            first = bits(launch(cuda, d[False], P, k, (source, "pixel"), "pixel", gain, dt, False))
            for off in (False, True):
                for cl in (LAYOUTS if source != "bytes" else ["pixel"]):
                    for nl in LAYOUTS:
                        again = bits(launch(cuda, d[off], P, k, (source, cl), nl, gain, dt, off))
                        assert torch.equal(first, again), (dt, source, off, cl, nl)
        from_bytes = bits(launch(cuda, d[False], P, k, ("bytes", "pixel"), "pixel", gain, dt, False))
        from_maps = bits(launch(cuda, dd, P, k, ("rgb", "pixel"), "pixel", gain, dt, False))
        assert torch.equal(from_bytes, from_maps), dt


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_unit_gain_is_the_plain_relight(cuda, k, P):
    """gain = 1 with finite normals and finite coefficients is relight_hsh8 / relight_rgb / relight bit for bit."""
    basis = f"hsh{k}"
    finite = np.nan_to_num(normals(P), nan=0.0)
    d = prepare(cuda, P, k, False, n=finite)
    raw, qp = d["bytes"]
    want = {"bytes": rti.relight_hsh8(rti.QuantisedHSH(raw, qp, basis), LU, LV),
            "rgb": rti.relight_rgb(d["rgb", "pixel"], LU, LV, basis),
            "grey": rti.relight(d["grey", "pixel"], np.array(LU), np.array(LV), basis=basis).unsqueeze(-1)}
    for source in want:
        got = launch(cuda, d, P, k, (source, "pixel"), "pixel", 1.0, torch.float32, False)
        assert torch.equal(bits(got), bits(want[source].reshape(got.shape))), source


@pytest.mark.parametrize("k", KS)
def test_a_light_at_the_normal_gives_the_anchor(cuda, k):
    """With direction e set to pixel p_e's (n_x, n_y) -- a seeded pixel of each workgroup, the pole (3, 131) and the
    two rim normals (11, 12) among them -- pixel p_e of image e is rti.relight's value there bit for bit for every
    gain, and gain = 0 gives that value at p_e under every direction to 1e-6."""
    P, basis = 1279, f"hsh{k}"
    pixels = [0, 3, 11, 12, 64, 131, 255, 256, 1278]
    n = normals(P)
    assert not np.isnan(n[pixels]).any()
    lu, lv = [float(n[p, 0]) for p in pixels], [float(n[p, 1]) for p in pixels]
    idx = torch.arange(len(pixels))
    d = prepare(cuda, P, k, False)
    for source in ("bytes", "rgb", "grey"):
        if source == "bytes":
            m = rti.dequantise_hsh(rti.QuantisedHSH(d["bytes"][0].clone(), d["bytes"][1], basis))
        else:
            m = d[source, "pixel"].reshape(-1, P, k)
        # [E, P, C]: the plain relight of every channel at the nine directions
        plain = torch.stack([rti.relight(m[c].contiguous(), np.array(lu), np.array(lv), basis=basis) for c in range(m.shape[0])], -1)
        anchor = plain[idx, pixels]  # [E, C]: pixel p_e under its own direction
        for gain in GAINS:
            got = launch(cuda, d, P, k, (source, "pixel"), "pixel", gain, torch.float32, False, lu, lv)
            assert torch.equal(bits(got[idx, pixels]), bits(anchor)), (source, gain)
        flat = launch(cuda, d, P, k, (source, "pixel"), "pixel", 0.0, torch.float32, False, lu, lv)[:, pixels]  # [E', E, C]
        err = (flat.double() - anchor.double()[None]).abs() / anchor.double().abs().clamp(min=1.0)[None]
        assert float(err.max()) <= 1e-6, (source, float(err.max()))


# ---- 3. several directions -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_sixteen_directions_in_one_launch_are_sixteen_launches(cuda, k):
    from relight_ref import dirs

    P, gain = 257, 2.5
    lu, lv = (x.tolist() for x in dirs(16))
    d = prepare(cuda, P, k, False)
    for form in (("bytes", "pixel"), ("rgb", "pixel"), ("grey", "planar")):
        for dt in OUT_DTYPES:
            one = launch(cuda, d, P, k, form, "pixel", gain, dt, False, lu, lv)
            each = torch.cat([launch(cuda, d, P, k, form, "pixel", gain, dt, False, lu[e:e + 1], lv[e:e + 1])
                              for e in range(16)])
            assert one.shape[0] == 16 and torch.equal(bits(one), bits(each)), (form, dt)
    with pytest.raises(ValueError, match="16 directions"):
        launch(cuda, d, P, k, ("rgb", "pixel"), "pixel", gain, torch.float32, False, lu + [0.0], lv + [0.0])


# ---- 4. non-finite inputs --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [63, 65, 255, 260, 1279])
@pytest.mark.parametrize("k", KS)
def test_non_finite_coefficients_and_normals(cuda, k, P):
    """mixed_hsh maps (NaN, ±inf) under normals with NaNs: the NaN / +inf / -inf pattern of the fp32 image is the
    reference's, and so are the finite values.  (The sizes below 256 carry the mixed patterns; the others are NaN
    throughout.)"""
    for offset in (False, True):
        d = prepare(cuda, P, k, offset, "mixed")
        for gain in GAINS:
            ref = reference(P, k, "mixed", gain)
            for cl in LAYOUTS:
                got = launch(cuda, d, P, k, ("rgb", cl), "pixel", gain, torch.float32, offset)
                for test in (np.isnan, np.isposinf, np.isneginf):
                    assert np.array_equal(test(got.cpu().numpy()), test(ref)), (offset, gain, cl, test.__name__)
                check_against_reference(got, ref, torch.float32, (offset, gain, cl))
    assert np.isnan(ref).any()


# ---- 5. shapes, ops, graphs ------------------------------------------------------------------------------------------

def test_api_shapes_and_refusals(cuda):
    H, W, k = 18, 71, 16
    P = H * W
    c3 = torch.as_tensor(maps(P, k, "fp32").reshape(3, H, W, k), device=cuda)
    n = torch.as_tensor(normals(P).reshape(H, W, 3), device=cuda)
    q = rti.quantise_hsh(c3)
    kw = dict(gain=2.5)
    rgb = rti.relight_hsh_gain(c3, n, LU, LV, **kw)
    assert rgb.shape == (3, H, W, 3) and rgb.dtype == torch.float32
    one = rti.relight_hsh_gain(c3, n, 0.3, -0.45, out_dtype=torch.uint8, **kw)
    assert one.shape == (H, W, 3) and one.dtype == torch.uint8
    grey = rti.relight_hsh_gain(c3[0], n, LU, LV, **kw)
    assert grey.shape == (3, H, W) and torch.equal(bits(grey), bits(rgb[..., 0]))
    assert rti.relight_hsh_gain(c3[0], n, 0.3, -0.45, out_dtype=torch.int32, **kw).shape == (H, W)
    planar = rti.relight_hsh_gain(c3.permute(0, 3, 1, 2).contiguous(), n.permute(2, 0, 1).contiguous(), LU, LV,
                                  layout="planar", normal_layout="planar", **kw)
    assert torch.equal(bits(planar), bits(rgb))
    flat = rti.relight_hsh_gain(c3.reshape(3, P, k), n.reshape(P, 3), LU, LV, **kw)
    assert flat.shape == (3, P, 3) and torch.equal(bits(flat), bits(rgb.reshape(3, P, 3)))
    c9 = c3[..., :9].contiguous()
    assert rti.relight_hsh_gain(c9, n, 0.3, -0.45, "hsh9", **kw).shape == (H, W, 3)
    b8 = rti.relight_hsh8_gain(q, n, LU, LV, **kw)
    assert b8.shape == (3, H, W, 3) and b8.dtype == torch.float32
    assert torch.equal(bits(b8), bits(rti.relight_hsh_gain(rti.dequantise_hsh(q), n, LU, LV, **kw)))
    assert rti.relight_hsh8_gain(q, n, 0.3, -0.45, out_dtype=torch.uint8, **kw).shape == (H, W, 3)
    ref = gain_ref(maps(P, k, "fp32"), normals(P), LU, LV, k, 2.5)
    check_against_reference(rgb.reshape(3, P, 3), ref, torch.float32, "api")
    with pytest.raises(ValueError, match="match"):
        rti.relight_hsh_gain(c3, n[:, :-1].contiguous(), 0.3, -0.45)
    with pytest.raises(ValueError, match="match"):
        rti.relight_hsh8_gain(q, n.reshape(W, H, 3), 0.3, -0.45)
    with pytest.raises(ValueError, match="terms"):
        rti.relight_hsh_gain(c3, n, 0.3, -0.45, "hsh9")
    with pytest.raises(ValueError):
        rti.relight_hsh_gain(c3, n, 0.3, -0.45, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        rti.relight_hsh_gain(c3, n.double(), 0.3, -0.45)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gain"):
            rti.relight_hsh_gain(c3, n, 0.3, -0.45, gain=bad)
        with pytest.raises(ValueError, match="gain"):
            rti.relight_hsh8_gain(q, n, 0.3, -0.45, gain=bad)
    with pytest.raises(ValueError, match="out"):
        rti.relight_hsh_gain_into(c3, n, 0.3, -0.45, torch.empty((1, P, 1), device=cuda))
    with pytest.raises(NotImplementedError, match="relight_rgb_enhanced"):
        rti.relight_hsh_gain(c3[..., :6].contiguous(), n, 0.3, -0.45, "ptm")


@pytest.mark.parametrize("k", KS)
def test_torch_ops(cuda, k):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P, gain = 260, 2.5
    d = prepare(cuda, P, k, False)
    luv = torch.as_tensor(np.array(DIRS))
    checks = ("test_schema", "test_faketensor")
    for dt in OUT_DTYPES:
        for planar in (False, True):
            cl = nl = "planar" if planar else "pixel"
            for source in ("rgb", "grey"):
                args = (d[source, cl], d["n", nl], luv, k, gain, planar, planar, dt)
                got = torch.ops.rti.relight_hsh_gain(*args)
                want = launch(cuda, d, P, k, (source, cl), nl, gain, dt, False)
                assert got.dtype == dt and got.shape == ((3, P, 3) if source == "rgb" else (3, P))
                assert torch.equal(bits(got), bits(want.view(got.shape))), (dt, planar, source)
                torch.library.opcheck(torch.ops.rti.relight_hsh_gain.default, args, test_utils=checks)
            args = (*d["bytes"], d["n", nl], luv, gain, planar, dt)
            got = torch.ops.rti.relight_hsh8_gain(*args)
            want = launch(cuda, d, P, k, ("bytes", "pixel"), nl, gain, dt, False)
            assert got.dtype == dt and got.shape == (3, P, 3) and torch.equal(bits(got), bits(want))
            torch.library.opcheck(torch.ops.rti.relight_hsh8_gain.default, args, test_utils=checks)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_hsh_gain(d["rgb", "pixel"], d["n", "planar"], luv, k)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_hsh8_gain(d["bytes"][0][:, :2], d["bytes"][1], d["n", "pixel"], luv)
    with pytest.raises(NotImplementedError):
        torch.ops.rti.relight_hsh_gain(d["rgb", "pixel"], d["n", "pixel"], luv, 6)


def test_graph_capture_replays_the_eager_bits(cuda):
    """One relight_hsh8_gain_into call, captured once (a single launch, no parallel branches; the directions and the
    gain are part of the capture) and replayed once on other normals."""
    P, k, gain = 1279, 16, 2.5
    d = prepare(cuda, P, k, False)
    n = d["n", "pixel"].clone()
    out8 = torch.empty((3, P, 3), dtype=torch.uint8, device=cuda)

    def call():
        rti.relight_hsh8_gain_into(*d["bytes"], n, LU, LV, out8, basis="hsh16", gain=gain)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        call()  # loads the kernel before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    n.copy_(torch.as_tensor(normals(1279)[::-1].copy(), device=cuda))
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = out8.clone()
    call()
    assert torch.equal(replayed, out8) and bool(replayed.any())


# ---- 6. end to end ---------------------------------------------------------------------------------------------------

def test_end_to_end_from_a_fit_through_a_file(cuda, tmp_path):
    """A 32 x 32 RGB Lambertian stack fitted with HSH-16 -> write_rti -> read_rti(quantised=True) -> hsh8_normals ->
    relight_hsh8_gain: gain = 1 is relight_hsh8 bit for bit, and under gain = 3 every finite pixel's deviation from
    its anchor (the gain = 0 image) is three times the gain = 1 deviation, to 1e-5 of max(|value|, 1)."""
    import rti_oracle as o

    H = W = 32
    lu, lv = o.synth_dirs(40, 1)
    lw = np.sqrt(np.maximum(0.0, 1.0 - lu.astype(np.float64) ** 2 - lv.astype(np.float64) ** 2))
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    tilt, az = np.radians(30.0 * np.sqrt(yy)), 2 * np.pi * xx + 0.1
    truth = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1)
    shade = np.maximum(0.0, np.einsum("nc,hwc->nhw", np.stack([lu, lv, lw], 1), truth))
    I = np.stack([a * shade for a in (200.0, 150.0, 100.0)]).astype(np.float32)
    coef = rti.fit(torch.tensor(I, device=cuda), lu, lv, basis="hsh16")
    path = rti.write_rti(str(tmp_path / "object.rti"), coef.cpu().numpy(), "hsh16")
    basis, q = rti.read_rti(path, quantised=True)
    q = q.to(cuda)
    n = rti.hsh8_normals(q)
    assert basis in ("hsh", "hsh16") and n.shape == (H, W, 3)
    unit = rti.relight_hsh8_gain(q, n, LU, LV, gain=1.0)
    finite = torch.isfinite(n).all(-1)
    assert float(finite.double().mean()) > 0.9
    plain = rti.relight_hsh8(q, LU, LV)
    assert unit.shape == plain.shape == (3, H, W, 3)
    assert torch.equal(bits(unit[:, finite]), bits(plain[:, finite]))
    anchor = rti.relight_hsh8_gain(q, n, LU, LV, gain=0.0).double()
    three = rti.relight_hsh8_gain(q, n, LU, LV, gain=3.0).double()
    dev1, dev3 = unit.double() - anchor, three - anchor
    err = ((dev3 - 3.0 * dev1).abs() / three.abs().clamp(min=1.0))[:, finite]
    print(f"worst |dev3 - 3 dev1| / max(|value|, 1): {float(err.max()):.3g}; largest gain = 1 deviation "
          f"{float(dev1[:, finite].abs().max()):.3g}")
    assert float(err.max()) <= 1e-5
    assert float(dev1[:, finite].abs().max()) > 1.0  # the lights are off the normals: there is something to multiply
    img = rti.relight_hsh8_gain(q, n, 0.3, -0.2, gain=3.0, out_dtype=torch.uint8)
    assert img.shape == (H, W, 3) and img.dtype == torch.uint8 and int(img.max()) > int(img.min())
