"""Specular enhancement of HSH maps under a normal map on the GPU (rti_hsh_specular.hip) against
tests/hsh_specular_ref.py (the header's arithmetic line by line in NumPy), and bit for bit against the entries that
already exist: relight_hsh8 / relight_rgb / relight, shade_normals and dequantise_hsh.

Sizes: one pixel per lane, 64 per wave, 256 per workgroup.  1 and 63 are a partial wave, 64 a full one, 65 a full wave
and one pixel, 255 / 256 / 257 the workgroup seam, 260 a second workgroup with P % 4 == 0 (uint8 rows leave as dwords),
1279 five workgroups less a pixel.  Every size runs with 16-byte aligned tensors (the staged paths) and with tensors
offset by one element (coefficients, bytes, normals and uint8 output then go per lane); every output lies between
guard elements."""
import numpy as np
import pytest
import torch

import rti
from hsh_specular_ref import (DIRS, KS, NEAR_INTEGER_CAP, PARAMS, SIZES, convert, excluded, maps, normals, reference,
                              specular_ref)

pytestmark = pytest.mark.gpu

OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]
LAYOUTS = ["pixel", "planar"]
LU, LV = (list(x) for x in zip(*DIRS))
FORMS = [("bytes", "pixel"), ("rgb", "pixel"), ("rgb", "planar"), ("grey", "pixel"), ("grey", "planar")]
REF_OF = {"bytes": "bytes", "rgb": "fp32", "grey": "grey"}


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


def launch(cuda, d, P, k, form, nl, params, dt, offset, lu=LU, lv=LV):
    """One launch through the _into forms into a guarded output -> the device image [E, P, C]."""
    source, cl = form
    kd, ks, exp = params
    C, E = (1 if source == "grey" else 3), len(lu)
    buf, view, lead, fill = guarded(cuda, E * P * C, dt, offset)
    kw = dict(basis=f"hsh{k}", kd=kd, ks=ks, exp=exp, normal_layout=nl)
    if source == "bytes":
        rti.relight_hsh8_specular_into(*d["bytes"], d["n", nl], lu, lv, view, **kw)
    else:
        rti.relight_hsh_specular_into(d[source, cl], d["n", nl], lu, lv, view, layout=cl, **kw)
    assert guards_untouched(buf, lead, E * P * C, fill), (form, nl, params, dt, offset)
    return view.view(E, P, C)


def check_against_reference(got, ref, dt, what):
    """got [E, P, C] of the device against the fp64 reference: item 1 of the module's contract."""
    got = got.cpu().numpy()
    assert got.shape == ref.shape, what
    if dt == torch.float32:
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what
        ok = ~np.isnan(ref)
        err = np.abs(got.astype(np.float64)[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1.0)
        worst = float(err.max()) if err.size else 0.0
        assert worst <= 1e-6, (what, worst)
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
    one launch, every parameter tuple and output type."""
    worst = 0.0
    for offset in (False, True):
        d = prepare(cuda, P, k, offset)
        for form in FORMS:
            for nl in LAYOUTS:
                for params in PARAMS:
                    ref = reference(P, k, REF_OF[form[0]], params)
                    for dt in OUT_DTYPES:
                        got = launch(cuda, d, P, k, form, nl, params, dt, offset)
                        worst = max(worst, check_against_reference(got, ref, dt, (form, nl, params, dt, offset)))
    print(f"k={k} P={P}: worst |got - ref| / max(|ref|, 1) of the fp32 images {worst:.3g}")


# ---- 2. bit identities against entries that already exist ------------------------------------------------------------

@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_paths_layouts_and_the_bytes_agree_to_the_bit(cuda, k, P):
    """Aligned and offset tensors, planar and pixel-major inputs give the same bits, and the image from the bytes is
    that of the dequantised maps, every output type."""
    params = PARAMS[2]
    d = {off: prepare(cuda, P, k, off) for off in (False, True)}
    raw, qp = d[False]["bytes"]
    deq = rti.dequantise_hsh(rti.QuantisedHSH(raw.clone(), qp, f"hsh{k}"))  # [3, P, k]
    dd = dict(d[False])
    dd["rgb", "pixel"] = deq
    for dt in OUT_DTYPES:
        for source in ("bytes", "rgb", "grey"):
            first = bits(launch(cuda, d[False], P, k, (source, "pixel"), "pixel", params, dt, False))
            for off in (False, True):
                for cl in (LAYOUTS if source != "bytes" else ["pixel"]):
                    for nl in LAYOUTS:
                        again = bits(launch(cuda, d[off], P, k, (source, cl), nl, params, dt, off))
                        assert torch.equal(first, again), (dt, source, off, cl, nl)
        from_bytes = bits(launch(cuda, d[False], P, k, ("bytes", "pixel"), "pixel", params, dt, False))
        from_maps = bits(launch(cuda, dd, P, k, ("rgb", "pixel"), "pixel", params, dt, False))
        assert torch.equal(from_bytes, from_maps), dt


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_plain_parameters_give_the_existing_entries(cuda, k, P):
    """kd = 1, ks = 0 with finite normals is relight_hsh8 / relight_rgb / relight as values (a -0 becomes +0); kd = 0
    with finite coefficients and one map is shade_normals(kd = 0) bit for bit, NaN normals included."""
    basis = f"hsh{k}"
    finite = np.nan_to_num(normals(P), nan=0.0)
    d = prepare(cuda, P, k, False, n=finite)
    raw, qp = d["bytes"]
    want = {"bytes": rti.relight_hsh8(rti.QuantisedHSH(raw, qp, basis), LU, LV),
            "rgb": rti.relight_rgb(d["rgb", "pixel"], LU, LV, basis),
            "grey": rti.relight(d["grey", "pixel"], np.array(LU), np.array(LV), basis=basis).unsqueeze(-1)}
    for source in want:
        got = launch(cuda, d, P, k, (source, "pixel"), "pixel", (1.0, 0.0, 1), torch.float32, False)
        assert np.array_equal(got.cpu().numpy(), want[source].cpu().numpy()), source
    d = prepare(cuda, P, k, False)
    for params in ((0.0, 150.25, 75), (0.0, 150.0, 1)):
        got = launch(cuda, d, P, k, ("grey", "pixel"), "pixel", params, torch.float32, False)
        for e, (lu, lv) in enumerate(DIRS):
            shaded = rti.shade_normals(d["n", "pixel"], lu, lv, kd=0.0, ks=params[1], exp=params[2])
            assert torch.equal(bits(got[e, :, 0]), bits(shaded)), (params, e)


@pytest.mark.parametrize("k", KS)
def test_sixteen_directions_in_one_launch_are_sixteen_launches(cuda, k):
    from relight_ref import dirs

    P, params = 257, PARAMS[2]
    lu, lv = (x.tolist() for x in dirs(16))
    d = prepare(cuda, P, k, False)
    for form in (("bytes", "pixel"), ("rgb", "pixel"), ("grey", "planar")):
        for dt in OUT_DTYPES:
            one = launch(cuda, d, P, k, form, "pixel", params, dt, False, lu, lv)
            each = torch.cat([launch(cuda, d, P, k, form, "pixel", params, dt, False, lu[e:e + 1], lv[e:e + 1])
                              for e in range(16)])
            assert one.shape[0] == 16 and torch.equal(bits(one), bits(each)), (form, dt)
    with pytest.raises(ValueError, match="16 directions"):
        launch(cuda, d, P, k, ("rgb", "pixel"), "pixel", params, torch.float32, False, lu + [0.0], lv + [0.0])


# ---- 3. non-finite inputs --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [63, 65, 255, 260, 1279])
@pytest.mark.parametrize("k", KS)
def test_non_finite_coefficients_and_normals(cuda, k, P):
    """mixed_hsh maps (NaN, ±inf) under normals with NaNs: the NaN / +inf / -inf pattern of the fp32 image is the
    reference's.  (The sizes below 256 carry the mixed patterns; the others are NaN throughout.)"""
    for offset in (False, True):
        d = prepare(cuda, P, k, offset, "mixed")
        for params in PARAMS:
            ref = reference(P, k, "mixed", params)
            for cl in LAYOUTS:
                got = launch(cuda, d, P, k, ("rgb", cl), "pixel", params, torch.float32, offset).cpu().numpy()
                for test in (np.isnan, np.isposinf, np.isneginf):
                    assert np.array_equal(test(got), test(ref)), (offset, params, cl, test.__name__)
    # from 256 pixels on mixed_hsh makes term 7 NaN everywhere, and with it every value
    assert np.isnan(ref).any() and (P >= 256 or np.isinf(reference(P, k, "mixed", PARAMS[1])).any())


# ---- 4. shapes, ops, graphs ------------------------------------------------------------------------------------------

def test_api_shapes_and_refusals(cuda):
    H, W, k = 18, 71, 16
    P = H * W
    c3 = torch.as_tensor(maps(P, k, "fp32").reshape(3, H, W, k), device=cuda)
    n = torch.as_tensor(normals(P).reshape(H, W, 3), device=cuda)
    q = rti.quantise_hsh(c3)
    kw = dict(kd=0.4, ks=150.0, exp=75)
    rgb = rti.relight_hsh_specular(c3, n, LU, LV, **kw)
    assert rgb.shape == (3, H, W, 3) and rgb.dtype == torch.float32
    one = rti.relight_hsh_specular(c3, n, 0.3, -0.45, out_dtype=torch.uint8, **kw)
    assert one.shape == (H, W, 3) and one.dtype == torch.uint8
    grey = rti.relight_hsh_specular(c3[0], n, LU, LV, **kw)
    assert grey.shape == (3, H, W) and torch.equal(bits(grey), bits(rgb[..., 0]))
    assert rti.relight_hsh_specular(c3[0], n, 0.3, -0.45, out_dtype=torch.int32, **kw).shape == (H, W)
    planar = rti.relight_hsh_specular(c3.permute(0, 3, 1, 2).contiguous(), n.permute(2, 0, 1).contiguous(), LU, LV,
                                      layout="planar", normal_layout="planar", **kw)
    assert torch.equal(bits(planar), bits(rgb))
    flat = rti.relight_hsh_specular(c3.reshape(3, P, k), n.reshape(P, 3), LU, LV, **kw)
    assert flat.shape == (3, P, 3) and torch.equal(bits(flat), bits(rgb.reshape(3, P, 3)))
    c9 = c3[..., :9].contiguous()
    assert rti.relight_hsh_specular(c9, n, 0.3, -0.45, "hsh9", **kw).shape == (H, W, 3)
    b8 = rti.relight_hsh8_specular(q, n, LU, LV, **kw)
    assert b8.shape == (3, H, W, 3) and b8.dtype == torch.float32
    assert torch.equal(bits(b8), bits(rti.relight_hsh_specular(rti.dequantise_hsh(q), n, LU, LV, **kw)))
    assert rti.relight_hsh8_specular(q, n, 0.3, -0.45, out_dtype=torch.uint8, **kw).shape == (H, W, 3)
    ref = specular_ref(maps(P, k, "fp32"), normals(P), LU, LV, k, 0.4, 150.0, 75)
    check_against_reference(rgb.reshape(3, P, 3), ref, torch.float32, "api")
    with pytest.raises(ValueError, match="match"):
        rti.relight_hsh_specular(c3, n[:, :-1].contiguous(), 0.3, -0.45)
    with pytest.raises(ValueError, match="match"):
        rti.relight_hsh8_specular(q, n.reshape(W, H, 3), 0.3, -0.45)
    with pytest.raises(ValueError, match="terms"):
        rti.relight_hsh_specular(c3, n, 0.3, -0.45, "hsh9")
    with pytest.raises(ValueError):
        rti.relight_hsh_specular(c3, n, 0.3, -0.45, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        rti.relight_hsh_specular(c3, n.double(), 0.3, -0.45)
    with pytest.raises(ValueError, match="spec_exp"):
        rti.relight_hsh_specular(c3, n, 0.3, -0.45, exp=256)
    with pytest.raises(ValueError, match="out"):
        rti.relight_hsh_specular_into(c3, n, 0.3, -0.45, torch.empty((1, P, 1), device=cuda))
    with pytest.raises(NotImplementedError, match="relight_rgb_enhanced"):
        rti.relight_hsh_specular(c3[..., :6].contiguous(), n, 0.3, -0.45, "ptm")


@pytest.mark.parametrize("k", KS)
def test_torch_ops(cuda, k):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P, (kd, ks, exp) = 260, PARAMS[2]
    d = prepare(cuda, P, k, False)
    luv = torch.as_tensor(np.array(DIRS))
    checks = ("test_schema", "test_faketensor")
    for dt in OUT_DTYPES:
        for planar in (False, True):
            cl = nl = "planar" if planar else "pixel"
            for source in ("rgb", "grey"):
                args = (d[source, cl], d["n", nl], luv, k, kd, ks, exp, planar, planar, dt)
                got = torch.ops.rti.relight_hsh_specular(*args)
                want = launch(cuda, d, P, k, (source, cl), nl, PARAMS[2], dt, False)
                assert got.dtype == dt and got.shape == ((3, P, 3) if source == "rgb" else (3, P))
                assert torch.equal(bits(got), bits(want.view(got.shape))), (dt, planar, source)
                torch.library.opcheck(torch.ops.rti.relight_hsh_specular.default, args, test_utils=checks)
            args = (*d["bytes"], d["n", nl], luv, kd, ks, exp, planar, dt)
            got = torch.ops.rti.relight_hsh8_specular(*args)
            want = launch(cuda, d, P, k, ("bytes", "pixel"), nl, PARAMS[2], dt, False)
            assert got.dtype == dt and got.shape == (3, P, 3) and torch.equal(bits(got), bits(want))
            torch.library.opcheck(torch.ops.rti.relight_hsh8_specular.default, args, test_utils=checks)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_hsh_specular(d["rgb", "pixel"], d["n", "planar"], luv, k)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_hsh8_specular(d["bytes"][0][:, :2], d["bytes"][1], d["n", "pixel"], luv)
    with pytest.raises(NotImplementedError):
        torch.ops.rti.relight_hsh_specular(d["rgb", "pixel"], d["n", "pixel"], luv, 6)


def test_graph_capture_replays_the_eager_bits(cuda):
    """One relight_hsh8_specular_into and one relight_hsh_specular_into call, captured once (a single chain, no
    parallel branches; the directions are part of the capture) and replayed once on other normals."""
    P, k, params = 1279, 16, PARAMS[2]
    d = prepare(cuda, P, k, False)
    n = d["n", "pixel"].clone()
    out8 = torch.empty((3, P, 3), dtype=torch.uint8, device=cuda)
    out32 = torch.empty((3, P, 3), dtype=torch.float32, device=cuda)
    kw = dict(basis="hsh16", kd=params[0], ks=params[1], exp=params[2])

    def chain():
        rti.relight_hsh8_specular_into(*d["bytes"], n, LU, LV, out8, **kw)
        rti.relight_hsh_specular_into(d["rgb", "pixel"], n, LU, LV, out32, **kw)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    n.copy_(torch.as_tensor(normals(1279)[::-1].copy(), device=cuda))
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = out8.clone(), out32.clone()
    chain()
    assert torch.equal(replayed[0], out8) and torch.equal(bits(replayed[1]), bits(out32))
    assert bool(replayed[0].any())


# ---- 5. end to end on a file -----------------------------------------------------------------------------------------

def test_end_to_end_on_a_file(cuda, tmp_path):
    """write_rti -> read_rti(quantised=True) -> hsh8_normals -> normals_unsharp -> relight_hsh8_specular(uint8) on a
    32 x 48 object, against the NumPy reference under the device's normals (item 1's rule as it stands) and against
    the composed route relight_hsh8 -> shade_normals(kd = 0) -> scale and add.  shade_normals rounds its highlight to
    fp32, so the composed value lies within ks·2^-24 of the fused one: the integer boundaries left out of that second
    comparison are those within 1e-6 + ks·2^-24 of it."""
    from unsharp_ref import NEAR_INTEGER

    H, W, k, (kd, ks, exp), (lu, lv) = 32, 48, 9, PARAMS[2], DIRS[1]
    P = H * W
    m = maps(P, k, "fp32").reshape(3, H, W, k)
    path = rti.write_rti(str(tmp_path / "object.rti"), m, "hsh9")
    basis, q = rti.read_rti(path, quantised=True)
    q = q.to(cuda)
    n = rti.normals_unsharp(rti.hsh8_normals(q), 2.0, 1.5)
    got = rti.relight_hsh8_specular(q, n, lu, lv, kd=kd, ks=ks, exp=exp, out_dtype=torch.uint8)
    assert basis == "hsh9" and got.shape == (H, W, 3) and got.dtype == torch.uint8 and n.shape == (H, W, 3)
    got = got.cpu().numpy().reshape(P, 3)
    finite = torch.isfinite(n).all(-1).reshape(P).cpu().numpy()
    assert finite.mean() > 0.9
    deq = rti.dequantise_hsh(q).cpu().numpy().reshape(3, P, k)
    ref = specular_ref(deq, n.cpu().numpy().reshape(P, 3), [lu], [lv], k, kd, ks, exp)
    check_against_reference(torch.as_tensor(got[None]), ref, torch.uint8, "file")
    plain = rti.relight_hsh8(q, lu, lv).double().reshape(P, 3)
    shine = rti.shade_normals(n, lu, lv, kd=0.0, ks=ks, exp=exp).double().reshape(P, 1)
    composed = (kd * plain + shine).cpu().numpy()
    near = np.abs(composed - np.rint(composed)) < NEAR_INTEGER + ks * 2.0 ** -24
    skip = (near & (np.rint(composed) != 0.0)) | ~finite[:, None]
    print(f"left out of the composed comparison: {skip.mean():.4f} of the elements")
    assert skip[finite].mean() <= NEAR_INTEGER_CAP
    assert np.array_equal(got[~skip], convert(composed, "uint8")[~skip])
    assert got.min() < 255 and got.max() > 0  # an image, not a saturated frame
