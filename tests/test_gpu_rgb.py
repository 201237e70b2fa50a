"""Three fp32 RGB maps rendered in one pass on the GPU (rti_rgb.hip) held to the entries they
replace: rti.relight of each map, rti.normals of the fp32 luminance, rti.relight_enhanced under a unit weight, the
rti_rgb8 entries for maps that are dequantised bytes, and tests/rgb_ref.py.  Every comparison is exact: byte strings
of fp32 / int32 / uint8.

Sizes: the PTM-6 kernels give a lane 4 pixels, a wave 256 and a workgroup 1024, so 1 and 7 are a partial wave on
the one-pixel path, 255 and 256 straddle a wave, 1023 and 1024 a workgroup, 1028 gives a second workgroup of 4
pixels (P % 4 == 0: the vector path and a partial chunk), 3077 several workgroups with P % 4 != 0.  The HSH kernels
give a lane one pixel, a wave 64 and a workgroup 256, so they also run 63, 64, 65 and 257, and E = 65 crosses their
table of 64 directions.  Maps run in both layouts, dense, with a channel stride padded by 8 and by 6 (off the vector
path) and 4 bytes off 16 through the C ABI (the stride is an argument only there); every output lies between guard
elements, 16-byte aligned and 4 bytes off."""
import numpy as np
import pytest
import torch

import far_ref as fr
import rti
from enhance_rgb_ref import MODES, peaked_rgb, peaked_rgb8
from hsh8_ref import host_dequantise as hsh_dequantise
from hsh8_ref import host_qparams as hsh_qparams
from hsh8_ref import host_quantise as hsh_quantise
from hsh8_ref import mixed_hsh
from rgb8_ref import LUMA, host_dequantise, host_qparams, host_quantise, luminance, mixed_rgb
from rgb_ref import (TERMS, bad_pixels, far_maps_plan, nonfinite_hsh, nonfinite_rgb, relight_rgb_ref, rgb_enhanced,
                     rgb_normals_ref)
from rti import _lib as L
from rti import api
from test_gpu_rgb8 import bits, dirs, guarded, guards_untouched, on_device, same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 255, 256, 1023, 1024, 1028, 3077]
HSH_SIZES = sorted(SIZES + [63, 64, 65, 257])
ES = [1, 3]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]
NP_NAME = {torch.float32: "float32", torch.int32: "int32", torch.uint8: "uint8"}
VARIANTS = {"dense": dict(), "padded": dict(pad=8), "padded off the vector": dict(pad=6),
            "offset": dict(offset=4, out_offset=4)}
KW = dict(gain=2.5, kd=0.4, ks=150.0, exp=20)
LU, LV = 0.3, -0.45


def mixed(basis, P):
    """rgb8_ref.mixed_rgb / hsh8_ref.mixed_hsh: NaN and ±inf among the values and, for P >= 256, one term NaN in
    every pixel (every image of such a map is NaN: the conversions of NaN are what it checks)"""
    return mixed_rgb(P, 7000 + P) if basis == "ptm" else mixed_hsh(P, TERMS[basis], 8000 + P)


def maps(basis, P):
    """finite maps with a handful of pixels that carry NaN or ±inf in one channel: fp32 [3, P, k], never written"""
    return nonfinite_rgb(P) if basis == "ptm" else nonfinite_hsh(P, TERMS[basis])


def laid_out(cuda, m, layout, pad=0, offset=0):
    """m [3, P, k] on the device in `layout`, the channels `pad` elements apart beyond dense (the padding holds
    NaN) and the first `offset` bytes off 16 -> (tensor [3, stride], the stride argument)."""
    k, P = m.shape[2], m.shape[1]
    laid = np.ascontiguousarray(m.transpose(0, 2, 1)) if layout == "planar" else m
    host = np.full((3, k * P + pad), np.nan, np.float32)
    host[:, :k * P] = laid.reshape(3, -1)
    return on_device(cuda, host, offset), (k * P + pad if pad else 0)


def call(fn, *args):
    st = fn(*args)
    assert st == L.RTI_OK, rti.load().rti_last_error()


def abi_relight(cuda, m, basis, layout, E, dt, pad=0, offset=0, out_offset=0):
    """rti_relight_rgb through the C ABI, the output between guards -> [E, P, 3]."""
    P = m.shape[1]
    md, stride = laid_out(cuda, m, layout, pad, offset)
    luv = torch.as_tensor(np.stack(dirs(E), -1), device=cuda)
    n = E * P * 3
    buf, view, lead, fill = guarded(cuda, n, dt, out_offset)
    call(rti.load().rti_relight_rgb, api._vp(md), api.basis_id(basis), api._layout_id(layout), stride, P, api._vp(luv),
         E, api._vp(view), api._ENHANCED_DTYPES[dt], api._stream_of(md))
    assert guards_untouched(buf, lead, n, fill), (basis, layout, E, dt)
    return view.view(E, P, 3)


def abi_enhanced(cuda, m, layout, mode, dt, weights=None, pad=0, offset=0, out_offset=0, **kw):
    P = m.shape[1]
    md, stride = laid_out(cuda, m, layout, pad, offset)
    buf, view, lead, fill = guarded(cuda, 3 * P, dt, out_offset)
    call(rti.load().rti_relight_rgb_enhanced, api._vp(md), api._layout_id(layout), stride, P, api._luma_weights(weights),
         *api._enhance_scalars(mode, kw["gain"], kw["kd"], kw["ks"], kw["exp"], LU, LV), api._vp(view),
         api._ENHANCED_DTYPES[dt], api._stream_of(md))
    assert guards_untouched(buf, lead, 3 * P, fill), (layout, mode, dt)
    return view.view(P, 3)


def abi_normals(cuda, m, layout, nl, weights=None, pad=0, offset=0, out_offset=0):
    """-> (normals [P, 3] or [3, P], kind [P], peak [P]), each between guards."""
    P = m.shape[1]
    md, stride = laid_out(cuda, m, layout, pad, offset)
    nbuf, n, nlead, nfill = guarded(cuda, 3 * P, torch.float32, out_offset)
    kbuf, kind, klead, kfill = guarded(cuda, P, torch.uint8, out_offset // 4)
    pbuf, peak, plead, pfill = guarded(cuda, P, torch.float32, out_offset)
    call(rti.load().rti_rgb_normals, api._vp(md), api._layout_id(layout), stride, P, api._luma_weights(weights),
         api._vp(n), api._normal_layout_id(nl), api._vp(kind), api._vp(peak), api._stream_of(md))
    assert guards_untouched(nbuf, nlead, 3 * P, nfill) and guards_untouched(kbuf, klead, P, kfill)
    assert guards_untouched(pbuf, plead, P, pfill)
    return n.view((P, 3) if nl == "pixel" else (3, P)), kind, peak


def equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---- 1. rti_relight_rgb is rti_relight of each map ---------------------------------------------------------------

def relight_is_relight(cuda, basis, P, es):
    for m in (maps(basis, P), mixed(basis, P)):
        md = torch.as_tensor(m, device=cuda)
        want = {(E, dt): relight_rgb_ref(rti, md, *dirs(E), basis, dt) for E in es for dt in OUT_DTYPES}
        for layout in ("pixel", "planar"):
            for name, kw in VARIANTS.items():
                for (E, dt), w in want.items():
                    got = abi_relight(cuda, m, basis, layout, E, dt, **kw)
                    assert equal(got, w.view(E, P, 3)), (basis, P, layout, name, E, dt)
        if m is maps(basis, P) and P >= 255:  # images, not NaN or zero frames: at most 9 pixels are not finite
            f = want[(es[0], torch.float32)]
            assert int((torch.isfinite(f) & (f != 0)).all(-1).sum()) >= es[0] * (P - 9)


@pytest.mark.parametrize("P", SIZES)
def test_relight_rgb_ptm_is_relight_of_each_map(cuda, P):
    relight_is_relight(cuda, "ptm", P, ES)


@pytest.mark.parametrize("P", HSH_SIZES)
@pytest.mark.parametrize("basis", ["hsh9", "hsh16"])
def test_relight_rgb_hsh_is_relight_of_each_map(cuda, basis, P):
    relight_is_relight(cuda, basis, P, ES)


@pytest.mark.parametrize("basis", ["hsh9", "hsh16"])
def test_relight_rgb_hsh_across_the_direction_table(cuda, basis):
    """E = 65: the second table of the HSH kernel holds one direction."""
    rng = np.random.default_rng(12)
    lu, lv = rng.uniform(-0.7, 0.7, 65), rng.uniform(-0.7, 0.7, 65)
    for P in (65, 257):
        md = torch.as_tensor(maps(basis, P), device=cuda)
        for dt in (torch.float32, torch.uint8):
            got = rti.relight_rgb(md, lu, lv, basis, out_dtype=dt)
            assert equal(got, relight_rgb_ref(rti, md, lu, lv, basis, dt)), (basis, P, dt)


# ---- 2. maps that are dequantised bytes: the rti_rgb8 / rti_hsh8 entries -------------------------------------------

@pytest.mark.parametrize("P", SIZES)
def test_dequantised_rgb8_maps_render_as_the_bytes(cuda, P):
    for raw, qp, deq in ((None, None, None), peaked_rgb8(P)):
        if raw is None:
            m = mixed_rgb(P, 7000 + P)
            qp = host_qparams(m)
            raw = host_quantise(m, qp)
            deq = host_dequantise(raw, qp)
        q = rti.QuantisedRGB(torch.as_tensor(raw, device=cuda), torch.as_tensor(qp, device=cuda))
        md = rti.dequantise_rgb(q)
        assert same_bits(md.cpu().numpy(), deq)
        for dt in OUT_DTYPES:
            assert equal(rti.relight_rgb(md, *dirs(3), out_dtype=dt), rti.relight_rgb8(q, *dirs(3), out_dtype=dt)), dt
            for mode in MODES:
                got = rti.relight_rgb_enhanced(md, LU, LV, mode, out_dtype=dt, **KW)
                assert equal(got, rti.relight_rgb8_enhanced(q, LU, LV, mode, out_dtype=dt, **KW)), (dt, mode)
        for nl in ("pixel", "planar"):
            a = rti.rgb_normals(md, normal_layout=nl, return_kind=True, return_peak=True)
            b = rti.rgb8_normals(q, normal_layout=nl, return_kind=True, return_peak=True)
            assert all(equal(x, y) for x, y in zip(a, b)), nl


@pytest.mark.parametrize("P", [63, 64, 257, 1028, 3077])
@pytest.mark.parametrize("basis", ["hsh9", "hsh16"])
def test_dequantised_hsh8_maps_render_as_the_bytes(cuda, basis, P):
    m = mixed_hsh(P, TERMS[basis], 8000 + P)
    qp = hsh_qparams(m)
    raw = hsh_quantise(m, qp)
    q = rti.QuantisedHSH(torch.as_tensor(raw, device=cuda), torch.as_tensor(qp, device=cuda), basis)
    md = rti.dequantise_hsh(q)
    assert same_bits(md.cpu().numpy(), hsh_dequantise(raw, qp))
    for dt in OUT_DTYPES:
        assert equal(rti.relight_rgb(md, *dirs(3), basis, out_dtype=dt), rti.relight_hsh8(q, *dirs(3), out_dtype=dt)), dt


# ---- 3. rti_rgb_normals is rti_ptm_normals of the fp32 luminance ---------------------------------------------------

@pytest.mark.parametrize("weights", [None, (0.2, 0.5, 0.3)])
@pytest.mark.parametrize("P", SIZES)
def test_normals_are_normals_of_the_luminance(cuda, P, weights):
    m = nonfinite_rgb(P)
    lum = torch.as_tensor(luminance(m, LUMA if weights is None else weights), device=cuda)  # built on the host
    rn, rkind, rpeak = rgb_normals_ref(m, weights)
    for nl in ("pixel", "planar"):
        wn, wkind, wpeak = rti.normals(lum, normal_layout=nl, return_kind=True, return_peak=True)
        for layout in ("pixel", "planar"):
            for name, kw in VARIANTS.items():
                n, kind, peak = abi_normals(cuda, m, layout, nl, weights, **kw)
                assert equal(n, wn) and equal(kind, wkind) and equal(peak, wpeak), (P, nl, layout, name)
        assert np.array_equal(wkind.cpu().numpy(), rkind)  # and tests/rgb_ref.py names the same kinds
    kinds = set(rkind.tolist())
    print(f"P={P}: kinds {sorted(kinds)}")
    assert np.array_equal(rkind == 4, bad_pixels(m))
    if P >= 255:
        assert kinds == {0, 1, 2, 4}
    md = torch.as_tensor(m, device=cuda)
    only = rti.rgb_normals(md, weights=weights)
    assert equal(only, rti.normals(lum)) and only.shape == (P, 3)
    # without kind and peak the kernel takes its other branches
    a = rti.rgb_normals(md, weights=weights, return_kind=True)
    assert equal(a[0], only) and np.array_equal(a[1].cpu().numpy(), rkind)


# ---- 4. rti_relight_rgb_enhanced -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", SIZES)
def test_enhanced_is_the_reference(cuda, P, mode):
    for m in (nonfinite_rgb(P), mixed_rgb(P, 7000 + P)):
        for weights in (None, (0.2, 0.5, 0.3)):
            want = {dt: rgb_enhanced(m, LU, LV, mode, NP_NAME[dt], weights=weights, **KW) for dt in OUT_DTYPES}
            for layout in ("pixel", "planar"):
                for name, kw in VARIANTS.items():
                    for dt in OUT_DTYPES:
                        got = abi_enhanced(cuda, m, layout, mode, dt, weights, **kw, **KW)
                        assert same_bits(got.cpu().numpy(), want[dt]), (P, mode, weights, layout, name, dt)
    bad = bad_pixels(nonfinite_rgb(P))
    got = rti.relight_rgb_enhanced(torch.as_tensor(nonfinite_rgb(P), device=cuda), LU, LV, mode, **KW)
    assert bool(torch.isnan(got[torch.as_tensor(bad, device=cuda)]).all())  # kind 4: NaN in three channels
    assert bool(torch.isfinite(got[torch.as_tensor(~bad, device=cuda)]).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", [7, 1028, 3077])
def test_enhanced_channel_with_unit_weight_is_relight_enhanced(cuda, P, mode):
    md = torch.as_tensor(nonfinite_rgb(P), device=cuda)
    for c in range(3):
        w = [0.0, 0.0, 0.0]
        w[c] = 1.0
        for dt in OUT_DTYPES:
            got = rti.relight_rgb_enhanced(md, LU, LV, mode, out_dtype=dt, weights=w, **KW)
            want = rti.relight_enhanced(md[c], LU, LV, mode, out_dtype=dt, **KW)
            # a non-finite value in ANOTHER channel makes the weighted sum NaN (0·inf, 0·NaN): those pixels are
            # kind 4 here and finite in the grey map
            same = ~torch.as_tensor(bad_pixels(nonfinite_rgb(P)), device=cuda)
            assert torch.equal(bits(got[..., c].contiguous())[same], bits(want)[same]), (P, mode, c, dt)


@pytest.mark.parametrize("P", [255, 1028, 3077])
def test_diffuse_gain_one_is_relight_where_the_luminance_peaks(cuda, P):
    m = peaked_rgb(P)
    md = torch.as_tensor(m, device=cuda)
    has_max = torch.as_tensor(np.isin(rgb_normals_ref(m)[1], (0, 1)), device=cuda)
    assert bool(has_max.any()) and not bool(has_max.all())
    got = rti.relight_rgb_enhanced(md, LU, LV, "diffuse_gain", gain=1.0)
    # gain 1 leaves a' = a exactly (g·a_j = a_j; h = 0, so b_3 = 0·x + a_3 = a_3, likewise b_4 and b_5), and L' is
    # summed as rti_relight's F64 path sums it: the image is rti.relight of the maps widened to fp64, rounded once
    exact = torch.stack([rti.relight(md[c].double(), LU, LV, out_dtype=torch.float32) for c in range(3)], -1)
    assert equal(got, exact)
    # and relight_rgb, which sums the same six terms in fp32: its basis row carries one rounding per entry, its
    # chain one per term and the fp64 value one more, each at most 2^-24 of a term bounded by |a_j| (|b_j| <= 1):
    # 8·2^-24·Σ|a_j| covers them; 12 leaves room for the second-order terms
    want = rti.relight_rgb(md, LU, LV).double()
    tol = 12 * 2.0 ** -24 * torch.as_tensor(np.abs(m).astype(np.float64).sum(-1).T, device=cuda)
    assert bool(((got.double() - want).abs() <= tol)[has_max].all())
    assert bool(((got.double() - want).abs() > 0).any())  # fp64 against fp32 sums: not the same kernel twice


# ---- 5. the vector path and the one-pixel path on the same data --------------------------------------------------

@pytest.mark.parametrize("P", [256, 1028])
def test_paths_agree_to_the_bit(cuda, P):
    for basis in TERMS:
        m = maps(basis, P)
        for layout in ("pixel", "planar"):
            for dt in OUT_DTYPES:
                ref = bits(abi_relight(cuda, m, basis, layout, 3, dt))
                small = 4 if dt != torch.uint8 else 1
                for kw in (dict(offset=4), dict(pad=6), dict(pad=8), dict(out_offset=small), dict(out_offset=2 * small)):
                    assert torch.equal(bits(abi_relight(cuda, m, basis, layout, 3, dt, **kw)), ref), (basis, layout, dt, kw)
    m = nonfinite_rgb(P)
    for layout in ("pixel", "planar"):
        for mode in MODES:
            for dt in OUT_DTYPES:
                ref = bits(abi_enhanced(cuda, m, layout, mode, dt, **KW))
                small = 4 if dt != torch.uint8 else 1
                for kw in (dict(offset=4), dict(pad=6), dict(pad=8), dict(out_offset=small)):
                    assert torch.equal(bits(abi_enhanced(cuda, m, layout, mode, dt, **kw, **KW)), ref), (layout, mode, dt, kw)
        for nl in ("pixel", "planar"):
            ref = [bits(t).clone() for t in abi_normals(cuda, m, layout, nl)]
            for kw in (dict(offset=4), dict(pad=6), dict(pad=8), dict(out_offset=4)):
                got = abi_normals(cuda, m, layout, nl, **kw)
                assert all(torch.equal(bits(x), y) for x, y in zip(got, ref)), (layout, nl, kw)


# ---- 6. graph capture ----------------------------------------------------------------------------------------------

def test_graph_capture_replays_the_eager_bytes(cuda):
    """The three launchers (and the HSH kernel) on one stream, captured once (a single chain, no parallel
    branches) and replayed once on other data."""
    P = 3076
    first, second = nonfinite_rgb(P), peaked_rgb(P)
    h_first, h_second = mixed_hsh(P, 16, 3), mixed_hsh(P, 16, 9)
    md, hd = on_device(cuda, first), on_device(cuda, h_first)
    luv = torch.as_tensor(np.stack(dirs(2), -1), device=cuda)
    out = torch.empty((2, P, 3), dtype=torch.uint8, device=cuda)
    hout = torch.empty((2, P, 3), dtype=torch.float32, device=cuda)
    enh = torch.empty((P, 3), dtype=torch.float32, device=cuda)
    n = torch.empty((P, 3), dtype=torch.float32, device=cuda)
    kind = torch.empty(P, dtype=torch.uint8, device=cuda)
    peak = torch.empty(P, dtype=torch.float32, device=cuda)

    def chain():
        rti.relight_rgb_into(md, luv, out)
        rti.relight_rgb_into(hd, luv, hout, basis="hsh16")
        rti.relight_rgb_enhanced_into(md, LU, LV, "specular", enh, **KW)
        rti.rgb_normals_into(md, n, kind, peak)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    md.copy_(torch.as_tensor(second, device=cuda))
    hd.copy_(torch.as_tensor(h_second, device=cuda))
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = [t.clone() for t in (out, hout, enh, n, kind, peak)]
    assert equal(replayed[0], rti.relight_rgb(md, *dirs(2), out_dtype=torch.uint8)) and bool(replayed[0].any())
    assert equal(replayed[1], rti.relight_rgb(hd, *dirs(2), "hsh16"))
    assert equal(replayed[2], rti.relight_rgb_enhanced(md, LU, LV, "specular", **KW))
    want = rti.rgb_normals(md, return_kind=True, return_peak=True)
    assert all(equal(x, y) for x, y in zip(replayed[3:], want))


# ---- 7. torch.ops ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P = 1028
    layout = "planar" if planar else "pixel"
    checks = ("test_schema", "test_faketensor")
    lu, lv = dirs(2)
    luv = torch.as_tensor(np.stack([lu, lv], -1))
    for basis in TERMS:
        m = maps(basis, P)
        md = on_device(cuda, np.ascontiguousarray(m.transpose(0, 2, 1)) if planar else m)
        b = api.basis_id(basis)
        for dt in OUT_DTYPES:
            got = torch.ops.rti.relight_rgb(md, luv, b, planar, dt)
            want = rti.relight_rgb(md, lu, lv, basis, layout=layout, out_dtype=dt)
            assert got.dtype == dt and equal(got, want) and got.shape == (2, P, 3), (basis, dt)
        torch.library.opcheck(torch.ops.rti.relight_rgb.default, (md, luv, b, planar, torch.uint8), test_utils=checks)
    m = nonfinite_rgb(P)
    md = on_device(cuda, np.ascontiguousarray(m.transpose(0, 2, 1)) if planar else m)
    w = [0.2, 0.5, 0.3]
    for mode in MODES:
        mid = api.ENHANCE_MODES[mode]
        for dt in OUT_DTYPES:
            got = torch.ops.rti.relight_rgb_enhanced(md, LU, LV, mid, KW["gain"], KW["kd"], KW["ks"], KW["exp"], planar,
                                                     w, dt)
            want = rti.relight_rgb_enhanced(md, LU, LV, mode, layout=layout, out_dtype=dt, weights=w, **KW)
            assert got.dtype == dt and equal(got, want) and got.shape == (P, 3), (mode, dt)
        torch.library.opcheck(torch.ops.rti.relight_rgb_enhanced.default, (md, LU, LV, mid), dict(planar=planar),
                              test_utils=checks)
    for nplanar in (False, True):
        got = torch.ops.rti.rgb_normals(md, planar, nplanar, w)
        want = rti.rgb_normals(md, layout=layout, normal_layout="planar" if nplanar else "pixel", weights=w,
                               return_kind=True, return_peak=True)
        assert all(equal(x, y) for x, y in zip(got, want))
        torch.library.opcheck(torch.ops.rti.rgb_normals.default, (md, planar, nplanar, None), test_utils=checks)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_rgb(md[:2], luv, L.RTI_BASIS_PTM6, planar, torch.float32)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_rgb(md, luv, L.RTI_BASIS_HSH9, planar, torch.float32)
    with pytest.raises(ValueError):
        torch.ops.rti.rgb_normals(md.transpose(1, 2).contiguous(), planar, False, None)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_rgb_enhanced(md, LU, LV, api.ENHANCE_MODES["specular"], 1.0, 1.0, 0.0, 1, planar, None,
                                           torch.float64)


# ---- 8. far channel strides ----------------------------------------------------------------------------------------
# The buffers are built as tests/test_gpu_far_strides.py builds FarIn (restated: the plans are this file's, not
# far_ref.PLANS'): one poisoned allocation of Plan.length floats holding the three maps a far stride apart; the
# outputs are small and guarded.  Channel 1 lies past 2^32 bytes, channel 2 past 2^31 elements.

PF = fr.P16


@pytest.fixture
def release():
    yield
    torch.cuda.empty_cache()


def far_maps(cuda, m, variant):
    """m [3, PF·k] -> (keep-alive tensor, pointer to the payload base, the channel stride)"""
    import ctypes

    p = far_maps_plan(m.shape[1] // PF, variant)
    assert p.nbytes() <= fr.CAP_BYTES
    t = torch.full((p.length,), float("nan"), dtype=torch.float32, device=cuda)
    assert t.data_ptr() % 16 == 0
    off = p.block_offsets()
    d = torch.as_tensor(m, device=cuda)
    for c in range(3):
        t.narrow(0, p.base + int(off[c, 0]), p.inner).copy_(d[c])
    return t, ctypes.c_void_p(t.data_ptr() + 4 * p.base), p.strides[0]


def far_case(cuda, m, variant, run):
    """run(pointer, stride, layout id) -> tensors; the far call against the dense one, both layouts"""
    t, fp, fs = far_maps(cuda, m, variant)
    dense = on_device(cuda, m)
    for lid in (L.RTI_COEF_PIXEL_MAJOR, L.RTI_COEF_PLANAR):
        far = run(fp, fs, lid)
        want = run(api._vp(dense), 0, lid)
        torch.cuda.synchronize(cuda)
        assert all(equal(a, b) for a, b in zip(far, want)), (variant, lid, "differs from the dense call")
        assert not any(bool(torch.isnan(b.float()).all()) for b in want)
    del t


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("basis", ["ptm", "hsh16"])
def test_far_channel_stride_relight(cuda, release, basis, variant):
    k = TERMS[basis]
    m = np.random.default_rng(50 + k).uniform(-40.0, 90.0, (3, PF * k)).astype(np.float32)
    luv = torch.as_tensor(np.stack(dirs(3), -1), device=cuda)

    def run(cp, cs, lid):
        buf, view, lead, fill = guarded(cuda, 3 * PF * 3, torch.float32)
        call(rti.load().rti_relight_rgb, cp, api.basis_id(basis), lid, cs, PF, api._vp(luv), 3, api._vp(view), L.RTI_F32,
             api._stream_of(luv))
        assert guards_untouched(buf, lead, 3 * PF * 3, fill)
        return (view,)

    far_case(cuda, m, variant, run)


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_far_channel_stride_enhanced(cuda, release, variant):
    m = np.ascontiguousarray(peaked_rgb(PF).reshape(3, -1))  # read as [p][6] and as [6][p]: the same numbers
    luv = torch.empty(1, device=cuda)

    def run(cp, cs, lid):
        outs = []
        for mode in MODES:
            buf, view, lead, fill = guarded(cuda, 3 * PF, torch.float32)
            call(rti.load().rti_relight_rgb_enhanced, cp, lid, cs, PF, None,
                 *api._enhance_scalars(mode, KW["gain"], KW["kd"], KW["ks"], KW["exp"], LU, LV), api._vp(view),
                 L.RTI_F32, api._stream_of(luv))
            assert guards_untouched(buf, lead, 3 * PF, fill)
            outs.append(view)
        return outs

    far_case(cuda, m, variant, run)


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_far_channel_stride_normals(cuda, release, variant):
    m = np.ascontiguousarray(peaked_rgb(PF).reshape(3, -1))
    luv = torch.empty(1, device=cuda)

    def run(cp, cs, lid):
        nbuf, n, nlead, nfill = guarded(cuda, 3 * PF, torch.float32)
        kbuf, kind, klead, kfill = guarded(cuda, PF, torch.uint8)
        pbuf, peak, plead, pfill = guarded(cuda, PF, torch.float32)
        call(rti.load().rti_rgb_normals, cp, lid, cs, PF, None, api._vp(n), 0, api._vp(kind), api._vp(peak),
             api._stream_of(luv))
        assert guards_untouched(nbuf, nlead, 3 * PF, nfill) and guards_untouched(kbuf, klead, PF, kfill)
        assert guards_untouched(pbuf, plead, PF, pfill)
        return n, kind, peak

    far_case(cuda, m, variant, run)
