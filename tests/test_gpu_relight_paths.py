"""rti_relight and rti_relight_frame (rti_relight.hip) held to tests/relight_ref.py, an exact NumPy
restatement that shares no code with the library, on every launch path at the smallest shapes that reach it.  Every
comparison is on bit patterns: values that are not NaN have equal bits, NaN stands where NaN stands, the integer
outputs are equal, and no pixel is exempt.

Eval-major (relight_eval_major): a lane owns VEC pixels, a wave 64 lanes, a workgroup 4 waves and up to ECH = 64
directions.  launch_t takes VEC = 4 when P % 4 == 0 and the coefficients are 16-byte and the output 4-element
aligned, else VEC = 1.  With VEC = 4 a pixel-major map whose 256-pixel rows fit the LDS slab (fp32 PTM-6 and HSH-9,
fp64 PTM-6) is read through load_coef_staged by every wave whose whole chunk lies in the image; the other waves,
the other maps and planar maps load per lane.

    P = 4      one lane, VEC = 4, per-lane loads
    P = 256    one wave, one staged chunk
    P = 260    a staged wave, then a wave whose only live lane loads for itself
    P = 1020   three staged waves and a 252-pixel fourth in one workgroup, around the same slabs
    P = 1028   a full workgroup and one lane of the next
    P = 1, 3, 257, 1029   VEC = 1: a lane, a partial wave, a second wave, a second workgroup
    E = 1, 64, 65, 130    one direction; a full table; a second block of one; three blocks, the last of two

Pixel-major (relight_pixel_major): a block is 8 pixels by 256 directions: (P, E) = (7, 1), (8, 256), (9, 257),
(260, 70).  The frame (relight_frame_k) stages whole chunks whatever P % 4 is when the source is 16-byte aligned and
handles a tail of fewer than 4 pixels: P = 256, 259, 515."""
import functools

import numpy as np
import pytest
import torch

import relight_ref as R
import rti
import rti_oracle as o
from rti import _lib as L
from rti import api
from test_gpu_rgb8 import guarded, guards_untouched, on_device, same_bits

pytestmark = pytest.mark.gpu

BASES = ["ptm", "hsh9", "hsh"]
CNAMES = ["float32", "float64"]
LAYOUTS = ["pixel", "planar"]
OUT = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}
VEC_SIZES = [4, 256, 260, 1020, 1028]
SCALAR_SIZES = [1, 3, 257, 1029]
ES = [1, 64, 65, 130]
PIXEL_MAJOR = [(7, 1), (8, 256), (9, 257), (260, 70)]
FRAME_SIZES = [256, 259, 515]
FRAME_DIRS = [(0.3, -0.25), (0.8, 0.75), (0.0, 0.0)]  # inside the disc, outside it (lw = 0), the pole


def coef_host(basis, cname, P, seed=0):
    """the seeded map [P, k] in the coefficient type: the fp64 map holds the fp32 values"""
    return R.maps(P, R.TERMS[basis], 1000 + P + seed).astype(cname)


@functools.lru_cache(maxsize=None)
def reference(basis, cname, P, E):
    """relight_ref of coef_host at dirs(E) -> [E, P], computed once for both layouts and never written; dirs(E') is
    a prefix of dirs(E), so the first E' rows are the reference of a launch of E' directions"""
    ref = R.relight_ref(coef_host(basis, cname, P), *R.dirs(E), basis)
    assert ref.shape == (E, P) and ref.dtype == np.dtype(cname)
    ref.setflags(write=False)
    return ref


def upload(cuda, c, layout, offset=0):
    """[P, k] on the device as [P, k] or [k, P], `offset` bytes off a 16-byte boundary"""
    return on_device(cuda, c.T if layout == "planar" else c, offset)


def differences(got, want):
    """'' when got (a device tensor) is want (NumPy) to the bit, NaN for NaN; else what differs"""
    g = got.cpu().numpy()
    if g.shape != want.shape or g.dtype != want.dtype:
        return f"{g.dtype}{g.shape} for {want.dtype}{want.shape}"
    w = want
    if g.dtype.kind == "f":
        gn, wn = np.isnan(g), np.isnan(w)
        if not np.array_equal(gn, wn):
            return f"NaN at {int(gn.sum())} places for {int(wn.sum())}, first at {np.argwhere(gn != wn)[0].tolist()}"
        zero = g.dtype.type(0)
        g, w = np.where(gn, zero, g), np.where(wn, zero, w)
    if same_bits(g, w):
        return ""
    u = f"u{g.dtype.itemsize}"
    bad = np.argwhere(np.ascontiguousarray(g).view(u) != np.ascontiguousarray(w).view(u))
    i = tuple(bad[0])
    return f"{len(bad)} of {g.size} differ, first at {list(i)}: {g[i]!r} for {w[i]!r}"


def abi_relight(cuda, c, basis, layout, P, E, oname, out_offset=0, out_layout=L.RTI_OUT_EVAL_MAJOR):
    """rti_relight through the C ABI into an output between guards, `out_offset` bytes off 16 -> E·P elements"""
    luv = torch.as_tensor(np.stack(R.dirs(E), -1), device=cuda)
    buf, view, lead, fill = guarded(cuda, E * P, OUT[oname], out_offset)
    if not out_offset:
        assert view.data_ptr() % (4 * view.element_size()) == 0  # what launch_t asks of the vector stores
    st = L.lib().rti_relight(api._vp(c), api._COEF_DTYPES[c.dtype], api.basis_id(basis), P, api._layout_id(layout),
                             api._vp(luv), E, api._vp(view), api._OUT_DTYPES[OUT[oname]], out_layout, api._stream_of(c))
    L.check(st, "rti_relight")
    assert guards_untouched(buf, lead, E * P, fill), (basis, layout, P, E, oname, out_offset)
    return view


# ---- 1. eval-major: the vector, staged and scalar paths ----------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("basis", BASES)
def test_eval_major_is_the_reference(cuda, basis, cname, layout):
    for P in VEC_SIZES + SCALAR_SIZES:
        c = upload(cuda, coef_host(basis, cname, P), layout)
        ref = reference(basis, cname, P, max(ES))
        assert P < 256 or np.isfinite(ref).mean() > 0.9  # images, not NaN frames
        for E in ES:
            lu, lv = R.dirs(E)
            for oname, odt in OUT.items():
                got = rti.relight(c, lu, lv, basis=basis, layout=layout, out_dtype=odt)
                d = differences(got, R.convert(ref[:E], oname))
                assert not d, (P, E, oname, d)


# ---- 2. pixel-major output ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("basis", BASES)
def test_pixel_major_is_the_reference(cuda, basis, cname, layout):
    for P, E in PIXEL_MAJOR:
        c = upload(cuda, coef_host(basis, cname, P), layout)
        ref = reference(basis, cname, P, E)
        lu, lv = R.dirs(E)
        for oname, odt in OUT.items():
            got = rti.relight(c, lu, lv, basis=basis, layout=layout, out_dtype=odt, out_layout="pixel")
            d = differences(got, np.ascontiguousarray(R.convert(ref, oname).T))
            assert not d, (P, E, oname, d)


# ---- 3. misaligned buffers and guard bands, through the C ABI ------------------------------------------------------

@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("basis", BASES)
def test_misaligned_buffers_and_guard_bands(cuda, basis, cname):
    """Aligned (the vector path; a vector store past P would land in the guards), the coefficients one element off
    16 bytes, and the output one element off: launch_t falls to VEC = 1 for the last two."""
    E = 65
    esize = np.dtype(cname).itemsize
    for P in (256, 1028):
        ref = reference(basis, cname, P, max(ES))[:E]
        for layout in LAYOUTS:
            for oname, odt in OUT.items():
                want = R.convert(ref, oname).ravel()
                osize = want.dtype.itemsize
                for coef_offset, out_offset in ((0, 0), (esize, 0), (0, osize)):
                    c = upload(cuda, coef_host(basis, cname, P), layout, coef_offset)
                    assert c.data_ptr() % 16 == coef_offset
                    got = abi_relight(cuda, c, basis, layout, P, E, oname, out_offset)
                    d = differences(got, want)
                    assert not d, (P, layout, oname, coef_offset, out_offset, d)
    # the pixel-major kernel's scalar stores, between guards as well
    P, E = 9, 257
    ref = reference(basis, cname, P, E)
    for layout in LAYOUTS:
        c = upload(cuda, coef_host(basis, cname, P), layout)
        for oname in OUT:
            got = abi_relight(cuda, c, basis, layout, P, E, oname, out_layout=L.RTI_OUT_PIXEL_MAJOR)
            d = differences(got, np.ascontiguousarray(R.convert(ref, oname).T).ravel())
            assert not d, (layout, oname, d)


# ---- 4. the basis table alone ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("basis", BASES)
def test_identity_map_returns_the_basis_table(cuda, basis, cname):
    """Pixel p holds e_(p mod k), so its image at direction e is b_k(e): every other term adds a zero.  A mismatch
    here is the table's, one elsewhere only the chain's.  A value that is not zero keeps its bits; a zero keeps its
    value, and its sign is the chain's (the 0·b_j terms are signed zeros: +0 + -0 = +0), which the comparison with
    relight_ref holds to the bit."""
    k, P = R.TERMS[basis], 260
    lu, lv = R.dirs(64)
    B = (R.basis32 if cname == "float32" else R.basis64)(lu, lv, basis)
    eye = np.eye(k, dtype=cname)[np.arange(P) % k]
    want = B[:, np.arange(P) % k]
    assert not np.isnan(want).any() and (want != 0).mean() > 0.8
    exact = R.relight_ref(eye, lu, lv, basis)
    assert np.array_equal(exact, want)
    u = f"u{want.dtype.itemsize}"
    for layout in LAYOUTS:
        got = rti.relight(upload(cuda, eye, layout), lu, lv, basis=basis, layout=layout, out_dtype=OUT[cname])
        g = got.cpu().numpy()
        assert g.dtype == want.dtype and np.array_equal(g, want), layout
        nz = want != 0
        assert np.array_equal(g.view(u)[nz], np.ascontiguousarray(want).view(u)[nz]), layout
        d = differences(got, exact)
        assert not d, (layout, d)


# ---- 5. rti_relight_frame from coefficients -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hsv_host(P):
    hsv = np.random.default_rng(300 + P).integers(0, 256, (1, P, 3)).astype(np.uint8)
    hsv.setflags(write=False)
    return hsv


@functools.lru_cache(maxsize=None)
def frame_reference(basis, cname, P, lu, lv):
    """the oracle's relighting_event image of relight_ref's int32 values -> uint8 [1, P, 3]"""
    values = R.convert(R.relight_ref(coef_host(basis, cname, P), [lu], [lv], basis), "int32")
    return o.relighting_event_image(values.reshape(1, P), hsv_host(P))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("basis", BASES)
def test_frame_is_the_reference(cuda, basis, cname, layout):
    lib = L.lib()
    for P in FRAME_SIZES:
        c = upload(cuda, coef_host(basis, cname, P), layout)
        hsv = on_device(cuda, hsv_host(P))
        # one element off 16 bytes (the staged kernel's fallback to per-lane loads), hsv and bgr on odd addresses
        c_off = upload(cuda, coef_host(basis, cname, P), layout, np.dtype(cname).itemsize)
        hsv_off = on_device(cuda, hsv_host(P), 1)
        for lu, lv in FRAME_DIRS:
            want = frame_reference(basis, cname, P, lu, lv)
            assert P < 256 or len(np.unique(want)) > 100  # an image
            got = rti.relight_frame(c, hsv, lu, lv, basis=basis, layout=layout)
            assert np.array_equal(got.cpu().numpy(), want), (P, lu, lv)
            for src, h, out_offset in ((c_off, hsv, 0), (c, hsv_off, 0), (c, hsv, 1), (c_off, hsv_off, 1)):
                buf, bgr, lead, fill = guarded(cuda, 3 * P, torch.uint8, out_offset)
                st = lib.rti_relight_frame(api._vp(src), api._COEF_DTYPES[src.dtype], api.basis_id(basis),
                                           api._layout_id(layout), P, lu, lv, api._vp(h), api._vp(bgr),
                                           api._stream_of(src))
                L.check(st, "rti_relight_frame")
                assert guards_untouched(buf, lead, 3 * P, fill), (P, lu, lv, out_offset)
                assert np.array_equal(bgr.cpu().numpy().reshape(1, P, 3), want), (P, lu, lv, out_offset)


# ---- 6. torch.ops.rti.relight and rti.relight_rgb, once each ----------------------------------------------------------

@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("basis", BASES)
def test_torch_op_is_the_reference(cuda, basis, cname):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P, E = 1020, 8
    c = upload(cuda, coef_host(basis, cname, P), "pixel")
    luv = torch.as_tensor(np.stack(R.dirs(E), -1))
    got = torch.ops.rti.relight(c, luv, api.basis_id(basis))
    d = differences(got, reference(basis, cname, P, max(ES))[:E])
    assert not d, d


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("basis", BASES)
def test_relight_rgb_is_the_reference_per_channel(cuda, basis, layout):
    P, E = 1020, 8
    lu, lv = R.dirs(E)
    m = np.stack([coef_host(basis, "float32", P, seed=31 * ch) for ch in range(3)])
    md = on_device(cuda, m.transpose(0, 2, 1) if layout == "planar" else m)
    ref = np.stack([R.relight_ref(m[ch], lu, lv, basis) for ch in range(3)], -1)  # [E, P, 3]
    for oname in ("float32", "int32", "uint8"):
        got = rti.relight_rgb(md, lu, lv, basis, layout=layout, out_dtype=OUT[oname])
        d = differences(got, R.convert(ref, oname))
        assert not d, (oname, d)
