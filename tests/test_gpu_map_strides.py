"""The stride arguments of the entries added after tests/test_gpu_strides.py (include/rti.h), driven on the GPU through
ctypes: coef_channel_stride of rti_relight_hsh_gain, rti_relight_hsh_specular, rti_light_scores and rti_relight_field,
and light_stride / channel_stride of rti_photometric_stereo.

rti/api.py passes stride 0 (gain, specular), the stride of a tensor view (multi-light) or N·light_stride (photometric
stereo), so this module calls rti._lib.lib() directly.  The plumbing (dev, ptr, stream, bits_equal, LAYOUTS) is
test_gpu_strides.py's and the views are stride_ref's: dense data embedded in one poisoned allocation (fp32 maps: NaN;
stacks: NaN / 128 / 255 as test_fit_shared_robust chooses them) and every output between guards in a buffer of
NaN-pattern words.  Every call is held to the three checks of test_gpu_strides.py:

 (a) guards: every byte outside the payload of every output keeps the NaN pattern;
 (b) reference: the entry's NumPy restatement on the dense data, with the check of the entry's own dense test (imported:
     test_gpu_hsh_gain.check_against_reference, test_gpu_hsh_specular.check_against_reference, test_gpu_ps.check,
     multilight_ref.scores_within_bound and same_bits);
 (c) bits: equal to the dense call (stride 0, or the dense strides) on the same data, bit for bit, for every output.
     include/rti.h and the kernel sources state for each of these entries that every path runs the same per-pixel
     arithmetic (rti_hsh_render_px.h: "every path runs the policy's prepare and value"; rti_multilight.hip: load_px
     and store_dir; rti_ps.hip: "the same arithmetic in the same order"), so (c) is asserted in every form.

Forms (stride_ref.form_pads adapted to three maps / three channels; vec = 4 elements, 16 for uint8 stacks):
  aligned  every stride a multiple of vec and padded by at least vec, bases 16-byte aligned: maps_staged holds and the
           pixel-major maps move as 16-byte pieces through LDS; photometric stereo stages its tile by 16-byte loads;
  odd      the aligned extent + 3 (stacks: + 1 per plane), so the stride is no multiple of vec: one element per lane;
  offset   the aligned strides with the input bases (maps, normals, stacks) one element off a 16-byte boundary.

Shapes.  Renderers: P = 1076 = 4·256 + 3·64 + 52 (whole workgroups, three staged waves and a ragged one: far_ref's size
for map readers), E = 3, and P = 1075 for uint8 (P % 4 != 0: rows_as_dwords is false).  Multi-light: 19 × 37 with T = 8
(3 × 5 tiles ragged both ways; ten full waves and a tail of 63 in the pixel-order kernel).  Photometric stereo: N = 20,
P = 1316 = P0 of test_gpu_strides.py (five tiles of 256 and a tail of 36)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import hsh_gain_ref as G
import hsh_specular_ref as S
import multilight_ref as M
import rti
import stride_ref as sr
import test_gpu_hsh_gain as tg
import test_gpu_hsh_specular as tsp
import test_gpu_multilight as tm
import test_gpu_ps as tp
import test_gpu_strides as ts
from relight_ref import TERMS
from rti import _lib as L

pytestmark = pytest.mark.gpu

lib, ptr, stream, dev = L.lib, ts.ptr, ts.stream, ts.dev
BITS = int(sr.NAN_BITS)
FORMS = ("aligned", "odd", "offset")
OUT_NP = {"f32": np.float32, "i32": np.int32, "u8": np.uint8}
OUT_TORCH = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}
NORMAL_LAYOUTS = (("pixel", L.RTI_NORMAL_PIXEL_MAJOR), ("planar", L.RTI_NORMAL_PLANAR))
PM, PM_ODD = 1076, 1075
GAIN = 2.5  # hsh_gain_ref.GAINS: gm1 = 1.5, both terms of v = V + gm1·(V − A) live
SPEC = S.PARAMS[2]  # (0.4, 150.0, 75): kd, ks > 0 and spec_exp > 1
assert GAIN in G.GAINS and SPEC[1] > 0 and SPEC[2] > 1
LUV = np.ascontiguousarray(np.array(G.DIRS, np.float64))  # E = 3: rows e > 0 of the output are addressed
assert G.DIRS == S.DIRS and LUV.shape == (3, 2)
HW, TILE = (19, 37), 8
PS_N, PS_P = 20, ts.P0


def up(x, m):
    return -(-int(x) // m) * m


def dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- buffers --------------------------------------------------------------------------------------------------------
class OutBuf:
    """n dense elements of `dtype` on the device, 64 words into an allocation of NaN-pattern words that ends 64 words
    (or more: a uint8 payload is rounded up to a word) after them.  The entries' outputs have no stride arguments."""

    def __init__(self, cuda, n, dtype=np.float32):
        self.dtype, self.nbytes = np.dtype(dtype), int(n) * np.dtype(dtype).itemsize
        self.lo = 4 * sr.GUARD
        self.t = torch.full((2 * sr.GUARD + -(-self.nbytes // 4),), BITS, dtype=torch.int32, device=cuda)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + self.lo)

    def take(self, what):
        """(a), then the payload"""
        torch.cuda.synchronize()
        raw = self.t.cpu().numpy().view(np.uint8)
        fill = np.full(self.t.numel(), BITS, np.int32).view(np.uint8)
        outside = np.ones(raw.size, bool)
        outside[self.lo:self.lo + self.nbytes] = False
        bad = np.flatnonzero(outside & (raw != fill))
        assert bad.size == 0, (what, "written outside the payload at bytes", (bad[:8] - self.lo).tolist(), "of", self.nbytes)
        return raw[self.lo:self.lo + self.nbytes].copy().view(self.dtype)


def map_stride(form, n):
    """(coef_channel_stride, base offset) of maps of n elements each"""
    cs = up(n, 4) + (3 if form == "odd" else 8)
    assert cs >= n and (cs % 4 != 0) == (form == "odd")
    return cs, 1 if form == "offset" else 0


class Maps:
    """C fp32 maps [C, n] on the device: dense (form None, stride argument 0) or a channel stride apart between NaN"""

    def __init__(self, cuda, flat, form):
        flat = np.asarray(flat, np.float32)
        self.C, n = flat.shape
        if form is None:
            self.t, self.cs, off = dev(flat.copy(), cuda), 0, 0  # a copy: the cached maps are read-only
        else:
            self.cs, off = map_stride(form, n)
            buf, b, _, cs = sr.embed_stack(flat[:, None, :], 0, self.cs - n, off)
            assert cs == self.cs and b.start == off
            self.t = dev(buf, cuda)
        self.ptr = ptr(self.t, off)

    def staged(self, layout):
        """hsh_px::maps_staged of this view"""
        return layout == "pixel" and self.ptr.value % 16 == 0 and (self.C == 1 or (self.cs or 4) % 4 == 0)


def flat_maps(m, layout):
    """fp32 [C, P, k] -> [C, P·k] as the layout stores a map"""
    m = np.asarray(m, np.float32)
    return np.ascontiguousarray(m if layout == "pixel" else m.transpose(0, 2, 1)).reshape(m.shape[0], -1)


class Flat:
    """a dense fp32 input (a normal map, a light field) on the device, `off` elements into a NaN-poisoned allocation"""

    def __init__(self, cuda, a, off=0):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        buf = np.full(off + a.size + sr.GUARD, np.nan, np.float32)
        buf[off:off + a.size] = a
        self.t = dev(buf, cuda)
        self.ptr = ptr(self.t, off)


def normal_map(cuda, n, nl, form):
    return Flat(cuda, n if nl == "pixel" else n.T, 1 if form == "offset" else 0)


# ---- rti_relight_hsh_gain, rti_relight_hsh_specular -----------------------------------------------------------------
# (reference module, the dense test's check, the fp32 bound that check asserts, the parameters); both checks hold the
# fp32 image to 1e-6 of max(|ref|, 1) (tg.F32_BOUND, which test_gpu_hsh_gain.py takes from test_gpu_hsh_specular.py's
# check_against_reference) and the integer images to equality off the near-integer elements
RENDER = {"gain": (G, tg.check_against_reference, tg.F32_BOUND, GAIN),
          "specular": (S, tsp.check_against_reference, tg.F32_BOUND, SPEC)}


def render(cuda, entry, coef, cs, layout_id, k, C, P, normals, nl_id, dt, what):
    """one call into a guarded output -> the image [E, P, C]"""
    E = LUV.shape[0]
    out = OutBuf(cuda, E * P * C, OUT_NP[dt])
    head = (coef, rti.api.basis_id(f"hsh{k}"), layout_id, C, cs, P, normals, nl_id)
    tail = (dptr(LUV), E, out.ptr, ts.RTI_DT[dt], stream(cuda))
    if entry == "gain":
        st = lib().rti_relight_hsh_gain(*head, GAIN, *tail)
    else:
        st = lib().rti_relight_hsh_specular(*head, float(SPEC[0]), float(SPEC[1]), int(SPEC[2]), *tail)
    assert st == L.RTI_OK, (what, lib().rti_last_error())
    return out.take(what).reshape(E, P, C)


def check_render(entry, got, P, k, C, dt, what):
    """(b): the entry's dense test's check against its restatement -> the worst fp32 error in units of its bound"""
    ref_mod, check, bound, params = RENDER[entry]
    ref = ref_mod.reference(P, k, "fp32" if C == 3 else "grey", params)
    return check(torch.as_tensor(got), ref, OUT_TORCH[dt], what) / bound


RENDER_OUTS = (("f32", PM), ("i32", PM), ("u8", PM), ("u8", PM_ODD))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", G.KS)
@pytest.mark.parametrize("entry", sorted(RENDER))
def test_render_padded_channel_stride(cuda, entry, k, form):
    """Three maps a padded coef_channel_stride apart, both coefficient and normal layouts, F32 / I32 / U8 at P = 1076
    (uint8 rows leave as dwords) and U8 at P = 1075 (they do not): (a), (b) and (c) for every call."""
    normals_of = RENDER[entry][0].normals
    worst = 0.0
    for dt, P in RENDER_OUTS:
        m = G.maps(P, k, "fp32")
        for layout, lid in ts.LAYOUTS:
            far, dense = Maps(cuda, flat_maps(m, layout), form), Maps(cuda, flat_maps(m, layout), None)
            assert far.staged(layout) == (layout == "pixel" and form == "aligned") and dense.staged(layout) == (layout == "pixel")
            for nl, nid in NORMAL_LAYOUTS:
                what = f"rti_relight_hsh_{entry} k={k} {layout} normals {nl} {dt} P={P} {form}"
                n_far, n_dense = normal_map(cuda, normals_of(P), nl, form), normal_map(cuda, normals_of(P), nl, None)
                got = render(cuda, entry, far.ptr, far.cs, lid, k, 3, P, n_far.ptr, nid, dt, what)
                worst = max(worst, check_render(entry, got, P, k, 3, dt, what))
                want = render(cuda, entry, dense.ptr, 0, lid, k, 3, P, n_dense.ptr, nid, dt, what + " dense")
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, "differs from the dense call")
    print(f"rti_relight_hsh_{entry} k={k} {form}: worst fp32 error {worst:.3g} of its bound")


@pytest.mark.parametrize("k", G.KS)
@pytest.mark.parametrize("entry", sorted(RENDER))
def test_render_one_map_never_uses_its_channel_stride(cuda, entry, k):
    """C = 1 with coef_channel_stride = 2^40 + 3: the bits of stride 0, and the reference."""
    P = PM
    m = G.maps(P, k, "fp32")[:1]
    normals_of = RENDER[entry][0].normals
    for layout, lid in ts.LAYOUTS:
        one = Maps(cuda, flat_maps(m, layout), None)
        for nl, nid in NORMAL_LAYOUTS:
            n = normal_map(cuda, normals_of(P), nl, None)
            for dt in ("f32", "u8"):
                what = f"rti_relight_hsh_{entry} k={k} C=1 {layout} normals {nl} {dt}"
                got = render(cuda, entry, one.ptr, (1 << 40) + 3, lid, k, 1, P, n.ptr, nid, dt, what)
                check_render(entry, got, P, k, 1, dt, what)
                want = render(cuda, entry, one.ptr, 0, lid, k, 1, P, n.ptr, nid, dt, what)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, "differs from stride 0")


# ---- rti_light_scores, rti_relight_field ----------------------------------------------------------------------------
BASIS_OF = {6: "ptm", 9: "hsh9", 16: "hsh16"}
CANDIDATES = M.candidates(17)


@functools.lru_cache(maxsize=None)
def scores_reference(k):
    H, W = HW
    return M.scores_ref(M.image_maps(H, W, k, 3), H, W, TILE, CANDIDATES, BASIS_OF[k])


@functools.lru_cache(maxsize=None)
def pixel_lights():
    """a light per pixel, inside and outside the unit disc, one of them not finite"""
    H, W = HW
    light = np.random.default_rng(8).uniform(-0.9, 0.9, (H * W, 2)).astype(np.float32)
    light[40, 1] = np.nan
    light.setflags(write=False)
    return light


def light_scores(cuda, coef, cs, layout_id, k, what):
    """-> scores fp64 [Ty, Tx, E, 2], count int32 [Ty, Tx]"""
    H, W = HW
    Ty, Tx = M.tile_grid(H, W, TILE)
    E = CANDIDATES.shape[0]
    scores, count = OutBuf(cuda, Ty * Tx * E * 2, np.float64), OutBuf(cuda, Ty * Tx, np.int32)
    st = lib().rti_light_scores(coef, rti.api.basis_id(BASIS_OF[k]), layout_id, 3, cs, H, W, TILE, None, dptr(CANDIDATES), E,
                                scores.ptr, count.ptr, stream(cuda))
    assert st == L.RTI_OK, (what, lib().rti_last_error())
    return scores.take(what + " scores").reshape(Ty, Tx, E, 2), count.take(what + " count").reshape(Ty, Tx)


def relight_field(cuda, coef, cs, layout_id, k, light, tiled, dt, what):
    """-> the image [P, 3]"""
    H, W = HW
    out = OutBuf(cuda, H * W * 3, OUT_NP[dt])
    st = lib().rti_relight_field(coef, rti.api.basis_id(BASIS_OF[k]), layout_id, 3, cs, H, W, light,
                                 L.RTI_LIGHT_TILES if tiled else L.RTI_LIGHT_PIXELS, TILE if tiled else 0, out.ptr,
                                 ts.RTI_DT[dt], stream(cuda))
    assert st == L.RTI_OK, (what, lib().rti_last_error())
    return out.take(what).reshape(H * W, 3)


def check_multilight(cuda, k, layout, lid, src, dense, what, field_forms=(True, False)):
    """scores, count and the relit image of the maps at `src` = (pointer, stride) under (a), (b) and (c), the dense
    call being that of `dense` -> the worst score error in units of its bound"""
    H, W = HW
    m = M.image_maps(H, W, k, 3)
    ref = scores_reference(k)
    scores, count = light_scores(cuda, *src, lid, k, what)
    assert np.array_equal(count, ref["count"]), (what, "count differs from the reference")
    ok, worst = M.scores_within_bound(scores, ref)
    assert ok, (what, "scores", worst)
    dscores, dcount = light_scores(cuda, *dense, lid, k, what + " dense")
    assert np.array_equal(scores.view(np.int64), dscores.view(np.int64)), (what, "scores differ from the dense call")
    assert np.array_equal(count, dcount), (what, "count differs from the dense call")
    field = tm.random_field(H, W, TILE)
    for tiled in field_forms:
        light = Flat(cuda, field if tiled else pixel_lights())
        lu, lv = M.bilinear_ref(field, H, W, TILE) if tiled else (pixel_lights()[:, 0], pixel_lights()[:, 1])
        for dt in ("f32", "u8"):
            w = f"{what} relight_field {'tiles' if tiled else 'pixels'} {dt}"
            got = relight_field(cuda, *src, lid, k, light.ptr, tiled, dt, w)
            want = M.relight_field_ref(m, lu, lv, BASIS_OF[k], np.dtype(OUT_NP[dt]).name)
            assert M.same_bits(got, want), (w, "differs from the reference")
            again = relight_field(cuda, *dense, lid, k, light.ptr, tiled, dt, w + " dense")
            assert np.array_equal(got.view(np.uint8), again.view(np.uint8)), (w, "differs from the dense call")
    return worst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", sorted(BASIS_OF))
def test_multilight_padded_channel_stride(cuda, k, form):
    """rti_light_scores (scores, count) and rti_relight_field (a tile field and lights per pixel, F32 and U8) over three
    maps a padded coef_channel_stride apart, both layouts."""
    assert TERMS[BASIS_OF[k]] == k
    m = M.image_maps(*HW, k, 3)
    for layout, lid in ts.LAYOUTS:
        far, dense = Maps(cuda, flat_maps(m, layout), form), Maps(cuda, flat_maps(m, layout), None)
        assert far.staged(layout) == (layout == "pixel" and form == "aligned")
        what = f"multi-light k={k} {layout} {form}"
        worst = check_multilight(cuda, k, layout, lid, (far.ptr, far.cs), (dense.ptr, 0), what)
        print(f"{what}: worst score error {worst:.3f} of its bound")


# ---- rti_photometric_stereo -----------------------------------------------------------------------------------------
PS_DTYPES = (("f32", None), ("i32", 128), ("u8", None))  # the poison as test_fit_shared_robust chooses it
PS_RUNS = ((0, 0), (2, 0), (2, L.RTI_KERNEL_ONE_LAUNCH))  # (iters, kernel): streaming, resident, streaming with IRLS
PS_VIEWS = (("chan", 3), ("light", 1), ("light", 3))  # the padded stride and C


def ps_window(dt):
    """integer stacks are the scene rounded under the window 1..254 (test_gpu_ps.test_integer_stacks)"""
    return (tp.LO, tp.HI) if dt == "f32" else (1.0, 254.0)


def ps_stack(dt, C):
    """the scene of test_gpu_ps.py at N = 20, P = 1316 -> [C, N, P]"""
    return tp.stack(PS_P, C, PS_N, dt != "f32")[3].reshape(C, PS_N, PS_P)


def ps_strides(view, form, dt):
    """(light_stride, channel pad, base offset) in elements"""
    vec = ts.vec_of(dt)
    ls = up(PS_P, vec) + (0 if view == "chan" else vec) + (form == "odd" and view == "light")
    cpad = 0 if view == "light" else 3 if form == "odd" else 2 * vec
    return ls, cpad, 1 if form == "offset" else 0


def ps_vec(base, ls, cs, es, C):
    """rti_ps.hip's predicate for 16-byte tile loads"""
    return base % 16 == 0 and ls * es % 16 == 0 and (C == 1 or cs * es % 16 == 0)


def ps_call(cuda, src, dt, P, C, ls, cs, iters, kernel, nl_id, what):
    """one call with every optional output requested -> [normals, albedo [C, P], kind, res [C, P], kept [C, P],
    fallback count], each array under (a)"""
    lo, hi = ps_window(dt)
    A = dev(tp.stack(P, C, PS_N, dt != "f32")[2], cuda)
    outs = [OutBuf(cuda, 3 * P), OutBuf(cuda, C * P), OutBuf(cuda, P, np.uint8), OutBuf(cuda, C * P),
            OutBuf(cuda, C * P, np.int32)]
    fb = torch.zeros(1, dtype=torch.int32, device=cuda)
    st = lib().rti_photometric_stereo(ptr(A), PS_N, src, ts.RTI_DT[dt], P, C, ls, cs, lo, hi, 3, iters, 5.0, None,
                                      outs[0].ptr, nl_id, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, ptr(fb),
                                      kernel, stream(cuda))
    assert st == L.RTI_OK, (what, lib().rti_last_error())
    n, albedo, kind, res, kept = (o.take(f"{what} {name}") for o, name in
                                  zip(outs, ("normals", "albedo", "kind", "res", "kept")))
    return [n, albedo.reshape(C, P), kind, res.reshape(C, P), kept.reshape(C, P), int(fb.item())]


def ps_plan(dt, C, iters, kernel):
    tile = int(lib().rti_photometric_stereo_plan(PS_N, ts.RTI_DT[dt], C, iters, kernel))
    assert tile == (256 if iters > 0 and kernel == 0 else 0), (dt, C, iters, kernel, tile)  # 60 planes of 256: <= 60 KiB
    return tile


def ps_ratios(n, got, ref):
    """figures only: the worst normal angle, albedo and res error of a call in units of test_gpu_ps.check's tolerances
    (0.01 degrees, 4e-4·‖g_c‖, 1e-3 + 1e-4·|res|); n [P, 3]"""
    ok = ref["kind"] <= 1
    chord = np.linalg.norm(n[ok].astype(np.float64) - ref["normals"][ok], axis=-1)
    angle = float(np.degrees(2.0 * np.arcsin(0.5 * chord)).max(initial=0.0)) / 0.01
    albedo = max(float((np.abs(got[1][c][ok] - ref["albedo"][c][ok]) / (4e-4 * np.linalg.norm(ref["g"][c][ok], axis=1))).max(initial=0.0))
                 for c in range(got[1].shape[0]))
    res = float((np.abs(got[3] - ref["res"]) / (1e-3 + 1e-4 * np.abs(ref["res"]))).max())
    return angle, albedo, res


def check_ps(cuda, src, dt, C, ls, cs, what):
    """every (iters, kernel) of PS_RUNS and both normal layouts on the stack at `src` under (a), (b) and (c) -> the tile
    sizes that ran"""
    P = PS_P
    integer = dt != "f32"
    dense = ts.In(cuda, ps_stack(dt, C), None, dt)
    tiles, worst = set(), (0.0, 0.0, 0.0)
    for iters, kernel in PS_RUNS:
        tiles.add(ps_plan(dt, C, iters, kernel))
        ref = tp.reference(P, C, iters, PS_N, integer)
        for nl, nid in NORMAL_LAYOUTS:
            w = f"{what} iters={iters} kernel={kernel:#x} normals {nl}"
            got = ps_call(cuda, src, dt, P, C, ls, cs, iters, kernel, nid, w)
            want = ps_call(cuda, dense.ptr, dt, P, C, P, PS_N * P, iters, kernel, nid, w + " dense")
            assert np.array_equal(got[4], want[4]), (w, "kept differs from the dense call")
            assert np.array_equal(got[4], ref["kept"]), (w, "kept differs from the reference")
            n = got[0].reshape((3, P) if nl == "planar" else (P, 3))
            tp.check([n, got[1].T if C == 3 else got[1][0], got[2], got[3], got[4], got[5]], ref, planar=nl == "planar")
            worst = tuple(max(a, b) for a, b in zip(worst, ps_ratios(n.T if nl == "planar" else n, got, ref)))
            for name, a, b in zip(("normals", "albedo", "kind", "res", "kept"), got, want):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (w, name, "differs from the dense call")
            assert got[5] == want[5] == ref["fallback_px"], (w, "fallback count")
    print(f"{what}: worst normal angle {worst[0]:.3g}, albedo {worst[1]:.3g}, res {worst[2]:.3g} of their bounds")
    return tiles


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt,poison", PS_DTYPES, ids=[d for d, _ in PS_DTYPES])
@pytest.mark.parametrize("view,C", PS_VIEWS, ids=[f"{v}-C{c}" for v, c in PS_VIEWS])
def test_photometric_stereo_padded_strides(cuda, view, C, dt, poison, form):
    """A padded channel_stride (C = 3) or a padded light_stride (C = 1 and 3), iters 0 and 2, both normal layouts, the
    six outputs.  kept is compared exactly with the dense call and with ps_ref: the window drops a sample it does not
    like without a sign, so a poison sample read as data shows there.  The streaming form (iters = 0, and
    RTI_KERNEL_ONE_LAUNCH with iters = 2) and the resident form of 256 pixels each run: in the aligned form the tile is
    staged by 16-byte loads, in the other two by elements."""
    ls, cpad, off = ps_strides(view, form, dt)
    buf, b, ls2, cs = sr.embed_stack(ps_stack(dt, C).astype(ts.NP_DT[dt]), ls - PS_P, cpad, off, poison)
    assert ls2 == ls and b.start == off
    t = dev(buf, cuda)
    src = ptr(t, off)
    assert ps_vec(src.value, ls, cs, t.element_size(), C) == (form == "aligned")
    tiles = check_ps(cuda, src, dt, C, ls, cs, f"rti_photometric_stereo {view} C={C} {dt} {form}")
    assert tiles == {0, 256}, tiles
