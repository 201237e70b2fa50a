"""rti_relight_rgb / rti_relight_rgb_enhanced / rti_rgb_normals without a GPU: the symbols are bound, every argument
check answers before any HIP call (the pointers below are never dereferenced; w is a host array) with a message
that names the entry, the Python layer refuses what it can judge without a device, tests/rgb_ref.py agrees with the
references it is assembled from, and the far-stride plans of tests/test_gpu_rgb.py keep far_ref's promises."""
import ctypes

import numpy as np
import pytest
import torch

import far_ref as fr
import rti
from enhance_rgb_ref import MODES
from normals_ref import normals_ref, relight_enhanced_ref
from rgb8_ref import LUMA, luminance
from rgb_ref import TERMS, bad_pixels, far_maps_plan, nonfinite_rgb, rgb_enhanced, rgb_normals_ref
from rti import _lib as L

P_ = ctypes.c_void_p(4096)  # aligned for every vector access
W3 = (ctypes.c_float * 3)
NAN, INF = float("nan"), float("inf")
DG, SP = L.RTI_ENHANCE_DIFFUSE_GAIN, L.RTI_ENHANCE_SPECULAR


def relight_call(coef=P_, basis=L.RTI_BASIS_PTM6, layout=0, stride=0, P=64, luv=P_, E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_rgb(coef, basis, layout, stride, P, luv, E, out, odt, None)


def enhanced_call(coef=P_, layout=0, stride=0, P=64, w=None, mode=DG, gain=1.0, kd=1.0, ks=0.0, exp=1, lu=0.1, lv=0.2,
                  out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_rgb_enhanced(coef, layout, stride, P, w, mode, gain, kd, ks, exp, lu, lv, out, odt,
                                               None)


def normals_call(coef=P_, layout=0, stride=0, P=64, w=None, normals=P_, nl=0, kind=None, peak=None):
    return rti.load().rti_rgb_normals(coef, layout, stride, P, w, normals, nl, kind, peak, None)


MAPS_BAD = {"null coef": dict(coef=None), "P = 0": dict(P=0), "P < 0": dict(P=-4), "layout": dict(layout=2),
            "layout < 0": dict(layout=-1), "stride below dense": dict(stride=6 * 64 - 1), "stride < 0": dict(stride=-8)}
WEIGHTS_BAD = {"NaN weight": dict(w=W3(0.3, NAN, 0.1)), "inf weight": dict(w=W3(INF, 0.5, 0.1)),
               "-inf weight": dict(w=W3(0.3, 0.5, -INF))}
RELIGHT_BAD = dict(MAPS_BAD, **{
    "null luv": dict(luv=None), "null out": dict(out=None), "E = 0": dict(E=0), "E < 0": dict(E=-2),
    "unknown basis": dict(basis=7), "basis < 0": dict(basis=-1),
    "hsh9 stride below dense": dict(basis=L.RTI_BASIS_HSH9, stride=9 * 64 - 1),
    "hsh16 stride of ptm": dict(basis=L.RTI_BASIS_HSH16, stride=6 * 64)})
OUT_UNSUPPORTED = {"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "out dtype < 0": dict(odt=-1)}
ENHANCED_BAD = dict(MAPS_BAD, **WEIGHTS_BAD, **{
    "null out": dict(out=None), "mode 0": dict(mode=0), "mode 3": dict(mode=3), "NaN lu": dict(lu=NAN),
    "inf lv": dict(lv=INF), "NaN gain": dict(gain=NAN), "inf kd": dict(kd=INF), "NaN ks": dict(mode=SP, ks=NAN),
    "gain < 0": dict(gain=-0.5), "exp = 0": dict(mode=SP, exp=0), "exp = 256": dict(mode=SP, exp=256),
    "exp < 0": dict(mode=SP, exp=-3)})
NORMALS_BAD = dict(MAPS_BAD, **WEIGHTS_BAD, **{
    "null normals": dict(normals=None), "normal layout": dict(nl=2), "normal layout < 0": dict(nl=-1)})


@pytest.mark.parametrize("case", sorted(RELIGHT_BAD))
def test_relight_rgb_bad_arguments(case):
    assert relight_call(**RELIGHT_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_relight_rgb:" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(OUT_UNSUPPORTED))
def test_relight_rgb_unsupported(case):
    for basis in (L.RTI_BASIS_PTM6, L.RTI_BASIS_HSH9, L.RTI_BASIS_HSH16):
        assert relight_call(basis=basis, **OUT_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, (case, basis)
        assert b"rti_relight_rgb:" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(ENHANCED_BAD))
def test_relight_rgb_enhanced_bad_arguments(case):
    assert enhanced_call(**ENHANCED_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_relight_rgb_enhanced:" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(OUT_UNSUPPORTED))
def test_relight_rgb_enhanced_unsupported(case):
    for mode in (DG, SP):
        assert enhanced_call(mode=mode, **OUT_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, (case, mode)
        assert b"rti_relight_rgb_enhanced:" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(NORMALS_BAD))
def test_rgb_normals_bad_arguments(case):
    assert normals_call(**NORMALS_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_rgb_normals:" in rti.load().rti_last_error()


def test_spec_exp_is_judged_in_specular_mode_only():
    """Diffuse gain ignores spec_exp, so an exponent outside [1, 255] is no error there: the next check (a
    non-finite weight) answers instead of it."""
    w = W3(NAN, 0.5, 0.1)
    assert enhanced_call(mode=DG, exp=0, w=w) == L.RTI_ERR_BAD_ARG
    assert b"weight" in rti.load().rti_last_error()
    assert enhanced_call(mode=SP, exp=0, w=w) == L.RTI_ERR_BAD_ARG
    assert b"spec_exp" in rti.load().rti_last_error()


def test_symbols_are_bound():
    lib = rti.load()
    for name in ("rti_relight_rgb", "rti_relight_rgb_enhanced", "rti_rgb_normals"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("relight_rgb", "relight_rgb_into", "relight_rgb_enhanced", "relight_rgb_enhanced_into",
                 "rgb_normals", "rgb_normals_into"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name
    assert lib.rti_version() == 100


def test_python_layer_refuses_before_any_launch():
    m = torch.zeros((3, 4, 4, 6))
    luv = torch.zeros((1, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb(m, 0.1, 0.2)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb_enhanced(m, 0.1, 0.2, "diffuse_gain")
    with pytest.raises(ValueError, match="CUDA"):
        rti.rgb_normals(m)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb_into(m, luv, torch.zeros((1, 16, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb_enhanced_into(m, 0.1, 0.2, "specular", torch.zeros((16, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.rgb_normals_into(m, torch.zeros((16, 3)))
    # the two PTM-only functions name a basis they do not read before they look at the tensor
    for basis in ("hsh9", "hsh16", L.RTI_BASIS_HSH16):
        with pytest.raises(NotImplementedError, match="PTM-6"):
            rti.relight_rgb_enhanced(m, 0.1, 0.2, "diffuse_gain", basis=basis)
        with pytest.raises(NotImplementedError, match="PTM-6"):
            rti.rgb_normals(m, basis=basis)
        with pytest.raises(NotImplementedError, match="PTM-6"):
            rti.relight_rgb_enhanced_into(m, 0.1, 0.2, "specular", torch.zeros((16, 3)), basis=basis)
        with pytest.raises(NotImplementedError, match="PTM-6"):
            rti.rgb_normals_into(m, torch.zeros((16, 3)), basis=basis)
    for fn in (lambda: rti.relight_rgb(m, 0.1, 0.2, basis="rbf"), lambda: rti.rgb_normals(m, basis="nope"),
               lambda: rti.relight_rgb(m, 0.1, 0.2, layout="rows"), lambda: rti.rgb_normals(m, normal_layout="rows"),
               lambda: rti.relight_rgb_enhanced(m, 0.1, 0.2, "glossy", layout="rows")):
        with pytest.raises(ValueError):
            fn()


# ---- tests/rgb_ref.py against the references it is assembled from -----------------------------------------------

@pytest.mark.parametrize("P", [7, 255, 1028])
def test_ref_normals_are_the_luminance_maps(P):
    m = nonfinite_rgb(P)
    for w in (None, (0.2, 0.5, 0.3)):
        n, kind, peak = rgb_normals_ref(m, w)
        r = normals_ref(luminance(m, LUMA if w is None else w))
        assert n.dtype == peak.dtype == np.float32 and kind.dtype == np.uint8 and n.shape == (P, 3)
        assert np.array_equal(kind, r["kind"]) and np.array_equal(kind == 4, bad_pixels(m))
        assert np.isnan(n[kind == 4]).all() and np.isnan(peak[kind == 4]).all() and np.isfinite(n[kind != 4]).all()
    if P >= 255:
        assert set(rgb_normals_ref(m)[1].tolist()) == {0, 1, 2, 4}


@pytest.mark.parametrize("mode", MODES)
def test_ref_channel_with_unit_weight_is_the_grey_reference(mode):
    """With the weight on channel c the luminance IS that map (1·x + 0·y + 0·z is exact for finite values), so the
    channel is normals_ref.relight_enhanced_ref of it; non-finite pixels are NaN in three channels."""
    P = 255
    m = nonfinite_rgb(P)
    kw = dict(gain=2.5, kd=0.4, ks=150.0, exp=20)
    fin = ~bad_pixels(m)
    for c in range(3):
        w = [0.0, 0.0, 0.0]
        w[c] = 1.0
        got = rgb_enhanced(m, 0.3, -0.45, mode, "float32", weights=w, **kw)
        grey = {k: v for k, v in kw.items() if (k == "gain") == (mode == "diffuse_gain")}
        want = relight_enhanced_ref(m[c], 0.3, -0.45, mode, **grey).astype(np.float32)
        assert np.array_equal(got[fin, c].view(np.uint32), want[fin].view(np.uint32)), c
        assert np.isnan(got[~fin]).all()
    assert rgb_enhanced(m, 0.3, -0.45, mode, "uint8", **kw).dtype == np.uint8
    assert rgb_enhanced(m, 0.3, -0.45, mode, "int32", **kw)[~fin].tolist() == [[-2 ** 31] * 3] * int((~fin).sum())


# ---- the far-stride plans of tests/test_gpu_rgb.py ------------------------------------------------------------------

@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("basis", sorted(TERMS))
def test_far_plans_keep_far_refs_promises(basis, variant):
    """What tests/test_far_ref.py checks for far_ref.PLANS: the far offsets pass both limits, every 32-bit
    truncation of a corner offset lies inside the allocation and outside every payload, and the allocation is
    under the memory cap."""
    k = TERMS[basis]
    p = far_maps_plan(k, variant)
    assert p.counts == (3, 1) and p.inner == fr.P16 * k and p.es == 4
    assert p.nbytes() <= fr.CAP_BYTES, p.describe()
    cs = p.strides[0]
    assert cs * 4 > fr.LIM_BYTES and 2 * cs > fr.LIM_ELEMS and cs >= p.inner
    assert (cs % 4 == 0) == (variant == "aligned") and p.base % 4 == 0
    for e in p.corner_offsets():
        assert 0 <= p.base + e < p.length
        for t in fr.truncations(e, 4):
            assert 0 <= p.base + t < p.length, (e, t)
            assert t == e or not p.in_payload(t), (e, t)
