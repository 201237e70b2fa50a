"""rti_relight_lrgb_enhanced / rti_relight_lrgb8_enhanced / rti_relight_rgb8_enhanced without a GPU: the symbols are
bound, every argument check answers before any HIP call (the pointers below are never dereferenced) with a message
that names the function, the Python layer refuses host tensors, and tests/enhance_rgb_ref.py has the properties
DESIGN.md §4.12 claims for the arithmetic: a channel transformed about a peak that is not its own keeps its value and
gradient there and has g times its curvature, and the reference reduces to normals_ref.relight_enhanced_ref."""
import ctypes

import numpy as np
import pytest
import torch

import rti
from enhance_rgb_ref import (MODES, dequantise_lrgb_ref, diffuse_gain_coef_at, kinds_of, lrgb_enhanced_ref, peaked_rgb,
                             peaked_rgb8, rgb_enhanced_ref)
from lrgb_ref import mixed_lrgb
from normals_ref import peak_ref, ptm_value, relight_enhanced_ref
from rgb8_ref import LUMA, luminance
from rti import _lib as L

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
ODD = ctypes.c_void_p(4098)  # 2 bytes off: not 8-byte aligned
W3 = (ctypes.c_float * 3)
NAN, INF = float("nan"), float("inf")
DG, SPEC = L.RTI_ENHANCE_DIFFUSE_GAIN, L.RTI_ENHANCE_SPECULAR


def lrgb_call(lrgb=P_, layout=0, P=64, mode=SPEC, gain=1.0, kd=1.0, ks=0.5, exp=5, lu=0.1, lv=0.2, out=P_,
              odt=L.RTI_F32):
    return rti.load().rti_relight_lrgb_enhanced(lrgb, layout, P, mode, gain, kd, ks, exp, lu, lv, out, odt, None)


def lrgb8_call(coef8=P_, rgb8=P_, P=64, qparams=P_, mode=SPEC, gain=1.0, kd=1.0, ks=0.5, exp=5, lu=0.1, lv=0.2,
               out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_lrgb8_enhanced(coef8, rgb8, P, qparams, mode, gain, kd, ks, exp, lu, lv, out, odt,
                                                 None)


def rgb8_call(coef8=P_, P=64, qparams=P_, w=None, mode=SPEC, gain=1.0, kd=1.0, ks=0.5, exp=5, lu=0.1, lv=0.2, out=P_,
              odt=L.RTI_F32):
    return rti.load().rti_relight_rgb8_enhanced(coef8, P, qparams, w, mode, gain, kd, ks, exp, lu, lv, out, odt, None)


# what the three entries share
COMMON_BAD = {"null out": dict(out=None), "P = 0": dict(P=0), "P < 0": dict(P=-3), "mode 0": dict(mode=0),
              "mode 3": dict(mode=3), "mode < 0": dict(mode=-1), "NaN lu": dict(lu=NAN), "inf lv": dict(lv=INF),
              "NaN gain": dict(gain=NAN), "inf gain": dict(gain=INF), "NaN kd": dict(kd=NAN), "inf kd": dict(kd=-INF),
              "NaN ks": dict(ks=NAN), "inf ks": dict(ks=INF), "gain < 0": dict(gain=-0.5),
              "gain < 0, diffuse gain": dict(mode=DG, gain=-1e-9), "spec_exp 0": dict(exp=0),
              "spec_exp 256": dict(exp=256), "spec_exp < 0": dict(exp=-2)}
LRGB_BAD = dict(COMMON_BAD, **{"null lrgb": dict(lrgb=None), "layout 2": dict(layout=2), "layout < 0": dict(layout=-1)})
BYTES_BAD = dict(COMMON_BAD, **{"null coef8": dict(coef8=None), "null qparams": dict(qparams=None),
                                "qparams off a double": dict(qparams=ODD)})
LRGB8_BAD = dict(BYTES_BAD, **{"null rgb8": dict(rgb8=None)})
RGB8_BAD = dict(BYTES_BAD, **{"NaN weight": dict(w=W3(0.3, NAN, 0.1)), "inf weight": dict(w=W3(INF, 0.5, 0.1)),
                              "-inf weight": dict(w=W3(0.2, 0.5, -INF))})
UNSUPPORTED = {"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "out dtype < 0": dict(odt=-1)}
ENTRIES = {"rti_relight_lrgb_enhanced": (lrgb_call, LRGB_BAD), "rti_relight_lrgb8_enhanced": (lrgb8_call, LRGB8_BAD),
           "rti_relight_rgb8_enhanced": (rgb8_call, RGB8_BAD)}


def test_symbols_are_bound():
    lib = rti.load()
    for name in ENTRIES:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("relight_lrgb_enhanced", "relight_lrgb8_enhanced", "relight_rgb8_enhanced",
                 "relight_lrgb_enhanced_into", "relight_lrgb8_enhanced_into", "relight_rgb8_enhanced_into"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    for name in ("relight_lrgb_enhanced", "relight_lrgb8_enhanced", "relight_rgb8_enhanced"):
        assert hasattr(torch.ops.rti, name), name


@pytest.mark.parametrize("entry,case", [(e, c) for e in sorted(ENTRIES) for c in sorted(ENTRIES[e][1])])
def test_bad_arguments(entry, case):
    call, bad = ENTRIES[entry]
    assert call(**bad[case]) == L.RTI_ERR_BAD_ARG, case
    assert entry.encode() in rti.load().rti_last_error()


@pytest.mark.parametrize("entry,case", [(e, c) for e in sorted(ENTRIES) for c in sorted(UNSUPPORTED)])
def test_unsupported_output_types(entry, case):
    assert ENTRIES[entry][0](**UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert entry.encode() in rti.load().rti_last_error()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_spec_exp_is_not_read_in_diffuse_gain_mode(entry):
    """spec_exp outside [1, 255] is refused in specular mode only: with it and nothing else wrong, a diffuse gain
    call passes every check and the next refusal is the one planted behind it (an unsupported output type)."""
    assert ENTRIES[entry][0](mode=DG, exp=0, odt=L.RTI_F64) == L.RTI_ERR_UNSUPPORTED
    assert ENTRIES[entry][0](mode=SPEC, exp=0, odt=L.RTI_F64) == L.RTI_ERR_BAD_ARG


def test_python_layer_rejects_cpu_tensors_and_wrong_types():
    m = torch.zeros((4, 4, 9))
    ql = rti.QuantisedLRGB(torch.zeros((4, 4, 6), dtype=torch.uint8), torch.zeros((4, 4, 3), dtype=torch.uint8),
                           torch.ones(13, dtype=torch.float64))
    qr = rti.QuantisedRGB(torch.zeros((3, 4, 4, 6), dtype=torch.uint8), torch.ones(12, dtype=torch.float64))
    out = torch.zeros((16, 3))
    for call in (lambda: rti.relight_lrgb_enhanced(m, 0.1, 0.2, "specular"),
                 lambda: rti.relight_lrgb8_enhanced(ql, 0.1, 0.2, "diffuse_gain"),
                 lambda: rti.relight_rgb8_enhanced(qr, 0.1, 0.2, "specular"),
                 lambda: rti.relight_lrgb_enhanced_into(m, 0.1, 0.2, "specular", out),
                 lambda: rti.relight_lrgb8_enhanced_into(ql.coef, ql.rgb, ql.qparams, 0.1, 0.2, "specular", out),
                 lambda: rti.relight_rgb8_enhanced_into(qr.coef, qr.qparams, 0.1, 0.2, "specular", out)):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="QuantisedLRGB"):
        rti.relight_lrgb8_enhanced(qr, 0.1, 0.2, "specular")
    with pytest.raises(ValueError, match="QuantisedRGB"):
        rti.relight_rgb8_enhanced(ql, 0.1, 0.2, "specular")


# ---- the reference's properties ----------------------------------------------------------------------------------

@pytest.mark.parametrize("weights", [None, (0.2, 0.5, 0.3), (0.0, 0.0, 1.0)])
def test_a_channel_keeps_value_and_gradient_at_the_luminance_peak(weights):
    """For a channel a under the luminance's stationary point (u0, v0), which is not the channel's own (the
    channels are 0.8, 1.0 and 1.15 times one surface plus noise): L' has a's value and gradient there and g times
    a's second derivatives.  Bounds as tests/test_normals_abi.py derives them: the height sums ~20 terms <= 2e3 at
    2.2e-16 relative each, 1e-9 leaves 100x; a gradient component sums ~10 rounded terms no larger than a few
    times the largest coefficient, 1e-12 of that leaves 100x over 10·1.1e-16."""
    P = 3077
    deq = peaked_rgb8(P)[2]
    lum = luminance(deq, LUMA if weights is None else weights)
    k = peak_ref(lum)
    has = k["has_max"]
    assert has.sum() >= P // 2
    u0, v0 = k["u0"][has], k["v0"][has]

    def grad(c):
        return np.stack([2.0 * c[:, 0] * u0 + c[:, 2] * v0 + c[:, 3], 2.0 * c[:, 1] * v0 + c[:, 2] * u0 + c[:, 4]], -1)

    for ch in range(3):
        a = deq[ch].astype(np.float64)
        own = peak_ref(deq[ch])
        both = has & own["has_max"]
        if weights != (0.0, 0.0, 1.0) or ch != 2:  # the luminance's point is not the channel's
            assert np.abs(own["u0"][both] - k["u0"][both]).max() > 1e-6
        scale = np.abs(a[has]).max(1, keepdims=True)
        for g in (0.0, 0.5, 3.5, 10.0):
            b = diffuse_gain_coef_at(deq[ch], k, g)
            assert np.array_equal(b[~has], a[~has])                      # no maximum: the coefficients stay
            assert np.array_equal(b[has][:, :3], np.float64(g) * a[has][:, :3])  # the second derivatives, exactly
            herr = np.abs(ptm_value(b[has], u0, v0) - ptm_value(a[has], u0, v0)).max()
            gerr = (np.abs(grad(b[has]) - grad(a[has])) / scale).max()
            print(f"channel {ch} g={g}: height error {herr:.3g}, gradient error / scale {gerr:.3g}")
            assert herr <= 1e-9 and gerr <= 1e-12


def test_lrgb_with_unit_chroma_is_the_grey_reference():
    m = mixed_lrgb(2313, 3).copy()
    m[:, 6:] = 1.0
    grey = m[:, :6]
    fin = np.isfinite(grey).all(1)
    assert set(np.unique(kinds_of(grey))) == {0, 1, 2, 4}
    for lu, lv in ((0.3, -0.45), (0.8, 0.75), (0.0, 0.0)):
        for mode, kw in (("diffuse_gain", dict(gain=3.5)), ("diffuse_gain", dict(gain=0.0)),
                         ("specular", dict(kd=0.4, ks=150.0, exp=75)), ("specular", dict(kd=1.0, ks=2.0, exp=1))):
            want = relight_enhanced_ref(grey, lu, lv, mode, **kw)
            got = lrgb_enhanced_ref(m, lu, lv, mode, **kw)
            assert np.isnan(got[~fin]).all() and not np.isnan(got[fin]).any()
            for c in range(3):
                assert np.array_equal(got[fin, c].view(np.int64), want[fin].view(np.int64)), (mode, kw, c)


def test_lrgb_nan_chroma_and_nan_luminance():
    m = mixed_lrgb(255, 11).copy()
    fin = np.isfinite(m[:, :6]).all(1)
    px = np.flatnonzero(fin)[:3]
    m[px[0], 6], m[px[1], 7], m[px[2], 8] = np.nan, np.nan, np.nan
    for mode in MODES:
        got = lrgb_enhanced_ref(m, 0.3, -0.45, mode, gain=2.0, kd=0.4, ks=150.0, exp=9)
        assert np.isnan(got[~fin]).all()
        nan = np.isnan(got[px])
        assert np.array_equal(nan, np.eye(3, dtype=bool)), mode  # its own channel only


@pytest.mark.parametrize("ch", [0, 1, 2])
def test_rgb_with_a_unit_weight_is_the_grey_reference_of_that_channel(ch):
    P = 3077
    deq = peaked_rgb8(P)[2]
    w = tuple(1.0 if c == ch else 0.0 for c in range(3))
    assert np.array_equal(luminance(deq, w), deq[ch])
    assert set(np.unique(kinds_of(deq[ch]))) == {0, 1, 2}
    for lu, lv in ((0.3, -0.45), (0.8, 0.75), (0.0, 0.0)):
        for mode, kw in (("diffuse_gain", dict(gain=3.5)), ("specular", dict(kd=0.4, ks=150.0, exp=75))):
            want = relight_enhanced_ref(deq[ch], lu, lv, mode, **kw)
            got = rgb_enhanced_ref(deq, lu, lv, mode, weights=w, **kw)
            assert np.array_equal(got[:, ch].view(np.int64), want.view(np.int64)), (mode, lu, lv)


def test_identities_reproduce_the_plain_colour_image():
    """g = 1 and (kd, ks) = (1, 0) are the plain renderings, exactly: chroma·L for LRGB, L_c for RGB."""
    m = mixed_lrgb(1028, 4)
    fin = np.isfinite(m[:, :6]).all(1)
    deq = peaked_rgb8(1028)[2]
    for lu, lv in ((0.3, -0.45), (0.8, 0.75)):
        plain = m[:, 6:].astype(np.float64) * ptm_value(m[:, :6].astype(np.float64), np.float64(lu), np.float64(lv))[:, None]
        chan = np.stack([ptm_value(deq[c].astype(np.float64), np.float64(lu), np.float64(lv)) for c in range(3)], -1)
        for mode, kw in (("diffuse_gain", dict(gain=1.0)), ("specular", dict(kd=1.0, ks=0.0, exp=75))):
            got = lrgb_enhanced_ref(m, lu, lv, mode, **kw)
            assert np.array_equal(got[fin], plain[fin], equal_nan=True) and np.isnan(got[~fin]).all()
            assert np.array_equal(rgb_enhanced_ref(deq, lu, lv, mode, **kw), chan)


def test_dequantise_lrgb_ref_is_read_ptms_map(tmp_path):
    m = mixed_lrgb(300, 8).reshape(12, 25, 9)
    with np.errstate(all="ignore"):
        path = rti.write_ptm(str(tmp_path / "m.ptm"), m)
    fmt, back = rti.read_ptm(path)
    q = rti.read_ptm(path, quantised=True)[1]
    got = dequantise_lrgb_ref(q.coef.numpy().reshape(-1, 6), q.rgb.numpy().reshape(-1, 3), q.qparams.numpy())
    assert fmt == "lrgb" and np.array_equal(got.view(np.uint32), back.reshape(-1, 9).view(np.uint32))
