"""rti_ptm_normals / rti_relight_enhanced without a GPU: every argument check answers before any HIP call (the
pointers below are never dereferenced) with a message that names the function, both symbols are bound, and the
NumPy restatement (tests/normals_ref.py) is checked against coefficients constructed with known peaks."""
import ctypes

import numpy as np
import pytest

import rti
from normals_ref import (diffuse_gain_coef, mixed_coef, normals_ref, peak_ref, peaked_coef, ptm_value,
                         relight_enhanced_ref)
from rti import _lib as L

P_ = ctypes.c_void_p(4096)
NAN, INF = float("nan"), float("inf")


def normals_call(coef=P_, dt=L.RTI_F32, basis=L.RTI_BASIS_PTM6, layout=0, P=64, normals=P_, nl=0, kind=None, peak=None):
    return rti.load().rti_ptm_normals(coef, dt, basis, layout, P, normals, nl, kind, peak, None)


def enhanced_call(coef=P_, dt=L.RTI_F32, basis=L.RTI_BASIS_PTM6, layout=0, P=64, mode=L.RTI_ENHANCE_DIFFUSE_GAIN,
                  gain=1.0, kd=1.0, ks=0.0, e=1, lu=0.1, lv=0.2, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_enhanced(coef, dt, basis, layout, P, mode, gain, kd, ks, e, lu, lv, out, odt, None)


NORMALS_BAD = {
    "null coef": dict(coef=None), "null normals": dict(normals=None), "P = 0": dict(P=0), "P < 0": dict(P=-4),
    "coef layout": dict(layout=2), "normal layout": dict(nl=2), "normal layout < 0": dict(nl=-1),
}
NORMALS_UNSUPPORTED = {
    "hsh16": dict(basis=L.RTI_BASIS_HSH16), "hsh9": dict(basis=L.RTI_BASIS_HSH9), "unknown basis": dict(basis=99),
    "u8 coef": dict(dt=L.RTI_U8), "i32 coef": dict(dt=L.RTI_I32), "unknown coef dtype": dict(dt=7),
}
SPEC = dict(mode=L.RTI_ENHANCE_SPECULAR)
ENHANCED_BAD = {
    "null coef": dict(coef=None), "null out": dict(out=None), "P = 0": dict(P=0), "coef layout": dict(layout=-1),
    "mode 0": dict(mode=0), "mode 3": dict(mode=3),
    "NaN lu": dict(lu=NAN), "inf lv": dict(lv=INF), "NaN gain": dict(gain=NAN), "inf gain": dict(gain=INF),
    "NaN kd": dict(kd=NAN, **SPEC), "inf ks": dict(ks=-INF, **SPEC), "NaN ks in diffuse mode": dict(ks=NAN),
    "gain < 0": dict(gain=-0.5), "gain < 0 in specular mode": dict(gain=-1.0, **SPEC),
    "exp 0": dict(e=0, **SPEC), "exp 256": dict(e=256, **SPEC), "exp < 0": dict(e=-3, **SPEC),
}
ENHANCED_UNSUPPORTED = {
    "hsh16": dict(basis=L.RTI_BASIS_HSH16), "hsh9": dict(basis=L.RTI_BASIS_HSH9, **SPEC),
    "unknown basis": dict(basis=-1), "u8 coef": dict(dt=L.RTI_U8), "i32 coef": dict(dt=L.RTI_I32),
    "f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9, **SPEC),
}


@pytest.mark.parametrize("case", sorted(NORMALS_BAD))
def test_normals_bad_arguments(case):
    assert normals_call(**NORMALS_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_ptm_normals" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(NORMALS_UNSUPPORTED))
def test_normals_unsupported(case):
    assert normals_call(**NORMALS_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_ptm_normals" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(ENHANCED_BAD))
def test_enhanced_bad_arguments(case):
    assert enhanced_call(**ENHANCED_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_relight_enhanced" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(ENHANCED_UNSUPPORTED))
def test_enhanced_unsupported(case):
    assert enhanced_call(**ENHANCED_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_relight_enhanced" in rti.load().rti_last_error()


def test_spec_exp_is_checked_in_specular_mode_only():
    # an exponent outside [1, 255] is no error in diffuse gain mode: the call gets past it to the next check
    assert enhanced_call(e=0, odt=L.RTI_F64) == L.RTI_ERR_UNSUPPORTED
    assert b"out dtype" in rti.load().rti_last_error()


def test_symbols_and_constants():
    assert "rti_ptm_normals" in L.SIGNATURES and "rti_relight_enhanced" in L.SIGNATURES
    lib = rti.load()
    assert hasattr(lib, "rti_ptm_normals") and hasattr(lib, "rti_relight_enhanced")
    assert (L.RTI_ENHANCE_DIFFUSE_GAIN, L.RTI_ENHANCE_SPECULAR) == (1, 2)
    # the Python layer shapes normal maps with the coefficient-layout helpers: the values must coincide
    assert (L.RTI_NORMAL_PIXEL_MAJOR, L.RTI_NORMAL_PLANAR) == (L.RTI_COEF_PIXEL_MAJOR, L.RTI_COEF_PLANAR) == (0, 1)
    assert rti.api.ENHANCE_MODES == {"diffuse_gain": 1, "specular": 2}


def test_python_layer_rejects_cpu_tensors_and_wrong_shapes():
    import torch

    with pytest.raises(ValueError, match="CUDA"):
        rti.normals(torch.zeros((4, 4, 6)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_enhanced(torch.zeros((4, 4, 6)), 0.1, 0.2, "diffuse_gain")
    with pytest.raises(ValueError, match="CUDA"):
        rti.ptm_normals_into(torch.zeros((16, 6)), torch.zeros((16, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_enhanced_into(torch.zeros((16, 6)), 0.1, 0.2, "specular", torch.zeros(16))


# ---- the reference against construction -----------------------------------------------------------------------

def constructed(seed=5, P=4000):
    rng = np.random.default_rng(seed)
    inner, ui, vi, hi = peaked_coef(rng, P, 0.0, 0.9)
    outer, uo, vo, ho = peaked_coef(rng, P, 1.1, 2.0)
    coef = np.concatenate([inner, outer]).astype(np.float32)  # stored as the fit stores them
    return coef, np.concatenate([ui, uo]), np.concatenate([vi, vo]), np.concatenate([hi, ho]), P


def test_reference_recovers_constructed_normals():
    """Peaks placed at known (u0, v0): interior ones give n = (u0, v0, sqrt(1 − r²)), outer ones (u0, v0, 0)/r.
    Bound 1e-5: the fp32 rounding of the stored coefficients moves the normal by 2.5e-7 (printed), 40x below."""
    coef, u0, v0, h, P = constructed()
    r = normals_ref(coef)
    assert (r["kind"][:P] == 0).all() and (r["kind"][P:] == 1).all()
    rad = np.hypot(u0, v0)
    want = np.stack([u0, v0, np.sqrt(np.maximum(0.0, 1.0 - rad * rad))], -1)
    want[P:] = np.stack([u0[P:] / rad[P:], v0[P:] / rad[P:], np.zeros(P)], -1)
    err = np.abs(r["n"] - want).max()
    print(f"normal recovery error {err:.3g}")
    assert err <= 1e-5
    assert np.abs(np.linalg.norm(r["n"], axis=1) - 1.0).max() <= 1e-12
    # the peak value at an interior maximum is the constructed height (fp32 coefficient rounding: |a5| <= 1e3
    # and five more terms of that size, each rounded to 2^-24 relative)
    assert np.abs(r["peak"][:P] - h[:P]).max() <= 6 * 1e3 * 2.0 ** -24


def test_reference_classes():
    rng = np.random.default_rng(2)
    saddle = peaked_coef(rng, 500, 0.0, 2.0, "saddle")[0].astype(np.float32)
    r = normals_ref(saddle)
    assert (r["kind"] == 2).all() and (r["D"] / r["S"] <= -0.5).all()
    g = np.stack([saddle[:, 3], saddle[:, 4], np.maximum(saddle[:, 5], 0)], -1).astype(np.float64)
    assert np.abs(r["n"] - g / np.linalg.norm(g, axis=1, keepdims=True)).max() <= 1e-15
    minima = peaked_coef(rng, 500, 0.0, 2.0, 1.0)[0].astype(np.float32)
    assert (normals_ref(minima)["kind"] == 2).all()
    z = normals_ref(np.zeros((3, 6), np.float32))
    assert (z["kind"] == 2).all() and np.array_equal(z["n"], np.tile([0.0, 0.0, 1.0], (3, 1))) and not z["peak"].any()
    bad = np.tile(peaked_coef(rng, 1, 0.0, 0.5)[0], (18, 1))
    for i in range(6):
        bad[3 * i, i], bad[3 * i + 1, i], bad[3 * i + 2, i] = np.nan, np.inf, -np.inf
    b = normals_ref(bad)
    assert (b["kind"] == 4).all() and np.isnan(b["n"]).all() and np.isnan(b["peak"]).all()
    for mode in ("diffuse_gain", "specular"):
        assert np.isnan(relight_enhanced_ref(bad, 0.2, 0.1, mode, gain=2.0, kd=0.4, ks=150.0, exp=9)).all()
    m = normals_ref(mixed_coef(2313, 0))
    assert set(np.unique(m["kind"])) == {0, 1, 2, 4}
    far = m["finite"] & (m["S"] > 0)
    assert (np.abs(m["D"][far] / m["S"][far]) >= 0.5).all()  # far from the maximum test's threshold
    assert (np.abs(m["r2"][m["has_max"]] - 1.0) >= 0.15).all()  # and from the disc's edge


def test_diffuse_gain_keeps_the_peak():
    """L' has the stationary point and the height of L there, and g times its curvature.  Bounds, for |u0| <= 2,
    curvatures <= 200 and values <= 1e3 (so intermediate terms <= 2e3): the location is a 2x2 solve of condition
    <= 4 on numbers that carry ~10 roundings, 1e-12 leaves 100x over 4·10·2.2e-16·(1 + |u0|); the height sums ~20
    terms <= 2e3 at 2.2e-16 relative each = 9e-12, 1e-9 leaves 100x."""
    coef, u0, v0, h, P = constructed(seed=8, P=2000)
    base = normals_ref(coef)
    L0 = ptm_value(base["a"], base["u0"], base["v0"])
    for g in (0.0, 0.5, 3.0, 10.0):
        b = diffuse_gain_coef(coef, g)
        assert np.array_equal(b[:, :3], g * base["a"][:, :3])
        if g > 0:
            k = peak_ref(b)
            assert k["has_max"].all()
            assert max(np.abs(k["u0"] - base["u0"]).max(), np.abs(k["v0"] - base["v0"]).max()) <= 1e-12
        else:  # a plane: its gradient vanishes and its value is the peak's everywhere
            assert np.abs(b[:, 3:5]).max() <= 1e-10
        assert np.abs(ptm_value(b, base["u0"], base["v0"]) - L0).max() <= 1e-9


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identities_reproduce_the_plain_value(dtype):
    """g = 1 and (kd, ks) = (1, 0) are the plain PTM value, exactly: (1 − g) = 0 multiplies finite numbers, so
    a3', a4', a5' are a3 + 0, a4 + 0, a5 + 0, and 1·L + 0·x = L."""
    coef = mixed_coef(2313, 3, dtype)
    a = coef.astype(np.float64)
    fin = np.isfinite(a).all(1)
    for lu, lv in ((0.0, 0.0), (0.3, -0.45), (0.8, 0.75)):
        plain = ptm_value(a, np.float64(lu), np.float64(lv))
        for got in (relight_enhanced_ref(coef, lu, lv, "diffuse_gain", gain=1.0),
                    relight_enhanced_ref(coef, lu, lv, "specular", kd=1.0, ks=0.0, exp=75)):
            assert np.array_equal(got[fin], plain[fin]) and np.isnan(got[~fin]).all()
