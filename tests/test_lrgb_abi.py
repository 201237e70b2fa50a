"""rti_lrgb_from_rgb / rti_relight_lrgb without a GPU: every argument check answers before any HIP call (the
pointers below are never dereferenced) with a message that names the function, both symbols are bound, rti.gram is
AᵀA, and the NumPy restatement (tests/lrgb_ref.py) is checked against the least-squares colour computed directly
from a stack."""
import ctypes

import numpy as np
import pytest

import rti
from lrgb_ref import lrgb_ref, luminance_ref, relight_lrgb_ref, synth_dirs, to_int32, to_uint8
from rti import _lib as L

P_ = ctypes.c_void_p(4096)
NAN, INF = float("nan"), float("inf")
EYE = np.eye(6)


def dbl(values):
    return None if values is None else (ctypes.c_double * len(values))(*values)


def compress_call(coef=P_, layout=0, stride=0, P=64, gram=EYE.ravel(), weights=None, lrgb=P_, ol=0):
    g = dbl(None if gram is None else list(gram))
    return rti.load().rti_lrgb_from_rgb(coef, layout, stride, P, g, dbl(weights), lrgb, ol, None)


def relight_call(lrgb=P_, layout=0, P=64, luv=P_, E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_lrgb(lrgb, layout, P, luv, E, out, odt, None)


def gram_with(i, v):
    g = EYE.ravel().copy()
    g[i] = v
    return g


COMPRESS_BAD = {
    "null coef": dict(coef=None), "null gram": dict(gram=None), "null lrgb": dict(lrgb=None),
    "P = 0": dict(P=0), "P < 0": dict(P=-4),
    "coef layout": dict(layout=2), "coef layout < 0": dict(layout=-1), "lrgb layout": dict(ol=2),
    "lrgb layout < 0": dict(ol=-1),
    "stride below dense": dict(stride=6 * 64 - 1), "stride < 0": dict(stride=-6 * 64),
    "NaN gram": dict(gram=gram_with(0, NAN)), "inf gram": dict(gram=gram_with(35, INF)),
    "-inf gram": dict(gram=gram_with(17, -INF)),
    "negative weight": dict(weights=[0.5, -0.1, 0.6]), "NaN weight": dict(weights=[NAN, 0.5, 0.5]),
    "inf weight": dict(weights=[0.5, 0.5, INF]), "zero weights": dict(weights=[0.0, 0.0, 0.0]),
}
RELIGHT_BAD = {
    "null lrgb": dict(lrgb=None), "null luv": dict(luv=None), "null out": dict(out=None),
    "P = 0": dict(P=0), "P < 0": dict(P=-1), "E = 0": dict(E=0), "layout": dict(layout=2),
    "layout < 0": dict(layout=-1),
}
RELIGHT_UNSUPPORTED = {"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "out dtype < 0": dict(odt=-1)}


@pytest.mark.parametrize("case", sorted(COMPRESS_BAD))
def test_lrgb_from_rgb_bad_arguments(case):
    assert compress_call(**COMPRESS_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_lrgb_from_rgb" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(RELIGHT_BAD))
def test_relight_lrgb_bad_arguments(case):
    assert relight_call(**RELIGHT_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_relight_lrgb" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(RELIGHT_UNSUPPORTED))
def test_relight_lrgb_unsupported(case):
    assert relight_call(**RELIGHT_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_relight_lrgb" in rti.load().rti_last_error()


def test_symbols_are_bound():
    assert "rti_lrgb_from_rgb" in L.SIGNATURES and "rti_relight_lrgb" in L.SIGNATURES
    lib = rti.load()
    assert hasattr(lib, "rti_lrgb_from_rgb") and hasattr(lib, "rti_relight_lrgb")
    for name in ("gram", "lrgb_from_rgb", "lrgb_from_rgb_into", "fit_lrgb", "relight_lrgb", "relight_lrgb_into",
                 "lrgb_luminance", "read_ptm", "write_ptm"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name


def test_gram_is_the_designs():
    lu, lv = synth_dirs(12, 3)
    A = rti.design_matrix(lu, lv)
    G = rti.gram(lu, lv)
    assert G.shape == (6, 6) and G.dtype == np.float64
    assert np.array_equal(G, A.T @ A)


def test_python_layer_rejects_cpu_tensors_and_wrong_shapes():
    import torch

    g = np.eye(6)
    with pytest.raises(ValueError, match="CUDA"):
        rti.lrgb_from_rgb(torch.zeros((3, 4, 4, 6)), g)
    with pytest.raises(ValueError, match="CUDA"):
        rti.lrgb_from_rgb_into(torch.zeros((3, 16, 6)), g, torch.zeros((16, 9)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.fit_lrgb(torch.zeros((3, 8, 4, 4)), np.zeros(8), np.zeros(8))
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_lrgb(torch.zeros((4, 4, 9)), 0.1, 0.2)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_lrgb_into(torch.zeros((16, 9)), torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 16, 3)))
    # the luminance view is host-side: same storage, no copy; pixel-major maps are refused
    m = torch.arange(9 * 3 * 5, dtype=torch.float32).reshape(9, 3, 5)
    lum = rti.lrgb_luminance(m)
    assert lum.shape == (6, 3, 5) and lum.data_ptr() == m.data_ptr() and lum.is_contiguous()
    assert torch.equal(lum, m[:6])
    with pytest.raises(ValueError, match="planar"):
        rti.lrgb_luminance(m.permute(1, 2, 0).contiguous(), layout="pixel")
    with pytest.raises(ValueError):
        rti.lrgb_luminance(torch.zeros((6, 3, 5)))


# ---- the restatement's mathematics, from a stack -----------------------------------------------------------------

def stack_case(seed=11):
    """A random [3, 12, 5, 7] fp64 stack, its per-channel least-squares coefficients [3, P, 6], A and G."""
    rng = np.random.default_rng(seed)
    lu, lv = synth_dirs(12, seed)
    A = rti.design_matrix(lu, lv)
    I = rng.uniform(5.0, 250.0, (3, 12, 35))
    coef = np.stack([np.linalg.lstsq(A, I[c], rcond=None)[0].T for c in range(3)])
    return I, coef, A, A.T @ A


@pytest.mark.parametrize("weights", [None, (0.299, 0.587, 0.114)])
def test_reference_chroma_is_the_least_squares_colour(weights):
    I, coef, A, G = stack_case()
    m = lrgb_ref(coef, G, weights)
    w = np.full(3, 1.0 / 3.0) if weights is None else np.asarray(weights)
    a = np.einsum("c,cpj->pj", w, coef)
    assert np.abs(m[:, :6] - a).max() <= 1e-12 * np.abs(a).max()
    Lhat = A @ m[:, :6].T  # [N, P]: the fitted luminance at every light
    direct = np.stack([(I[c] * Lhat).sum(0) / (Lhat * Lhat).sum(0) for c in range(3)], -1)
    rel = np.abs(m[:, 6:] - direct) / np.abs(direct)
    print(f"chroma vs direct least squares: {rel.max():.3g}")
    assert rel.max() <= 1e-9
    assert np.abs(m[:, 6:] @ w - 1.0).max() <= 1e-12


def test_reference_separates_a_rank_one_stack():
    """I_c,n = k_c·m_n: chroma = k_c/Σ w·k and L = Σ w·k · fit(m), for both weightings."""
    rng = np.random.default_rng(4)
    lu, lv = synth_dirs(12, 4)
    A = rti.design_matrix(lu, lv)
    mono = rng.uniform(5.0, 250.0, (12, 35))
    fit_m = np.linalg.lstsq(A, mono, rcond=None)[0].T  # [P, 6]
    k = np.array([1.7, 0.9, 0.25])
    coef = k[:, None, None] * fit_m[None]
    for weights in (None, (0.299, 0.587, 0.114)):
        w = np.full(3, 1.0 / 3.0) if weights is None else np.asarray(weights)
        m = lrgb_ref(coef, A.T @ A, weights)
        wk = float(w @ k)
        assert np.abs(m[:, 6:] - k / wk).max() <= 1e-12
        assert np.abs(m[:, :6] - wk * fit_m).max() <= 1e-12 * np.abs(fit_m).max()


def test_reference_black_and_nan_pixels():
    _, coef, _, G = stack_case(seed=12)
    coef = coef.astype(np.float32)
    coef[:, 3] = 0.0          # black: d = 0
    coef[1, 5, 2] = np.nan    # one NaN coefficient
    coef[2, 6, 0] = np.inf    # one infinite coefficient
    m = lrgb_ref(coef, G)
    assert np.array_equal(m[3], [0, 0, 0, 0, 0, 0, 1, 1, 1])
    assert np.isnan(m[5]).all() and np.isnan(m[6]).all()
    rest = np.delete(np.arange(35), [5, 6])
    assert np.isfinite(m[rest]).all()


def test_reference_relight_and_conversions():
    """chroma · L with L the plain PTM value; the integer conversions of rti_convert.h."""
    rng = np.random.default_rng(9)
    m = np.concatenate([rng.normal(0, 50, (20, 6)), rng.uniform(0.2, 1.8, (20, 3))], -1).astype(np.float32)
    lu, lv = np.array([0.0, 0.3, 0.8]), np.array([0.0, -0.45, 0.75])
    out = relight_lrgb_ref(m, lu, lv)
    assert out.shape == (3, 20, 3)
    a = m[:, :6].astype(np.float64)
    for e in range(3):
        L = a @ np.array([lu[e] ** 2, lv[e] ** 2, lu[e] * lv[e], lu[e], lv[e], 1.0])
        assert np.abs(luminance_ref(a, lu[e], lv[e]) - L).max() <= 1e-12 * np.abs(a).max()
        assert np.array_equal(out[e], m[:, 6:].astype(np.float64) * luminance_ref(a, lu[e], lv[e])[:, None])
    assert np.array_equal(out[0], m[:, 6:].astype(np.float64) * a[:, 5:6])  # (0, 0): the constant term alone
    x = np.array([0.0, -0.9, 0.9, 254.99, 255.0, 300.7, -3.2, 2147483647.5, 2147483648.0, -2147483649.0, NAN, INF, -INF])
    assert np.array_equal(to_int32(x), [0, 0, 0, 254, 255, 300, -3, 2147483647] + [-2 ** 31] * 5)
    assert np.array_equal(to_uint8(x), [0, 0, 0, 254, 255, 255, 0, 255, 0, 0, 0, 0, 0])
