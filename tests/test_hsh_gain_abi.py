"""rti_relight_hsh_gain / rti_relight_hsh8_gain without a GPU: the symbols and signatures are there, every argument
check answers before any HIP call (the device pointers below are never dereferenced; luv is a real host array, the
entry reads it) with a message that names the function, the Python layer refuses what it documents, and the NumPy
reference alone holds the identities of the header and keeps the near-integer set of every GPU case under the cap the
GPU tests assert."""
import ctypes

import numpy as np
import pytest

import rti
from hsh_gain_ref import (DIRS, GAINS, KS, NEAR_INTEGER_CAP, RIM, SIZES, anchor_ref, excluded, gain_ref, maps, normals,
                          reference)
from rti import _lib as L

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
ODD = ctypes.c_void_p(4098)  # 2 bytes off a dword
H16, H9 = L.RTI_BASIS_HSH16, L.RTI_BASIS_HSH9
MAXE = 16


def luv_of(values):
    a = np.ascontiguousarray(values, np.float64)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a  # the array is kept alive by the caller


LUV, _LUV_KEEP = luv_of([[0.3, -0.45]] * MAXE + [[0.0, 0.0]])  # one spare: E = 17 must be refused before it is read
BAD_LUV = {name: luv_of([[0.1, 0.2], pair]) for name, pair in
           {"nan lu": [np.nan, 0.0], "inf lv": [0.0, np.inf], "-inf lu": [-np.inf, 0.0]}.items()}


def fp32_call(coef=P_, basis=H16, layout=0, C=3, stride=0, P=64, normals=P_, nl=0, gain=2.5, luv=LUV, E=1, out=P_,
              odt=L.RTI_F32):
    return rti.load().rti_relight_hsh_gain(coef, basis, layout, C, stride, P, normals, nl, gain, luv, E, out, odt, None)


def bytes_call(coef8=P_, basis=H16, P=64, qparams=P_, normals=P_, nl=0, gain=2.5, luv=LUV, E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_hsh8_gain(coef8, basis, P, qparams, normals, nl, gain, luv, E, out, odt, None)


FRAME_BAD = {
    "null normals": dict(normals=None), "null luv": dict(luv=None), "null out": dict(out=None), "P = 0": dict(P=0),
    "P < 0": dict(P=-4), "E = 0": dict(E=0), "E < 0": dict(E=-1), "E = 17": dict(E=MAXE + 1),
    "normal layout": dict(nl=2), "normal layout < 0": dict(nl=-1), "nan gain": dict(gain=np.nan),
    "inf gain": dict(gain=np.inf), "-inf gain": dict(gain=-np.inf),
}
FRAME_BAD.update({f"luv: {name}": dict(luv=ptr, E=2) for name, (ptr, _) in BAD_LUV.items()})
FP32_BAD = dict(FRAME_BAD, **{
    "null coef": dict(coef=None), "C = 0": dict(C=0), "C = 2": dict(C=2), "C = 4": dict(C=4), "C < 0": dict(C=-1),
    "coef layout": dict(layout=2), "coef layout < 0": dict(layout=-1),
    "stride below dense, hsh16": dict(stride=64 * 16 - 1), "stride below dense, hsh9": dict(basis=H9, stride=64 * 9 - 1),
    "stride below dense, planar": dict(layout=1, stride=100), "stride < 0": dict(stride=-1),
})
BYTES_BAD = dict(FRAME_BAD, **{"null coef8": dict(coef8=None), "null qparams": dict(qparams=None),
                               "qparams off a dword": dict(qparams=ODD)})
UNSUPPORTED = {"ptm": dict(basis=L.RTI_BASIS_PTM6), "unknown basis": dict(basis=7), "basis < 0": dict(basis=-1),
               "f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "out dtype < 0": dict(odt=-1)}


def answers(call, cases, case, status, name):
    assert call(**cases[case]) == status, case
    msg = rti.load().rti_last_error()
    assert name in msg and len(msg) > len(name), msg


@pytest.mark.parametrize("case", sorted(FP32_BAD))
def test_relight_hsh_gain_bad_arguments(case):
    answers(fp32_call, FP32_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_relight_hsh_gain")


@pytest.mark.parametrize("case", sorted(BYTES_BAD))
def test_relight_hsh8_gain_bad_arguments(case):
    answers(bytes_call, BYTES_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_relight_hsh8_gain")


@pytest.mark.parametrize("case", sorted(UNSUPPORTED))
def test_gain_unsupported(case):
    answers(fp32_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_relight_hsh_gain")
    answers(bytes_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_relight_hsh8_gain")


def test_a_single_map_ignores_its_channel_stride():
    """C = 1 never uses the stride (as rti_relight_hsh_specular): a value below dense passes that check and the call
    goes on to the next one it fails."""
    assert fp32_call(C=1, stride=5, gain=np.nan) == L.RTI_ERR_BAD_ARG
    assert b"gain" in rti.load().rti_last_error()


def test_symbols_constants_and_exports():
    lib = rti.load()
    for name in ("rti_relight_hsh_gain", "rti_relight_hsh8_gain"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["rti_relight_hsh_gain"][1]) == 14
    assert len(L.SIGNATURES["rti_relight_hsh8_gain"][1]) == 12
    assert L.RTI_SPECULAR_MAX_DIRS == MAXE
    assert lib.rti_version() == 100
    for name in ("relight_hsh_gain", "relight_hsh8_gain", "relight_hsh_gain_into", "relight_hsh8_gain_into"):
        assert callable(getattr(rti, name)) and callable(getattr(rti.api, name)) and name in rti.__all__, name
    from rti import ops  # noqa: F401  registers torch.ops.rti.*
    import torch

    assert callable(torch.ops.rti.relight_hsh_gain) and callable(torch.ops.rti.relight_hsh8_gain)


def test_python_layer_refusals():
    import torch

    c3, c1 = torch.zeros((3, 4, 5, 16)), torch.zeros((4, 5, 16))
    n = torch.zeros((4, 5, 3))
    q = rti.QuantisedHSH(torch.zeros((4, 5, 3, 16), dtype=torch.uint8), torch.ones(32), "hsh16")
    many = np.zeros(MAXE + 1)
    # more than 16 directions: refused, not looped over (before anything touches a device)
    with pytest.raises(ValueError, match="16 directions"):
        rti.relight_hsh_gain(c3, n, many, many, gain=2.0)
    with pytest.raises(ValueError, match="16 directions"):
        rti.relight_hsh8_gain(q, n, many, many, gain=2.0)
    with pytest.raises(ValueError, match="same number"):
        rti.relight_hsh_gain(c3, n, [0.1, 0.2], [0.1])
    # PTM maps have entries of their own
    for call in (lambda: rti.relight_hsh_gain(torch.zeros((3, 4, 5, 6)), n, 0.1, 0.2, "ptm"),
                 lambda: rti.relight_hsh_gain_into(c3, n, 0.1, 0.2, n, basis="ptm"),
                 lambda: rti.relight_hsh8_gain_into(q.coef, q.qparams, n, 0.1, 0.2, n, basis=L.RTI_BASIS_PTM6)):
        with pytest.raises(NotImplementedError, match="relight_rgb_enhanced"):
            call()
    # no CPU path
    for call in (lambda: rti.relight_hsh_gain(c3, n, 0.1, 0.2), lambda: rti.relight_hsh_gain(c1, n, 0.1, 0.2),
                 lambda: rti.relight_hsh8_gain(q, n, 0.1, 0.2),
                 lambda: rti.relight_hsh_gain_into(c3, n, 0.1, 0.2, torch.zeros((1, 20, 3))),
                 lambda: rti.relight_hsh8_gain_into(q.coef, q.qparams, n, 0.1, 0.2, torch.zeros((1, 20, 3)))):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="QuantisedHSH"):
        rti.relight_hsh8_gain(c3, n, 0.1, 0.2)
    with pytest.raises(ValueError, match="layout"):
        rti.relight_hsh_gain(c3, n, 0.1, 0.2, layout="rows")
    with pytest.raises(ValueError, match="layout"):
        rti.relight_hsh8_gain(q, n, 0.1, 0.2, normal_layout="rows")


# ---- the reference alone -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["fp32", "grey", "bytes"])
@pytest.mark.parametrize("k", KS)
def test_reference_keeps_the_near_integer_set_under_the_cap(k, source):
    """What the GPU tests leave out of their integer comparisons, per size, gain and direction."""
    worst = (-1.0, ())
    for P in SIZES:
        for gain in GAINS:
            ref = reference(P, k, source, gain)
            assert ref.shape == (len(DIRS), P, 1 if source == "grey" else 3)
            for e in range(len(DIRS)):
                share = excluded(ref[e])[1]
                worst = max(worst, (share, (P, gain, DIRS[e])))
                assert share <= NEAR_INTEGER_CAP, (P, gain, DIRS[e], share)
    print(f"k={k} {source}: worst near-integer share {worst[0]:.4f} at {worst[1]}")


@pytest.mark.parametrize("k", KS)
def test_reference_semantics(k):
    """The anchor is relight_ref at the pixel's own direction bit for bit, gain = 1 is relight_ref's values exactly,
    gain = 0 is the anchor at every direction, a light at a pixel's (n_x, n_y) gives the anchor there for every gain,
    and a NaN normal gives NaN."""
    from relight_ref import relight_ref

    P = 257
    c, n = maps(P, k, "fp32"), normals(P)
    assert all(np.array_equal(n[p], np.float32(v)) for p, v in RIM.items())
    A = anchor_ref(c, n, k)
    ok = ~np.isnan(n).any(1)
    pixels = [0, 3, 11, 12, 64, 131, 256]  # the pole (3, 131) and the two rim normals among them
    for p in pixels:
        for ch in range(3):
            at_normal = relight_ref(c[ch, p:p + 1], [float(n[p, 0])], [float(n[p, 1])], f"hsh{k}")[0, 0]
            assert at_normal.view(np.uint32) == A[ch, p].view(np.uint32), (p, ch)
    lu, lv = zip(*DIRS)
    V = np.stack([relight_ref(c[ch], lu, lv, f"hsh{k}") for ch in range(3)], -1).astype(np.float64)  # [E, P, C]
    plain = gain_ref(c, n, lu, lv, k, 1.0)
    assert np.array_equal(plain[:, ok], V[:, ok]) and np.isnan(plain[:, ~ok]).all() and (~ok).sum() == len(range(7, P, 97))
    zero = gain_ref(c, n, lu, lv, k, 0.0)
    want = np.broadcast_to(A.T.astype(np.float64)[None], zero.shape)
    assert np.allclose(zero[:, ok], want[:, ok], rtol=1e-15, atol=1e-12)
    for p in pixels:
        for gain in GAINS:
            r = gain_ref(c, n, [float(n[p, 0])], [float(n[p, 1])], k, gain)[0, p]
            assert np.array_equal(r, A[:, p].astype(np.float64)), (p, gain)


def test_the_ptm_identity():
    """For a PTM whose gradient vanishes at its peak (u0, v0), the six transformed coefficients of Malzbender et al.
    (normals_ref.diffuse_gain_coef) evaluate to L + (g − 1)·(L − L(u0, v0)): the form the HSH entries use names no
    curvature.  1000 random concave PTMs, g = 3.5, to 1e-9 relative."""
    from normals_ref import diffuse_gain_coef, peak_ref, peaked_coef, ptm_value

    g = 3.5
    a, _, _, _ = peaked_coef(np.random.default_rng(77), 1000, 0.0, 0.9)
    k = peak_ref(a)
    assert k["has_max"].all()
    b = diffuse_gain_coef(a, g)
    peak = ptm_value(a, k["u0"], k["v0"])
    worst = 0.0
    for lu, lv in DIRS + [(-0.6, 0.2), (0.05, 0.9)]:
        L0 = ptm_value(a, lu, lv)
        paper = ptm_value(b, lu, lv)
        ours = L0 + (g - 1.0) * (L0 - peak)
        worst = max(worst, float((np.abs(paper - ours) / np.maximum(np.abs(paper), 1.0)).max()))
    print(f"worst relative difference {worst:.3g}")
    assert worst <= 1e-9
