"""rti_relight_hsh_specular / rti_relight_hsh8_specular without a GPU: the symbols, constants and signatures are there,
every argument check answers before any HIP call (the device pointers below are never dereferenced; luv is a real host
array, the entry reads it) with a message that names the function, the Python layer refuses what it documents, and the
NumPy reference alone keeps the near-integer set of every GPU case under the cap the GPU tests assert."""
import ctypes

import numpy as np
import pytest

import rti
from hsh_specular_ref import DIRS, KS, NEAR_INTEGER_CAP, PARAMS, SIZES, excluded, reference
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


def fp32_call(coef=P_, basis=H16, layout=0, C=3, stride=0, P=64, normals=P_, nl=0, kd=0.4, ks=150.0, exp=75, luv=LUV,
              E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_hsh_specular(coef, basis, layout, C, stride, P, normals, nl, kd, ks, exp, luv, E, out,
                                               odt, None)


def bytes_call(coef8=P_, basis=H16, P=64, qparams=P_, normals=P_, nl=0, kd=0.4, ks=150.0, exp=75, luv=LUV, E=1, out=P_,
               odt=L.RTI_F32):
    return rti.load().rti_relight_hsh8_specular(coef8, basis, P, qparams, normals, nl, kd, ks, exp, luv, E, out, odt,
                                                None)


FRAME_BAD = {
    "null normals": dict(normals=None), "null luv": dict(luv=None), "null out": dict(out=None), "P = 0": dict(P=0),
    "P < 0": dict(P=-4), "E = 0": dict(E=0), "E < 0": dict(E=-1), "E = 17": dict(E=MAXE + 1),
    "normal layout": dict(nl=2), "normal layout < 0": dict(nl=-1), "nan kd": dict(kd=np.nan), "inf kd": dict(kd=np.inf),
    "nan ks": dict(ks=np.nan), "-inf ks": dict(ks=-np.inf), "exp = 0": dict(exp=0), "exp < 0": dict(exp=-3),
    "exp = 256": dict(exp=256),
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
def test_relight_hsh_specular_bad_arguments(case):
    answers(fp32_call, FP32_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_relight_hsh_specular")


@pytest.mark.parametrize("case", sorted(BYTES_BAD))
def test_relight_hsh8_specular_bad_arguments(case):
    answers(bytes_call, BYTES_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_relight_hsh8_specular")


@pytest.mark.parametrize("case", sorted(UNSUPPORTED))
def test_specular_unsupported(case):
    answers(fp32_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_relight_hsh_specular")
    answers(bytes_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_relight_hsh8_specular")


def test_a_single_map_ignores_its_channel_stride():
    """C = 1 never uses the stride (as rti_hsh_normals): a value below dense passes that check and the call goes on to
    the next one it fails."""
    assert fp32_call(C=1, stride=5, exp=0) == L.RTI_ERR_BAD_ARG
    assert b"spec_exp" in rti.load().rti_last_error()


def test_symbols_constants_and_exports():
    lib = rti.load()
    for name in ("rti_relight_hsh_specular", "rti_relight_hsh8_specular"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["rti_relight_hsh_specular"][1]) == 16
    assert len(L.SIGNATURES["rti_relight_hsh8_specular"][1]) == 14
    assert L.RTI_SPECULAR_MAX_DIRS == MAXE
    assert lib.rti_version() == 100
    for name in ("relight_hsh_specular", "relight_hsh8_specular", "relight_hsh_specular_into",
                 "relight_hsh8_specular_into"):
        assert callable(getattr(rti, name)) and callable(getattr(rti.api, name)) and name in rti.__all__, name
    from rti import ops  # noqa: F401  registers torch.ops.rti.*
    import torch

    assert callable(torch.ops.rti.relight_hsh_specular) and callable(torch.ops.rti.relight_hsh8_specular)


def test_python_layer_refusals():
    import torch

    c3, c1 = torch.zeros((3, 4, 5, 16)), torch.zeros((4, 5, 16))
    n = torch.zeros((4, 5, 3))
    q = rti.QuantisedHSH(torch.zeros((4, 5, 3, 16), dtype=torch.uint8), torch.ones(32), "hsh16")
    many = np.zeros(MAXE + 1)
    # more than 16 directions: refused, not looped over (before anything touches a device)
    with pytest.raises(ValueError, match="16 directions"):
        rti.relight_hsh_specular(c3, n, many, many)
    with pytest.raises(ValueError, match="16 directions"):
        rti.relight_hsh8_specular(q, n, many, many)
    with pytest.raises(ValueError, match="same number"):
        rti.relight_hsh_specular(c3, n, [0.1, 0.2], [0.1])
    # PTM maps have entries of their own
    for call in (lambda: rti.relight_hsh_specular(torch.zeros((3, 4, 5, 6)), n, 0.1, 0.2, "ptm"),
                 lambda: rti.relight_hsh_specular_into(c3, n, 0.1, 0.2, n, basis="ptm"),
                 lambda: rti.relight_hsh8_specular_into(q.coef, q.qparams, n, 0.1, 0.2, n, basis=L.RTI_BASIS_PTM6)):
        with pytest.raises(NotImplementedError, match="relight_rgb_enhanced"):
            call()
    # no CPU path
    for call in (lambda: rti.relight_hsh_specular(c3, n, 0.1, 0.2), lambda: rti.relight_hsh_specular(c1, n, 0.1, 0.2),
                 lambda: rti.relight_hsh8_specular(q, n, 0.1, 0.2),
                 lambda: rti.relight_hsh_specular_into(c3, n, 0.1, 0.2, torch.zeros((1, 20, 3))),
                 lambda: rti.relight_hsh8_specular_into(q.coef, q.qparams, n, 0.1, 0.2, torch.zeros((1, 20, 3)))):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="QuantisedHSH"):
        rti.relight_hsh8_specular(c3, n, 0.1, 0.2)
    with pytest.raises(ValueError, match="layout"):
        rti.relight_hsh_specular(c3, n, 0.1, 0.2, layout="rows")
    with pytest.raises(ValueError, match="layout"):
        rti.relight_hsh8_specular(q, n, 0.1, 0.2, normal_layout="rows")


# ---- the reference alone -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["fp32", "grey", "bytes"])
@pytest.mark.parametrize("k", KS)
def test_reference_keeps_the_near_integer_set_under_the_cap(k, source):
    """What the GPU tests leave out of their integer comparisons, per size, parameter tuple and direction."""
    worst = (-1.0, ())
    for P in SIZES:
        for params in PARAMS:
            ref = reference(P, k, source, params)
            assert ref.shape == (len(DIRS), P, 1 if source == "grey" else 3)
            for e in range(len(DIRS)):
                share = excluded(ref[e])[1]
                worst = max(worst, (share, (P, params, DIRS[e])))
                assert share <= NEAR_INTEGER_CAP, (P, params, DIRS[e], share)
    print(f"k={k} {source}: worst near-integer share {worst[0]:.4f} at {worst[1]}")


def test_reference_semantics():
    """The planted pixels do what the header says: a flat normal at the pole renders kd·V + ks exactly, a NaN normal
    gives NaN whatever ks is, and kd = 1, ks = 0 is the relit value."""
    from hsh_specular_ref import maps, normals, specular_ref
    from relight_ref import relight_ref

    P, k = 257, 9
    c, n = maps(P, k, "fp32"), normals(P)
    V = np.stack([relight_ref(c[ch], [0.0], [0.0], "hsh9")[0] for ch in range(3)], -1).astype(np.float64)
    r = specular_ref(c, n, [0.0], [0.0], k, 0.4, 150.0, 75)[0]
    assert np.array_equal(r[3], 0.4 * V[3] + 150.0) and np.array_equal(r[131], 0.4 * V[131] + 150.0)
    assert np.isnan(r[7]).all() and np.isnan(r[104]).all() and np.isnan(r).any(1).sum() == len(range(7, P, 97))
    plain = specular_ref(c, n, [0.0], [0.0], k, 1.0, 0.0, 1)[0]
    ok = ~np.isnan(n).any(1)
    assert np.array_equal(plain[ok], V[ok])
    assert np.isnan(specular_ref(c, n, [0.3], [-0.45], k, 1.0, 0.0, 1)[0][7]).all()
