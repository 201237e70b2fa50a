"""rti_hsh_qparams_workspace / rti_hsh_qparams / rti_hsh_quantise / rti_relight_hsh8 without a GPU: the four symbols
are bound, every argument check answers before any HIP call (the pointers below are never dereferenced) with a
message that names the function, the workspace query is zero for bad arguments, monotone and bounded, and the Python
layer refuses CPU tensors, wrong shapes and other bases."""
import ctypes

import numpy as np
import pytest

import rti
from rti import _lib as L

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
ODD = ctypes.c_void_p(4098)  # 2 bytes off a dword
H16, H9 = L.RTI_BASIS_HSH16, L.RTI_BASIS_HSH9


def qparams_call(coef=P_, basis=H16, layout=0, stride=0, P=64, ws=P_, qparams=P_):
    return rti.load().rti_hsh_qparams(coef, basis, layout, stride, P, ws, qparams, None)


def quantise_call(coef=P_, basis=H16, layout=0, stride=0, P=64, qparams=P_, coef8=P_):
    return rti.load().rti_hsh_quantise(coef, basis, layout, stride, P, qparams, coef8, None)


def relight_call(coef8=P_, basis=H16, P=64, qparams=P_, luv=P_, E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_hsh8(coef8, basis, P, qparams, luv, E, out, odt, None)


MAPS_BAD = {
    "null coef": dict(coef=None), "null qparams": dict(qparams=None), "P = 0": dict(P=0), "P < 0": dict(P=-4),
    "layout": dict(layout=2), "layout < 0": dict(layout=-1), "qparams off a dword": dict(qparams=ODD),
    "stride below dense, hsh16": dict(stride=64 * 16 - 1), "stride below dense, hsh9": dict(basis=H9, stride=64 * 9 - 1),
    "stride below dense, planar": dict(layout=1, stride=100), "stride < 0": dict(stride=-1),
}
QPARAMS_BAD = dict(MAPS_BAD, **{"null workspace": dict(ws=None), "workspace off a dword": dict(ws=ODD)})
QUANTISE_BAD = dict(MAPS_BAD, **{"null coef8": dict(coef8=None)})
MAPS_UNSUPPORTED = {"ptm": dict(basis=L.RTI_BASIS_PTM6), "unknown basis": dict(basis=7), "basis < 0": dict(basis=-1)}
RELIGHT_BAD = {
    "null coef8": dict(coef8=None), "null qparams": dict(qparams=None), "null luv": dict(luv=None),
    "null out": dict(out=None), "P = 0": dict(P=0), "P < 0": dict(P=-1), "E = 0": dict(E=0), "E < 0": dict(E=-2),
    "qparams off a dword": dict(qparams=ODD),
}
RELIGHT_UNSUPPORTED = dict(MAPS_UNSUPPORTED, **{"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9),
                                                "out dtype < 0": dict(odt=-1)})


def answers(call, cases, case, status, name):
    assert call(**cases[case]) == status, case
    msg = rti.load().rti_last_error()
    assert name in msg and len(msg) > len(name), msg


@pytest.mark.parametrize("case", sorted(QPARAMS_BAD))
def test_hsh_qparams_bad_arguments(case):
    answers(qparams_call, QPARAMS_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_hsh_qparams")


@pytest.mark.parametrize("case", sorted(QUANTISE_BAD))
def test_hsh_quantise_bad_arguments(case):
    answers(quantise_call, QUANTISE_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_hsh_quantise")


@pytest.mark.parametrize("case", sorted(RELIGHT_BAD))
def test_relight_hsh8_bad_arguments(case):
    answers(relight_call, RELIGHT_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_relight_hsh8")


@pytest.mark.parametrize("case", sorted(MAPS_UNSUPPORTED))
def test_hsh_quantiser_unsupported(case):
    answers(qparams_call, MAPS_UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_hsh_qparams")
    answers(quantise_call, MAPS_UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_hsh_quantise")


@pytest.mark.parametrize("case", sorted(RELIGHT_UNSUPPORTED))
def test_relight_hsh8_unsupported(case):
    answers(relight_call, RELIGHT_UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_relight_hsh8")


def test_symbols_are_bound():
    lib = rti.load()
    for name in ("rti_hsh_qparams_workspace", "rti_hsh_qparams", "rti_hsh_quantise", "rti_relight_hsh8"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("QuantisedHSH", "quantise_hsh", "dequantise_hsh", "relight_hsh8", "hsh_qparams_into",
                 "hsh_quantise_into", "relight_hsh8_into", "hsh_qparams_workspace", "read_rti", "write_rti"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name


@pytest.mark.parametrize("k", [9, 16])
def test_workspace_query_is_zero_monotone_and_bounded(k):
    ws = rti.load().rti_hsh_qparams_workspace
    assert ws(k, 0) == 0 and ws(k, -5) == 0
    for bad_k in (0, 6, 8, 10, 15, 17, -9):
        assert ws(bad_k, 4096) == 0, bad_k
    sizes = [1, 2, 63, 64, 255, 256, 257, 1024, 4096, 768 * 256, 768 * 256 + 1, 2 ** 20, 3840 * 2160, 2 ** 31 + 7,
             2 ** 40, 2 ** 62]
    got = [ws(k, P) for P in sizes]
    assert all(g > 0 and g % 4 == 0 for g in got)
    assert got == sorted(got)
    assert got[0] == 2 * k * 4  # one workgroup's partial: k minima and k maxima
    assert got[-1] == got[-2] == 768 * 2 * k * 4  # bounded: the grid cap (include/rti.h)
    assert rti.hsh_qparams_workspace(1024, f"hsh{k}") == got[7]
    with pytest.raises(ValueError):
        rti.hsh_qparams_workspace(0, f"hsh{k}")
    with pytest.raises(NotImplementedError):
        rti.hsh_qparams_workspace(64, "ptm")


def test_python_layer_rejects_cpu_tensors_wrong_shapes_and_other_bases():
    import torch

    u8 = torch.uint8
    m = torch.zeros((3, 4, 4, 16))
    q = rti.QuantisedHSH(torch.zeros((4, 4, 3, 16), dtype=u8), torch.ones(32), "hsh16")
    assert q.shape == (4, 4) and q.k == 16 and q.basis == "hsh16" and q.device.type == "cpu"
    assert q.scale.shape == (16,) and q.bias.shape == (16,) and q.scale.dtype == np.float32
    assert "hsh16" in repr(q) and "(4, 4)" in repr(q)
    q9 = rti.QuantisedHSH(torch.zeros((5, 3, 9), dtype=u8), torch.ones(18), L.RTI_BASIS_HSH9)
    assert q9.shape == (5,) and q9.k == 9 and q9.basis == "hsh9" and q9.to("cpu").basis == "hsh9"
    with pytest.raises(ValueError, match="CUDA"):
        rti.quantise_hsh(m)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_hsh8(q, 0.1, 0.2)
    with pytest.raises(ValueError, match="CUDA"):
        rti.hsh_qparams_into(m, torch.zeros(64), torch.zeros(32))
    with pytest.raises(ValueError, match="CUDA"):
        rti.hsh_quantise_into(m, q.qparams, q.coef)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_hsh8_into(q.coef, q.qparams, torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 16, 3)))
    with pytest.raises(ValueError, match="QuantisedHSH"):
        rti.relight_hsh8(m, 0.1, 0.2)
    with pytest.raises(ValueError, match="QuantisedHSH"):
        rti.dequantise_hsh(m)
    for call in (lambda: rti.quantise_hsh(m, "ptm"), lambda: rti.QuantisedHSH(q.coef, q.qparams, "ptm"),
                 lambda: rti.write_rti("unused.rti", m.numpy(), "ptm")):
        with pytest.raises(NotImplementedError):
            call()
    # the holder checks its parts and is immutable
    with pytest.raises(ValueError, match="coef"):
        rti.QuantisedHSH(torch.zeros((4, 4, 3, 9), dtype=u8), q.qparams, "hsh16")
    with pytest.raises(ValueError, match="coef"):
        rti.QuantisedHSH(torch.zeros((4, 4, 3, 16)), q.qparams, "hsh16")
    with pytest.raises(ValueError, match="coef"):
        rti.QuantisedHSH(torch.zeros((4, 4, 2, 16), dtype=u8), q.qparams, "hsh16")
    with pytest.raises(ValueError, match="qparams"):
        rti.QuantisedHSH(q.coef, torch.ones(18), "hsh16")
    with pytest.raises(ValueError, match="qparams"):
        rti.QuantisedHSH(q.coef, torch.ones(32, dtype=torch.float64), "hsh16")
    with pytest.raises(AttributeError):
        q.coef = q.coef
    with pytest.raises(AttributeError):
        q.extra = 1
    # dequantise_hsh is plain torch: it runs on the host, a division, a multiply and an add in fp32
    qp = torch.tensor([510.0] * 9 + [3.0] * 9)
    d = rti.dequantise_hsh(rti.QuantisedHSH(torch.full((2, 3, 9), 7, dtype=u8), qp, "hsh9"))
    assert d.shape == (3, 2, 9) and d.dtype == torch.float32 and d.is_contiguous()
    assert np.array_equal(d.numpy(), np.full((3, 2, 9), 17.0, np.float32))
