"""rti_lrgb_qparams_workspace / rti_lrgb_qparams / rti_lrgb_quantise / rti_relight_lrgb8 without a GPU: the four
symbols are bound, every argument check answers before any HIP call (the pointers below are never dereferenced)
with a message that names the function, the workspace query is positive and monotone, and the Python layer
refuses CPU tensors and wrong shapes."""
import ctypes

import numpy as np
import pytest

import rti
from rti import _lib as L

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
ODD = ctypes.c_void_p(4098)  # 2 bytes off: neither 4- nor 8-byte aligned


def qparams_call(lrgb=P_, layout=0, P=64, ws=P_, qparams=P_):
    return rti.load().rti_lrgb_qparams(lrgb, layout, P, ws, qparams, None)


def quantise_call(lrgb=P_, layout=0, P=64, qparams=P_, coef8=P_, rgb8=P_):
    return rti.load().rti_lrgb_quantise(lrgb, layout, P, qparams, coef8, rgb8, None)


def relight_call(coef8=P_, rgb8=P_, P=64, qparams=P_, luv=P_, E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_lrgb8(coef8, rgb8, P, qparams, luv, E, out, odt, None)


QPARAMS_BAD = {
    "null lrgb": dict(lrgb=None), "null workspace": dict(ws=None), "null qparams": dict(qparams=None),
    "P = 0": dict(P=0), "P < 0": dict(P=-4), "layout": dict(layout=2), "layout < 0": dict(layout=-1),
    "workspace off a dword": dict(ws=ODD), "qparams off a double": dict(qparams=ODD),
}
QUANTISE_BAD = {
    "null lrgb": dict(lrgb=None), "null qparams": dict(qparams=None), "null coef8": dict(coef8=None),
    "null rgb8": dict(rgb8=None), "P = 0": dict(P=0), "P < 0": dict(P=-1), "layout": dict(layout=2),
    "layout < 0": dict(layout=-1), "qparams off a double": dict(qparams=ODD),
}
RELIGHT_BAD = {
    "null coef8": dict(coef8=None), "null rgb8": dict(rgb8=None), "null qparams": dict(qparams=None),
    "null luv": dict(luv=None), "null out": dict(out=None), "P = 0": dict(P=0), "P < 0": dict(P=-1),
    "E = 0": dict(E=0), "E < 0": dict(E=-2), "qparams off a double": dict(qparams=ODD),
}
RELIGHT_UNSUPPORTED = {"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "out dtype < 0": dict(odt=-1)}


@pytest.mark.parametrize("case", sorted(QPARAMS_BAD))
def test_lrgb_qparams_bad_arguments(case):
    assert qparams_call(**QPARAMS_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_lrgb_qparams" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(QUANTISE_BAD))
def test_lrgb_quantise_bad_arguments(case):
    assert quantise_call(**QUANTISE_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_lrgb_quantise" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(RELIGHT_BAD))
def test_relight_lrgb8_bad_arguments(case):
    assert relight_call(**RELIGHT_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_relight_lrgb8" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(RELIGHT_UNSUPPORTED))
def test_relight_lrgb8_unsupported(case):
    assert relight_call(**RELIGHT_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_relight_lrgb8" in rti.load().rti_last_error()


def test_symbols_are_bound():
    lib = rti.load()
    for name in ("rti_lrgb_qparams_workspace", "rti_lrgb_qparams", "rti_lrgb_quantise", "rti_relight_lrgb8"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("QuantisedLRGB", "quantise_lrgb", "dequantise_lrgb", "relight_lrgb8", "lrgb_qparams_into",
                 "lrgb_quantise_into", "relight_lrgb8_into", "lrgb_qparams_workspace"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name


def test_workspace_query_is_positive_and_monotone():
    ws = rti.load().rti_lrgb_qparams_workspace
    assert ws(0) <= 0 and ws(-5) <= 0
    sizes = [1, 2, 255, 256, 1023, 1024, 1025, 4096, 2 ** 20, 3840 * 2160, 2 ** 31 + 7, 2 ** 40]
    got = [ws(P) for P in sizes]
    assert all(g > 0 and g % 4 == 0 for g in got)
    assert got == sorted(got)
    assert got[0] == 13 * 4  # one workgroup's partial: 13 floats
    assert rti.lrgb_qparams_workspace(1024) == got[5]
    with pytest.raises(ValueError):
        rti.lrgb_qparams_workspace(0)


def test_python_layer_rejects_cpu_tensors_and_wrong_shapes():
    import torch

    m = torch.zeros((4, 4, 9))
    q = rti.QuantisedLRGB(torch.zeros((4, 4, 6), dtype=torch.uint8), torch.zeros((4, 4, 3), dtype=torch.uint8),
                          torch.ones(13, dtype=torch.float64))
    assert q.shape == (4, 4) and q.s == 1.0 and q.scale.shape == (6,) and q.bias.shape == (6,)
    with pytest.raises(ValueError, match="CUDA"):
        rti.quantise_lrgb(m)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_lrgb8(q, 0.1, 0.2)
    with pytest.raises(ValueError, match="CUDA"):
        rti.lrgb_qparams_into(m.reshape(16, 9), torch.zeros(64), torch.zeros(13, dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        rti.lrgb_quantise_into(m.reshape(16, 9), q.qparams, q.coef, q.rgb)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_lrgb8_into(q.coef, q.rgb, q.qparams, torch.zeros((1, 2), dtype=torch.float64),
                               torch.zeros((1, 16, 3)))
    with pytest.raises(ValueError, match="QuantisedLRGB"):
        rti.relight_lrgb8(m, 0.1, 0.2)
    with pytest.raises(ValueError, match="QuantisedLRGB"):
        rti.dequantise_lrgb(m)
    # the holder checks its parts and is immutable
    u8 = torch.uint8
    with pytest.raises(ValueError, match="coef"):
        rti.QuantisedLRGB(torch.zeros((4, 4, 5), dtype=u8), q.rgb, q.qparams)
    with pytest.raises(ValueError, match="coef"):
        rti.QuantisedLRGB(torch.zeros((4, 4, 6)), q.rgb, q.qparams)
    with pytest.raises(ValueError, match="rgb"):
        rti.QuantisedLRGB(q.coef, torch.zeros((4, 3, 3), dtype=u8), q.qparams)
    with pytest.raises(ValueError, match="qparams"):
        rti.QuantisedLRGB(q.coef, q.rgb, torch.ones(12, dtype=torch.float64))
    with pytest.raises(ValueError, match="qparams"):
        rti.QuantisedLRGB(q.coef, q.rgb, torch.ones(13))
    with pytest.raises(AttributeError):
        q.coef = q.coef
    with pytest.raises(AttributeError):
        q.extra = 1
    # dequantise_lrgb is plain torch: it runs on the host with read_ptm's arithmetic
    qp = torch.tensor([0.5] * 6 + [3.0] * 6 + [1.0], dtype=torch.float64)
    q2 = rti.QuantisedLRGB(torch.full((2, 6), 7, dtype=u8), torch.full((2, 3), 51, dtype=u8), qp)
    d = rti.dequantise_lrgb(q2)
    assert d.shape == (2, 9) and d.dtype == torch.float32
    assert np.array_equal(d[0].numpy(), np.float32([2.0] * 6 + [0.2] * 3))
    f = q2.with_file_scales()
    assert np.array_equal(f.scale, q2.scale) and f.s == 1.0 and f.coef is q2.coef
