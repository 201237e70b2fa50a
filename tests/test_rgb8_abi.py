"""rti_rgb8_qparams_workspace / rti_rgb8_qparams / rti_rgb8_quantise / rti_relight_rgb8 / rti_rgb8_normals without a
GPU: the symbols are bound, every argument check answers before any HIP call (the pointers below are never
dereferenced) with a message that names the function, the workspace query is monotone and capped; QuantisedRGB
checks its parts; PTM_FORMAT_RGB files are read into and written from the bytes on the host, identical to the fp32
route; tests/rgb8_ref.py agrees with rti.io's quantiser."""
import ctypes

import numpy as np
import pytest
import torch

import rti
from rgb8_ref import finite_rgb, host_dequantise, host_qparams, host_quantise, mixed_rgb
from rti import _lib as L
from rti.io import _ptm_quantise

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
ODD = ctypes.c_void_p(4098)  # 2 bytes off: neither 4- nor 8-byte aligned
W3 = (ctypes.c_float * 3)


def qparams_call(coef=P_, layout=0, stride=0, P=64, ws=P_, qparams=P_):
    return rti.load().rti_rgb8_qparams(coef, layout, stride, P, ws, qparams, None)


def quantise_call(coef=P_, layout=0, stride=0, P=64, qparams=P_, coef8=P_):
    return rti.load().rti_rgb8_quantise(coef, layout, stride, P, qparams, coef8, None)


def relight_call(coef8=P_, P=64, qparams=P_, luv=P_, E=1, out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_rgb8(coef8, P, qparams, luv, E, out, odt, None)


def normals_call(coef8=P_, P=64, qparams=P_, w=None, normals=P_, nl=0, kind=None, peak=None):
    return rti.load().rti_rgb8_normals(coef8, P, qparams, w, normals, nl, kind, peak, None)


MAPS_BAD = {"null coef": dict(coef=None), "null qparams": dict(qparams=None), "P = 0": dict(P=0), "P < 0": dict(P=-4),
            "layout": dict(layout=2), "layout < 0": dict(layout=-1), "stride below dense": dict(stride=6 * 64 - 1),
            "stride < 0": dict(stride=-8), "qparams off a double": dict(qparams=ODD)}
QPARAMS_BAD = dict(MAPS_BAD, **{"null workspace": dict(ws=None), "workspace off a dword": dict(ws=ODD)})
QUANTISE_BAD = dict(MAPS_BAD, **{"null coef8": dict(coef8=None)})
RELIGHT_BAD = {"null coef8": dict(coef8=None), "null qparams": dict(qparams=None), "null luv": dict(luv=None),
               "null out": dict(out=None), "P = 0": dict(P=0), "P < 0": dict(P=-1), "E = 0": dict(E=0),
               "E < 0": dict(E=-2), "qparams off a double": dict(qparams=ODD)}
RELIGHT_UNSUPPORTED = {"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "out dtype < 0": dict(odt=-1)}
NORMALS_BAD = {"null coef8": dict(coef8=None), "null qparams": dict(qparams=None), "null normals": dict(normals=None),
               "P = 0": dict(P=0), "P < 0": dict(P=-1), "normal layout": dict(nl=2), "normal layout < 0": dict(nl=-1),
               "NaN weight": dict(w=W3(0.3, float("nan"), 0.1)), "inf weight": dict(w=W3(float("inf"), 0.5, 0.1)),
               "qparams off a double": dict(qparams=ODD)}


@pytest.mark.parametrize("case", sorted(QPARAMS_BAD))
def test_rgb8_qparams_bad_arguments(case):
    assert qparams_call(**QPARAMS_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_rgb8_qparams" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(QUANTISE_BAD))
def test_rgb8_quantise_bad_arguments(case):
    assert quantise_call(**QUANTISE_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_rgb8_quantise" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(RELIGHT_BAD))
def test_relight_rgb8_bad_arguments(case):
    assert relight_call(**RELIGHT_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_relight_rgb8" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(RELIGHT_UNSUPPORTED))
def test_relight_rgb8_unsupported(case):
    assert relight_call(**RELIGHT_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_relight_rgb8" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(NORMALS_BAD))
def test_rgb8_normals_bad_arguments(case):
    assert normals_call(**NORMALS_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_rgb8_normals" in rti.load().rti_last_error()


def test_symbols_are_bound():
    lib = rti.load()
    for name in ("rti_rgb8_qparams_workspace", "rti_rgb8_qparams", "rti_rgb8_quantise", "rti_relight_rgb8",
                 "rti_rgb8_normals"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("QuantisedRGB", "quantise_rgb", "dequantise_rgb", "relight_rgb8", "rgb8_normals",
                 "rgb8_qparams_workspace", "rgb8_qparams_into", "rgb8_quantise_into", "relight_rgb8_into",
                 "rgb8_normals_into", "read_ptm8"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name
    assert lib.rti_version() == 100


def test_workspace_query_is_monotone_and_capped():
    ws = rti.load().rti_rgb8_qparams_workspace
    assert ws(0) == 0 and ws(-5) == 0
    sizes = [1, 2, 255, 256, 1023, 1024, 1025, 4096, 2 ** 20, 3840 * 2160, 2 ** 31 + 7, 2 ** 40]
    got = [ws(P) for P in sizes]
    assert all(g > 0 and g % 4 == 0 for g in got)
    assert got == sorted(got)
    assert got[0] == 12 * 4 and got[6] == 2 * 12 * 4  # one workgroup's partial: 12 floats per 1024 pixels
    assert got[-1] == got[-2] == 36864                # 768 workgroups
    assert rti.rgb8_qparams_workspace(1024) == got[5]
    with pytest.raises(ValueError):
        rti.rgb8_qparams_workspace(0)


def test_quantised_rgb_checks_its_parts():
    u8 = torch.uint8
    qp = torch.tensor([0.5] * 6 + [3.0] * 6, dtype=torch.float64)
    q = rti.QuantisedRGB(torch.zeros((3, 4, 5, 6), dtype=u8), qp)
    assert q.shape == (4, 5) and q.scale.shape == (6,) and q.bias.shape == (6,) and q.device.type == "cpu"
    assert np.array_equal(q.scale, [0.5] * 6) and np.array_equal(q.bias, [3.0] * 6)
    assert rti.QuantisedRGB(torch.zeros((3, 7, 6), dtype=u8), qp).shape == (7,)
    assert q.to("cpu").shape == (4, 5)
    for bad in (torch.zeros((3, 4, 5, 5), dtype=u8), torch.zeros((2, 4, 5, 6), dtype=u8), torch.zeros((3, 4, 5, 6)),
                torch.zeros((3, 6), dtype=u8), torch.zeros((3, 0, 6), dtype=u8),
                torch.zeros((3, 4, 5, 12), dtype=u8)[..., ::2]):
        with pytest.raises(ValueError, match="coef"):
            rti.QuantisedRGB(bad, qp)
    for bad in (torch.ones(13, dtype=torch.float64), torch.ones(12), torch.ones((2, 6), dtype=torch.float64)):
        with pytest.raises(ValueError, match="qparams"):
            rti.QuantisedRGB(q.coef, bad)
    with pytest.raises(ValueError, match="tensors"):
        rti.QuantisedRGB(np.zeros((3, 4, 6), np.uint8), qp)
    with pytest.raises(AttributeError):
        q.coef = q.coef
    with pytest.raises(AttributeError):
        q.extra = 1
    # dequantise_rgb is plain torch: it runs on the host with read_ptm's arithmetic
    q2 = rti.QuantisedRGB(torch.full((3, 2, 6), 7, dtype=u8), qp)
    d = rti.dequantise_rgb(q2)
    assert d.shape == (3, 2, 6) and d.dtype == torch.float32 and np.array_equal(d.numpy(), np.full((3, 2, 6), 2.0, np.float32))
    f = rti.QuantisedRGB(q2.coef, torch.tensor([1 / 3] * 6 + [3.0] * 6, dtype=torch.float64)).with_file_scales()
    assert f.coef is q2.coef and np.array_equal(f.scale, [0.333333333] * 6) and np.array_equal(f.bias, [3.0] * 6)


def test_python_layer_rejects_cpu_tensors_and_wrong_types():
    m = torch.zeros((3, 4, 4, 6))
    q = rti.QuantisedRGB(torch.zeros((3, 4, 4, 6), dtype=torch.uint8), torch.ones(12, dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        rti.quantise_rgb(m)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb8(q, 0.1, 0.2)
    with pytest.raises(ValueError, match="CUDA"):
        rti.rgb8_normals(q)
    with pytest.raises(ValueError, match="CUDA"):
        rti.rgb8_qparams_into(m, torch.zeros(64), q.qparams)
    with pytest.raises(ValueError, match="CUDA"):
        rti.rgb8_quantise_into(m, q.qparams, q.coef)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb8_into(q.coef, q.qparams, torch.zeros((1, 2), dtype=torch.float64), torch.zeros((1, 16, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.rgb8_normals_into(q.coef, q.qparams, torch.zeros((16, 3)))
    for fn in (lambda x: rti.relight_rgb8(x, 0.1, 0.2), rti.rgb8_normals, rti.dequantise_rgb):
        with pytest.raises(ValueError, match="QuantisedRGB"):
            fn(m)


# ---- files ---------------------------------------------------------------------------------------------------------

def test_read_ptm8_of_a_file_spelled_out(tmp_path):
    """A 2 x 2 PTM_FORMAT_RGB file byte by byte: the header, then block R, G, B, each bottom row first."""
    def px(c, y, x):  # the six bytes of channel c at row y (top first), column x
        return [100 * c + 10 * (2 * y + x) + j for j in range(6)]

    payload = bytes(b for c in range(3) for y in (1, 0) for x in (0, 1) for b in px(c, y, x))
    head = b"PTM_1.2\nPTM_FORMAT_RGB\n2\n2\n0.5 1 2 0.25 4 0.125\n0 1 2 3 4 255\n"
    path = tmp_path / "spelled.ptm"
    path.write_bytes(head + payload)
    fmt, q = rti.read_ptm8(str(path))
    assert fmt == "rgb" and isinstance(q, rti.QuantisedRGB) and q.shape == (2, 2) and q.device.type == "cpu"
    assert q.coef.shape == (3, 2, 2, 6) and q.coef.dtype == torch.uint8 and q.coef.is_contiguous()
    for c in range(3):
        for y in range(2):
            for x in range(2):
                assert q.coef[c, y, x].tolist() == px(c, y, x), (c, y, x)
    assert np.array_equal(q.scale, [0.5, 1, 2, 0.25, 4, 0.125]) and np.array_equal(q.bias, [0, 1, 2, 3, 4, 255])
    want = (np.array([px(0, 1, 0)], np.float64) - q.bias) * q.scale
    assert np.array_equal(rti.dequantise_rgb(q)[0, 1, 0].numpy(), want[0].astype(np.float32))
    assert np.array_equal(rti.dequantise_rgb(q).numpy(), rti.read_ptm(str(path))[1])
    back = rti.write_ptm(str(tmp_path / "back.ptm"), q)
    assert open(back, "rb").read() == head + payload


@pytest.mark.parametrize("H,W", [(24, 20), (5, 7)])
def test_host_objects_write_the_file_of_the_arrays(tmp_path, H, W):
    m = mixed_rgb(H * W, 300 + H).reshape(3, H, W, 6)
    qp = host_qparams(m)
    q = rti.QuantisedRGB(torch.from_numpy(host_quantise(m, qp)), torch.from_numpy(qp))
    a = rti.write_ptm(str(tmp_path / "arrays.ptm"), m, format="rgb")
    b = rti.write_ptm(str(tmp_path / "object.ptm"), q)
    c = rti.write_ptm(str(tmp_path / "object_rgb.ptm"), q, format="rgb")
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    with pytest.raises(ValueError, match="format"):
        rti.write_ptm(str(tmp_path / "x.ptm"), q, format="lrgb")
    with pytest.raises(ValueError, match="rows"):
        rti.write_ptm(str(tmp_path / "x.ptm"), rti.QuantisedRGB(q.coef.reshape(3, H * W, 6), q.qparams))
    # the round trip: a loaded object, and the in-memory one with the header's nine digits, are read_ptm's map
    fmt, maps = rti.read_ptm(a)
    fmt8, loaded = rti.read_ptm8(a)
    assert fmt == fmt8 == "rgb" and torch.equal(loaded.coef, q.coef)
    for obj in (loaded, q.with_file_scales()):
        d = rti.dequantise_rgb(obj).numpy()
        assert d.shape == maps.shape and np.array_equal(d.view(np.uint32), maps.view(np.uint32))
    assert np.array_equal(host_dequantise(loaded.coef.numpy(), loaded.qparams.numpy()).view(np.uint32),
                          maps.view(np.uint32))
    with pytest.raises(NotImplementedError, match="RGB"):
        rti.read_ptm(a, quantised=True)


def test_read_ptm8_of_an_lrgb_file_is_read_ptm_quantised(tmp_path):
    rng = np.random.default_rng(3)
    m = np.concatenate([rng.normal(0, 40, (9, 11, 6)), rng.uniform(0.2, 1.4, (9, 11, 3))], -1).astype(np.float32)
    path = rti.write_ptm(str(tmp_path / "lrgb.ptm"), m)  # format=None means "lrgb" for arrays
    assert open(path, "rb").read() == open(rti.write_ptm(str(tmp_path / "l2.ptm"), m, format="lrgb"), "rb").read()
    fmt, a = rti.read_ptm8(path)
    fmt2, b = rti.read_ptm(path, quantised=True)
    assert fmt == fmt2 == "lrgb" and isinstance(a, rti.QuantisedLRGB)
    assert torch.equal(a.coef, b.coef) and torch.equal(a.rgb, b.rgb) and torch.equal(a.qparams, b.qparams)
    assert open(rti.write_ptm(str(tmp_path / "l3.ptm"), a), "rb").read() == open(path, "rb").read()


@pytest.mark.parametrize("P", [7, 255, 1028, 3077])
def test_ref_agrees_with_the_hosts_quantiser(P):
    for m in (finite_rgb(P, 40 + P), mixed_rgb(P, 50 + P)):
        raw, scale, bias = _ptm_quantise(m.astype(np.float64))
        qp = host_qparams(m)
        assert np.array_equal(qp[:6], scale) and np.array_equal(qp[6:], bias.astype(np.float64))
        assert np.array_equal(host_quantise(m, qp), raw)
