""".ptm files as 9 bytes per pixel on the host: read_ptm(path, quantised=True) returns the file's own bytes and header
values, write_ptm of that object reproduces the file byte for byte (the fp32 round trip is not guaranteed to), and
the default read is unchanged and equals dequantise_lrgb of the quantised one.  No GPU."""
import numpy as np
import pytest
import torch

import rti
from lrgb_ref import mixed_lrgb
from rti.io import _ptm_quantise, _ptm_tokens

SHAPES = [(24, 20), (5, 7), (1, 1)]


def lrgb_file(tmp_path, H, W):
    m = mixed_lrgb(H * W, 40 + H).reshape(H, W, 9)
    return m, rti.write_ptm(str(tmp_path / f"m{H}x{W}.ptm"), m)


@pytest.mark.parametrize("H,W", SHAPES)
def test_quantised_read_returns_the_files_bytes_and_header(tmp_path, H, W):
    m, path = lrgb_file(tmp_path, H, W)
    fmt, q = rti.read_ptm(path, quantised=True)
    assert fmt == "lrgb" and isinstance(q, rti.QuantisedLRGB)
    assert q.shape == (H, W) and q.device.type == "cpu"
    assert q.coef.dtype == torch.uint8 and q.coef.shape == (H, W, 6) and q.rgb.shape == (H, W, 3)
    assert q.qparams.dtype == torch.float64 and q.qparams.shape == (13,)
    buf = open(path, "rb").read()
    toks, end = _ptm_tokens(buf, 16)
    assert np.array_equal(q.scale, [float(t) for t in toks[4:10]])
    assert np.array_equal(q.bias, [int(t) for t in toks[10:16]]) and q.s == 1.0
    payload = np.frombuffer(buf, np.uint8, offset=end + 1)
    n = H * W
    assert payload.size == 9 * n
    # the file stores rows bottom first; the object holds them top first
    assert np.array_equal(q.coef.numpy()[::-1].ravel(), payload[:6 * n])
    assert np.array_equal(q.rgb.numpy()[::-1].ravel(), payload[6 * n:])
    # and they are the host quantiser's bytes of the map that was written
    m64 = m.astype(np.float64)
    fin = m64[..., 6:][np.isfinite(m64[..., 6:])]
    s = float(fin.max()) if fin.size and fin.max() > 0 else 1.0
    raw, scale, bias = _ptm_quantise(m64[..., :6] * s)
    assert np.array_equal(q.coef.numpy(), raw) and np.array_equal(q.bias, bias)
    assert np.array_equal(q.scale, [float("%.9g" % x) for x in scale])


@pytest.mark.parametrize("H,W", SHAPES)
def test_quantised_round_trip_is_lossless(tmp_path, H, W):
    _, path = lrgb_file(tmp_path, H, W)
    q = rti.read_ptm(path, quantised=True)[1]
    path2 = rti.write_ptm(str(tmp_path / "again.ptm"), q)
    assert open(path2, "rb").read() == open(path, "rb").read()
    q2 = rti.read_ptm(path2, quantised=True)[1]
    assert torch.equal(q2.coef, q.coef) and torch.equal(q2.rgb, q.rgb) and torch.equal(q2.qparams, q.qparams)
    assert q.with_file_scales().qparams.equal(q.qparams)  # a loaded map already has the file's scales


@pytest.mark.parametrize("H,W", SHAPES)
def test_default_read_is_unchanged_and_is_the_dequantised_map(tmp_path, H, W):
    _, path = lrgb_file(tmp_path, H, W)
    fmt, maps = rti.read_ptm(path)
    assert fmt == "lrgb" and isinstance(maps, np.ndarray) and maps.dtype == np.float32 and maps.shape == (H, W, 9)
    fmt2, maps2 = rti.read_ptm(path, quantised=False)
    assert fmt2 == "lrgb" and np.array_equal(maps.view(np.int32), maps2.view(np.int32))
    d = rti.dequantise_lrgb(rti.read_ptm(path, quantised=True)[1])
    assert d.dtype == torch.float32 and d.shape == (H, W, 9) and d.device.type == "cpu"
    assert np.array_equal(d.numpy().view(np.int32), maps.view(np.int32))


def test_rgb_files_and_bad_objects_are_refused(tmp_path):
    rng = np.random.default_rng(3)
    path = rti.write_ptm(str(tmp_path / "rgb.ptm"), rng.normal(0, 40, (3, 4, 5, 6)), format="rgb")
    assert rti.read_ptm(path)[0] == "rgb"
    with pytest.raises(NotImplementedError, match="RGB"):
        rti.read_ptm(path, quantised=True)
    _, lpath = lrgb_file(tmp_path, 5, 7)
    q = rti.read_ptm(lpath, quantised=True)[1]
    with pytest.raises(ValueError, match="format"):
        rti.write_ptm(str(tmp_path / "x.ptm"), q, format="rgb")
    flat = rti.QuantisedLRGB(q.coef.reshape(35, 6), q.rgb.reshape(35, 3), q.qparams)
    with pytest.raises(ValueError, match="rows"):
        rti.write_ptm(str(tmp_path / "x.ptm"), flat)
