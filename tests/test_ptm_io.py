""".ptm files (rti/io.py: write_ptm / read_ptm, the layout restated in DESIGN.md §4.7) without a GPU: two 2 x 2 files
compared byte for byte with files spelled out here (the header, the bottom-first rows and the block order), round
trips within the quantisation step, constant planes, a NaN pixel, a header with W and H on one line, and the
formats that are not built."""
import numpy as np
import pytest

import rti
from rti.io import read_ptm, write_ptm

SCALE = np.array([1.0, 0.5, 2.0, 0.25, 1.0, 4.0])
BIAS = np.array([0, 10, 100, 128, 200, 255])
# raw coefficient bytes [row][col][j], row 0 the TOP row; every coefficient has a 0 and a 255 somewhere
RAW = np.array([[[0, 255, 7, 0, 255, 30], [255, 0, 255, 64, 0, 255]],
                [[1, 2, 0, 255, 100, 0], [128, 200, 33, 5, 254, 77]]], np.uint8)
RGB = np.array([[[255, 0, 51], [153, 153, 153]],
                [[0, 255, 0], [51, 102, 204]]], np.uint8)
HEADER_TAIL = b"2\n2\n1 0.5 2 0.25 1 4\n0 10 100 128 200 255\n"


def coefficients(raw):
    return (raw.astype(np.float64) - BIAS) * SCALE


def test_lrgb_file_byte_for_byte(tmp_path):
    maps = np.concatenate([coefficients(RAW), RGB / 255.0], -1).astype(np.float32)
    path = write_ptm(str(tmp_path / "a.ptm"), maps)
    want = (b"PTM_1.2\nPTM_FORMAT_LRGB\n" + HEADER_TAIL
            # coefficients, bottom row first: (row 1, col 0), (row 1, col 1), (row 0, col 0), (row 0, col 1)
            + bytes([1, 2, 0, 255, 100, 0, 128, 200, 33, 5, 254, 77, 0, 255, 7, 0, 255, 30, 255, 0, 255, 64, 0, 255])
            # then R G B per pixel in the same order
            + bytes([0, 255, 0, 51, 102, 204, 255, 0, 51, 153, 153, 153]))
    assert open(path, "rb").read() == want
    fmt, back = read_ptm(path)
    assert fmt == "lrgb" and back.dtype == np.float32 and back.shape == (2, 2, 9)
    assert np.array_equal(back, maps)


def test_rgb_file_byte_for_byte(tmp_path):
    raw = np.stack([RAW, RAW[::-1], RAW[:, ::-1]])  # R, G, B: three different blocks
    maps = coefficients(raw).astype(np.float32)
    assert maps.shape == (3, 2, 2, 6)
    path = write_ptm(str(tmp_path / "b.ptm"), maps, format="rgb")
    r = [1, 2, 0, 255, 100, 0, 128, 200, 33, 5, 254, 77, 0, 255, 7, 0, 255, 30, 255, 0, 255, 64, 0, 255]
    g = [0, 255, 7, 0, 255, 30, 255, 0, 255, 64, 0, 255, 1, 2, 0, 255, 100, 0, 128, 200, 33, 5, 254, 77]
    b = [128, 200, 33, 5, 254, 77, 1, 2, 0, 255, 100, 0, 255, 0, 255, 64, 0, 255, 0, 255, 7, 0, 255, 30]
    want = b"PTM_1.2\nPTM_FORMAT_RGB\n" + HEADER_TAIL + bytes(r) + bytes(g) + bytes(b)
    assert open(path, "rb").read() == want
    fmt, back = read_ptm(path)
    assert fmt == "rgb" and back.dtype == np.float32 and back.shape == (3, 2, 2, 6)
    assert np.array_equal(back, maps)


def header_of(path):
    """(tokens of the first six lines, the payload) of a file write_ptm wrote."""
    lines = open(path, "rb").read().split(b"\n", 6)
    return lines[:6], lines[6]


def random_lrgb(rng, H, W):
    return np.concatenate([rng.normal(0.0, 50.0, (H, W, 6)), rng.uniform(0.2, 1.8, (H, W, 3))], -1).astype(np.float32)


def test_lrgb_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    m = random_lrgb(rng, 5, 7)
    path = write_ptm(str(tmp_path / "c.ptm"), m)
    head, payload = header_of(path)
    assert head[:4] == [b"PTM_1.2", b"PTM_FORMAT_LRGB", b"7", b"5"] and len(payload) == 5 * 7 * 9
    scale = np.array([float(t) for t in head[4].split()])
    fmt, back = read_ptm(path)
    assert fmt == "lrgb" and back.shape == (5, 7, 9)
    s = float(m[..., 6:].max())
    m64, b64 = m.astype(np.float64), back.astype(np.float64)
    for j in range(6):
        err = np.abs(b64[..., j] - s * m64[..., j]).max()
        print(f"a{j}: scale {scale[j]:.4g}, error {err:.4g}")
        assert err <= scale[j]
    assert np.abs(b64[..., 6:] * s - m64[..., 6:]).max() <= s / 510 + 1e-6
    # the product chroma · L survives: the constant term, i.e. the image lit from (0, 0).  With back_a5 = s·a5 + e1,
    # |e1| <= scale, and back_c = c/s + e2, |e2| <= 1/510 + 1e-6: the product is off by c/s·e1 + (s·a5 + e1)·e2
    img, img_back = m64[..., 6:] * m64[..., 5:6], b64[..., 6:] * b64[..., 5:6]
    bound = 1.8 / s * scale[5] + (s * np.abs(m64[..., 5]).max() + scale[5]) * (1 / 510 + 1e-6)
    assert np.abs(img_back - img).max() <= bound
    # a tensor is taken as an array is
    import torch

    path2 = write_ptm(str(tmp_path / "c2.ptm"), torch.as_tensor(m))
    assert open(path2, "rb").read() == open(path, "rb").read()


def test_rgb_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    m = rng.normal(0.0, 50.0, (3, 5, 7, 6)).astype(np.float32)
    path = write_ptm(str(tmp_path / "d.ptm"), m, "rgb")
    head, payload = header_of(path)
    assert head[:4] == [b"PTM_1.2", b"PTM_FORMAT_RGB", b"7", b"5"] and len(payload) == 3 * 5 * 7 * 6
    scale = np.array([float(t) for t in head[4].split()])
    fmt, back = read_ptm(path)
    assert fmt == "rgb" and back.shape == (3, 5, 7, 6)
    for j in range(6):
        lo, hi = float(m[..., j].min()), float(m[..., j].max())
        assert abs(scale[j] - (hi - lo) / 255) <= 1e-8 * scale[j]  # one scale per coefficient over all three channels
        assert np.abs(back[..., j].astype(np.float64) - m[..., j]).max() <= scale[j]


def test_constant_planes(tmp_path):
    """hi = lo: scale 1, bias = clip(rint(−v), 0, 255), raw = clip(rint(v + bias), 0, 255).  The bias is a byte, so a
    constant above 255 or below −255 saturates, and a fraction rounds to an integer (error <= the scale of 1)."""
    v = np.array([3.0, -7.0, 0.0, 0.3, 300.0, -300.0])
    m = np.concatenate([np.tile(v, (2, 3, 1)), np.ones((2, 3, 3))], -1)
    path = write_ptm(str(tmp_path / "e.ptm"), m)
    head, payload = header_of(path)
    assert head[4] == b"1 1 1 1 1 1" and head[5] == b"0 7 0 0 0 255"
    assert payload == bytes([3, 0, 0, 0, 255, 0]) * 6 + bytes([255]) * 18
    fmt, back = read_ptm(path)
    assert np.array_equal(back, np.tile(np.array([3, -7, 0, 0, 255, -255, 1, 1, 1], np.float32), (2, 3, 1)))
    # chroma without a positive finite value: s = 1, black bytes
    m[..., 6:] = 0.0
    assert header_of(write_ptm(path, m))[1][-18:] == bytes(18)


def test_nan_pixel(tmp_path):
    """A NaN pixel (nine NaNs, as rti_lrgb_from_rgb writes it) takes no part in the scales, writes raw = bias and
    black colour bytes, and reads back as zero coefficients and zero chroma."""
    rng = np.random.default_rng(3)
    m = random_lrgb(rng, 5, 7)
    m[2, 4] = np.nan
    ref = m.copy()
    ref[2, 4] = 0.0  # the same map with a black pixel of zero coefficients there (0 lies inside every plane's range)
    assert (ref[..., :6].min((0, 1)) < 0).all() and (ref[..., :6].max((0, 1)) > 0).all()
    path = write_ptm(str(tmp_path / "f.ptm"), m)
    head, payload = header_of(path)
    head0, payload0 = header_of(write_ptm(str(tmp_path / "f0.ptm"), ref))
    bias = [int(t) for t in head[5].split()]
    assert head == head0  # the NaN took no part in any scale or bias
    row = 5 - 1 - 2  # bottom first
    at = (row * 7 + 4) * 6
    assert payload[at:at + 6] == bytes(bias)
    rgb_at = 5 * 7 * 6 + (row * 7 + 4) * 3
    assert payload[rgb_at:rgb_at + 3] == bytes(3)
    assert payload == payload0
    fmt, back = read_ptm(path)
    assert not back[2, 4].any() and np.isfinite(back).all()


def test_header_tokens_may_share_lines(tmp_path):
    rng = np.random.default_rng(5)
    m = random_lrgb(rng, 5, 7)
    path = write_ptm(str(tmp_path / "g.ptm"), m)
    head, payload = header_of(path)
    want = read_ptm(path)[1]
    variants = [
        b"PTM_1.2\nPTM_FORMAT_LRGB\n7 5\n" + head[4] + b"\n" + head[5] + b"\n",
        b"PTM_1.2 PTM_FORMAT_LRGB\t7  5 \n\n" + head[4].replace(b" ", b"\n") + b" \t" + head[5] + b"\n",
        b"PTM_1.2\r\nPTM_FORMAT_LRGB\r\n7\r\n5\r\n" + head[4] + b"\r\n" + head[5] + b" ",
    ]
    for i, h in enumerate(variants):
        p = str(tmp_path / f"g{i}.ptm")
        open(p, "wb").write(h + payload)
        fmt, got = read_ptm(p)
        assert fmt == "lrgb" and got.shape == (5, 7, 9) and np.array_equal(got, want), i


@pytest.mark.parametrize("tag", ["PTM_FORMAT_LUM", "PTM_FORMAT_JPEG_LRGB", "PTM_FORMAT_JPEG_RGB"])
def test_formats_not_built(tmp_path, tag):
    p = str(tmp_path / "h.ptm")
    open(p, "wb").write(b"PTM_1.2\n" + tag.encode() + b"\n2\n2\n1 1 1 1 1 1\n0 0 0 0 0 0\n" + bytes(64))
    with pytest.raises(NotImplementedError, match=tag):
        read_ptm(p)


def test_bad_files_and_arguments(tmp_path):
    p = str(tmp_path / "i.ptm")
    good = b"PTM_1.2\nPTM_FORMAT_LRGB\n2\n2\n1 1 1 1 1 1\n0 0 0 0 0 0\n"
    cases = {
        "magic": b"PTM_1.1\nPTM_FORMAT_LRGB\n2\n2\n1 1 1 1 1 1\n0 0 0 0 0 0\n" + bytes(36),
        "no magic": b"P6\n2 2\n255\n" + bytes(36),
        "empty": b"",
        "unknown format": b"PTM_1.2\nPTM_FORMAT_XYZ\n2\n2\n1 1 1 1 1 1\n0 0 0 0 0 0\n" + bytes(36),
        "short payload": good + bytes(35),
        "short rgb payload": good.replace(b"LRGB", b"RGB") + bytes(71),
        "header ends early": b"PTM_1.2\nPTM_FORMAT_LRGB\n2\n2\n1 1 1",
        "size": b"PTM_1.2\nPTM_FORMAT_LRGB\n0\n2\n1 1 1 1 1 1\n0 0 0 0 0 0\n" + bytes(36),
        "not a number": b"PTM_1.2\nPTM_FORMAT_LRGB\n2\n2\n1 1 x 1 1 1\n0 0 0 0 0 0\n" + bytes(36),
    }
    for name, data in cases.items():
        open(p, "wb").write(data)
        with pytest.raises(ValueError):
            read_ptm(p)
        assert name
    open(p, "wb").write(good + bytes(36))
    assert read_ptm(p)[1].shape == (2, 2, 9)
    with pytest.raises(ValueError):
        write_ptm(p, np.zeros((2, 2, 6)))
    with pytest.raises(ValueError):
        write_ptm(p, np.zeros((2, 2, 9)), format="rgb")
    with pytest.raises(ValueError):
        write_ptm(p, np.zeros((2, 2, 9)), format="lum")
    assert rti.write_ptm is write_ptm and rti.read_ptm is read_ptm
