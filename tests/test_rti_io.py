"""rti.write_rti / rti.read_rti on the host (rti/io.py; layout in DESIGN.md §4.9) against tests/hsh8_ref.py: a file
round trip of fp32 maps is the reference's dequantise(quantise(m)) bit for bit, a quantised read written again is
the same file, the header is what the layout says byte for byte, rows are stored top first, and every malformed or
unbuilt header raises the stated exception."""
import struct

import numpy as np
import pytest
import torch

import rti
from hsh8_ref import finite_hsh, host_dequantise, host_qparams, host_quantise, mixed_hsh


def maps_of(H, W, k, seed=0):
    """mixed_hsh as [3, H, W, k]."""
    return mixed_hsh(H * W, k, 100 * H + W + seed).reshape(3, H, W, k)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def reference_round_trip(m):
    """[3, H, W, k] -> (qparams, raw [H, W, 3, k], fp32 [3, H, W, k]) of the reference."""
    _, H, W, k = m.shape
    flat = m.reshape(3, H * W, k)
    qp = host_qparams(flat)
    raw = host_quantise(flat, qp)
    return qp, raw.reshape(H, W, 3, k), host_dequantise(raw, qp).reshape(3, H, W, k)


@pytest.mark.parametrize("k", [9, 16])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (16, 16)])
def test_round_trip_is_the_reference(tmp_path, H, W, k):
    m = maps_of(H, W, k)
    qp, raw, want = reference_round_trip(m)
    path = rti.write_rti(str(tmp_path / "a.rti"), m, f"hsh{k}")
    basis, back = rti.read_rti(path)
    assert basis == f"hsh{k}" and back.dtype == np.float32 and same_bits(back, want)
    assert np.isfinite(back).all()  # a NaN is stored as byte 0: it reads back as the term's bias
    # tensors go the same way as arrays
    assert rti.write_rti(str(tmp_path / "t.rti"), torch.as_tensor(m), f"hsh{k}") != path
    assert open(tmp_path / "t.rti", "rb").read() == open(path, "rb").read()
    # the quantised read keeps the bytes and the header's floats, and writes the same file again
    basis, q = rti.read_rti(path, quantised=True)
    assert basis == f"hsh{k}" and isinstance(q, rti.QuantisedHSH) and q.shape == (H, W) and q.basis == basis
    assert q.device.type == "cpu" and np.array_equal(q.coef.numpy(), raw)
    assert same_bits(q.qparams.numpy(), qp)
    assert same_bits(rti.dequantise_hsh(q).numpy(), want)
    again = rti.write_rti(str(tmp_path / "b.rti"), q)
    assert open(again, "rb").read() == open(path, "rb").read()


def test_header_bytes_are_literal(tmp_path):
    H, W, k = 3, 5, 9
    m = maps_of(H, W, k)
    qp, raw, _ = reference_round_trip(m)
    buf = open(rti.write_rti(str(tmp_path / "a.rti"), m, "hsh9"), "rb").read()
    head = b"#HSH1.2\n3\n5 3 3\n9 2 1\n"
    assert buf[:len(head)] == head
    floats = struct.unpack("<18f", buf[len(head):len(head) + 72])
    assert same_bits(np.float32(floats), qp)  # nine scales, then nine biases
    assert buf[len(head) + 72:] == raw.tobytes() and len(buf) == len(head) + 72 + H * W * 27
    # pixel (0, 0) comes first: R's nine terms, then G's, then B's
    assert buf[len(head) + 72:len(head) + 72 + 27] == raw[0, 0].tobytes()


def test_rows_are_stored_top_first(tmp_path):
    H, W, k = 4, 3, 9
    m = np.zeros((3, H, W, k), np.float32)
    m[...] = np.arange(H, dtype=np.float32)[None, :, None, None]  # row y holds y: bytes 0, 85, 170, 255
    path = rti.write_rti(str(tmp_path / "rows.rti"), m, "hsh9")
    buf = open(path, "rb").read()
    payload = np.frombuffer(buf[-H * W * 27:], np.uint8).reshape(H, W * 27)
    assert [set(r) for r in payload] == [{0}, {85}, {170}, {255}]
    back = rti.read_rti(path)[1]
    assert np.allclose(back, m, rtol=0, atol=1e-6)  # 85·fl(3/255) need not be 1 to the bit
    q = rti.read_rti(path, quantised=True)[1]
    assert [int(q.coef[y].unique()) for y in range(H)] == [0, 85, 170, 255]


@pytest.mark.parametrize("k", [9, 16])
def test_nan_constant_and_empty_terms_round_trip(tmp_path, k):
    H, W = 16, 16
    m = finite_hsh(H * W, k, 3).reshape(3, H, W, k).copy()
    m[..., 0] = np.nan               # no finite value: scale 1, bias 0, bytes 0
    m[..., 1] = -3.25                # constant: scale 1, bias -3.25, bytes 0
    m[1, 2, 3, 2] = np.nan           # a NaN in a live term: byte 0 = the term's minimum
    m[0, 4, 5, 3], m[2, 6, 7, 3] = np.inf, -np.inf  # saturate; the extremes skip them
    _, q = rti.read_rti(rti.write_rti(str(tmp_path / "a.rti"), m, f"hsh{k}"), quantised=True)
    assert q.scale[0] == 1.0 and q.bias[0] == 0.0 and not q.coef[..., 0].any()
    assert q.scale[1] == 1.0 and q.bias[1] == np.float32(-3.25) and not q.coef[..., 1].any()
    assert int(q.coef[2, 3, 1, 2]) == 0
    assert int(q.coef[4, 5, 0, 3]) == 255 and int(q.coef[6, 7, 2, 3]) == 0
    fin3 = m[..., 3][np.isfinite(m[..., 3])]
    assert q.bias[3] == fin3.min() and q.scale[3] == np.float32(fin3.max() - fin3.min())
    back = rti.read_rti(str(tmp_path / "a.rti"))[1]
    assert np.array_equal(back[..., 0], np.zeros((3, H, W), np.float32))
    assert np.array_equal(back[..., 1], np.full((3, H, W), -3.25, np.float32))
    assert back[1, 2, 3, 2] == q.bias[2]
    qp, _, want = reference_round_trip(m)
    assert same_bits(back, want) and same_bits(q.qparams.numpy(), qp)
    # finite terms come back within half a step (and fp32 rounding of the two operations)
    j = 4
    step = q.scale[j] / np.float32(255.0)
    slack = 4 * 2.0 ** -23 * np.abs(m[..., j]).max()
    assert np.abs(back[..., j].astype(np.float64) - m[..., j]).max() <= 0.5 * step + slack


def header(magic=b"#HSH1.2", ftype=b"3", size=b"2 2 3", terms=b"9 2 1", comment=None):
    lines = [magic] + ([comment] if comment else []) + [ftype, size, terms]
    return b"\n".join(lines) + b"\n"


def body(k=9, n=4):
    return np.ones(2 * k, "<f4").tobytes() + bytes(n * 3 * k)


BAD = {
    "bad magic": (header(magic=b"#HSH1.1"), ValueError),
    "ptm magic": (header(magic=b"PTM_1.2"), ValueError),
    "empty file": (b"", ValueError),
    "width 0": (header(size=b"0 2 3"), ValueError),
    "height < 0": (header(size=b"2 -1 3"), ValueError),
    "one channel": (header(size=b"2 2 1"), ValueError),
    "four channels": (header(size=b"2 2 4"), ValueError),
    "header ends early": (b"#HSH1.2\n3\n2 2 3", ValueError),
    "not a number": (header(size=b"2 x 3"), ValueError),
    "ptm file type": (header(ftype=b"1"), NotImplementedError),
    "sh file type": (header(ftype=b"2"), NotImplementedError),
    "adaptive file type": (header(ftype=b"4"), NotImplementedError),
    "four terms": (header(terms=b"4 2 1"), NotImplementedError),
    "25 terms": (header(terms=b"25 2 1"), NotImplementedError),
    "basis type 1": (header(terms=b"9 1 1"), NotImplementedError),
    "two-byte elements": (header(terms=b"9 2 2"), NotImplementedError),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_headers_raise(tmp_path, case):
    head, exc = BAD[case]
    path = tmp_path / "bad.rti"
    path.write_bytes(head + body())
    for quantised in (False, True):
        with pytest.raises(exc):
            rti.read_rti(str(path), quantised=quantised)


def test_short_payloads_raise_and_comments_are_skipped(tmp_path):
    path = tmp_path / "a.rti"
    good = header() + body()
    path.write_bytes(good)
    assert rti.read_rti(str(path))[1].shape == (3, 2, 2, 9)
    for cut in (1, 4 * 27, 4 * 27 + 1, 4 * 27 + 71):  # into the payload, the biases and the scales
        path.write_bytes(good[:-cut])
        with pytest.raises(ValueError, match="short"):
            rti.read_rti(str(path))
    path.write_bytes(header(comment=b"# made by a test") + body())
    assert rti.read_rti(str(path))[0] == "hsh9"
    path.write_bytes(good + b"trailing bytes are ignored")
    assert rti.read_rti(str(path))[1].shape == (3, 2, 2, 9)


def test_write_rti_refuses_wrong_shapes(tmp_path):
    p = str(tmp_path / "x.rti")
    with pytest.raises(ValueError):
        rti.write_rti(p, np.zeros((3, 4, 4, 9), np.float32), "hsh16")
    with pytest.raises(ValueError):
        rti.write_rti(p, np.zeros((4, 4, 16), np.float32), "hsh16")
    with pytest.raises(ValueError):
        rti.write_rti(p, np.zeros((3, 0, 4, 16), np.float32), "hsh16")
    flat = rti.QuantisedHSH(torch.zeros((6, 3, 9), dtype=torch.uint8), torch.ones(18), "hsh9")
    with pytest.raises(ValueError, match="rows"):
        rti.write_rti(p, flat)
