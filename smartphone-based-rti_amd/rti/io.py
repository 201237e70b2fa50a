"""The reference's on-disk formats (Utils/utilities.py:48-101), read safely.

* Frames dataset ``<name>.pbz2`` (analysis.py:434, :460): bz2-compressed cPickle of
  ``list[(V uint8[R, R], camera_position float64[3])]`` — what
  ``FeatureMatcher.extractFeatures`` returns per frame.
* Relight tables ``<name>.pickle`` (analysis.py:475, interactive_relighting.py:95):
  plain pickle of ``list[list[int32[R, R]]]`` indexed ``[ly][lx]``.

Reading uses a restricted unpickler that only rebuilds NumPy arrays, dtypes and
builtin containers/scalars; any other global in the stream raises
``pickle.UnpicklingError`` instead of being imported or called.  Writing
produces files the reference itself can load.
"""
from __future__ import annotations

import bz2
import io
import os
import pickle

import numpy as np

_ALLOWED = {
    ("numpy", "ndarray"), ("numpy", "dtype"),
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
    ("builtins", "list"), ("builtins", "tuple"), ("builtins", "dict"), ("builtins", "set"),
    ("builtins", "frozenset"), ("builtins", "bytearray"), ("builtins", "complex"),
    ("_codecs", "encode"),  # protocol-2 bytes payloads of ndarray.__reduce__
}


class _SafeUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing to load global {module}.{name} from an RTI data file")


def safe_loads(buf):
    """Unpickle ``buf`` allowing only NumPy arrays and builtin containers."""
    return _SafeUnpickler(io.BytesIO(buf)).load()


def _path(filename, compressed):
    return filename + (".pbz2" if compressed else ".pickle")


def write_on_file(data, filename, compressed=True):
    """Utils/utilities.py:48-70: ``<filename>.pbz2`` (bz2 cPickle) or ``<filename>.pickle``."""
    path = _path(filename, compressed)
    if compressed:
        with bz2.BZ2File(path, "wb") as f:
            pickle.dump(data, f)
    else:
        with open(path, "wb") as f:
            pickle.dump(data, f)
    return path


def read_from_file(filename, compressed=True):
    """Utils/utilities.py:73-101 with a restricted unpickler; same missing-file error."""
    path = _path(filename, compressed)
    if not os.path.isfile(path):
        raise Exception("Storage file not found!")
    if compressed:
        with bz2.BZ2File(path, "rb") as f:
            return safe_loads(f.read())
    with open(path, "rb") as f:
        return safe_loads(f.read())


def frames_to_stack(results_frames):
    """list[(V uint8[R,R], cam f64[3])] -> (frames uint8 [N, R, R] light-major, cams f64 [N, 3]).

    The light-major stack is what ``rti.fit(..., cams=cams, mode="perpixel")`` consumes
    (compute_intensities + fit fused on the GPU)."""
    if results_frames is None or len(results_frames) <= 0:
        raise Exception("Error computing intensities: results are empty")
    frames = np.stack([np.asarray(f) for f, _ in results_frames])
    cams = np.stack([np.asarray(c, np.float64).ravel()[:3] for _, c in results_frames])
    return frames, cams


def read_frames(filename, compressed=True):
    """Load a reference frames dataset straight into GPU-ready arrays (frames, cams)."""
    return frames_to_stack(read_from_file(filename, compressed))


def tables_to_reference(tables):
    """int32 [G, G, R, R] -> the reference's ``list[list[int32[R, R]]]`` ([ly][lx])."""
    t = np.asarray(tables)
    return [[np.ascontiguousarray(t[i, j], dtype=np.int32) for j in range(t.shape[1])] for i in range(t.shape[0])]


def write_tables(tables, filename):
    """Write relight tables in the format interactive_relighting.compute() loads (:95)."""
    return write_on_file(tables_to_reference(tables), filename, compressed=False)


def read_tables(filename):
    """Read the reference's relight tables back as an int32 ndarray [G, G, R, R]."""
    return np.asarray(read_from_file(filename, compressed=False), dtype=np.int32)


# ---- .ptm files (PTM 1.2, the uncompressed LRGB and RGB payloads; layout restated in DESIGN.md §4.7) ----------
#   header, ASCII tokens: PTM_1.2, PTM_FORMAT_LRGB | PTM_FORMAT_RGB, W, H, six scales, six biases
#   payload, unsigned bytes, scanlines bottom row first; coefficient = (raw − bias_j)·scale_j
#     LRGB: H·W·6 coefficient bytes (a0..a5 per pixel), then H·W·3 bytes R G B per pixel
#     RGB:  three such coefficient blocks, R then G then B
_PTM_MAGIC = b"PTM_1.2"
_PTM_FORMATS = {b"PTM_FORMAT_LRGB": "lrgb", b"PTM_FORMAT_RGB": "rgb"}
_PTM_NOT_BUILT = (b"PTM_FORMAT_LUM", b"PTM_FORMAT_JPEG_LRGB", b"PTM_FORMAT_JPEG_RGB")


def _host_f64(maps):
    """A map as a host fp64 array; CUDA (or any torch) tensors are brought to the host."""
    if hasattr(maps, "detach"):
        maps = maps.detach().cpu().numpy()
    return np.asarray(maps, dtype=np.float64)


def _ptm_quantise(v):
    """v [..., 6] fp64 -> (raw uint8 [..., 6], scale fp64 [6], bias int [6]): per coefficient j over the finite
    values, scale = (hi − lo)/255 (1 when hi = lo or nothing is finite), bias = clip(rint(−lo/scale), 0, 255),
    raw = clip(rint(v/scale + bias), 0, 255); a NaN writes raw = bias."""
    scale, bias = np.ones(6), np.zeros(6, np.int64)
    raw = np.empty(v.shape, np.uint8)
    for j in range(6):
        x = v[..., j]
        fin = x[np.isfinite(x)]
        if fin.size and fin.max() > fin.min():
            scale[j] = (fin.max() - fin.min()) / 255.0
        if fin.size:
            bias[j] = int(np.clip(np.rint(-fin.min() / scale[j]), 0, 255))
        with np.errstate(invalid="ignore"):
            q = np.clip(np.rint(x / scale[j] + bias[j]), 0, 255)
        raw[..., j] = np.where(np.isnan(x), bias[j], q).astype(np.uint8)
    return raw, scale, bias


def write_ptm(path, maps, format=None):
    """Write an uncompressed PTM 1.2 file.  format="lrgb" (what None means for arrays): maps [H, W, 9]
    (``fit_lrgb``, pixel-major); format="rgb": maps [3, H, W, 6] (``fit`` of a colour stack).  Arrays or tensors on
    any device.

    Coefficients are quantised to bytes per coefficient plane (one scale and bias per coefficient, shared by the
    three channels of an RGB file); a plane whose values do not straddle zero loses what lies above 255·scale,
    because the format's bias is a byte.  LRGB colours are stored as bytes of chroma/s with s the largest finite
    chroma, and the luminance is multiplied by s: the product chroma·L survives, the normalisation
    Σ w·chroma = 1 does not.  Returns path.

    maps may also be a quantised object with rows, whose bytes and header doubles are copied to the host and
    written as they are, with the same header: a ``QuantisedLRGB`` [H, W] (``quantise_lrgb``, ``read_ptm8``)
    writes PTM_FORMAT_LRGB, a ``QuantisedRGB`` [H, W] (``quantise_rgb``, ``read_ptm8``) PTM_FORMAT_RGB.  format
    None means the object's own; one that contradicts it raises ValueError."""
    from .api import QuantisedLRGB, QuantisedRGB

    if isinstance(maps, QuantisedLRGB):
        if format not in (None, "lrgb"):
            raise ValueError(f"a QuantisedLRGB is an LRGB payload; got format {format!r}")
        if len(maps.shape) != 2:
            raise ValueError(f"a file needs a map with rows: QuantisedLRGB [H, W]; got {maps.shape}")
        raw, rgb = maps.coef.detach().cpu().numpy(), maps.rgb.detach().cpu().numpy()
        return _ptm_write(path, b"PTM_FORMAT_LRGB", maps.shape, maps.scale, maps.bias, [raw[::-1], rgb[::-1]])
    if isinstance(maps, QuantisedRGB):
        if format not in (None, "rgb"):
            raise ValueError(f"a QuantisedRGB is an RGB payload; got format {format!r}")
        if len(maps.shape) != 2:
            raise ValueError(f"a file needs a map with rows: QuantisedRGB [H, W]; got {maps.shape}")
        raw = maps.coef.detach().cpu().numpy()
        return _ptm_write(path, b"PTM_FORMAT_RGB", maps.shape, maps.scale, maps.bias,
                          [raw[c, ::-1] for c in range(3)])
    if format is None:
        format = "lrgb"
    m = _host_f64(maps)
    if format == "lrgb":
        if m.ndim != 3 or m.shape[2] != 9:
            raise ValueError(f"an LRGB map is [H, W, 9]; got {m.shape}")
        H, W = m.shape[:2]
        chroma = m[..., 6:]
        fin = chroma[np.isfinite(chroma)]
        s = float(fin.max()) if fin.size and fin.max() > 0 else 1.0
        with np.errstate(invalid="ignore"):
            rgb = np.clip(np.rint(255.0 * chroma / s), 0, 255)
        rgb = np.where(np.isnan(chroma), 0, rgb).astype(np.uint8)
        raw, scale, bias = _ptm_quantise(m[..., :6] * s)
        blocks = [raw[::-1], rgb[::-1]]
        tag = b"PTM_FORMAT_LRGB"
    elif format == "rgb":
        if m.ndim != 4 or m.shape[0] != 3 or m.shape[3] != 6:
            raise ValueError(f"RGB coefficient maps are [3, H, W, 6]; got {m.shape}")
        H, W = m.shape[1:3]
        raw, scale, bias = _ptm_quantise(m)
        blocks = [raw[c, ::-1] for c in range(3)]
        tag = b"PTM_FORMAT_RGB"
    else:
        raise ValueError(f"unknown PTM format {format!r} (expected 'lrgb' or 'rgb')")
    if H < 1 or W < 1:
        raise ValueError(f"empty map {m.shape}")
    return _ptm_write(path, tag, (H, W), scale, bias, blocks)


def _ptm_write(path, tag, shape, scale, bias, blocks):
    """The header (scales as %.9g, biases as integers) and the payload blocks, already bottom row first."""
    H, W = shape
    head = b"\n".join([_PTM_MAGIC, tag, b"%d" % W, b"%d" % H, " ".join("%.9g" % x for x in scale).encode(),
                       " ".join("%d" % b for b in bias).encode()]) + b"\n"
    with open(path, "wb") as f:
        f.write(head)
        for b in blocks:
            f.write(np.ascontiguousarray(b).tobytes())
    return path


def _ptm_tokens(buf, n):
    """The first n whitespace-separated tokens of buf and the offset of the byte after the last one."""
    toks, i = [], 0
    while len(toks) < n:
        while i < len(buf) and buf[i:i + 1].isspace():
            i += 1
        j = i
        while j < len(buf) and not buf[j:j + 1].isspace():
            j += 1
        if j == i:
            raise ValueError("PTM header ends early")
        toks.append(buf[i:j])
        i = j
    return toks, i


def _ptm_read(path):
    """An uncompressed PTM 1.2 file -> (format, H, W, scale fp64 [6], bias fp64 [6], payload bytes), checked."""
    with open(path, "rb") as f:
        buf = f.read()
    (magic, tag), _ = _ptm_tokens(buf, 2)
    if magic != _PTM_MAGIC:
        raise ValueError(f"not a PTM 1.2 file: magic {magic[:16]!r}")
    if tag in _PTM_NOT_BUILT:
        raise NotImplementedError(f"{tag.decode()} files are not built (uncompressed LRGB and RGB only)")
    if tag not in _PTM_FORMATS:
        raise ValueError(f"unknown PTM format {tag[:32]!r}")
    toks, end = _ptm_tokens(buf, 16)
    try:
        W, H = int(toks[2]), int(toks[3])
        scale = np.array([float(t) for t in toks[4:10]])
        bias = np.array([int(t) for t in toks[10:16]], np.float64)
    except ValueError:
        raise ValueError("malformed PTM header") from None
    if W < 1 or H < 1:
        raise ValueError(f"PTM header: bad size {W} x {H}")
    fmt = _PTM_FORMATS[tag]
    need = (9 if fmt == "lrgb" else 18) * H * W
    data = np.frombuffer(buf, np.uint8, offset=min(end + 1, len(buf)))
    if data.size < need:
        raise ValueError(f"short PTM payload: {data.size} of {need} bytes")
    return fmt, H, W, scale, bias, data


def _ptm_quantised(fmt, H, W, scale, bias, data):
    """The payload as it is: a QuantisedLRGB or QuantisedRGB [H, W] of host tensors, rows top first."""
    import torch

    from .api import QuantisedLRGB, QuantisedRGB

    n = H * W
    if fmt == "lrgb":
        blocks = [data[a * n:b * n].reshape(H, W, b - a)[::-1].copy(order="C") for a, b in ((0, 6), (6, 9))]
        qparams = np.concatenate([scale, bias, [1.0]])
        return QuantisedLRGB(*(torch.from_numpy(x) for x in blocks + [qparams]))
    raw = data[:18 * n].reshape(3, H, W, 6)[:, ::-1].copy(order="C")
    return QuantisedRGB(torch.from_numpy(raw), torch.from_numpy(np.concatenate([scale, bias])))


def read_ptm(path, quantised=False):
    """Read an uncompressed PTM 1.2 file -> ``(format, maps)``: ("lrgb", fp32 [H, W, 9]) or ("rgb", fp32
    [3, H, W, 6]), rows top first as ``write_ptm`` takes them.  Any whitespace may separate the header's tokens;
    the payload starts one byte after the last bias.  LRGB chroma is byte/255.  The LUM and JPEG formats raise
    NotImplementedError, a bad magic or a short payload ValueError.

    quantised=True keeps an LRGB file's 9 bytes per pixel: ("lrgb", ``QuantisedLRGB`` [H, W]) of host tensors,
    rows top first, the header's scales and biases and s = 1; ``.to(device)`` moves it to the GPU for
    ``relight_lrgb8``.  RGB files raise NotImplementedError here: ``read_ptm8`` keeps the bytes of either format
    and returns a ``QuantisedRGB`` for them."""
    fmt, H, W, scale, bias, data = _ptm_read(path)
    n = H * W
    if quantised:
        if fmt != "lrgb":
            raise NotImplementedError("read_ptm(quantised=True) keeps LRGB payloads only; read_ptm8(path) returns "
                                      "the 18 bytes per pixel of an RGB file as a QuantisedRGB")
        return fmt, _ptm_quantised(fmt, H, W, scale, bias, data)
    if fmt == "lrgb":
        coef = (data[:6 * n].reshape(H, W, 6)[::-1].astype(np.float64) - bias) * scale
        rgb = data[6 * n:9 * n].reshape(H, W, 3)[::-1].astype(np.float64) / 255.0
        return fmt, np.concatenate([coef, rgb], -1).astype(np.float32)
    coef = (data[:18 * n].reshape(3, H, W, 6)[:, ::-1].astype(np.float64) - bias) * scale
    return fmt, coef.astype(np.float32)


def read_ptm8(path):
    """Read an uncompressed PTM 1.2 file and keep its bytes -> ``(format, q)``: ("lrgb", ``QuantisedLRGB`` [H, W])
    with s = 1, exactly what ``read_ptm(path, quantised=True)`` returns, or ("rgb", ``QuantisedRGB`` [H, W]).  Host
    tensors, rows top first, the header's scales and biases; ``.to(device)`` moves the object to the GPU for
    ``relight_lrgb8`` or ``relight_rgb8`` / ``rgb8_normals``.  ``dequantise_lrgb`` / ``dequantise_rgb`` of it equal
    ``read_ptm(path)[1]`` to the bit.  Errors as ``read_ptm``."""
    fmt, H, W, scale, bias, data = _ptm_read(path)
    return fmt, _ptm_quantised(fmt, H, W, scale, bias, data)


# ---- .rti files (HSH 1.2, uncompressed RGB hemispherical harmonics; layout restated in DESIGN.md §4.9) --------
#   ASCII lines; a line that starts with '#' after the first is a comment:
#     #HSH1.2
#     3                 the RTI file type: HSH
#     W H 3             width, height, colour channels
#     k 2 1             terms per channel (9 or 16), basis type (2 = HSH), bytes per element
#   then k little-endian fp32 scales and k little-endian fp32 biases, shared by the three channels
#   then H·W·3·k payload bytes: rows top first, per pixel the k bytes of R, then of G, then of B;
#     coefficient = (float)raw·(scale_j/255) + bias_j in fp32, term j = column j of rti_basis_eval
#   No file of another writer was available to this build: the row order, and the order and signs of the
#   sin / cos terms relative to other HSH writers, are this build's restatement and unverified.  Each is one
#   constant below.
_RTI_MAGIC = b"#HSH1.2"
_RTI_TYPE_HSH = 3
_RTI_BASIS_HSH = 2
_RTI_ROW_STEP = 1                    # 1: the file's first row is the map's top row; -1 would store bottom first
_RTI_TERM_ORDER = tuple(range(16))   # file term i of a pixel is column _RTI_TERM_ORDER[i] of rti_basis_eval
_RTI_BASES = {9: "hsh9", 16: "hsh16"}


def _rti_terms(basis):
    from .api import _HSH8_TERMS, _hsh8_basis

    return _HSH8_TERMS[_hsh8_basis(basis)]


def hsh_qparams_host(m):
    """m fp32 [3, ..., k] -> (scale fp32 [k], bias fp32 [k]), rti_hsh_qparams' arithmetic (include/rti.h): over
    the finite values of term j in the three channels, bias = lo (a zero as +0), scale = hi − lo in fp32 where
    that is finite and > 0, else 1; a term without a finite value gets (1, 0)."""
    k = m.shape[-1]
    scale, bias = np.ones(k, np.float32), np.zeros(k, np.float32)
    with np.errstate(all="ignore"):
        for j in range(k):
            x = m[..., j]
            fin = x[np.isfinite(x)]
            if fin.size:
                lo, hi = np.float32(fin.min()), np.float32(fin.max())
                bias[j] = lo + np.float32(0.0)
                d = np.float32(hi - lo)
                if np.isfinite(d) and d > 0:
                    scale[j] = d
    return scale, bias


def hsh_quantise_host(m, scale, bias):
    """m fp32 [..., k] -> uint8 of the same shape, rti_hsh_quantise's arithmetic: step = scale/255 in fp32, then
    raw = clip(rint((x − bias)/step), 0, 255) in fp64; a NaN writes 0, ±inf saturates."""
    with np.errstate(all="ignore"):
        step = np.asarray(scale, np.float32) / np.float32(255.0)
        t = (m.astype(np.float64) - np.asarray(bias, np.float32).astype(np.float64)) / step.astype(np.float64)
        raw = np.clip(np.rint(t), 0.0, 255.0)
        return np.where(np.isnan(t), 0.0, raw).astype(np.uint8)


def hsh_dequantise_host(raw, scale, bias):
    """uint8 [..., k] -> fp32, the map read_rti builds: (float)raw·(scale/255) + bias, every operation in fp32."""
    with np.errstate(all="ignore"):
        step = np.asarray(scale, np.float32) / np.float32(255.0)
        t = raw.astype(np.float32) * step
        return (t + np.asarray(bias, np.float32)).astype(np.float32)


def write_rti(path, maps, basis="hsh16"):
    """Write an uncompressed HSH ``.rti`` file (``#HSH1.2``, RGB, one byte per coefficient).

    maps: a ``QuantisedHSH`` [H, W] (``quantise_hsh``, or ``read_rti(path, quantised=True)``), whose bytes and
    2k floats are copied to the host and written as they are (its own basis is used); or three fp32 maps
    [3, H, W, k] (``fit`` of a colour stack with an HSH basis), an array or a tensor on any device, quantised on
    the host with the arithmetic of ``rti_hsh_qparams`` / ``rti_hsh_quantise``, so both routes write the same
    file.  The header holds the scales and biases as binary fp32: a round trip through a file is exact.  Returns
    path."""
    from .api import QuantisedHSH

    if isinstance(maps, QuantisedHSH):
        if len(maps.shape) != 2:
            raise ValueError(f"a file needs a map with rows: QuantisedHSH [H, W]; got {maps.shape}")
        k = maps.k
        raw, scale, bias = maps.coef.detach().cpu().numpy(), maps.scale, maps.bias
    else:
        k = _rti_terms(basis)
        if hasattr(maps, "detach"):
            maps = maps.detach().cpu().numpy()
        m = np.asarray(maps, dtype=np.float32)
        if m.ndim != 4 or m.shape[0] != 3 or m.shape[3] != k:
            raise ValueError(f"RGB HSH maps are [3, H, W, {k}]; got {m.shape}")
        if m.shape[1] < 1 or m.shape[2] < 1:
            raise ValueError(f"empty map {m.shape}")
        scale, bias = hsh_qparams_host(m)
        raw = hsh_quantise_host(m, scale, bias).transpose(1, 2, 0, 3)
    H, W = raw.shape[:2]
    order = list(_RTI_TERM_ORDER[:k])
    head = b"\n".join([_RTI_MAGIC, b"%d" % _RTI_TYPE_HSH, b"%d %d 3" % (W, H), b"%d %d 1" % (k, _RTI_BASIS_HSH)])
    with open(path, "wb") as f:
        f.write(head + b"\n")
        f.write(np.asarray(scale, np.float32)[order].astype("<f4").tobytes())
        f.write(np.asarray(bias, np.float32)[order].astype("<f4").tobytes())
        f.write(np.ascontiguousarray(raw[::_RTI_ROW_STEP][..., order]).tobytes())
    return path


def _rti_line(buf, pos, what):
    """The next header line of buf from pos (comment lines skipped) as integer tokens, and the offset after it."""
    while True:
        end = buf.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"RTI header ends early ({what})")
        line, pos = buf[pos:end].strip(), end + 1
        if not line.startswith(b"#"):
            break
    try:
        return [int(t) for t in line.split()], pos
    except ValueError:
        raise ValueError(f"malformed RTI header ({what}): {line[:32]!r}") from None


def read_rti(path, quantised=False):
    """Read an uncompressed HSH ``.rti`` file -> ``(basis, maps)``: ("hsh9" | "hsh16", fp32 [3, H, W, k]), rows
    top first as ``write_rti`` takes them, each coefficient (float)raw·(scale/255) + bias in fp32.

    quantised=True keeps the file's 3k bytes per pixel: (basis, ``QuantisedHSH`` [H, W]) of host tensors with
    the header's scales and biases; ``.to(device)`` moves it to the GPU for ``relight_hsh8``.

    A bad magic, a short payload, W or H < 1 or a channel count other than 3 raise ValueError; a term count other
    than 9 / 16, a basis type other than 2 (HSH), an element size other than 1 and the other RTI file types raise
    NotImplementedError."""
    with open(path, "rb") as f:
        buf = f.read()
    end = buf.find(b"\n")
    if buf[:end if end >= 0 else len(buf)].strip() != _RTI_MAGIC:
        raise ValueError(f"not an HSH 1.2 .rti file: magic {buf[:16]!r}")
    ftype, pos = _rti_line(buf, end + 1, "file type")
    if len(ftype) != 1:
        raise ValueError(f"malformed RTI header (file type): {ftype}")
    if ftype[0] != _RTI_TYPE_HSH:
        raise NotImplementedError(f"RTI file type {ftype[0]} is not built (3 = HSH only)")
    size, pos = _rti_line(buf, pos, "size")
    terms, pos = _rti_line(buf, pos, "basis")
    if len(size) != 3 or len(terms) != 3:
        raise ValueError(f"malformed RTI header: size {size}, basis {terms}")
    (W, H, C), (k, btype, esize) = size, terms
    if W < 1 or H < 1:
        raise ValueError(f"RTI header: bad size {W} x {H}")
    if C != 3:
        raise ValueError(f"RTI header: {C} colour channels (3 expected)")
    if btype != _RTI_BASIS_HSH:
        raise NotImplementedError(f"RTI basis type {btype} is not built (2 = HSH only)")
    if esize != 1:
        raise NotImplementedError(f"RTI element size {esize} is not built (1 byte only)")
    if k not in _RTI_BASES:
        raise NotImplementedError(f"{k} HSH terms are not built (9 and 16 only)")
    need = 8 * k + H * W * 3 * k
    if len(buf) - pos < need:
        raise ValueError(f"short RTI payload: {max(len(buf) - pos, 0)} of {need} bytes")
    order = list(_RTI_TERM_ORDER[:k])
    qp = np.frombuffer(buf, "<f4", 2 * k, pos).astype(np.float32).reshape(2, k)
    scale, bias = np.empty(k, np.float32), np.empty(k, np.float32)
    scale[order], bias[order] = qp[0], qp[1]
    data = np.frombuffer(buf, np.uint8, H * W * 3 * k, pos + 8 * k).reshape(H, W, 3, k)[::_RTI_ROW_STEP]
    raw = np.empty((H, W, 3, k), np.uint8)
    raw[..., order] = data
    if quantised:
        import torch

        from .api import QuantisedHSH

        return _RTI_BASES[k], QuantisedHSH(torch.from_numpy(raw), torch.from_numpy(np.concatenate([scale, bias])),
                                           _RTI_BASES[k])
    return _RTI_BASES[k], np.ascontiguousarray(hsh_dequantise_host(raw, scale, bias).transpose(2, 0, 1, 3))
