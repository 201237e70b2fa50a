"""fp64 restatement of rti_relight_lrgb_enhanced / rti_relight_lrgb8_enhanced / rti_relight_rgb8_enhanced
(include/rti.h) in vectorised NumPy, built from the references the project already has
(normals_ref, rgb8_ref, lrgb_ref); it imports nothing from the package.  NumPy rounds every product, sum, quotient
and square root and fuses nothing, which is the arithmetic the header prescribes, and every expression keeps the
header's left-to-right order, so the fp64 value before the output conversion is the header's to the bit.  Also the
seeded maps the tests share."""
import functools

import numpy as np

from normals_ref import half_vector, normals_ref, peak_ref, peaked_coef, powi, ptm_value, to_int32, to_uint8
from rgb8_ref import LUMA, host_dequantise, host_qparams, host_quantise, luminance

F32 = np.float32
MODES = ("diffuse_gain", "specular")


def diffuse_gain_coef_at(coef, k, g):
    """normals_ref.diffuse_gain_coef with the peak k (peak_ref's dict) of ANOTHER map: the coefficients a' of
    a = coef [P, 6] under diffuse gain g about k's (u0, v0), fp64 [P, 6]; pixels where k has no maximum keep a."""
    a = np.asarray(coef).astype(np.float64).reshape(-1, 6)
    u0, v0 = k["u0"], k["v0"]
    g = np.float64(g)
    h = 1.0 - g
    with np.errstate(all="ignore"):
        b = np.empty_like(a)
        b[:, 0] = g * a[:, 0]
        b[:, 1] = g * a[:, 1]
        b[:, 2] = g * a[:, 2]
        b[:, 3] = h * (2.0 * a[:, 0] * u0 + a[:, 2] * v0) + a[:, 3]
        b[:, 4] = h * (2.0 * a[:, 1] * v0 + a[:, 2] * u0) + a[:, 4]
        b[:, 5] = (h * (a[:, 0] * (u0 * u0) + a[:, 1] * (v0 * v0) + a[:, 2] * u0 * v0) + (a[:, 3] - b[:, 3]) * u0
                   + (a[:, 4] - b[:, 4]) * v0 + a[:, 5])
    return np.where(k["has_max"][:, None], b, a)


def highlight(lum, lu, lv, exp):
    """S = max(0, n·H)^exp of the luminance map lum [P, 6], and normals_ref's dict of it."""
    assert 1 <= exp <= 255
    r = normals_ref(lum)
    hx, hy, hz = half_vector(lu, lv)
    with np.errstate(all="ignore"):
        c = r["n"][:, 0] * hx + r["n"][:, 1] * hy + r["n"][:, 2] * hz
        return powi(np.where(c > 0.0, c, 0.0), int(exp)), r


def lrgb_enhanced_ref(lrgb, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1):
    """lrgb [P, 9] as stored (fp32) -> the fp64 image [P, 3] before conversion."""
    m = np.asarray(lrgb).reshape(-1, 9)
    lum, chroma = m[:, :6], m[:, 6:].astype(np.float64)
    lu, lv = np.float64(lu), np.float64(lv)
    out = np.empty((m.shape[0], 3))
    with np.errstate(all="ignore"):
        if mode == "diffuse_gain":
            k = peak_ref(lum)
            G = ptm_value(diffuse_gain_coef_at(lum, k, gain), lu, lv)
            G = np.where(k["finite"], G, np.nan)
            for c in range(3):
                out[:, c] = chroma[:, c] * G
        else:
            assert mode == "specular"
            S, r = highlight(lum, lu, lv, exp)
            D = ptm_value(r["a"], lu, lv)
            for c in range(3):
                v = np.float64(kd) * (chroma[:, c] * D) + np.float64(ks) * S
                out[:, c] = np.where(r["finite"], v, np.nan)
    return out


def dequantise_lrgb_ref(raw, rgb, qparams):
    """The 9 bytes of a pixel -> the fp32 LRGB map read_ptm builds: (float)(((double)raw − bias)·scale) and
    (float)((double)byte/255.0)."""
    scale, bias = qparams[:6], qparams[6:12]
    with np.errstate(all="ignore"):
        a = ((raw.astype(np.float64) - bias) * scale).astype(F32)
        c = (rgb.astype(np.float64) / 255.0).astype(F32)
    return np.concatenate([a, c], -1)


def lrgb8_enhanced_ref(raw, rgb, qparams, lu, lv, mode, **kw):
    return lrgb_enhanced_ref(dequantise_lrgb_ref(raw, rgb, qparams), lu, lv, mode, **kw)


def rgb_enhanced_ref(deq, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1, weights=None):
    """deq: the dequantised fp32 maps [3, P, 6] -> the fp64 image [P, 3] before conversion.  The luminance is
    rgb8_ref.luminance (fp32) of the three maps."""
    lum = luminance(deq, LUMA if weights is None else weights)
    lu, lv = np.float64(lu), np.float64(lv)
    out = np.empty((deq.shape[1], 3))
    with np.errstate(all="ignore"):
        if mode == "diffuse_gain":
            k = peak_ref(lum)
            for c in range(3):
                out[:, c] = np.where(k["finite"], ptm_value(diffuse_gain_coef_at(deq[c], k, gain), lu, lv), np.nan)
        else:
            assert mode == "specular"
            S, r = highlight(lum, lu, lv, exp)
            for c in range(3):
                v = np.float64(kd) * ptm_value(deq[c].astype(np.float64), lu, lv) + np.float64(ks) * S
                out[:, c] = np.where(r["finite"], v, np.nan)
    return out


def rgb8_enhanced_ref(raw, qparams, lu, lv, mode, **kw):
    return rgb_enhanced_ref(host_dequantise(raw, qparams), lu, lv, mode, **kw)


def convert(x, dtype_name):
    """The fp64 image -> the stored one: "float32" rounded once, "int32" / "uint8" as rti_convert.h."""
    with np.errstate(all="ignore"):
        return {"float32": lambda v: v.astype(F32), "int32": to_int32, "uint8": to_uint8}[dtype_name](x)


def kinds_of(lum):
    return normals_ref(lum)["kind"]


# ---- seeded maps ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def peaked_rgb(P):
    """test_gpu_rgb8.py's peaked family, restated: three channels of one surface, interior maxima, maxima outside
    the disc and minima in equal parts, the channels 0.8, 1.0 and 1.15 times the biquadratic plus a little noise ->
    fp32 [3, P, 6].  (rgb8_ref.mixed_rgb will not do here: its quantised luminance has no maximum anywhere.)"""
    rng = np.random.default_rng(900 + P)
    n = [P - 2 * (P // 3), P // 3, P // 3]
    a = np.concatenate([peaked_coef(rng, n[0], 0.0, 0.9)[0], peaked_coef(rng, n[1], 1.1, 2.0)[0],
                        peaked_coef(rng, n[2], 0.0, 0.9, sign=1.0)[0]])
    a = a[rng.permutation(P)]
    m = np.stack([g * a for g in (0.8, 1.0, 1.15)]) + rng.normal(0, 0.05, (3, P, 6))
    m = m.astype(F32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def peaked_rgb8(P):
    """(raw uint8 [3, P, 6], qparams fp64 [12], dequantised fp32 [3, P, 6]) of peaked_rgb(P) by the host's
    quantiser -- computed once, shared and never written."""
    m = peaked_rgb(P)
    qp = host_qparams(m)
    raw = host_quantise(m, qp)
    deq = host_dequantise(raw, qp)
    for a in (qp, raw, deq):
        a.setflags(write=False)
    return raw, qp, deq
