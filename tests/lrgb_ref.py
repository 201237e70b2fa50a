"""fp64 restatement of rti_lrgb_from_rgb / rti_relight_lrgb (include/rti.h), written straight from
their formulas in vectorised NumPy; it imports nothing from the package.  NumPy rounds every product, sum and
quotient and fuses nothing, which is the arithmetic the header prescribes, and every expression below keeps the
header's left-to-right order.  Also the output conversions of rti_convert.h and the seeded maps the tests share."""
import numpy as np

from normals_ref import mixed_coef

INT32_MIN = -2 ** 31


def weights_of(weights):
    """NULL = 1.0/3.0 each, as the library fills it in."""
    return np.full(3, 1.0 / 3.0) if weights is None else np.asarray(weights, np.float64)


def lrgb_ref(coef, gram, weights=None):
    """coef [3, P, 6] (fp32 or fp64), gram [6, 6], weights [3] or None -> fp64 [P, 9]: (a0..a5, cR, cG, cB)."""
    x = np.asarray(coef).astype(np.float64)
    G = np.asarray(gram, np.float64)
    w = weights_of(weights)
    P = x.shape[1]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x).all(axis=(0, 2))
        a = [w[0] * x[0, :, j] + w[1] * x[1, :, j] + w[2] * x[2, :, j] for j in range(6)]
        t = []
        for i in range(6):
            acc = G[i, 0] * a[0]
            for j in range(1, 6):
                acc = acc + G[i, j] * a[j]
            t.append(acc)
        d = a[0] * t[0]
        for i in range(1, 6):
            d = d + a[i] * t[i]
        lit = np.isfinite(d) & (d > 0.0)
        out = np.empty((P, 9))
        for c in range(3):
            s = x[c, :, 0] * t[0]
            for i in range(1, 6):
                s = s + x[c, :, i] * t[i]
            out[:, 6 + c] = np.where(lit, s / np.where(lit, d, 1.0), 1.0)
        for j in range(6):
            out[:, j] = a[j]
    out[~finite] = np.nan
    return out


def ptm_basis(lu, lv):
    """rti_basis.h's ptm_eval in fp64: (lu², lv², lu·lv, lu, lv, 1)."""
    lu, lv = np.float64(lu), np.float64(lv)
    return [lu * lu, lv * lv, lu * lv, lu, lv, np.float64(1.0)]


def luminance_ref(a, lu, lv):
    """L of coefficients a [P, 6] (fp64) at one direction: rti_relight's dot_k<6>(double), the six products
    summed left to right."""
    b = ptm_basis(lu, lv)
    with np.errstate(all="ignore"):
        acc = a[:, 0] * b[0]
        for k in range(1, 6):
            acc = acc + a[:, k] * b[k]
    return acc


def relight_lrgb_ref(lrgb, lu, lv):
    """lrgb [P, 9] as stored (fp32), E directions -> the fp64 images [E, P, 3] before conversion."""
    m = np.asarray(lrgb).astype(np.float64).reshape(-1, 9)
    lu, lv = np.atleast_1d(np.asarray(lu, np.float64)), np.atleast_1d(np.asarray(lv, np.float64))
    out = np.empty((lu.size, m.shape[0], 3))
    with np.errstate(all="ignore"):
        for e in range(lu.size):
            L = luminance_ref(m[:, :6], lu[e], lv[e])
            for c in range(3):
                out[e, :, c] = m[:, 6 + c] * L
    return out


def to_int32(x):
    """rti_convert.h's int32: C truncation toward zero, NaN / out of range -> INT32_MIN."""
    x = np.asarray(x, np.float64)
    ok = np.abs(x) < 2147483648.0  # False for NaN
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), INT32_MIN).astype(np.int64).astype(np.int32)


def to_uint8(x):
    """rti_convert.h's uint8: the int32 value clipped to [0, 255]."""
    return np.clip(to_int32(x), 0, 255).astype(np.uint8)


# ---- seeded maps ----------------------------------------------------------------------------------------------

def synth_dirs(N, seed):
    """N light directions inside the unit disc, fp32."""
    rng = np.random.default_rng(seed)
    r, phi = np.sqrt(rng.uniform(0.0, 0.81, N)), rng.uniform(0, 2 * np.pi, N)
    return (r * np.cos(phi)).astype(np.float32), (r * np.sin(phi)).astype(np.float32)


def mixed_rgb_coef(P, seed):
    """Three PTM-6 maps [3, P, 6] fp32 in normals_ref.mixed_coef's style (every class of biquadratic, its NaN and
    ±inf rows in each channel), with planted black pixels (all 18 coefficients zero: chroma 1) and planted NaN
    pixels at the first and last pixels of the map and around a wave boundary when the map has them."""
    x = np.stack([mixed_coef(P, seed + 17 * c) for c in range(3)])
    if P >= 8:
        black = [0, P - 1] + ([255, 256] if P > 300 else [])
        nan = [1, P - 2] + ([257] if P > 300 else [])
        x[:, black] = 0.0
        x[:, nan] = 0.25
        x[np.arange(len(nan)) % 3, nan, np.arange(len(nan)) % 6] = np.nan
    return x


def mixed_lrgb(P, seed):
    """An LRGB map [P, 9] fp32: mixed_coef luminance (NaN / inf rows included) and chroma in [0.2, 1.8], with
    planted all-NaN pixels as rti_lrgb_from_rgb writes them."""
    rng = np.random.default_rng(seed + 5)
    m = np.concatenate([mixed_coef(P, seed), rng.uniform(0.2, 1.8, (P, 3))], -1).astype(np.float32)
    if P >= 8:
        m[[2, P - 3]] = np.nan
    return m
