"""NumPy restatement of the 8-bit RGB PTM arithmetic (include/rti.h), written op by op from the
header and importing nothing from the package: the quantiser and the dequantisation are float64 from the float32
inputs, the luminance is NumPy float32 operations (each rounded, nothing fused), everything runs under
np.errstate(all="ignore").  Also the seeded maps the tests share."""
import numpy as np

F32 = np.float32
K = 6
LUMA = (F32(0.299), F32(0.587), F32(0.114))


def finite_rgb(P, seed):
    """fp32 [3, P, 6], all finite: per-plane magnitudes spread over 1e-2 .. 1e3; plane 0 above zero only, plane 1
    below zero only, planes 2, 3 and 4 on both sides; plane 5 is 12.5 everywhere (the scale = 1 branch)."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.permutation(np.linspace(-2.0, 3.0, K))
    m = rng.uniform(-1.0, 1.0, (3, P, K))
    m[..., 0] = 0.25 + 0.75 * np.abs(m[..., 0])
    m[..., 1] = -0.25 - 0.75 * np.abs(m[..., 1])
    m *= mag
    m[..., 5] = 12.5
    return m.astype(F32)


def straddling_rgb(P, seed):
    """fp32 [3, P, 6], all finite, every plane with values on both sides of zero (the planes the format holds
    without clipping), magnitudes 1e-2 .. 1e3."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.permutation(np.linspace(-2.0, 3.0, K))
    return (rng.uniform(-1.0, 1.0, (3, P, K)) * mag).astype(F32)


def mixed_rgb(P, seed):
    """finite_rgb with about 0.5 % NaNs and a few ±inf spread over the channels (pixels 2, 3, 4 and P - 3 carry
    one of each kind in different channels when P >= 8) and, for P >= 256, plane 4 NaN everywhere (the
    no-finite-value branch)."""
    rng = np.random.default_rng(seed + 1)
    m = finite_rgb(P, seed)
    m[rng.random(m.shape) < 0.005] = np.nan
    n_inf = max(1, P // 400)
    for sign in (np.inf, -np.inf):
        m[rng.integers(0, 3, n_inf), rng.integers(0, P, n_inf), rng.integers(0, K, n_inf)] = sign
    if P >= 8:
        m[0, 2, 1], m[1, 3, 2], m[2, 4, 3] = np.nan, np.inf, -np.inf
        m[2, P - 3, 0], m[0, P - 3, 3], m[1, P - 3, 2] = np.nan, -np.inf, np.inf
    m[..., 5] = 12.5
    if P >= 256:
        m[..., 4] = np.nan
    return m


def host_qparams(m):
    """m fp32 [3, ..., 6] -> fp64 [12]: scale[0..5], bias[0..5]."""
    scale, bias = np.ones(K), np.zeros(K)
    with np.errstate(all="ignore"):
        for j in range(K):
            x = m[..., j].ravel()
            fin = x[np.abs(x) <= np.finfo(F32).max]  # false for NaN
            if fin.size == 0:
                continue
            lo, hi = np.float64(F32(fin.min())), np.float64(F32(fin.max()))
            if hi > lo:
                scale[j] = (hi - lo) / 255.0
            b = np.rint(-lo / scale[j])
            bias[j] = (b if b < 255.0 else 255.0) if b > 0.0 else 0.0
    return np.concatenate([scale, bias])


def host_quantise(m, qparams):
    """m fp32 [3, ..., 6] -> uint8 of the same shape."""
    scale, bias = qparams[:K], qparams[K:]
    with np.errstate(all="ignore"):
        x = m.astype(np.float64)
        t = x / scale + bias
        r = np.rint(t)
        r = np.where(r > 0.0, np.where(r < 255.0, r, 255.0), 0.0)
        r = np.where(x != x, bias, r)  # a NaN writes the bias
    return r.astype(np.uint8)


def host_dequantise(raw, qparams):
    """uint8 [3, ..., 6] -> fp32: (float)(((double)raw − bias)·scale)."""
    scale, bias = qparams[:K], qparams[K:]
    with np.errstate(all="ignore"):
        return ((raw.astype(np.float64) - bias) * scale).astype(F32)


def luminance(c, w=LUMA):
    """fp32 [3, ..., 6] -> fp32 [..., 6]: (w0·r + w1·g) + w2·b, two products and two sums, each rounded to fp32."""
    w = [F32(x) for x in w]
    with np.errstate(all="ignore"):
        rg = (w[0] * c[0]).astype(F32) + (w[1] * c[1]).astype(F32)
        return (rg.astype(F32) + (w[2] * c[2]).astype(F32)).astype(F32)
