"""NumPy restatement of the 8-bit HSH arithmetic (include/rti.h), written op by op from the header
and importing nothing from the package: fp32 operations are NumPy float32 operations (each rounded, nothing fused),
the quantiser is float64, everything runs under np.errstate(all="ignore").  Also the seeded maps the tests share."""
import numpy as np

F32 = np.float32


def finite_hsh(P, k, seed):
    """fp32 [3, P, k], all finite: per-term ranges that differ by orders of magnitude (1e-2 .. 1e3), a third of
    the terms above zero only, a third below zero only, the rest on both sides; term 5 is 12.5 everywhere (the
    scale = 1 branch)."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.permutation(np.linspace(-2.0, 3.0, k))
    m = rng.uniform(-1.0, 1.0, (3, P, k))
    for j in range(k):
        if j % 3 == 0:
            m[..., j] = 0.25 + 0.75 * np.abs(m[..., j])
        elif j % 3 == 1:
            m[..., j] = -0.25 - 0.75 * np.abs(m[..., j])
    m *= mag
    m[..., 5] = 12.5
    return m.astype(F32)


def mixed_hsh(P, k, seed):
    """finite_hsh with about 0.5 % NaNs and a few ±inf spread over the channels (pixels 2, 3, 4 and P - 3 carry
    one of each kind in different channels when P >= 8) and, for P >= 256, term 7 NaN everywhere (the
    no-finite-value branch)."""
    rng = np.random.default_rng(seed + 1)
    m = finite_hsh(P, k, seed)
    m[rng.random(m.shape) < 0.005] = np.nan
    n_inf = max(1, P // 400)
    for sign in (np.inf, -np.inf):
        m[rng.integers(0, 3, n_inf), rng.integers(0, P, n_inf), rng.integers(0, k, n_inf)] = sign
    if P >= 8:
        m[0, 2, 1], m[1, 3, 2], m[2, 4, 3] = np.nan, np.inf, -np.inf
        m[2, P - 3, 0], m[0, P - 3, 4], m[1, P - 3, 6] = np.nan, -np.inf, np.inf
    m[..., 5] = 12.5
    if P >= 256:
        m[..., 7] = np.nan
    return m


def host_qparams(m):
    """m fp32 [3, P, k] -> fp32 [2k]: scale[0..k-1], bias[0..k-1]."""
    k = m.shape[-1]
    scale, bias = np.ones(k, F32), np.zeros(k, F32)
    with np.errstate(all="ignore"):
        for j in range(k):
            x = m[..., j].ravel()
            fin = x[np.abs(x) <= np.finfo(F32).max]  # false for NaN
            if fin.size == 0:
                continue
            lo, hi = F32(fin.min()), F32(fin.max())
            bias[j] = lo + F32(0.0)  # a zero of either sign is written as +0
            d = F32(hi - lo)
            if d > 0 and d <= np.finfo(F32).max:
                scale[j] = d
    return np.concatenate([scale, bias])


def host_steps(qparams):
    k = qparams.size // 2
    with np.errstate(all="ignore"):
        return (qparams[:k].astype(F32) / F32(255.0)).astype(F32), qparams[k:].astype(F32)


def host_quantise(m, qparams):
    """m fp32 [3, P, k] -> uint8 [P, 3, k]."""
    step, bias = host_steps(qparams)
    with np.errstate(all="ignore"):
        t = (m.astype(np.float64) - bias.astype(np.float64)) / step.astype(np.float64)
        r = np.rint(t)
        r = np.where(r > 0.0, np.where(r < 255.0, r, 255.0), 0.0)  # NaN -> 0
    return np.ascontiguousarray(r.astype(np.uint8).transpose(1, 0, 2))


def host_dequantise(raw, qparams):
    """uint8 [P, 3, k] -> fp32 [3, P, k]: (float)raw · step, then + bias, two rounded fp32 operations."""
    step, bias = host_steps(qparams)
    with np.errstate(all="ignore"):
        t = (raw.astype(F32) * step).astype(F32)
        c = (t + bias).astype(F32)
    return np.ascontiguousarray(c.transpose(1, 0, 2))
