"""fp64 restatement of rti_ptm_normals / rti_relight_enhanced (include/rti.h), written straight
from their formulas in vectorised NumPy; it imports nothing from the package.  NumPy rounds every product, sum,
quotient and square root and fuses nothing, which is the arithmetic the header prescribes, and every expression
below keeps the header's left-to-right order.  Also the seeded coefficient families the tests share."""
import numpy as np

INT32_MIN = -2 ** 31
D_TOL = 1e-6


def ptm_value(a, u, v):
    """L(u, v) of coefficients a [P, 6] (fp64), the six terms summed left to right."""
    with np.errstate(all="ignore"):
        acc = a[:, 0] * (u * u)
        acc = acc + a[:, 1] * (v * v)
        acc = acc + a[:, 2] * (u * v)
        acc = acc + a[:, 3] * u
        acc = acc + a[:, 4] * v
        return acc + a[:, 5]


def peak_ref(coef):
    """coef [P, 6] (fp32 or fp64) -> dict(a fp64, finite, has_max, u0, v0, r2, D, S)."""
    a = np.asarray(coef).astype(np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        finite = np.isfinite(a).all(1)
        a22 = a[:, 2] * a[:, 2]
        D = 4.0 * a[:, 0] * a[:, 1] - a22
        S = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + 0.5 * a22
        has_max = finite & (D > D_TOL * S) & (a[:, 0] < 0.0)
        u0 = (a[:, 2] * a[:, 4] - 2.0 * a[:, 1] * a[:, 3]) / D
        v0 = (a[:, 2] * a[:, 3] - 2.0 * a[:, 0] * a[:, 4]) / D
        r2 = u0 * u0 + v0 * v0
    return dict(a=a, finite=finite, has_max=has_max, u0=u0, v0=v0, r2=r2, D=D, S=S)


def normals_ref(coef):
    """coef [P, 6] -> dict(n fp64 [P, 3], kind uint8 [P], peak fp64 [P]) plus peak_ref's entries."""
    k = peak_ref(coef)
    a, has_max = k["a"], k["has_max"]
    with np.errstate(all="ignore"):
        inside = has_max & (k["r2"] <= 1.0)
        outside = has_max & ~inside
        g2 = np.where(a[:, 5] > 0.0, a[:, 5], 0.0)
        gg = a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4] + g2 * g2
        n = np.empty((a.shape[0], 3))
        # kind 0: (u0, v0, sqrt(1 - r²))
        s0 = np.sqrt(1.0 - k["r2"])
        # kind 1: (u0, v0, 0) / sqrt(r²)
        s1 = np.sqrt(k["r2"])
        # kind 2: g / ‖g‖, (0, 0, 1) when ‖g‖ = 0
        s2 = np.sqrt(gg)
        flat = ~has_max & (s2 == 0.0)
        n[:, 0] = np.where(inside, k["u0"], np.where(outside, k["u0"] / s1, np.where(flat, 0.0, a[:, 3] / s2)))
        n[:, 1] = np.where(inside, k["v0"], np.where(outside, k["v0"] / s1, np.where(flat, 0.0, a[:, 4] / s2)))
        n[:, 2] = np.where(inside, s0, np.where(outside, 0.0, np.where(flat, 1.0, g2 / s2)))
        n[~k["finite"]] = np.nan
        kind = np.where(~k["finite"], 4, np.where(inside, 0, np.where(outside, 1, 2))).astype(np.uint8)
        peak = np.where(k["finite"], ptm_value(a, n[:, 0], n[:, 1]), np.nan)
    return dict(k, n=n, kind=kind, peak=peak)


def diffuse_gain_coef(coef, g):
    """The coefficients L' of diffuse gain g, fp64 [P, 6]: pixels with a maximum transformed about their
    unprojected stationary point, the others unchanged."""
    k = peak_ref(coef)
    a, u0, v0 = k["a"], k["u0"], k["v0"]
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


def powi(x, e):
    """x^e by repeated squaring, the header's order: r = 1, b = x; per bit of e from the lowest."""
    r, b = np.ones_like(x), x.copy()
    while True:
        if e & 1:
            r = r * b
        e >>= 1
        if not e:
            return r
        b = b * b


def half_vector(lu, lv):
    lu, lv = np.float64(lu), np.float64(lv)
    lw2 = 1.0 - lu * lu - lv * lv
    hz = (np.sqrt(lw2) if lw2 > 0.0 else 0.0) + 1.0
    hn = np.sqrt(lu * lu + lv * lv + hz * hz)
    return lu / hn, lv / hn, hz / hn


def relight_enhanced_ref(coef, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1):
    """coef [P, 6] -> the fp64 image [P] of mode "diffuse_gain" or "specular" (NaN for non-finite pixels)."""
    lu, lv = np.float64(lu), np.float64(lv)
    with np.errstate(all="ignore"):
        if mode == "diffuse_gain":
            r = peak_ref(coef)
            v = ptm_value(diffuse_gain_coef(coef, np.float64(gain)), lu, lv)
        else:
            assert mode == "specular" and 1 <= exp <= 255
            r = normals_ref(coef)
            hx, hy, hz = half_vector(lu, lv)
            c = r["n"][:, 0] * hx + r["n"][:, 1] * hy + r["n"][:, 2] * hz
            v = np.float64(kd) * ptm_value(r["a"], lu, lv) + np.float64(ks) * powi(np.where(c > 0.0, c, 0.0), int(exp))
    return np.where(r["finite"], v, np.nan)


def to_int32(x):
    """rti_convert.h's int32: C truncation toward zero, NaN / out of range -> INT32_MIN."""
    x = np.asarray(x, np.float64)
    ok = np.abs(x) < 2147483648.0  # False for NaN
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), INT32_MIN).astype(np.int64).astype(np.int32)


def to_uint8(x):
    return np.clip(to_int32(x), 0, 255).astype(np.uint8)


# ---- seeded coefficient families ------------------------------------------------------------------------------

def peaked_coef(rng, P, r_lo, r_hi, sign=-1.0):
    """Biquadratics with Hessian sign·R·diag(s1, s2)·Rᵀ, s in [50, 200], stationary at a known (u0, v0) with
    radius in [r_lo, r_hi] and value h in [20, 250] there -> (coef fp64 [P, 6], u0, v0, h).  sign = -1: maxima;
    +1: minima; "saddle": diag(-s1, +s2)."""
    s1, s2 = rng.uniform(50, 200, P), rng.uniform(50, 200, P)
    if sign == "saddle":
        e1, e2 = -s1, s2
    else:
        e1, e2 = sign * s1, sign * s2
    t = rng.uniform(0, np.pi, P)
    c, s = np.cos(t), np.sin(t)
    hxx = c * c * e1 + s * s * e2
    hyy = s * s * e1 + c * c * e2
    hxy = c * s * (e1 - e2)
    a0, a1, a2 = 0.5 * hxx, 0.5 * hyy, hxy
    r, phi = rng.uniform(r_lo, r_hi, P), rng.uniform(0, 2 * np.pi, P)
    u0, v0 = r * np.cos(phi), r * np.sin(phi)
    a3 = -(2 * a0 * u0 + a2 * v0)
    a4 = -(a2 * u0 + 2 * a1 * v0)
    h = rng.uniform(20, 250, P)
    a5 = h - (a0 * u0 * u0 + a1 * v0 * v0 + a2 * u0 * v0 + a3 * u0 + a4 * v0)
    return np.stack([a0, a1, a2, a3, a4, a5], -1), u0, v0, h


def mixed_coef(P, seed, dtype=np.float32):
    """P rows mixing the classes of rti_ptm_normals, each far from every branch threshold: interior maxima
    (r <= 0.9), maxima outside the disc (r in [1.1, 2]), saddles (D/S <= -0.94) and minima (a0 > 0), all-zero
    rows (one, plus one per 4000: they relight to exact or near integers, which the integer-output checks must
    leave out) and NaN / ±inf rows, in a seeded random order."""
    rng = np.random.default_rng(seed)
    cls = rng.choice(6, P, p=[0.4, 0.25, 0.17, 0.13, 0.0, 0.05])
    cls[rng.choice(P, P // 4000, replace=False)] = 4
    if P >= 6:
        cls[rng.choice(P, 6, replace=False)] = np.arange(6)  # every class is present
    out = np.zeros((P, 6))
    for c, args in ((0, (0.0, 0.9, -1.0)), (1, (1.1, 2.0, -1.0)), (2, (0.0, 2.0, "saddle")), (3, (0.0, 2.0, 1.0))):
        m = cls == c
        out[m] = peaked_coef(rng, int(m.sum()), *args)[0]
    bad = np.flatnonzero(cls == 5)
    out[bad] = peaked_coef(rng, bad.size, 0.0, 0.9)[0]
    out[bad, rng.integers(0, 6, bad.size)] = rng.choice([np.nan, np.inf, -np.inf], bad.size)
    return out.astype(dtype)
