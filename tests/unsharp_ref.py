"""fp64 restatement of rti_gauss_taps / rti_map_unsharp / rti_shade_normals (include/rti.h), written
straight from their formulas in vectorised NumPy; it imports nothing from the package.  NumPy has no fma: every
product here is rounded before its sum, which is what the map tests' second tolerance term covers.  Also the seeded
inputs the tests share."""
import numpy as np

from normals_ref import half_vector, mixed_coef, normals_ref, powi

MAX_RADIUS = 32


def gauss_radius(sigma):
    if not np.isfinite(sigma) or sigma <= 0:
        return -1
    return max(1, int(np.ceil(3.0 * sigma)))


def gauss_taps(sigma, radius=None):
    """taps[0..R]: e_d = exp(−d²/(2σ²)), Z = e_0 + 2·Σ_{d>=1} e_d (d ascending), e_d/Z."""
    R = gauss_radius(sigma) if radius is None else radius
    sigma = np.float64(sigma)
    e = np.exp(-(np.arange(R + 1, dtype=np.float64) ** 2) / (2.0 * sigma * sigma))
    tail = np.float64(0.0)
    for d in range(1, R + 1):
        tail = tail + e[d]
    return e / (e[0] + 2.0 * tail)


def _pass(a, w, axis):
    """Σ_{d=−R..R ascending} w|d|·a[.. + d ..] along `axis`, zeros outside the array."""
    R = len(w) - 1
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (R, R)
    p = np.pad(a, pad)
    acc = np.zeros_like(a)
    for d in range(-R, R + 1):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(R + d, R + d + n)
        acc = acc + w[abs(d)] * p[tuple(sl)]
    return acc


def unsharp_ref(src, sigma, amount, radius=None, renorm=False):
    """src [H, W, C] fp32 (pixel-major) -> (out fp64 [H, W, C] unrounded, valid bool [H, W]); invalid pixels carry
    their source values (the kernel copies their bits)."""
    src = np.asarray(src)
    assert src.ndim == 3
    v = src.astype(np.float64)
    m = np.isfinite(v).all(-1)
    w = gauss_taps(sigma, radius)
    vz = np.where(m[..., None], v, 0.0)
    with np.errstate(all="ignore"):
        num = _pass(_pass(vz, w, 1), w, 0)
        den = _pass(_pass(m.astype(np.float64), w, 1), w, 0)
        blur = num / den[..., None]
        o = vz + np.float64(amount) * (vz - blur)
        if renorm:
            assert src.shape[-1] == 3
            nrm = np.sqrt(o[..., 0] * o[..., 0] + o[..., 1] * o[..., 1] + o[..., 2] * o[..., 2])
            unit = ~((nrm > 0.0) & np.isfinite(nrm))
            o = np.where(unit[..., None], np.array([0.0, 0.0, 1.0]), o / nrm[..., None])
    return np.where(m[..., None], o, v), m


def map_tolerance(ref, valid, src, amount):
    """|got − ref| <= 2^-23·|ref| + 1e-10·(1 + |amount|)·M, M = max|src| over the valid pixels."""
    M = np.abs(np.asarray(src, np.float64)[valid]).max() if valid.any() else 0.0
    return 2.0 ** -23 * np.abs(ref) + 1e-10 * (1.0 + abs(amount)) * M


def shade_ref(n, lu, lv, albedo=None, kd=1.0, ks=0.0, exp=1):
    """n [P, 3] fp32, albedo None or [P] fp32 -> fp64 [P]."""
    n = np.asarray(n).astype(np.float64).reshape(-1, 3)
    a = np.ones(n.shape[0]) if albedo is None else np.asarray(albedo).astype(np.float64).ravel()
    lu, lv = np.float64(lu), np.float64(lv)
    lw2 = 1.0 - lu * lu - lv * lv
    lw = np.sqrt(lw2) if lw2 > 0.0 else np.float64(0.0)
    hx, hy, hz = half_vector(lu, lv)
    with np.errstate(all="ignore"):
        d = n[:, 0] * lu + n[:, 1] * lv + n[:, 2] * lw
        h = n[:, 0] * hx + n[:, 1] * hy + n[:, 2] * hz
        v = np.float64(kd) * a * np.where(d > 0.0, d, 0.0) + np.float64(ks) * powi(np.where(h > 0.0, h, 0.0), int(exp))
    return np.where(np.isnan(n).any(1) | np.isnan(a), np.nan, v)


# ---- seeded inputs ----------------------------------------------------------------------------------------------

SHADE_SIZES = [1, 3, 4, 255, 256, 260, 1279]
SHADE_DIRS = [(0.0, 0.0), (0.3, -0.45), (0.8, 0.75)]  # the last has lu² + lv² > 1
SHADE_PARAMS = [(1.0, 0.0, 1), (0.4, 150.0, 1), (0.4, 150.0, 75), (0.4, 150.0, 255)]  # test_gpu_normals.SPECULAR
NEAR_INTEGER = 1e-6


def shade_inputs(P):
    """(normals fp32 [P, 3], albedo fp32 [P]): the normals of every class of PTM pixel (NaN rows included) and
    albedos in [20, 250] with a NaN every 97 pixels."""
    n = normals_ref(mixed_coef(P, 2000 + P))["n"].astype(np.float32)
    a = np.random.default_rng(3000 + P).uniform(20.0, 250.0, P).astype(np.float32)
    a[5::97] = np.nan
    n.setflags(write=False)
    a.setflags(write=False)
    return n, a


def near_integer(ref):
    """Pixels whose fp64 reference lies within NEAR_INTEGER of a boundary of the integer conversions: truncation
    toward zero maps all of (−1, 1) to 0, so its boundaries are the non-zero integers (a value just above 0, a faint
    highlight on a pixel facing away from the light, is no such case)."""
    with np.errstate(invalid="ignore"):
        k = np.rint(ref)
        return (np.abs(ref - k) < NEAR_INTEGER) & (k != 0.0)


def map_input(H, W, C, seed, bad=True):
    """A [H, W, C] fp32 map of magnitude ~100 with NaN and inf at a corner, on an edge, in an interior 3×3 block,
    along a whole row and in one channel only of a pixel (where the map is large enough to have them)."""
    rng = np.random.default_rng(seed)
    a = (100.0 * rng.standard_normal((H, W, C))).astype(np.float32)
    if bad:
        a[0, 0, :] = np.nan  # a corner
        if H >= 5 and W >= 5:
            a[H // 2, W - 1, :] = np.inf  # an edge
            a[H // 2 - 1:H // 2 + 2, W // 3:W // 3 + 3, :] = np.nan  # an interior block
            a[1, 2, C - 1] = -np.inf  # one channel only
        if H >= 12:
            a[H - 4, :, :] = np.nan  # a whole row
    return a
