"""NumPy restatement of rti_relight_hsh_specular / rti_relight_hsh8_specular (include/rti.h), line by
line from the header and importing nothing from the package: V is relight_ref's exact fp32 chain, everything after it
is fp64 with every product and sum rounded and nothing fused, under np.errstate(all="ignore").  Also the seeded inputs
the tests share."""
import functools

import numpy as np

from hsh8_ref import finite_hsh, host_dequantise, host_qparams, host_quantise, mixed_hsh
from normals_ref import half_vector, powi
from relight_ref import convert, relight_ref
from unsharp_ref import near_integer

F32, F64 = np.float32, np.float64

SIZES = [1, 63, 64, 65, 255, 256, 257, 260, 1279]
KS = [9, 16]
DIRS = [(0.0, 0.0), (0.3, -0.45), (0.8, 0.75)]  # the last has lu² + lv² > 1
# (kd, ks, exp); the last has a non-integer ks on purpose: with kd = 0 and ks = 150 the flat normals render exactly
# 150 at (0, 0), an integer boundary
PARAMS = [(1.0, 0.0, 1), (0.4, 150.0, 1), (0.4, 150.0, 75), (0.4, 150.0, 255), (0.0, 150.25, 75)]
NEAR_INTEGER_CAP = 0.01  # the share of near-integer elements a case may leave out (tests/test_gpu_unsharp.py's)


def specular_ref(coef, n, lu, lv, k, kd, ks, exp):
    """coef fp32 [C, P, k], n fp32 [P, 3], E directions -> fp64 [E, P, C] before the conversion."""
    coef, n = np.asarray(coef), np.asarray(n)
    assert coef.dtype == F32 and coef.ndim == 3 and coef.shape[2] == k and n.dtype == F32 and n.shape == (coef.shape[1], 3)
    lu, lv = np.atleast_1d(np.asarray(lu, F64)), np.atleast_1d(np.asarray(lv, F64))
    # V_c: rti_relight's F32 value, [C, E, P]
    V = np.stack([relight_ref(coef[c], lu, lv, f"hsh{k}") for c in range(coef.shape[0])])
    assert V.dtype == F32
    nx, ny, nz = (n[:, i].astype(F64) for i in range(3))
    out = np.empty((lu.size, coef.shape[1], coef.shape[0]))
    with np.errstate(all="ignore"):
        for e in range(lu.size):
            hx, hy, hz = half_vector(lu[e], lv[e])
            h = nx * hx + ny * hy + nz * hz
            S = F64(ks) * powi(np.where(h > 0.0, h, 0.0), int(exp))
            for c in range(coef.shape[0]):
                out[e, :, c] = F64(kd) * V[c, e].astype(F64) + S
    out[:, np.isnan(n).any(1), :] = np.nan
    return out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def normals(P):
    """fp32 [P, 3], never written: seeded random unit vectors with n_z >= 0, (0, 0, 1) at pixels 3::128, a NaN
    y-component at 7::97."""
    v = np.random.default_rng(5000 + P).standard_normal((P, 3))
    v[:, 2] = np.abs(v[:, 2])
    v /= np.sqrt((v * v).sum(1, keepdims=True))
    n = v.astype(F32)
    n[3::128] = (0.0, 0.0, 1.0)
    n[7::97, 1] = np.nan
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def maps(P, k, source="fp32"):
    """The coefficients of a case, never written: fp32 [3, P, k] of finite_hsh(P, k, 4000 + P) ("fp32"), those
    quantised on the host (raw uint8 [P, 3, k], qparams [2k], dequantised fp32 [3, P, k]) ("bytes"), or mixed_hsh's
    with NaN and ±inf ("mixed")."""
    if source == "mixed":
        m = mixed_hsh(P, k, 4000 + P)
        m.setflags(write=False)
        return m
    m = finite_hsh(P, k, 4000 + P)
    m.setflags(write=False)
    if source == "fp32":
        return m
    qp = host_qparams(m)
    raw = host_quantise(m, qp)
    deq = host_dequantise(raw, qp)
    for a in (qp, raw, deq):
        a.setflags(write=False)
    return raw, qp, deq


@functools.lru_cache(maxsize=None)
def reference(P, k, source, params):
    """specular_ref of a case at the three DIRS in one go, fp64 [3, P, C], never written.  source: "fp32" (C = 3),
    "grey" (channel 0 of the fp32 maps, C = 1), "bytes" (the dequantised maps) or "mixed"."""
    kd, ks, exp = params
    c = maps(P, k, "bytes")[2] if source == "bytes" else maps(P, k, "fp32")[:1] if source == "grey" else maps(P, k, source)
    lu, lv = zip(*DIRS)
    ref = specular_ref(c, normals(P), lu, lv, k, kd, ks, exp)
    ref.setflags(write=False)
    return ref


def excluded(ref):
    """near_integer's mask of a reference, and its share of the elements."""
    m = near_integer(ref)
    return m, float(m.mean())


__all__ = ["SIZES", "KS", "DIRS", "PARAMS", "NEAR_INTEGER_CAP", "specular_ref", "normals", "maps", "reference",
           "excluded", "convert"]
