"""NumPy restatement of rti_relight_hsh_gain / rti_relight_hsh8_gain (include/rti.h), line by line
from the header and importing nothing from the package: V is relight_ref's exact fp32 chain at the light, A the same
chain on relight_ref.basis32 at each pixel's own (n_x, n_y), everything after them is fp64 with every product and sum
rounded and nothing fused, under np.errstate(all="ignore").  Also the seeded inputs the tests share."""
import functools

import numpy as np

import hsh_specular_ref as S
from hsh_specular_ref import DIRS, KS, NEAR_INTEGER_CAP, SIZES, excluded, maps
from relight_ref import basis32, convert, fma32, relight_ref

F32, F64 = np.float32, np.float64

GAINS = [1.0, 0.0, 2.5, 10.0, -1.0]
RIM = {11: (0.6, 0.8, 0.0), 12: (0.0, -1.0, 0.0)}  # rim normals planted when P > 20


def anchor_ref(coef, n, k):
    """coef fp32 [C, P, k], n fp32 [P, 3] -> fp32 [C, P]: rti_relight's F32 value of every pixel at its own
    (n_x, n_y)."""
    B = basis32(n[:, 0], n[:, 1], f"hsh{k}")  # [P, k]: per-pixel directions
    assert B.dtype == F32 and B.shape == (n.shape[0], k)
    with np.errstate(all="ignore"):
        acc = coef[:, :, 0] * B[None, :, 0]
        for j in range(1, k):
            acc = fma32(coef[:, :, j], B[None, :, j], acc)
    assert acc.dtype == F32
    return acc


def gain_ref(coef, n, lu, lv, k, gain):
    """coef fp32 [C, P, k], n fp32 [P, 3], E directions -> fp64 [E, P, C] before the conversion."""
    coef, n = np.asarray(coef), np.asarray(n)
    assert coef.dtype == F32 and coef.ndim == 3 and coef.shape[2] == k and n.dtype == F32 and n.shape == (coef.shape[1], 3)
    lu, lv = np.atleast_1d(np.asarray(lu, F64)), np.atleast_1d(np.asarray(lv, F64))
    # V_c: rti_relight's F32 value, [C, E, P]
    V = np.stack([relight_ref(coef[c], lu, lv, f"hsh{k}") for c in range(coef.shape[0])])
    A = anchor_ref(coef, n, k)  # [C, P]
    assert V.dtype == F32
    gm1 = F64(gain) - F64(1.0)
    out = np.empty((lu.size, coef.shape[1], coef.shape[0]))
    with np.errstate(all="ignore"):
        for e in range(lu.size):
            for c in range(coef.shape[0]):
                d = V[c, e].astype(F64) - A[c].astype(F64)
                out[e, :, c] = V[c, e].astype(F64) + gm1 * d
    out[:, np.isnan(n).any(1), :] = np.nan
    return out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def normals(P):
    """hsh_specular_ref.normals(P) (the pole at 3::128, a NaN y-component at 7::97), never written, with the two rim
    normals of RIM at pixels 11 and 12 when P > 20."""
    n = S.normals(P).copy()
    if P > 20:
        for p, v in RIM.items():
            n[p] = v
    n.setflags(write=False)
    return n


@functools.lru_cache(maxsize=None)
def reference(P, k, source, gain):
    """gain_ref of a case at the three DIRS in one go, fp64 [3, P, C], never written.  source: "fp32" (C = 3), "grey"
    (channel 0 of the fp32 maps, C = 1), "bytes" (the dequantised maps) or "mixed"."""
    c = maps(P, k, "bytes")[2] if source == "bytes" else maps(P, k, "fp32")[:1] if source == "grey" else maps(P, k, source)
    lu, lv = zip(*DIRS)
    ref = gain_ref(c, normals(P), lu, lv, k, gain)
    ref.setflags(write=False)
    return ref


__all__ = ["SIZES", "KS", "DIRS", "GAINS", "RIM", "NEAR_INTEGER_CAP", "anchor_ref", "gain_ref", "normals", "maps",
           "reference", "excluded", "convert"]
