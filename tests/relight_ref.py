"""Exact NumPy restatement of rti_relight (csrc/rti_relight.hip, rti_basis.h, rti_convert.h), written
operation by operation from those files and importing nothing from the package.  Nothing in the kernel is an
approximation, so nothing here is either: the basis row is separately rounded operations in the coefficient type
(the header turns contraction off), the fp32 sum is one rounded product followed by fused multiply-adds in index
order, the fp64 sum is rounded products added left to right, and the four outputs are rti_convert.h's.  NumPy has no
fused multiply-add, so fma32 builds one: the product of two fp32 values is exact in fp64, the fp64 sum with the
addend is rounded to odd with the TwoSum error term, and 53 bits rounded to odd then to 24 is one rounding.
Everything runs under np.errstate(all="ignore").  Also the seeded maps and directions the tests share."""
import functools

import numpy as np

from lrgb_ref import to_int32, to_uint8

F32, F64 = np.float32, np.float64
TERMS = {"ptm": 6, "hsh9": 9, "hsh": 16, "hsh16": 16}

# rti_basis.h's K_l^m, as the header spells them (doubles, cast to the arithmetic type where they are used)
SQRT2 = 1.41421356237309504880
K00 = 0.39894228040143267794
K10 = 0.69098829894267095853
K11 = 0.48860251190291992159
K20 = 0.89206205807638555727
K21 = 0.36418281019735969018
K22 = 0.18209140509867984509
K30 = 1.05550206141118803141
K31 = 0.30469719964297715744
K32 = 0.09635371475468513518
K33 = 0.03933623932844290069


def const_column(basis):
    """the term that is constant over the hemisphere: a5 of the PTM row, H_0^0 of the harmonics"""
    return 5 if basis == "ptm" else 0


# ---- the fp32 fused multiply-add ------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 values, exact: round(a·b + c) with one rounding."""
    a, b, c = (np.asarray(x, F32).astype(F64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b  # exact: 24 + 24 bits
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)  # TwoSum: p + c = s + e exactly, when s is finite
        even = (np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0
        move = np.isfinite(s) & (e != 0) & even  # inexact and even: the odd neighbour lies on e's side
        s = np.where(move, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


# ---- rti_basis.h ----------------------------------------------------------------------------------------------------

def _ptm_eval(lu, lv, T):
    return [lu * lu, lv * lv, lu * lv, lu, lv, np.ones_like(lu)]


def _hsh_eval(lu, lv, k, T):
    zero, one, two, three, five = T(0), T(1), T(2), T(3), T(5)
    r2 = lu * lu + lv * lv
    lw2 = one - r2
    lw = np.where(lw2 > zero, np.sqrt(np.where(lw2 > zero, lw2, zero)), zero)
    t = two * lw - one
    st2 = (one - t) * (one + t)
    st = np.where(st2 > zero, np.sqrt(np.where(st2 > zero, st2, zero)), zero)
    s = np.sqrt(r2)
    lit = s > zero
    safe = np.where(lit, s, one)
    c1 = np.where(lit, lu / safe, one)
    s1 = np.where(lit, lv / safe, zero)
    c2, s2 = c1 * c1 - s1 * s1, two * s1 * c1
    c3, s3 = c1 * c2 - s1 * s2, s1 * c2 + c1 * s2
    r = T(SQRT2)
    out = [np.full_like(lu, T(K00))]
    p11 = st
    out.append(r * T(K11) * s1 * p11)
    out.append(T(K10) * t)
    out.append(r * T(K11) * c1 * p11)
    p20 = (three * t * t - one) * T(0.5)
    p21 = three * t * st
    p22 = three * st2
    out.append(r * T(K22) * s2 * p22)
    out.append(r * T(K21) * s1 * p21)
    out.append(T(K20) * p20)
    out.append(r * T(K21) * c1 * p21)
    out.append(r * T(K22) * c2 * p22)
    if k <= 9:
        return out
    p30 = (five * t * t * t - three * t) * T(0.5)
    p31 = T(1.5) * (five * t * t - one) * st
    p32 = T(15) * t * st2
    p33 = T(15) * st2 * st
    out.append(r * T(K33) * s3 * p33)
    out.append(r * T(K32) * s2 * p32)
    out.append(r * T(K31) * s1 * p31)
    out.append(T(K30) * p30)
    out.append(r * T(K31) * c1 * p31)
    out.append(r * T(K32) * c2 * p32)
    out.append(r * T(K33) * c3 * p33)
    return out


def _basis(lu, lv, basis, T):
    """basis_eval<T> at E directions -> [E, k] of T.  The directions arrive as fp64 and are cast first, as the
    kernel casts luv[...]."""
    lu = np.atleast_1d(np.asarray(lu, F64)).astype(T)
    lv = np.atleast_1d(np.asarray(lv, F64)).astype(T)
    with np.errstate(all="ignore"):
        cols = _ptm_eval(lu, lv, T) if basis == "ptm" else _hsh_eval(lu, lv, TERMS[basis], T)
    out = np.stack(cols, -1)
    assert out.dtype == T and out.shape == (lu.size, TERMS[basis])
    return out


def basis32(lu, lv, basis):
    return _basis(lu, lv, basis, F32)


def basis64(lu, lv, basis):
    return _basis(lu, lv, basis, F64)


# ---- rti_relight ----------------------------------------------------------------------------------------------------

def relight_ref(coef, lu, lv, basis):
    """coef [P, k] fp32 or fp64, E directions -> [E, P] in coef's type: dot_k of rti_relight.hip."""
    c = np.asarray(coef)
    assert c.dtype in (F32, F64) and c.ndim == 2 and c.shape[1] == TERMS[basis]
    B = _basis(lu, lv, basis, c.dtype.type)
    with np.errstate(all="ignore"):
        acc = c[None, :, 0] * B[:, None, 0]
        for k in range(1, c.shape[1]):
            if c.dtype == F32:
                acc = fma32(c[None, :, k], B[:, None, k], acc)
            else:
                acc = acc + c[None, :, k] * B[:, None, k]
    assert acc.dtype == c.dtype
    return acc


def convert(x, dtype_name):
    """rti_convert.h's cvt_out: "float32" / "float64" are one rounding (or exact), "int32" / "uint8" lrgb_ref's."""
    with np.errstate(all="ignore"):
        if dtype_name in ("float32", "float64"):
            return np.asarray(x).astype(dtype_name)
        return {"int32": to_int32, "uint8": to_uint8}[dtype_name](x)


# ---- seeded maps and directions -------------------------------------------------------------------------------------

CONSTANTS = (-3.7, -0.5, 0.0, 0.99, 254.6, 255.0, 300.2)  # tests/test_gpu_perpixel_relight.py::test_relight_int_semantics
EDGES = (2147483648.0, -2147483648.0, 3e9)  # the int32 conversion's edges
# (value, pure): pure pixels hold the value in the constant term and zero elsewhere, the others keep the seeded
# pixel and take the value in one coefficient.  The first is planted at the last pixel and so is all of a
# one-pixel map.
ROWS = ((300.2, True), (np.nan, False), (np.inf, False), (-np.inf, False)) + \
    tuple((v, True) for v in CONSTANTS[:-1] + EDGES)


def special(P, k):
    """The planted pixels of a P-pixel map of k terms -> [(pixel, column, value, pure)].  They alternate between
    the end of the map and its start (P-1, 0, P-2, 1, ...), then the two sides of the first wave seam (255, 256)
    when the map has a third chunk to put them apart from the rest: so one lies in the first 256-pixel chunk and,
    when P % 256 != 0, one in the last P % 256 pixels.  A map shorter than twice the rows plants one pixel in two."""
    basis = {6: "ptm", 9: "hsh9", 16: "hsh"}[k]
    n = min(len(ROWS), max(1, P // 2))
    spots = [P - 1 - i // 2 if i % 2 == 0 else i // 2 for i in range(n)]
    if P > 512:
        spots[-2:] = [255, 256]
    assert len(set(spots)) == n and all(0 <= p < P for p in spots)
    out = []
    for i, (p, (value, pure)) in enumerate(zip(spots, ROWS)):
        out.append((p, const_column(basis) if pure else (2 * i + 1) % k, value, pure))
    return out


@functools.lru_cache(maxsize=None)
def maps(P, k, seed):
    """fp32 [P, k], never written: uniform in [-60, 60] with +140 on the constant term, rounded to fp32 so that
    the fp32 and the fp64 cases share values (the fp64 map is .astype(float64)), with special(P, k) planted."""
    basis = {6: "ptm", 9: "hsh9", 16: "hsh"}[k]
    rng = np.random.default_rng(seed)
    m = rng.uniform(-60.0, 60.0, (P, k))
    m[:, const_column(basis)] += 140.0
    m = m.astype(F32)
    for p, col, value, pure in special(P, k):
        if pure:
            m[p] = 0.0
        m[p, col] = value
    m.setflags(write=False)
    return m


RIM = (F32(0.6), F32(0.8))  # lu² + lv² == 1 in fp32 (tests/test_relight_ref.py checks it)


@functools.lru_cache(maxsize=None)
def _all_dirs(n=320):
    rng = np.random.default_rng(44)
    r, phi = np.sqrt(rng.uniform(0.0, 0.81, n)), rng.uniform(0, 2 * np.pi, n)
    lu, lv = r * np.cos(phi), r * np.sin(phi)  # fp64, not fp32 values: the kernel's cast to fp32 rounds them
    fixed = [(0.0, 0.0), (0.5, 0.0), (-0.75, 0.0), (0.0, 0.25), (0.0, -1.0), (float(RIM[0]), float(RIM[1])),
             (0.8, 0.75)]
    # one seeded direction leads, so that a single direction is not the pole (where most terms vanish)
    lu = np.concatenate([lu[:1], [f[0] for f in fixed], lu[1:]])
    lv = np.concatenate([lv[:1], [f[1] for f in fixed], lv[1:]])
    lu.setflags(write=False)
    lv.setflags(write=False)
    return lu, lv


def dirs(E):
    """E directions as fp64 (lu, lv), each dirs(E) a prefix of the longer ones: a seeded one, the pole, points on
    both axes (one of them on the rim), a point off the axes on the rim with lu² + lv² = 1 in fp32, a point outside
    it (lw2 < 0, so lw = 0), then seeded points inside the disc of radius 0.9."""
    lu, lv = _all_dirs()
    assert 1 <= E <= lu.size
    return lu[:E], lv[:E]
