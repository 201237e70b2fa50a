"""tests/relight_ref.py held to what stands outside it, on the CPU: its fused multiply-add to exact rational
arithmetic, its basis rows to the host build of rti_basis.h, its fp64 PTM sum to the oracle's grid evaluation bit for
bit, every basis and type to the oracle's matrix product within rounding (a wrong term order would pass a bit-exact
self-check), and its planted pixels to the places tests/test_gpu_relight_paths.py counts on."""
from fractions import Fraction

import numpy as np
import pytest

import relight_ref as R
import rti
import rti_oracle as o
from conftest import golden

F32, F64 = np.float32, np.float64
# every pixel count tests/test_gpu_relight_paths.py launches
GPU_SIZES = [1, 3, 4, 7, 8, 9, 256, 257, 259, 260, 515, 1020, 1028, 1029]


def round_to_f32(q):
    """The fp32 value nearest the rational q, ties to even, in integer arithmetic."""
    if q == 0:
        return F32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = q / quantum
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    v = lo * quantum
    if v >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(v))  # 24 bits: exact in a double


def exact_fma(a, b, c):
    return np.array([round_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], F32)


def random_f32(rng, n, lo=-30, hi=30):
    """fp32 values with full random significands and exponents in [lo, hi]"""
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(lo, hi + 1, n)).astype(F32)


def test_round_to_f32_knows_ties_and_the_ends():
    """the checker checked: ties go to even, the subnormal step is 2^-149, the overflow threshold is a tie"""
    one, ulp = Fraction(1), Fraction(2) ** -23
    assert round_to_f32(one + ulp / 2) == F32(1.0) and round_to_f32(one + 3 * ulp / 2) == F32(1.0) + F32(2.0 ** -22)
    assert round_to_f32(one + ulp / 2 + Fraction(2) ** -80) == F32(1.0) + F32(2.0 ** -23)
    assert round_to_f32(Fraction(2) ** -150) == 0 and round_to_f32(Fraction(3, 2) * Fraction(2) ** -149) == F32(2.0 ** -148)
    big = Fraction(float(np.finfo(F32).max))
    assert round_to_f32(big + Fraction(2) ** 102) == np.finfo(F32).max and np.isinf(round_to_f32(big + Fraction(2) ** 103))
    assert round_to_f32(Fraction(-1, 3)) == F32(-1.0 / 3.0)


def test_fma32_is_exact_on_random_triples():
    rng = np.random.default_rng(7)
    a, b, c = (random_f32(rng, 3000) for _ in range(3))
    # and sums that cancel to the rounding error of the product, the case a separate multiply and add loses
    a2, b2 = random_f32(rng, 1000), random_f32(rng, 1000)
    c2 = -(a2 * b2)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    got, want = R.fma32(a, b, c), exact_fma(a, b, c)
    assert got.dtype == F32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    unfused = a * b + c
    assert (unfused != want).sum() > 500  # the triples tell a fused from an unfused sum


def test_fma32_is_exact_next_to_ties():
    """c a random fp32 value, a·b within 2^-46 (relative) of half its last place: the exact sum sits on a tie of
    the fp32 grid, or off it by less than the last place of the fp64 sum, or by a few of them."""
    rng = np.random.default_rng(8)
    n = 3000
    c = random_f32(rng, n, -20, 20)
    half = (np.spacing(np.abs(c)) / F32(2)).astype(F32)
    i, j = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
    j[: n // 2] = -i[: n // 2]  # a·b = half·(1 - i²·2^-46): below what the fp64 sum resolves
    a = (half.astype(F64) * (1.0 + i * 2.0 ** -23)).astype(F32)
    b = (rng.choice([-1.0, 1.0], n) * (1.0 + j * 2.0 ** -23)).astype(F32)
    assert np.array_equal(a.astype(F64), half.astype(F64) * (1.0 + i * 2.0 ** -23))  # all of it exact in fp32
    got, want = R.fma32(a, b, c), exact_fma(a, b, c)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    twice = (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)  # rounded to fp64, then to fp32
    print(f"{int((twice != want).sum())} of {n} sums are rounded wrongly by two roundings")
    assert (twice != want).sum() > 100  # the cases are the ones the round to odd is there for


def test_fma32_passes_on_nan_and_infinities():
    inf, nan = F32(np.inf), F32(np.nan)
    got = R.fma32(F32([inf, inf, 2.0, 0.0, -0.0, -0.0, 3e38]), F32([0.0, 1.0, nan, 5.0, 5.0, 5.0, 3.0]),
                  F32([1.0, -inf, 1.0, -0.0, -0.0, 0.0, -3e38]))
    assert np.isnan(got[:3]).all()
    assert np.array_equal(got[3:].view(np.int32), F32([0.0, -0.0, 0.0, np.inf]).view(np.int32))


@pytest.mark.parametrize("basis", ["ptm", "hsh9", "hsh"])
def test_basis64_is_the_host_build_of_the_header(basis):
    lu, lv = R.dirs(64)
    got, want = R.basis64(lu, lv, basis), rti.basis_eval(lu, lv, basis)
    assert got.shape == want.shape == (64, R.TERMS[basis])
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    b32 = R.basis32(lu, lv, basis)
    assert b32.dtype == F32
    inside = lu * lu + lv * lv <= 0.81  # sqrt(1 - r²) is well conditioned there
    assert np.abs(b32[inside].astype(F64) - want[inside]).max() <= 32 * 2.0 ** -24


def test_dirs_hold_what_they_name():
    lu, lv = R.dirs(64)
    u, v = lu.astype(F32), lv.astype(F32)
    r2 = u * u + v * v
    assert (lu[1], lv[1]) == (0.0, 0.0)
    assert ((lu != 0) & (lv == 0)).any() and ((lu == 0) & (lv != 0)).any()
    assert ((r2 == F32(1.0)) & (u != 0) & (v != 0)).any() and (r2 > F32(1.0)).sum() == 1
    assert ((lu.astype(F32).astype(F64) != lu).sum()) > 50  # the cast to fp32 rounds most of them
    for E in (1, 65, 130, 257):
        a = R.dirs(E)
        assert a[0].shape == a[1].shape == (E,) and np.array_equal(a[0], R.dirs(257)[0][:E])


def test_fp64_ptm_sum_is_the_oracles_grid():
    d = golden("ptm_shared_256x256_N20.npz")
    px = d["grid_px"]
    coef = d["coef"][px[:, 0], px[:, 1]]
    xf = o.grid_axis()
    got = R.relight_ref(coef, np.tile(xf, 100), np.repeat(xf, 100), "ptm")  # [E, P], E = [lv][lu]
    want = o.ptm_eval_grid(coef, xf)
    assert got.dtype == F64 and np.array_equal(got.T.reshape(-1, 100, 100).view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("basis", ["ptm", "hsh9", "hsh"])
def test_agrees_with_the_oracle_within_rounding(basis, T):
    """Against oracle.relight (its own basis code: Legendre recursion and cos / sin of atan2, one matrix product).
    The oracle takes fp32 directions, so the directions are fp32 values; they lie inside r <= 0.9, where
    lw = sqrt(1 - r²) does not amplify a rounding.  Every basis value is at most 1.1 in magnitude and comes from
    fewer than 16 roundings of well-conditioned operations, the chain adds k <= 16 more, and the oracle a few of
    fp64: |ref - oracle| <= 64·eps·Σ_k|c_k| with eps = 2^-24 (fp32) or 2^-53 (fp64).  The oracle's PTM row is the
    reference's fp32 products (lu**2 in fp32), so PTM is held to the fp32 bound in both types; its fp64 sum is held
    bit for bit by test_fp64_ptm_sum_is_the_oracles_grid.  Swapped terms are an error of order Σ|c_k|."""
    k = R.TERMS[basis]
    lu, lv = R.dirs(64)
    lu, lv = lu.astype(F32).astype(F64), lv.astype(F32).astype(F64)
    inside = lu * lu + lv * lv <= 0.81
    lu, lv = lu[inside], lv[inside]
    assert lu.size >= 60
    m = R.maps(1029, k, 5)
    finite = np.isfinite(m).all(-1) & (np.abs(m) < 1e6).all(-1)
    c = m[finite].astype(T)
    got = R.relight_ref(c, lu, lv, basis).astype(F64)
    c16 = np.zeros((c.shape[0], 6 if basis == "ptm" else 16))
    c16[:, :k] = c
    want = o.relight(c16, "ptm" if basis == "ptm" else "hsh", lu, lv)
    eps = 2.0 ** -24 if (T is F32 or basis == "ptm") else 2.0 ** -53
    bound = 64 * eps * np.abs(c).astype(F64).sum(-1)[None, :]
    err = np.abs(got - want)
    print(f"{basis} {T.__name__}: max error / bound {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()
    assert basis == "ptm" or T is F32 or err.max() > 0  # not the same code twice


def test_convert_is_the_four_outputs():
    x = np.array([-3.7, -0.5, 0.0, 0.99, 254.6, 255.0, 300.2, np.nan, 2147483648.0, -2147483648.0, 3e9, -np.inf,
                  2147483647.5, 1.0 + 2.0 ** -30])
    lo = np.iinfo(np.int32).min
    assert R.convert(x, "int32").tolist() == [-3, 0, 0, 0, 254, 255, 300, lo, lo, lo, lo, lo, 2147483647, 1]
    assert R.convert(x, "uint8").tolist() == [0, 0, 0, 0, 254, 255, 255, 0, 0, 0, 0, 0, 255, 1]
    assert R.convert(x, "float32").dtype == F32 and R.convert(x, "float32")[-1] == F32(1.0)
    assert R.convert(x.astype(F32), "float64").dtype == F64
    assert np.array_equal(R.convert(x.astype(F32), "int32"), R.convert(x.astype(F32).astype(F64), "int32"))


@pytest.mark.parametrize("k", [6, 9, 16])
@pytest.mark.parametrize("P", GPU_SIZES)
def test_special_pixels_lie_where_they_say(P, k):
    sp = R.special(P, k)
    px = [s[0] for s in sp]
    assert len(set(px)) == len(px) and all(0 <= p < P for p in px)
    assert any(p < 256 for p in px)
    if P % 256:
        assert any(p >= P - P % 256 for p in px)
    if P >= 26:
        assert len(sp) == len(R.ROWS)
    m = R.maps(P, k, 1)
    assert m.dtype == F32 and m.shape == (P, k) and not m.flags.writeable
    const = 5 if k == 6 else 0
    for p, col, value, pure in sp:
        assert np.array_equal(m[p, col], F32(value), equal_nan=True)
        if pure:
            assert col == const and not np.delete(m[p], col).any()
        else:
            assert np.isfinite(np.delete(m[p], col)).all() and np.delete(m[p], col).any()
    rest = np.delete(m, px, axis=0)
    assert np.isfinite(rest).all() and (np.abs(rest[rest != 0]) > 1e-30).all()  # normal range
    assert (np.abs(np.delete(rest, const, axis=1)) <= 60).all() and (np.abs(rest[:, const] - 140) <= 60).all()
