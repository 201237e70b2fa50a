"""tests/fit_domain_ref.py alone satisfies the conditions the GPU tests hold the kernels to: two fp32 emulations of the
sum in different orders stay inside the derived bound, three seeded mutants of the reference break it, the exact
VALU chain equals plain fp32 where every partial sum is representable, and the non-finite classes land on exactly the
poisoned pixels.  CPU only."""
import functools

import numpy as np
import pytest

import fit_domain_ref as fr
import rti_oracle as o

F32, F64 = np.float32, np.float64
TERMS = {"ptm": 6, "hsh9": 9, "hsh": 16}
SHAPES = [(b, N) for b in ("ptm", "hsh9", "hsh") for N in (17, 23, 37, 100, 260)]
P = 260


def weights(basis, N):
    """the fp32-rounded pseudo-inverse [k, N] of the oracle's synthetic light set"""
    lu, lv = o.synth_dirs(N, 11)
    k = TERMS[basis]
    A = o.design("ptm" if basis == "ptm" else "hsh", lu, lv)[:, :k]
    return np.linalg.pinv(A).astype(F32)


@functools.lru_cache(maxsize=None)
def case(basis, N):
    w = weights(basis, N)
    st = dict(fr.stacks(np.random.default_rng(1000 * fr_seed(basis) + N), 2, N, P))
    return w, st


def fr_seed(basis):
    return {"ptm": 1, "hsh9": 2, "hsh": 3}[basis]


def unfused4(w32, I):
    """fp32, no fused operations: rounded products, partial sums of 4 lights, each added to a running total"""
    w = np.asarray(w32, F32)
    x = np.asarray(I).astype(F32)
    C, N, _ = x.shape
    total = np.zeros((C, x.shape[2], w.shape[0]), F32)
    for n0 in range(0, N, 4):
        part = None
        for n in range(n0, min(n0 + 4, N)):
            prod = (w[None, None, :, n] * x[:, n, :, None]).astype(F32)
            part = prod if part is None else (part + prod).astype(F32)
        total = (total + part).astype(F32)
    return total


@pytest.mark.parametrize("basis,N", SHAPES)
def test_two_emulated_orders_stay_inside_the_bound(basis, N):
    w, st = case(basis, N)
    for name in ("signed", "wide", "i32"):
        ref, bnd = fr.reference(w, st[name]), fr.bound(w, st[name])
        assert np.isfinite(ref).all() and (bnd > 0).all()
        for order, got in (("fma chain", fr.valu_exact(w, st[name])), ("unfused by 4", unfused4(w, st[name]))):
            assert got.dtype == F32
            ratio, at = fr.worst_ratio(got, ref, bnd)
            print(f"{basis} N={N} {name} {order}: worst err/bound {ratio:.3f} at {at}")
            assert ratio < 1, (name, order, ratio, at)


@pytest.mark.parametrize("basis,N", SHAPES)
def test_mutants_of_the_reference_fail_the_bound(basis, N):
    w, st = case(basis, N)
    I = st["signed"]
    ref, bnd = fr.reference(w, I), fr.bound(w, I)

    def outside(got):
        return np.abs(got - ref) > bnd

    # the last light dropped
    dropped = outside(fr.reference(w[:, :-1], I[:, :-1]))
    print(f"{basis} N={N} last light dropped: {dropped.mean():.3f} of the elements outside")
    assert dropped.mean() > 0.5
    # two pixels swapped
    swapped = ref.copy()
    swapped[:, [3, 200]] = ref[:, [200, 3]]
    out = outside(swapped)
    assert out[:, 3].any() and out[:, 200].any() and out.sum() == out[:, [3, 200]].sum()
    # the smallest-magnitude coefficient row scaled by 1 + 1e-3
    row = int(np.argmin(np.median(np.abs(ref), axis=(0, 1))))
    scaled = ref.copy()
    scaled[..., row] *= 1.0 + 1e-3
    out = outside(scaled)
    med = float(np.median(np.abs(scaled - ref)[..., row] / bnd[..., row]))
    print(f"{basis} N={N} row {row} scaled by 1 + 1e-3: median err/bound {med:.1f}, {out[..., row].mean():.3f} outside")
    assert out[..., row].mean() > 0.5
    assert not np.delete(out, row, axis=-1).any()


def test_valu_exact_equals_plain_fp32_where_sums_are_exact():
    """Weights that are small multiples of 1/8 and 8-bit intensities: every product and partial sum is a multiple of
    1/8 below 2^24 / 8, so fp32 holds each of them exactly, in any order."""
    rng = np.random.default_rng(5)
    for k, N in ((6, 17), (9, 38), (16, 100)):
        w = (rng.integers(-32, 33, (k, N)) / 8.0).astype(F32)
        u8 = dict(fr.stacks(rng, 2, N, 67))["u8"]
        assert u8.dtype == np.uint8 and (u8[:, :, [1, 65]] == 0).all() and (u8[:, :, [2, 66]] == 255).all()
        exact = fr.valu_exact(w, u8)
        plain = np.swapaxes(u8.astype(F32), 1, 2) @ w.T
        assert plain.dtype == F32
        assert np.array_equal(exact.view(np.int32), plain.view(np.int32))
        assert np.array_equal(exact.astype(F64), fr.reference(w, u8))
        assert fr.worst_ratio(exact, fr.reference(w, u8), fr.bound(w, u8))[0] == 0


def test_fma32_chain_rounds_once_per_step():
    """A sum in which fusing matters: 1 + 2^-24·(1 − 2^-24) · (1 + 2^-23).  The product is 2^-24·(1 + 2^-24 − 2^-47):
    rounded on its own it is 2^-24, and 1 + 2^-24 ties to even, 1; fused, the sum is above the tie and rounds to the
    next fp32 after 1."""
    w = np.array([[1.0, 2.0 ** -24 * (1.0 - 2.0 ** -24)]], F32)
    assert float(w[0, 1]) == 2.0 ** -24 * (1.0 - 2.0 ** -24)
    I = np.array([[[1.0], [1.0 + 2.0 ** -23]]], F32)
    assert fr.valu_exact(w, I)[0, 0, 0] == F32(1.0 + 2.0 ** -23)
    assert unfused4(w, I)[0, 0, 0] == F32(1.0)


@pytest.mark.parametrize("basis,N,Pp", [("ptm", 17, 1028), ("hsh9", 23, 259), ("hsh", 38, 1028), ("ptm", 20, 68)])
def test_expected_class_marks_exactly_the_poisoned_pixels(basis, N, Pp):
    w = weights(basis, N)
    assert (w != 0).all()
    I = dict(fr.stacks(np.random.default_rng(N), 2, N, Pp))["signed"]
    clean = fr.expected_class(w, I)
    assert (clean == fr.FINITE).all()
    planted = fr.poison(I)
    assert len({(c, n, p) for c, n, p, _ in planted}) == 8 and all(not np.isfinite(I[c, n, p]) for c, n, p, _ in planted)
    assert np.isfinite(I).sum() == I.size - 8
    cls = fr.expected_class(w, I)
    hit = np.zeros(cls.shape[:2], bool)
    for c, n, p, v in planted:
        hit[c, p] = True
    # every coefficient of a poisoned pixel (no weight is zero), and no other
    assert np.array_equal((cls != fr.FINITE).all(-1), hit) and np.array_equal((cls != fr.FINITE).any(-1), hit)
    for c, n, p, v in planted:
        if np.isnan(v):
            assert (cls[c, p] == fr.NAN).all()
    # one infinity: its sign times the weight's
    c, n, p, v = planted[1]
    assert np.array_equal(cls[c, p], np.where(w[:, n] > 0, fr.POS_INF, fr.NEG_INF))
    c, n, p, v = planted[2]
    assert np.array_equal(cls[c, p], np.where(w[:, n] > 0, fr.NEG_INF, fr.POS_INF))
    # two infinities in one pixel: Inf where their weights agree in sign, NaN where they do not
    c, n, p, v = planted[4]
    agree = np.sign(w[:, n]) == np.sign(w[:, n + 1])
    assert np.array_equal(cls[c, p], np.where(agree, np.where(w[:, n] > 0, fr.POS_INF, fr.NEG_INF), fr.NAN))
    # the finite coefficients of a poisoned stack are still judged, the others are not
    ref, bnd = fr.reference(w, I), fr.bound(w, I)
    got = ref.astype(F32)
    ratio, at = fr.worst_ratio(got, ref, bnd)
    assert ratio < 1 and not hit[at[0], at[1]]
