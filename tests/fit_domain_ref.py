"""Reference, inputs and error bound of the shared-direction fits (rti_fit_shared, rti_fit_shared_pm) over their whole
input domain: signed, fractional, wide-range, full-range int32 and non-finite stacks.  NumPy only; imports nothing from
the package.

The fits compute coef[c][p][k] = Σ_n w[k][n] · float32(I[c][n][p]) in fp32.  Stacks here are light-major [C, N, P];
every result is [C, P, k].

Bound.  An N-term fp32 sum of products, in any order, fused or not, with the int32 -> fp32 conversion as one more
rounding, has forward error at most γ_{N+1} · Σ_n |w_kn| · |x_np|, γ_m = m·u / (1 − m·u), u = 2^-24 (Higham, Accuracy
and Stability of Numerical Algorithms, §3.1: each term passes through at most N + 1 roundings).  The matrix-core
kernels get γ_{2(N+1)}: the hardware's 4-term dot product is not documented to round once per operation, and two
roundings per term is the most a fused multiply-add pipeline can spend.  The bound is derived, not measured.

Everything runs under np.errstate(all="ignore")."""
import numpy as np

from relight_ref import fma32

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # fp32 unit roundoff

FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3  # classes of a coefficient


def gamma(m):
    return m * U / (1.0 - m * U)


# ---- seeded stacks --------------------------------------------------------------------------------------------------

def stacks(rng, C, N, P):
    """Yields (name, stack [C, N, P]): `signed` fp32 uniform(−1000, 1000); `wide` fp32 ±uniform(1, 2)·2^e with e
    uniform in −40..40 per element (no product or partial sum is subnormal or overflows); `i32` int32 over the full
    range with INT32_MIN, INT32_MAX and ±(2^24 + 1) planted; `u8` uint8 with an all-0 and an all-255 pixel."""
    shape = (C, N, P)
    yield "signed", rng.uniform(-1000.0, 1000.0, shape).astype(F32)
    m = rng.uniform(1.0, 2.0, shape).astype(F32)
    sign = np.where(rng.integers(0, 2, shape) == 1, F32(-1), F32(1))
    yield "wide", np.ldexp(sign * m, rng.integers(-40, 41, shape)).astype(F32)
    hi = min(P - 1, 258)  # a pixel of the ragged tail of the smallest GPU shape (P = 259)
    i32 = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    i32[0, 0, 0] = -2 ** 31
    i32[0, N - 1, 1] = 2 ** 31 - 1
    i32[C - 1, 1, 2] = 2 ** 24 + 1  # the first integers fp32 cannot hold: the conversion rounds
    i32[C - 1, N - 1, 3] = -(2 ** 24 + 1)
    i32[C - 1, N - 1, hi] = 2 ** 31 - 1
    i32[0, 0, hi] = -2 ** 31
    yield "i32", i32
    u8 = rng.integers(0, 256, shape, dtype=np.int64).astype(np.uint8)
    u8[:, :, 1] = 0
    u8[:, :, 2] = 255
    u8[:, :, hi - 1] = 0
    u8[:, :, hi] = 255
    yield "u8", u8


# ---- reference and bound --------------------------------------------------------------------------------------------

def reference(w32, I):
    """fp64 product of the fp32-rounded pseudo-inverse [k, N] (the operand the kernel is given) with the stack cast
    to fp64: [C, P, k]."""
    w = np.asarray(w32, F32).astype(F64)
    with np.errstate(all="ignore"):
        return np.swapaxes(np.asarray(I).astype(F64), -1, -2) @ w.T


def bound(w32, I, roundings=1):
    """γ_{roundings·(N+1)} · Σ_n |w_kn| · |x_np| : [C, P, k].  roundings = 1 for the VALU and lane kernels, 2 for the
    matrix-core kernels."""
    w = np.abs(np.asarray(w32, F32).astype(F64))
    N = w.shape[1]
    with np.errstate(all="ignore"):
        return gamma(roundings * (N + 1)) * (np.swapaxes(np.abs(np.asarray(I).astype(F64)), -1, -2) @ w.T)


def valu_exact(w32, I):
    """The exact fp32 values of the VALU stream: acc = 0; for n in range(N): acc = fmaf(w[k, n], float32(I[n, p]), acc)
    (fit_valu_body for every MODE but VM_ROT, every VEC and NC; fit_pm_lane): [C, P, k] fp32."""
    w = np.asarray(w32, F32)
    x = np.asarray(I).astype(F32)  # int32 -> fp32 rounds to nearest even, as v_cvt_f32_i32 does
    C, N, P = x.shape
    acc = np.zeros((C, P, w.shape[0]), F32)
    for n in range(N):
        acc = fma32(w[None, None, :, n], x[:, n, :, None], acc)
    return acc


def classify(x):
    """FINITE / POS_INF / NEG_INF / NAN per element."""
    x = np.asarray(x)
    out = np.full(x.shape, FINITE, np.int8)
    out[np.isposinf(x)] = POS_INF
    out[np.isneginf(x)] = NEG_INF
    out[np.isnan(x)] = NAN
    return out


def expected_class(w32, I):
    """The class of every reference coefficient.  The class of such a sum does not depend on the order of its terms:
    finite terms and one sign of infinity give that infinity, both signs or a NaN give NaN."""
    return classify(reference(w32, I))


# ---- poisoning ------------------------------------------------------------------------------------------------------

def poison(I, n0=3):
    """Plants non-finite values in an fp32 stack [C >= 2, N, P] (in place) at positions on the kernels' seams and
    returns them as (c, n, p, value).  Pixel positions past a small stack wrap (p % P)."""
    C, N, P = I.shape
    c0, c1 = 0, C - 1
    nan, inf = F32(np.nan), F32(np.inf)
    planted = [
        (c0, n0, (P // 2 + 1) % P, nan),
        (c0, N - 1, 5 % P, inf),          # the last light: the plane the padded lights of a 4-light step re-read
        (c0, N - 1, P - 1, -inf),         # ... at the last pixel of the channel
        (c1, 0, 0, nan),                  # the element right after channel 0's last plane in memory
        (c1, N // 2, 256 % P, inf),       # two infinities in one pixel: the weights' signs decide between Inf and NaN
        (c1, N // 2 + 1, 256 % P, inf),
        (c1, 1, 1023 % P, inf),           # last pixel of a 1024-pixel wave
        (c1, 2, 1024 % P, nan),           # first pixel of the next
    ]
    for c, n, p, v in planted:
        I[c, n, p] = v
    return planted


# ---- judging a result -----------------------------------------------------------------------------------------------

def worst_ratio(got, ref, bnd):
    """max |got − ref| / bound over the elements whose reference is finite, and its index (c, p, k).  A non-finite
    `got` where the reference is finite counts as infinitely far."""
    with np.errstate(all="ignore"):
        fin = np.isfinite(ref) & np.isfinite(bnd)
        err = np.abs(np.asarray(got, F64) - ref)
        ratio = np.where(fin, np.where(np.isfinite(err), err / np.maximum(bnd, np.finfo(F64).tiny), np.inf), 0.0)
        ratio = np.where(fin & (err == 0), 0.0, ratio)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)
