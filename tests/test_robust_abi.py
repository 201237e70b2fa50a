"""rti_fit_shared_robust without a GPU: every argument check answers before any HIP call (the pointers below are
never dereferenced), rti_fit_shared_robust_plan's tile rule, and the NumPy restatement (tests/robust_ref.py)
against the reference's plain least squares."""
import ctypes

import numpy as np
import pytest

import rti
import rti_oracle as o
from conftest import golden
from rti import _lib as L
from robust_ref import fit_robust_ref

P_ = ctypes.c_void_p(4096)
INF = float("inf")


def call(A=P_, k=6, N=20, I=P_, dt=L.RTI_F32, lo=-INF, hi=INF, min_lights=6, iters=0, delta=0.0, coef=P_, layout=0,
         kernel=0):
    return rti.load().rti_fit_shared_robust(A, k, N, I, dt, 64, 1, 0, 0, lo, hi, min_lights, iters, delta, coef, layout,
                                            0, None, None, None, kernel, None)


BAD = {
    "null A": dict(A=None), "null I": dict(I=None), "null coef": dict(coef=None),
    "N < k": dict(N=5, min_lights=5), "N < k (hsh9)": dict(k=9, N=8, min_lights=8),
    "lo > hi": dict(lo=200.0, hi=100.0), "NaN lo": dict(lo=float("nan")), "NaN hi": dict(hi=float("nan")),
    "min_lights < k": dict(min_lights=5), "min_lights > N": dict(min_lights=21),
    "iters < 0": dict(iters=-1), "iters > 16": dict(iters=17, delta=1.0),
    "delta = 0 with iters": dict(iters=1, delta=0.0), "delta < 0 with iters": dict(iters=2, delta=-1.0),
    "NaN delta with iters": dict(iters=1, delta=float("nan")),
    "layout": dict(layout=2),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments(case):
    assert call(**BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_fit_shared_robust" in rti.load().rti_last_error()


def test_unknown_kernel_bits_are_refused():
    lib = rti.load()
    for bit in range(0, 32):
        if (1 << bit) == L.RTI_KERNEL_ONE_LAUNCH:
            continue
        assert call(kernel=ctypes.c_int(1 << bit).value) == L.RTI_ERR_BAD_ARG, hex(1 << bit)
        assert b"kernel bits" in lib.rti_last_error()


def test_unsupported():
    assert call(k=16, N=100, min_lights=16) == L.RTI_ERR_UNSUPPORTED
    assert b"k=16" in rti.load().rti_last_error()
    assert call(k=7, N=100, min_lights=7) == L.RTI_ERR_UNSUPPORTED
    assert call(dt=L.RTI_F64) == L.RTI_ERR_UNSUPPORTED


def test_infinite_bounds_are_valid_arguments():
    # ±inf mean "no bound": the call gets past the argument checks (and, without a device, fails at the launch)
    assert call(lo=-INF, hi=INF, min_lights=99, N=20) == L.RTI_ERR_BAD_ARG  # only min_lights is wrong here
    assert b"min_lights" in rti.load().rti_last_error()


def test_plan_tile_rule():
    plan = rti.load().rti_fit_shared_robust_plan
    one = L.RTI_KERNEL_ONE_LAUNCH
    assert plan(6, 100, L.RTI_F32, 3, 0) == 256  # 100 KiB
    assert plan(6, 700, L.RTI_F32, 3, 0) == 0    # 64 pixels x 700 lights x 4 B = 175 KiB: no tile fits
    assert plan(9, 160, L.RTI_F32, 1, 0) == 256 and plan(9, 161, L.RTI_F32, 1, 0) == 128
    assert plan(6, 320, L.RTI_I32, 1, 0) == 128 and plan(6, 321, L.RTI_I32, 1, 0) == 64
    assert plan(6, 640, L.RTI_F32, 1, 0) == 64 and plan(6, 641, L.RTI_F32, 1, 0) == 0
    assert plan(6, 640, L.RTI_U8, 1, 0) == 256 and plan(6, 700, L.RTI_U8, 2, 0) == 128
    for k, N, dt in ((6, 100, L.RTI_F32), (9, 24, L.RTI_U8), (6, 700, L.RTI_F32)):
        assert plan(k, N, dt, 0, 0) == 0       # one pass: nothing to keep resident
        assert plan(k, N, dt, 3, one) == 0     # forced streaming
        assert plan(k, N, dt, 0, one) == 0
    assert plan(16, 100, L.RTI_F32, 3, 0) == 0


def test_reference_without_bounds_is_plain_least_squares():
    d = golden("ptm_shared_256x256_N20.npz")
    I = d["I"].astype(np.float64).reshape(20, -1)[:, ::97]
    A = o.ptm_design(d["lu"], d["lv"])
    r = fit_robust_ref(A, I)
    ref = o.fit_shared(I, o.pinv_shared("ptm", d["lu"], d["lv"]))
    assert np.abs(r["coef"] - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (r["kept"] == 20).all() and r["fallback_px"] == 0
    assert np.allclose(r["res"], np.sqrt(((I - A @ ref.T) ** 2).mean(0)), rtol=1e-9, atol=1e-9)
