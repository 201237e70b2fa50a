"""rti_photometric_stereo without a GPU: every argument check answers before any HIP call (the pointers below are
never dereferenced), rti_photometric_stereo_plan's tile rule at its edges, rti_ps_design against NumPy, and the
NumPy restatement (tests/ps_ref.py) on the synthetic Lambertian scene: the window recovers the surface, the plain
least squares does not."""
import ctypes

import numpy as np
import pytest

import rti
from ps_ref import angle_deg, check_ps_inputs, ps_design, ps_ref, scene
from rti import _lib as L

P_ = ctypes.c_void_p(4096)
INF = float("inf")
NAN = float("nan")


def call(A=P_, N=20, I=P_, dt=L.RTI_F32, P=64, C=1, ls=0, cs=0, lo=-INF, hi=INF, min_lights=3, iters=0, delta=0.0,
         w=None, normals=P_, layout=0, albedo=P_, kernel=0):
    wv = None if w is None else (ctypes.c_float * 3)(*w)
    return rti.load().rti_photometric_stereo(A, N, I, dt, P, C, ls, cs, lo, hi, min_lights, iters, delta, wv, normals,
                                             layout, albedo, None, None, None, None, kernel, None)


BAD = {
    "null A": dict(A=None), "null I": dict(I=None), "null normals": dict(normals=None), "null albedo": dict(albedo=None),
    "N < 3": dict(N=2, min_lights=2), "P < 1": dict(P=0),
    "lo > hi": dict(lo=200.0, hi=100.0), "NaN lo": dict(lo=NAN), "NaN hi": dict(hi=NAN),
    "min_lights < 3": dict(min_lights=2), "min_lights > N": dict(min_lights=21),
    "iters < 0": dict(iters=-1), "iters > 16": dict(iters=17, delta=1.0),
    "delta = 0 with iters": dict(iters=1, delta=0.0), "delta < 0 with iters": dict(iters=2, delta=-1.0),
    "NaN delta with iters": dict(iters=1, delta=NAN),
    "normal layout": dict(layout=2),
    "NaN weight": dict(C=3, w=(0.3, NAN, 0.1)), "inf weight": dict(C=3, w=(INF, 0.5, 0.1)),
    "light_stride < P": dict(ls=63),
    "channel stride below dense": dict(C=3, cs=20 * 64 - 1),
    "channel stride below padded planes": dict(C=3, ls=68, cs=20 * 68 - 1),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments(case):
    assert call(**BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_photometric_stereo" in rti.load().rti_last_error()


UNSUPPORTED = {"C = 2": dict(C=2), "C = 4": dict(C=4), "C = 0": dict(C=0), "fp64 stack": dict(dt=L.RTI_F64),
               "unknown dtype": dict(dt=7)}


@pytest.mark.parametrize("case", sorted(UNSUPPORTED))
def test_unsupported(case):
    assert call(**UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_photometric_stereo" in rti.load().rti_last_error()


def test_unknown_kernel_bits_are_refused():
    lib = rti.load()
    for bit in range(0, 32):
        if (1 << bit) == L.RTI_KERNEL_ONE_LAUNCH:
            continue
        assert call(kernel=ctypes.c_int(1 << bit).value) == L.RTI_ERR_BAD_ARG, hex(1 << bit)
        assert b"kernel bits" in lib.rti_last_error() and b"rti_photometric_stereo" in lib.rti_last_error()


def test_valid_arguments_pass_every_check():
    """±inf bounds, a grey stack's unread weights and channel stride, padded strides: the call gets past the
    argument checks, so the one wrong argument is the one reported."""
    for kw in (dict(lo=-INF, hi=INF), dict(C=1, w=(NAN, NAN, NAN)), dict(C=1, cs=1), dict(ls=68),
               dict(C=3, ls=68, cs=20 * 68 + 4), dict(kernel=L.RTI_KERNEL_ONE_LAUNCH), dict(iters=16, delta=0.5)):
        assert call(min_lights=99, **kw) == L.RTI_ERR_BAD_ARG, kw
        assert b"min_lights" in rti.load().rti_last_error(), kw


PLAN_F32 = {1: ((160, 256), (161, 128), (320, 128), (321, 64), (640, 64), (641, 0)),
            3: ((53, 256), (54, 128), (106, 128), (107, 64), (213, 64), (214, 0))}


@pytest.mark.parametrize("C", [1, 3])
def test_plan_tile_rule_at_its_edges(C):
    plan = rti.load().rti_photometric_stereo_plan
    one = L.RTI_KERNEL_ONE_LAUNCH
    for N, tp in PLAN_F32[C]:
        assert plan(N, L.RTI_F32, C, 1, 0) == tp, (N, tp)
        assert plan(N, L.RTI_I32, C, 3, 0) == tp, (N, tp)
        assert C * N * tp * 4 <= 160 * 1024
        assert plan(4 * N, L.RTI_U8, C, 2, 0) == tp, (4 * N, tp)  # a byte tile holds four times the lights
        for n, dt in ((N, L.RTI_F32), (4 * N, L.RTI_U8)):
            assert plan(n, dt, C, 0, 0) == 0      # one pass: nothing to keep resident
            assert plan(n, dt, C, 3, one) == 0    # forced streaming
            assert plan(n, dt, C, 0, one) == 0
    assert plan(100, L.RTI_F32, 2, 3, 0) == 0 and plan(100, L.RTI_F64, 1, 3, 0) == 0 and plan(2, L.RTI_F32, 1, 3, 0) == 0


def test_ps_design_matches_numpy():
    rng = np.random.default_rng(0)
    lu = rng.uniform(-0.7, 0.7, 40).astype(np.float32)
    lv = rng.uniform(-0.7, 0.7, 40).astype(np.float32)
    lu[:3], lv[:3] = (0.8, 1.0, 0.0), (0.8, 0.0, -1.25)  # lu² + lv² > 1, = 1, > 1
    A = rti.ps_design(lu, lv)
    assert A.dtype == np.float64 and A.shape == (40, 3)
    np.testing.assert_array_equal(A, ps_design(lu, lv))
    assert A[0, 2] == 0.0 and A[1, 2] == 0.0 and A[2, 2] == 0.0 and (A[3:, 2] > 0).all()
    np.testing.assert_array_equal(A[:, 0], lu.astype(np.float64))
    lz = rng.uniform(0.1, 1.0, 40)
    Az = rti.ps_design(lu, lv, lz)
    np.testing.assert_array_equal(Az[:, :2], A[:, :2])
    np.testing.assert_array_equal(Az[:, 2], lz)
    with pytest.raises(ValueError):
        rti.ps_design(lu, lv[:5])
    with pytest.raises(ValueError):
        rti.ps_design(lu, lv, lz[:5])
    assert rti.load().rti_ps_design(None, None, 3, None) == L.RTI_ERR_BAD_ARG


@pytest.mark.parametrize("rgb", [False, True])
def test_reference_window_recovers_the_scene(rgb):
    """The feature, not just the code path: on clipped and shadowed Lambertian samples the windowed fit returns the
    surface (normals to 1e-4°, albedo to 1e-6 relative) and the fit of every sample is off by degrees."""
    lu, lv, A, n_true, alb_true, I = scene(400, rgb=rgb)
    assert (I == 0).any() and (I == 255).any()
    ref = ps_ref(A, I, 0.5, 254.5, min_lights=3)
    check_ps_inputs(ref, I, 0.5, 254.5)
    assert ref["fallback_px"] == 0 and (ref["kind"] == 0).all() and ref["kept"].min() >= 3
    assert angle_deg(ref["normals"], n_true).max() <= 1e-4
    assert (np.abs(ref["albedo"] - alb_true) / alb_true).max() <= 1e-6
    plain = ps_ref(A, I)
    assert (plain["kept"] == 24).all()
    assert angle_deg(plain["normals"], n_true).max() > 5.0
