"""rti_photometric_stereo_near without a GPU: the symbol and its prototype, every argument check answering before any
HIP call (the pointers below are never dereferenced), the plan function against the far entry's, and the NumPy
restatement (tests/ps_near_ref.py) on the 64×64 near-light scene: what the shared-direction model costs there and what
the per-pixel rows and the height refinement recover."""
import ctypes
import os
import re

import numpy as np
import pytest

import rti
from ps_near_ref import ps_near_ref, refine_ref, scene
from ps_ref import angle_deg, ps_design, ps_ref
from rti import _lib as L

P_ = ctypes.c_void_p(4096)
INF = float("inf")
NAN = float("nan")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rti.h")


def call(lights=P_, N=20, I=P_, dt=L.RTI_F32, H=8, W=8, C=1, ls=0, cs=0, x0=0.0, y0=0.0, height=None, z_offset=0.0,
         falloff=1, r0=100.0, lo=-INF, hi=INF, min_lights=3, iters=0, delta=0.0, w=None, normals=P_, layout=0,
         albedo=P_, kernel=0):
    wv = None if w is None else (ctypes.c_float * 3)(*w)
    return rti.load().rti_photometric_stereo_near(lights, N, I, dt, H, W, C, ls, cs, x0, y0, height, z_offset, falloff,
                                                  r0, lo, hi, min_lights, iters, delta, wv, normals, layout, albedo,
                                                  None, None, None, None, kernel, None)


def test_symbol_and_prototype():
    """The library exports both symbols and include/rti.h declares them with the argument list the loader binds."""
    lib = rti.load()
    assert hasattr(lib, "rti_photometric_stereo_near") and hasattr(lib, "rti_photometric_stereo_near_plan")
    text = open(HEADER, encoding="utf-8").read()
    m = re.search(r"int rti_photometric_stereo_near\(([^;]*)\);", text)
    assert m, "rti_photometric_stereo_near is not declared in include/rti.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == [
        "const double* lights", "int N", "const void* I", "int in_dtype", "int H", "int W", "int C",
        "int64_t light_stride", "int64_t channel_stride", "double x0", "double y0", "const float* height",
        "double z_offset", "int falloff", "double r0", "float lo", "float hi", "int min_lights", "int iters",
        "float delta", "const float* w", "float* normals", "int normal_layout", "float* albedo", "uint8_t* kind",
        "float* res", "int32_t* kept", "int* fallback_px", "int kernel", "rti_stream_t stream"]
    assert len(L.SIGNATURES["rti_photometric_stereo_near"][1]) == len(params)
    assert re.search(r"int rti_photometric_stereo_near_plan\(int N, int in_dtype, int C, int iters, int kernel\);", text)


BAD = {
    # the far entry's
    "null lights": dict(lights=None), "null I": dict(I=None), "null normals": dict(normals=None),
    "null albedo": dict(albedo=None), "N < 3": dict(N=2, min_lights=2),
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
    # the near entry's own
    "H < 1": dict(H=0), "W < 1": dict(W=0), "H < 0": dict(H=-3), "H*W = 2^31": dict(H=1 << 16, W=1 << 15),
    "H*W > 2^31": dict(H=46341, W=46341),
    "falloff = 2": dict(falloff=2), "falloff = -1": dict(falloff=-1),
    "r0 = 0 with falloff": dict(r0=0.0), "r0 < 0 with falloff": dict(r0=-5.0), "NaN r0 with falloff": dict(r0=NAN),
    "inf r0 with falloff": dict(r0=INF),
    "NaN x0": dict(x0=NAN), "inf y0": dict(y0=-INF), "NaN z_offset": dict(z_offset=NAN), "inf z_offset": dict(z_offset=INF),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments(case):
    assert call(**BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_photometric_stereo_near" in rti.load().rti_last_error()


UNSUPPORTED = {"C = 2": dict(C=2), "C = 4": dict(C=4), "C = 0": dict(C=0), "fp64 stack": dict(dt=L.RTI_F64),
               "unknown dtype": dict(dt=7)}


@pytest.mark.parametrize("case", sorted(UNSUPPORTED))
def test_unsupported(case):
    assert call(**UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_photometric_stereo_near" in rti.load().rti_last_error()


def test_unknown_kernel_bits_are_refused():
    lib = rti.load()
    for bit in range(0, 32):
        if (1 << bit) == L.RTI_KERNEL_ONE_LAUNCH:
            continue
        assert call(kernel=ctypes.c_int(1 << bit).value) == L.RTI_ERR_BAD_ARG, hex(1 << bit)
        assert b"kernel bits" in lib.rti_last_error() and b"rti_photometric_stereo_near" in lib.rti_last_error()


def test_valid_arguments_pass_every_check():
    """Arguments that are allowed get past every check, so the one wrong argument is the one reported: r0 is read
    only with fall-off, a height map and an origin off the grid are fine, H·W just below 2^31."""
    for kw in (dict(falloff=0, r0=NAN), dict(falloff=0, r0=-1.0), dict(height=P_), dict(x0=-1e6, y0=3.25, z_offset=-7.5),
               dict(H=1, W=(1 << 31) - 1, ls=0), dict(H=1, W=1), dict(ls=68), dict(C=3, ls=68, cs=20 * 68 + 4),
               dict(kernel=L.RTI_KERNEL_ONE_LAUNCH), dict(iters=16, delta=0.5), dict(C=1, w=(NAN, NAN, NAN))):
        assert call(min_lights=99, **kw) == L.RTI_ERR_BAD_ARG, kw
        assert b"min_lights" in rti.load().rti_last_error(), kw


def test_plan_is_the_far_entrys():
    near, far = rti.load().rti_photometric_stereo_near_plan, rti.load().rti_photometric_stereo_plan
    one = L.RTI_KERNEL_ONE_LAUNCH
    for C in (1, 2, 3):
        for dt in (L.RTI_F32, L.RTI_U8, L.RTI_I32, L.RTI_F64):
            for N in (2, 3, 24, 53, 54, 106, 107, 160, 161, 213, 214, 320, 321, 640, 641, 2564):
                for iters in (0, 1, 3):
                    for kernel in (0, one):
                        assert near(N, dt, C, iters, kernel) == far(N, dt, C, iters, kernel), (N, dt, C, iters, kernel)
    assert near(24, L.RTI_F32, 3, 2, 0) == 256 and near(107, L.RTI_F32, 3, 2, 0) == 64 and near(24, L.RTI_F32, 3, 0, 0) == 0


def test_ps_near_lights():
    pos = np.arange(12.0).reshape(4, 3)
    t = rti.ps_near_lights(pos)
    assert t.dtype == np.float64 and t.shape == (4, 4)
    np.testing.assert_array_equal(t[:, :3], pos)
    np.testing.assert_array_equal(t[:, 3], 1.0)
    np.testing.assert_array_equal(rti.ps_near_lights(pos, [1, 2, 3, 4])[:, 3], [1, 2, 3, 4])
    with pytest.raises(ValueError):
        rti.ps_near_lights(pos[:, :2])
    with pytest.raises(ValueError):
        rti.ps_near_lights(pos, [1, 2, 3])


LO, HI = 0.5, 254.5


def test_reference_accuracy_on_the_near_scene():
    """The feature, not just the code path, with ps_near_ref alone on the 64×64 grey scene (24 lights at 2·W, bump of
    6 px, albedo 150..400, fall-off, window 0.5..254.5).  Measured, maximum (mean) normal error:
      shared-direction model (ps_ref on the spiral directions)   35.30° (15.87°), albedo 167..372 where 150..400 is true
      per-pixel rows, surface taken as the plane z = 0            1.215° (0.212°), albedo within 0.983..1.037 of true
      per-pixel rows, true height                                 2.8e-6° (6.3e-7°), albedo to 6.1e-8 relative
    and the alternation normals -> height (height_ref's system, solved directly) -> normals from the plane:
      round 0 1.215°, round 1 0.0739°, round 2 0.00399°.
    One of the scene's 98304 samples is the fp32 value 254.5 itself, so the scene does not meet the margin condition of
    check_ps_near_inputs; nothing here is compared with a GPU result, and the window compares that sample exactly."""
    sc = scene(64, 64)
    I = sc["I"]
    assert (I == 255).any()
    far = ps_ref(ps_design(sc["lu"], sc["lv"]), I, LO, HI)
    far_err = angle_deg(far["normals"], sc["n"])
    rounds = refine_ref(sc, 64, 64, 2, LO, HI)
    plane_err = angle_deg(rounds[0]["normals"], sc["n"])
    true = ps_near_ref(sc["lights"], I, 64, 64, height=sc["h"], r0=sc["r0"], lo=LO, hi=HI)
    true_err = angle_deg(true["normals"], sc["n"])
    errs = [angle_deg(r["normals"], sc["n"]).max() for r in rounds]
    print(f"far max {far_err.max():.4g} mean {far_err.mean():.4g}; plane max {plane_err.max():.4g} mean "
          f"{plane_err.mean():.4g}; true height max {true_err.max():.4g}; rounds {errs}")
    assert true_err.max() <= 1e-3
    assert plane_err.max() <= far_err.max() / 10.0
    assert far_err.mean() > 5.0
    assert (np.abs(true["albedo"] / sc["albedo"] - 1.0) <= 1e-6).all()
    assert errs[2] < errs[1] < errs[0]
    assert all(r["fallback_px"] == 0 and (r["kind"] == 0).all() for r in rounds)
