"""rti_gauss_* / rti_map_unsharp / rti_shade_normals without a GPU: the symbols are bound, the host taps agree with
their NumPy restatement (tests/unsharp_ref.py), every argument check answers before any HIP call (the pointers below
are never dereferenced) with a message that names the function, and the Python wrappers refuse what they cannot
launch."""
import ctypes

import numpy as np
import pytest

import rti
import unsharp_ref as ur
from rti import _lib as L

SRC, DST = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)  # 1 GiB apart: no map below overlaps
NAN, INF = float("nan"), float("inf")
SIGMAS = [0.3, 1.0, 2.5, 10.6]


def unsharp_call(src=SRC, ch=3, layout=0, H=16, W=16, sigma=2.0, radius=0, amount=1.0, renorm=0, dst=DST):
    return rti.load().rti_map_unsharp(src, ch, layout, H, W, sigma, radius, amount, renorm, dst, None)


def shade_call(n=SRC, nl=0, albedo=None, P=64, kd=1.0, ks=0.0, e=1, lu=0.1, lv=0.2, out=DST, odt=L.RTI_F32):
    return rti.load().rti_shade_normals(n, nl, albedo, P, kd, ks, e, lu, lv, out, odt, None)


def test_symbols_and_constants():
    lib = rti.load()
    for name in ("rti_gauss_radius", "rti_gauss_taps", "rti_map_unsharp", "rti_shade_normals"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert L.RTI_UNSHARP_MAX_RADIUS == ur.MAX_RADIUS == 32
    assert lib.rti_version() == 100
    for fn in ("unsharp", "normals_unsharp", "shade_normals", "gauss_taps", "map_unsharp_into", "shade_normals_into"):
        assert callable(getattr(rti, fn))
    assert rti.api.map_unsharp_into is rti.map_unsharp_into and rti.api.shade_normals_into is rti.shade_normals_into


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gauss_radius_and_taps(sigma):
    lib = rti.load()
    R = lib.rti_gauss_radius(sigma)
    assert R == ur.gauss_radius(sigma) == max(1, int(np.ceil(3 * sigma)))
    for radius in (R, 1, 32):
        want = ur.gauss_taps(sigma, radius)
        got = np.zeros(radius + 1)
        assert lib.rti_gauss_taps(sigma, radius, got.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == L.RTI_OK
        nz = want > 0
        assert np.array_equal(got[~nz], want[~nz])  # a tap that underflows to 0 does so in both
        assert (np.abs(got[nz] - want[nz]) <= 1e-15 * want[nz]).all()
        assert abs(got[0] + 2.0 * got[1:].sum() - 1.0) <= 1e-15
        assert np.array_equal(rti.gauss_taps(sigma, radius), got)
    assert np.array_equal(rti.gauss_taps(sigma), rti.gauss_taps(sigma, R))


def test_gauss_bad_arguments():
    lib = rti.load()
    buf = (ctypes.c_double * 40)()
    for sigma in (0.0, -1.0, NAN, INF, -INF):
        assert lib.rti_gauss_radius(sigma) == -1
        assert lib.rti_gauss_taps(sigma, 3, buf) == L.RTI_ERR_BAD_ARG
        assert b"rti_gauss_taps" in lib.rti_last_error()
        with pytest.raises(ValueError):
            rti.gauss_taps(sigma)
    for radius in (0, -1, 33):
        assert lib.rti_gauss_taps(2.0, radius, buf) == L.RTI_ERR_BAD_ARG
        assert b"rti_gauss_taps" in lib.rti_last_error()
    assert lib.rti_gauss_taps(2.0, 6, None) == L.RTI_ERR_BAD_ARG
    assert lib.rti_gauss_radius(1e300) > 32  # no overflow into a small or negative radius


UNSHARP_BAD = {
    "null src": dict(src=None), "null dst": dict(dst=None),
    "H = 0": dict(H=0), "W = 0": dict(W=0), "H < 0": dict(H=-3), "W < 0": dict(W=-1),
    "H*W*channels = 2^31": dict(H=1 << 15, W=1 << 14, ch=4), "H*W > 2^31": dict(H=1 << 20, W=1 << 20, ch=1),
    "channels 0": dict(ch=0), "channels 17": dict(ch=17), "channels < 0": dict(ch=-1),
    "layout 2": dict(layout=2), "layout -1": dict(layout=-1),
    "sigma 0": dict(sigma=0.0), "sigma < 0": dict(sigma=-2.0), "sigma NaN": dict(sigma=NAN), "sigma inf": dict(sigma=INF),
    "radius 33": dict(radius=33), "radius < 0": dict(radius=-1), "default radius 33": dict(sigma=10.7),
    "amount NaN": dict(amount=NAN), "amount inf": dict(amount=-INF),
    "renorm with 1 channel": dict(renorm=1, ch=1), "renorm with 6 channels": dict(renorm=1, ch=6),
    "in place": dict(dst=SRC), "dst inside src": dict(dst=ctypes.c_void_p((1 << 20) + 16 * 16 * 3 * 4 - 4)),
    "src inside dst": dict(src=ctypes.c_void_p((1 << 30) + 4)),
}
SHADE_BAD = {
    "null normals": dict(n=None), "null out": dict(out=None), "P = 0": dict(P=0), "P < 0": dict(P=-4),
    "normal layout 2": dict(nl=2), "normal layout -1": dict(nl=-1),
    "NaN kd": dict(kd=NAN), "inf kd": dict(kd=INF), "NaN ks": dict(ks=NAN), "inf ks": dict(ks=-INF),
    "NaN lu": dict(lu=NAN), "inf lu": dict(lu=INF), "NaN lv": dict(lv=NAN), "inf lv": dict(lv=-INF),
    "exp 0": dict(e=0), "exp 256": dict(e=256), "exp < 0": dict(e=-3),
}
SHADE_UNSUPPORTED = {"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9), "negative out dtype": dict(odt=-1)}


@pytest.mark.parametrize("case", sorted(UNSHARP_BAD))
def test_unsharp_bad_arguments(case):
    assert unsharp_call(**UNSHARP_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_map_unsharp" in rti.load().rti_last_error()


def test_default_radius_message():
    assert unsharp_call(sigma=11.0) == L.RTI_ERR_BAD_ARG
    msg = rti.load().rti_last_error()
    assert b"rti_map_unsharp" in msg and b"default radius" in msg and b"33" in msg
    assert unsharp_call(sigma=11.0, radius=40) == L.RTI_ERR_BAD_ARG
    assert b"default radius" not in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(SHADE_BAD))
def test_shade_bad_arguments(case):
    assert shade_call(**SHADE_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_shade_normals" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(SHADE_UNSUPPORTED))
def test_shade_unsupported(case):
    assert shade_call(**SHADE_UNSUPPORTED[case]) == L.RTI_ERR_UNSUPPORTED, case
    assert b"rti_shade_normals" in rti.load().rti_last_error()


def test_python_layer_rejects_what_it_cannot_launch():
    import torch

    with pytest.raises(ValueError, match="CUDA"):
        rti.unsharp(torch.zeros((8, 8, 6)), 2.0)
    with pytest.raises(ValueError, match="CUDA"):
        rti.normals_unsharp(torch.zeros((8, 8, 3)), 2.0)
    with pytest.raises(ValueError, match="CUDA"):
        rti.map_unsharp_into(torch.zeros((8, 8)), torch.zeros((8, 8)), sigma=2.0)
    with pytest.raises(ValueError, match="CUDA"):
        rti.shade_normals(torch.zeros((8, 8, 3)), 0.1, 0.2)
    with pytest.raises(ValueError, match="CUDA"):
        rti.shade_normals_into(torch.zeros((64, 3)), 0.1, 0.2, torch.zeros(64))
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    with pytest.raises(ValueError, match="CUDA"):
        torch.ops.rti.map_unsharp(torch.zeros((8, 8, 3)), 2.0)
    with pytest.raises(ValueError, match="CUDA"):
        torch.ops.rti.shade_normals(torch.zeros((64, 3)), 0.1, 0.2)
    # dtype, shape and renorm are judged before the device, so they are named even for a CPU tensor
    with pytest.raises(ValueError, match="float32"):
        rti.unsharp(torch.zeros((8, 8, 3), dtype=torch.float64), 2.0)
    with pytest.raises(ValueError, match="float32"):
        rti.map_unsharp_into(torch.zeros((8, 8), dtype=torch.int32), torch.zeros((8, 8)), sigma=2.0)
    for shape in ((2, 8, 8, 3), (8,)):
        with pytest.raises(ValueError, match=r"\[H, W\]"):
            rti.unsharp(torch.zeros(shape), 2.0)
    for shape, layout in (((8, 8, 6), "pixel"), ((8, 8), "pixel"), ((8, 8, 3), "planar")):
        with pytest.raises(ValueError, match="renorm"):
            rti.unsharp(torch.zeros(shape), 2.0, renorm=True, layout=layout)
        with pytest.raises(ValueError, match="renorm"):
            rti.normals_unsharp(torch.zeros(shape), 2.0, layout=layout)
    with pytest.raises(ValueError, match="contiguous"):
        rti.map_unsharp_into(torch.zeros((8, 8, 3)).permute(2, 0, 1), torch.zeros((3, 8, 8)), sigma=2.0, layout="planar")
    with pytest.raises(ValueError, match="layout"):
        rti.unsharp(torch.zeros((8, 8, 3)), 2.0, layout="rows")
    with pytest.raises(ValueError, match="float32"):
        rti.shade_normals(torch.zeros((8, 8, 3), dtype=torch.float64), 0.1, 0.2)
    with pytest.raises(ValueError, match="terms"):
        rti.shade_normals(torch.zeros((8, 8, 4)), 0.1, 0.2)
    with pytest.raises(ValueError, match="3 values"):
        rti.shade_normals_into(torch.zeros((64, 2)), 0.1, 0.2, torch.zeros(64))


def test_shade_inputs_stay_under_the_near_integer_cap():
    """The integer-output comparison of tests/test_gpu_unsharp.py leaves out the pixels whose fp64 reference lies
    within 1e-6 of an integer (exact integers are compared); with the shared inputs that is at most 1 % of every
    map, from the reference alone."""
    worst = 0.0
    for P in ur.SHADE_SIZES:
        n, a = ur.shade_inputs(P)
        for alb in (None, a):
            for lu, lv in ur.SHADE_DIRS:
                for kd, ks, e in ur.SHADE_PARAMS:
                    share = ur.near_integer(ur.shade_ref(n, lu, lv, alb, kd, ks, e)).mean()
                    worst = max(worst, share)
                    assert share <= 0.01, (P, lu, lv, kd, ks, e, share)
    print(f"worst near-integer share {worst:.4%}")


def test_reference_properties():
    """The restatement itself: a constant map and a ramp away from the borders are fixed points, amount = 0 is the
    identity, amount = −1 the blur, NaN stays where it is."""
    w = ur.gauss_taps(2.0)
    assert len(w) == 7
    const = np.full((20, 30, 2), 7.5, np.float32)
    out, m = ur.unsharp_ref(const, 2.0, 1.5)
    assert m.all() and np.abs(out - 7.5).max() <= 1e-12
    yy, xx = np.mgrid[0:40, 0:50]
    ramp = (3.0 * xx - 2.0 * yy + 11.0).astype(np.float32)[..., None]
    out, _ = ur.unsharp_ref(ramp, 2.0, 1.5)
    assert np.abs(out - ramp)[6:-6, 6:-6].max() <= 1e-10
    a = ur.map_input(24, 31, 3, 1)
    out0, m = ur.unsharp_ref(a, 2.0, 0.0)
    assert np.array_equal(out0[m], a.astype(np.float64)[m]) and not m.all() and m.any()
    out, _ = ur.unsharp_ref(a, 2.0, -1.0)
    assert np.isfinite(out[m]).all() and np.array_equal(np.isfinite(out).all(-1), m)
    n = np.zeros((5, 5, 3), np.float32)
    n[..., 2] = 1.0
    n[2, 2] = (0.6, 0.0, 0.8)
    out, _ = ur.unsharp_ref(n, 1.0, 1.5, renorm=True)
    assert np.abs(np.linalg.norm(out, axis=-1) - 1.0).max() <= 1e-15
