"""rti_peak_grid_points / rti_peak_table_bytes / rti_peak_table / rti_hsh_normals / rti_hsh8_normals without a GPU: the
symbols are bound, every argument check answers before any HIP call (the pointers below are never dereferenced) with
a message that names the function, the two queries count the grid, the Python layer refuses CPU tensors and other
bases, and the accuracy of the search itself (tests/hsh_normals_ref.py on the oracle's fp64 basis) is pinned."""
import ctypes

import numpy as np
import pytest

import rti
from hsh_normals_ref import grid_dirs, grid_points, luminance, peak_normal
from rti import _lib as L

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
OFF8 = ctypes.c_void_p(4104)  # 8 bytes off a 16-byte boundary
ODD = ctypes.c_void_p(4098)  # 2 bytes off a dword
H16, H9 = L.RTI_BASIS_HSH16, L.RTI_BASIS_HSH9
NAN3 = (ctypes.c_float * 3)(0.3, float("nan"), 0.1)
INF3 = (ctypes.c_float * 3)(float("inf"), 0.5, 0.1)


def table_call(basis=H16, grid=10, table=P_):
    return rti.load().rti_peak_table(basis, grid, table, None)


def maps_call(coef=P_, basis=H16, layout=0, C=3, stride=0, P=64, w=None, grid=10, table=P_, normals=P_, nl=0,
              kind=None, peak=None):
    return rti.load().rti_hsh_normals(coef, basis, layout, C, stride, P, w, grid, table, normals, nl, kind, peak, None)


def bytes_call(coef8=P_, basis=H16, P=64, qparams=P_, w=None, grid=10, table=P_, normals=P_, nl=0, kind=None,
               peak=None):
    return rti.load().rti_hsh8_normals(coef8, basis, P, qparams, w, grid, table, normals, nl, kind, peak, None)


SEARCH_BAD = {
    "null table": dict(table=None), "null normals": dict(normals=None), "P = 0": dict(P=0), "P < 0": dict(P=-3),
    "normal layout": dict(nl=2), "normal layout < 0": dict(nl=-1), "grid 3": dict(grid=3), "grid 17": dict(grid=17),
    "grid 0": dict(grid=0), "grid < 0": dict(grid=-10), "NaN weight": dict(w=NAN3), "inf weight": dict(w=INF3),
    "table off 16 bytes": dict(table=OFF8),
}
MAPS_BAD = dict(SEARCH_BAD, **{
    "null coef": dict(coef=None), "C = 0": dict(C=0), "C = 2": dict(C=2), "C = 4": dict(C=4),
    "layout": dict(layout=2), "layout < 0": dict(layout=-1), "stride below dense, hsh16": dict(stride=64 * 16 - 1),
    "stride below dense, hsh9": dict(basis=H9, stride=64 * 9 - 1), "stride below dense, planar": dict(layout=1, stride=100),
    "stride < 0": dict(stride=-1),
})
BYTES_BAD = dict(SEARCH_BAD, **{"null coef8": dict(coef8=None), "null qparams": dict(qparams=None),
                                "qparams off a dword": dict(qparams=ODD)})
TABLE_BAD = {"null table": dict(table=None), "grid 3": dict(grid=3), "grid 17": dict(grid=17),
             "table off 16 bytes": dict(table=OFF8)}
UNSUPPORTED = {"ptm": dict(basis=L.RTI_BASIS_PTM6), "unknown basis": dict(basis=7), "basis < 0": dict(basis=-1)}


def answers(call, cases, case, status, name):
    lib = rti.load()
    assert call(**cases[case]) == status, case
    msg = lib.rti_last_error()
    assert name in msg and len(msg) > len(name), msg


@pytest.mark.parametrize("case", sorted(MAPS_BAD))
def test_hsh_normals_bad_arguments(case):
    answers(maps_call, MAPS_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_hsh_normals")


@pytest.mark.parametrize("case", sorted(BYTES_BAD))
def test_hsh8_normals_bad_arguments(case):
    answers(bytes_call, BYTES_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_hsh8_normals")


@pytest.mark.parametrize("case", sorted(TABLE_BAD))
def test_peak_table_bad_arguments(case):
    answers(table_call, TABLE_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_peak_table")


@pytest.mark.parametrize("case", sorted(UNSUPPORTED))
def test_unsupported_bases(case):
    answers(maps_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_hsh_normals")
    answers(bytes_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_hsh8_normals")
    answers(table_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_peak_table")


def test_a_single_map_ignores_its_channel_stride():
    """C = 1 never uses the stride, so only C = 3 checks it (the rule of every entry that takes one)."""
    assert maps_call(C=1, stride=5, P=0) == L.RTI_ERR_BAD_ARG  # reaches the P check, and no launch
    assert b"P must be positive" in rti.load().rti_last_error()


def test_symbols_are_bound():
    lib = rti.load()
    for name in ("rti_peak_grid_points", "rti_peak_table_bytes", "rti_peak_table", "rti_hsh_normals",
                 "rti_hsh8_normals"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("hsh_normals", "hsh8_normals", "hsh_normals_into", "hsh8_normals_into", "peak_table",
                 "peak_grid_points"):
        assert callable(getattr(rti, name)) and name in rti.__all__, name
        assert callable(getattr(rti.api, name))


def test_grid_points_count_the_mask():
    lib = rti.load()
    for G in range(4, 17):
        want = sum(1 for i in range(-G, G + 1) for j in range(-G, G + 1) if i * i + j * j <= G * G)
        assert lib.rti_peak_grid_points(G) == want == len(grid_points(G)) == rti.peak_grid_points(G), G
        assert lib.rti_peak_table_bytes(H16, G) == (want * 16 * 4 + 15) // 16 * 16
        assert lib.rti_peak_table_bytes(H9, G) == (want * 9 * 4 + 15) // 16 * 16
    assert lib.rti_peak_grid_points(4) == 49 and lib.rti_peak_grid_points(10) == 317
    for G in (-4, 0, 1, 3, 17, 32, 1 << 20):
        assert lib.rti_peak_grid_points(G) == -1, G
        assert lib.rti_peak_table_bytes(H16, G) == 0 and lib.rti_peak_table_bytes(H9, G) == 0
        with pytest.raises(ValueError):
            rti.peak_grid_points(G)
    for G in (4, 10, 16):
        assert lib.rti_peak_table_bytes(L.RTI_BASIS_PTM6, G) == 0 and lib.rti_peak_table_bytes(9, G) == 0


def test_reference_grid_order_and_luminance():
    pts = grid_points(4)
    assert pts[0] == (0, -4) and pts[1] == (-2, -3) and pts[-1] == (0, 4) and pts[len(pts) // 2] == (0, 0)
    assert list(pts) == sorted(pts, key=lambda p: (p[1], p[0]))
    u, v = grid_dirs(10)
    assert u.dtype == np.float64 and u[0] == 0.0 and v[0] == -1.0 and (u * u + v * v <= 1.0 + 1e-15).all()
    m = np.float32([[[1.0, 3.0]], [[2.0, 5.0]], [[4.0, 7.0]]])
    f = np.float32
    want = f(f(f(0.299) * f(1.0)) + f(f(0.587) * f(2.0))) + f(f(0.114) * f(4.0))
    got = luminance(m)
    assert got.dtype == np.float32 and got.shape == (1, 2) and got[0, 0] == f(want)
    assert np.array_equal(luminance(m, (1, 0, 0)), m[0])


def test_reference_kinds_on_made_up_grid_values():
    G = 10
    pts = grid_points(G)
    E = len(pts)
    flat = np.full(E, 3.5, np.float32)
    n, kind, peak = peak_normal(flat, G)
    assert kind == 2 and n.tolist() == [0.0, 0.0, 1.0] and peak == np.float32(3.5)
    n, kind, peak = peak_normal(flat, G, finite=False)
    assert kind == 4 and np.isnan(n).all() and np.isnan(peak)
    # two equal maxima: the smaller index wins; its u-neighbours exist and are equal, so the step is 0
    V = np.zeros(E, np.float32)
    a, b = pts.index((-3, -2)), pts.index((5, 1))
    V[a] = V[b] = 9.0
    n, kind, peak = peak_normal(V, G)
    assert kind == 0 and peak == 9.0 and n[0] == np.float32(-0.3) and n[1] == np.float32(-0.2)
    # a parabola through (-1, 0, 1) -> (1, 4, 3): d = -4, step = 0.5·(1 − 3)/−4 = 0.25
    V = np.zeros(E, np.float32)
    V[pts.index((1, 0))], V[pts.index((2, 0))], V[pts.index((3, 0))] = 1.0, 4.0, 3.0
    n, kind, _ = peak_normal(V, G)
    assert kind == 0 and n[0] == np.float32(0.225) and n[1] == 0.0
    # a peak on the mask's edge: (0, -G) has no u-neighbours and no (0, -G-1): no step, r² = 1, n_z = 0
    V = np.zeros(E, np.float32)
    V[0] = 1.0
    n, kind, _ = peak_normal(V, G)
    assert kind == 0 and n.tolist() == [0.0, -1.0, 0.0]
    # kind 1 needs r² > 1.  A refined point is a convex combination of mask points, so only rounding gets there:
    # (6, 8)/10 squares to 1 + 2⁻⁵² in fp64
    V = np.zeros(E, np.float32)
    V[pts.index((6, 8))] = 1.0
    n, kind, _ = peak_normal(V, G)
    r2 = np.float64(0.6) * np.float64(0.6) + np.float64(0.8) * np.float64(0.8)
    assert kind == (1 if r2 > 1.0 else 0) and n[2] == 0.0
    assert abs(float(n[0]) - 0.6) < 1e-7 and abs(float(n[1]) - 0.8) < 1e-7


def lambertian_case(tilt_deg, az):
    import rti_oracle as o

    lu, lv = o.synth_dirs(40, 1)
    lw = np.sqrt(np.maximum(0.0, 1.0 - lu.astype(np.float64) ** 2 - lv.astype(np.float64) ** 2))
    t = np.radians(tilt_deg)
    n = np.array([np.sin(t) * np.cos(az), np.sin(t) * np.sin(az), np.cos(t)])
    I = 200.0 * np.maximum(0.0, np.stack([lu, lv, lw], 1) @ n)
    return n, np.linalg.pinv(o.hsh_basis(lu, lv, 3)) @ I


AZIMUTHS = np.linspace(0.1, 2 * np.pi + 0.1, 8, endpoint=False)
ACCURACY_BOUND_DEG = 1.5


def test_reference_accuracy_on_a_lambertian_fit():
    """The search applied to the oracle's fp64 hsh_basis values (rounded to fp32, as grid values are) of a
    pseudo-inverse HSH-16 fit of 200·max(0, n·l) under synth_dirs(40, 1), G = 10, 8 azimuths: the worst angular
    errors measured were 0.0°, 0.2° and 0.7° at tilts 0°, 15° and 30°; the bound is 1.5°."""
    import rti_oracle as o

    G = 10
    u, v = grid_dirs(G)
    B = o.hsh_basis(u, v, 3)
    for tilt in (0, 15, 30):
        worst = 0.0
        for az in AZIMUTHS:
            n, c = lambertian_case(tilt, az)
            got, kind, _ = peak_normal((B @ c).astype(np.float32), G)
            assert kind == 0
            worst = max(worst, float(np.degrees(np.arccos(np.clip(got.astype(np.float64) @ n, -1, 1)))))
        print(f"tilt {tilt}: worst angular error {worst:.2f} deg")
        assert worst <= ACCURACY_BOUND_DEG, (tilt, worst)


def test_python_layer_rejects_cpu_tensors_wrong_shapes_and_other_bases():
    import torch

    m = torch.zeros((3, 4, 4, 16))
    q = rti.QuantisedHSH(torch.zeros((4, 4, 3, 16), dtype=torch.uint8), torch.ones(32), "hsh16")
    with pytest.raises(ValueError, match="CUDA"):
        rti.hsh_normals(m)
    with pytest.raises(ValueError, match="CUDA"):
        rti.hsh8_normals(q)
    with pytest.raises(ValueError, match="QuantisedHSH"):
        rti.hsh8_normals(m)
    with pytest.raises(ValueError, match="CUDA"):
        rti.hsh_normals_into(m, torch.zeros(16, dtype=torch.uint8), torch.zeros((16, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.hsh8_normals_into(q.coef, q.qparams, torch.zeros(16, dtype=torch.uint8), torch.zeros((16, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        rti.peak_table("hsh16", 10, "cpu")
    with pytest.raises(NotImplementedError):
        rti.peak_table("ptm", 10, "cuda")
    with pytest.raises(ValueError, match="grid"):
        rti.peak_table("hsh16", 17, "cuda")
    # the PTM entries keep refusing HSH
    assert rti.load().rti_ptm_normals(P_, L.RTI_F32, H16, 0, 64, P_, 0, None, None, None) == L.RTI_ERR_UNSUPPORTED
