"""rti_light_scores / rti_light_field / rti_relight_field without a GPU: the symbols and signatures are there, every
argument check answers before any HIP call (the device pointers below are never dereferenced; luv and w are real host
arrays, the entries read them) with a message that names the function, light_candidates holds its contract, the Python
layer refuses what it documents, and the NumPy reference alone holds the identities of the header."""
import ctypes

import numpy as np
import pytest

import rti
from multilight_ref import (BASES, MAX_CANDIDATES, bilinear_ref, candidates, constant_term_maps, field_ref, image_maps,
                            relight_field_ref, same_bits, scores_ref, tile_grid)
from relight_ref import TERMS, relight_ref
from rti import _lib as L

P_ = ctypes.c_void_p(4096)   # aligned for every vector access
ODD = ctypes.c_void_p(4098)  # 2 bytes off a dword
PTM, H16, H9 = L.RTI_BASIS_PTM6, L.RTI_BASIS_HSH16, L.RTI_BASIS_HSH9
H_, W_ = 19, 37


def luv_of(values):
    a = np.ascontiguousarray(values, np.float64)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a  # the array is kept alive by the caller


def w_of(values):
    a = np.ascontiguousarray(values, np.float32)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a


LUV, _LUV_KEEP = luv_of([[0.3, -0.45]] * MAX_CANDIDATES + [[0.0, 0.0]])  # one spare: E = 65 is refused before it is read
BAD_LUV = {name: luv_of([[0.1, 0.2], pair]) for name, pair in
           {"nan lu": [np.nan, 0.0], "inf lv": [0.0, np.inf], "-inf lu": [-np.inf, 0.0]}.items()}
BAD_W = {name: w_of(v) for name, v in {"nan weight": [0.3, np.nan, 0.1], "inf weight": [np.inf, 0.5, 0.1]}.items()}
WS_BYTES = 32 * 3 * 5  # rti_light_field_workspace_bytes(3, 5)


def scores_call(coef=P_, basis=PTM, layout=0, C=3, stride=0, H=H_, W=W_, T=16, w=None, luv=LUV, E=17, scores=P_, count=P_):
    return rti.load().rti_light_scores(coef, basis, layout, C, stride, H, W, T, w, luv, E, scores, count, None)


def field_call(scores=P_, count=P_, Ty=3, Tx=5, luv=LUV, E=17, ws=1.0, wb=0.5, lu0=0.3, lv0=-0.45, smooth=2,
               workspace=P_, nbytes=WS_BYTES, field=P_, choice=P_):
    return rti.load().rti_light_field(scores, count, Ty, Tx, luv, E, ws, wb, lu0, lv0, smooth, workspace, nbytes, field,
                                      choice, None)


def relight_call(coef=P_, basis=PTM, layout=0, C=3, stride=0, H=H_, W=W_, light=P_, form=L.RTI_LIGHT_TILES, T=16,
                 out=P_, odt=L.RTI_F32):
    return rti.load().rti_relight_field(coef, basis, layout, C, stride, H, W, light, form, T, out, odt, None)


MAPS_BAD = {
    "null coef": dict(coef=None), "H = 0": dict(H=0), "W = 0": dict(W=0), "H < 0": dict(H=-3), "W < 0": dict(W=-1),
    "H*W = 2^31": dict(H=1 << 16, W=1 << 15), "C = 0": dict(C=0), "C = 2": dict(C=2), "C = 4": dict(C=4),
    "coef layout": dict(layout=2), "coef layout < 0": dict(layout=-1),
    "stride below dense, ptm": dict(stride=H_ * W_ * 6 - 1), "stride below dense, hsh16": dict(basis=H16, stride=H_ * W_ * 16 - 1),
    "stride below dense, planar": dict(layout=1, basis=H9, stride=100), "stride < 0": dict(stride=-1),
}
SCORES_BAD = dict(MAPS_BAD, **{
    "null luv": dict(luv=None), "null scores": dict(scores=None), "T = 12": dict(T=12), "T = 0": dict(T=0),
    "T = 64": dict(T=64), "T < 0": dict(T=-8), "E = 0": dict(E=0), "E < 0": dict(E=-1), "E = 65": dict(E=MAX_CANDIDATES + 1),
    "scores off 8 bytes": dict(scores=ODD),
})
SCORES_BAD.update({f"luv: {name}": dict(luv=ptr, E=2) for name, (ptr, _) in BAD_LUV.items()})
SCORES_BAD.update({name: dict(w=ptr) for name, (ptr, _) in BAD_W.items()})
FIELD_BAD = {
    "null scores": dict(scores=None), "null count": dict(count=None), "null luv": dict(luv=None),
    "null workspace": dict(workspace=None), "null field": dict(field=None), "Ty = 0": dict(Ty=0), "Tx = 0": dict(Tx=0),
    "Ty < 0": dict(Ty=-1), "E = 0": dict(E=0), "E = 65": dict(E=MAX_CANDIDATES + 1), "negative ws": dict(ws=-0.5),
    "negative wb": dict(wb=-1e-9), "nan ws": dict(ws=np.nan), "inf wb": dict(wb=np.inf), "nan lu0": dict(lu0=np.nan),
    "inf lv0": dict(lv0=-np.inf), "smooth = 9": dict(smooth=9), "smooth < 0": dict(smooth=-1),
    "workspace too small": dict(nbytes=WS_BYTES - 1), "workspace of nothing": dict(nbytes=0),
    "workspace off 8 bytes": dict(workspace=ODD), "scores off 8 bytes": dict(scores=ODD),
}
FIELD_BAD.update({f"luv: {name}": dict(luv=ptr, E=2) for name, (ptr, _) in BAD_LUV.items()})
RELIGHT_BAD = dict(MAPS_BAD, **{
    "null light": dict(light=None), "null out": dict(out=None), "light form": dict(form=2), "light form < 0": dict(form=-1),
    "T = 12": dict(T=12), "T = 0, tiles": dict(T=0), "light off 4 bytes": dict(light=ODD),
})
UNSUPPORTED = {"unknown basis": dict(basis=7), "basis < 0": dict(basis=-1)}
RELIGHT_UNSUPPORTED = dict(UNSUPPORTED, **{"f64 out": dict(odt=L.RTI_F64), "unknown out dtype": dict(odt=9),
                                           "out dtype < 0": dict(odt=-1)})


def answers(call, cases, case, status, name):
    assert call(**cases[case]) == status, case
    msg = rti.load().rti_last_error()
    assert name in msg and len(msg) > len(name), msg


@pytest.mark.parametrize("case", sorted(SCORES_BAD))
def test_light_scores_bad_arguments(case):
    answers(scores_call, SCORES_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_light_scores")


@pytest.mark.parametrize("case", sorted(FIELD_BAD))
def test_light_field_bad_arguments(case):
    answers(field_call, FIELD_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_light_field")


@pytest.mark.parametrize("case", sorted(RELIGHT_BAD))
def test_relight_field_bad_arguments(case):
    answers(relight_call, RELIGHT_BAD, case, L.RTI_ERR_BAD_ARG, b"rti_relight_field")


@pytest.mark.parametrize("case", sorted(RELIGHT_UNSUPPORTED))
def test_unsupported(case):
    answers(relight_call, RELIGHT_UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_relight_field")
    if case in UNSUPPORTED:
        answers(scores_call, UNSUPPORTED, case, L.RTI_ERR_UNSUPPORTED, b"rti_light_scores")


def test_what_may_be_null_or_unused():
    """C = 1 never uses its channel stride and the PIXELS form never reads T: such a call passes that check and goes on
    to the next one it fails."""
    assert scores_call(C=1, stride=5, T=12) == L.RTI_ERR_BAD_ARG and b"tile" in rti.load().rti_last_error()
    assert relight_call(form=L.RTI_LIGHT_PIXELS, T=12, odt=L.RTI_F64) == L.RTI_ERR_UNSUPPORTED
    assert b"out dtype" in rti.load().rti_last_error()


def test_symbols_constants_and_exports():
    lib = rti.load()
    for name, n in (("rti_light_scores", 14), ("rti_light_field_workspace_bytes", 2), ("rti_light_field", 16),
                    ("rti_relight_field", 13)):
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert len(L.SIGNATURES[name][1]) == n, name
    assert (L.RTI_LIGHT_MAX_CANDIDATES, L.RTI_LIGHT_TILES, L.RTI_LIGHT_PIXELS) == (MAX_CANDIDATES, 0, 1)
    assert lib.rti_light_field_workspace_bytes(3, 5) == WS_BYTES
    assert lib.rti_light_field_workspace_bytes(0, 5) == 0 and lib.rti_light_field_workspace_bytes(3, -1) == 0
    for name in ("light_candidates", "light_scores", "light_scores_into", "light_field", "light_field_into",
                 "light_field_workspace", "relight_field", "relight_field_into", "relight_multilight"):
        assert callable(getattr(rti, name)) and callable(getattr(rti.api, name)) and name in rti.__all__, name
    from rti import ops  # noqa: F401  registers torch.ops.rti.*
    import torch

    for name in ("light_scores", "light_field", "relight_field"):
        assert callable(getattr(torch.ops.rti, name)), name


def test_light_candidates_contract():
    c = rti.light_candidates(0.25, -0.4)
    assert c.dtype == np.float64 and c.shape == (17, 2) and tuple(c[0]) == (0.25, -0.4)
    r = np.hypot(c[1:, 0] - 0.25, c[1:, 1] + 0.4)
    assert np.allclose(r[:8], 0.15, rtol=0, atol=1e-15) and np.allclose(r[8:], 0.3, rtol=0, atol=1e-15)
    assert np.allclose(c[1], (0.4, -0.4), rtol=0, atol=1e-15)  # angle 0 first
    assert np.allclose(c[3], (0.25, -0.25), rtol=0, atol=1e-15)  # then counter-clockwise in (lu, lv)
    assert rti.light_candidates(0.1, 0.2, rings=0).shape == (1, 2)
    assert rti.light_candidates(0.1, 0.2, rings=7, per_ring=9).shape == (64, 2)
    # near and beyond the rim every point lies inside the unit disc, the main light still first
    for lu, lv in ((0.9, 0.3), (0.0, -1.0), (0.8, 0.75), (-0.6, 0.8)):
        c = rti.light_candidates(lu, lv, radius=0.5, rings=3, per_ring=12)
        assert c.shape == (37, 2) and (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] <= 1.0).all(), (lu, lv)
        n = max(1.0, np.hypot(lu, lv))
        assert np.allclose(c[0], (lu / n, lv / n), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="64 candidates"):
        rti.light_candidates(0.1, 0.2, rings=8, per_ring=8)
    for kw in (dict(radius=-0.1), dict(radius=np.nan), dict(rings=-1), dict(per_ring=0)):
        with pytest.raises(ValueError):
            rti.light_candidates(0.1, 0.2, **kw)
    with pytest.raises(ValueError):
        rti.light_candidates(np.inf, 0.2)


def test_python_layer_refusals():
    import torch

    c3, c1 = torch.zeros((3, 19, 37, 6)), torch.zeros((19, 37, 6))
    luv = rti.light_candidates(0.1, 0.2)
    scores, count = torch.zeros((2, 3, 17, 2), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.int32)
    field = torch.zeros((2, 3, 2))
    for tile in (12, 0, 64, True, 16.5):
        with pytest.raises(ValueError, match="tile"):
            rti.light_scores(c3, luv, tile=tile)
        with pytest.raises(ValueError, match="tile"):
            rti.relight_field(c3, field, tile=tile)
        with pytest.raises(ValueError, match="tile"):
            rti.relight_multilight(c3, 0.1, 0.2, tile=tile)
    with pytest.raises(ValueError, match="64 candidates"):
        rti.light_scores(c3, np.zeros((65, 2)))
    with pytest.raises(ValueError, match="64 candidates"):
        rti.light_field(scores, count, np.zeros((65, 2)), 0.1, 0.2)
    with pytest.raises(ValueError, match="64 candidates"):
        rti.relight_multilight(c3, 0.1, 0.2, rings=8, per_ring=8)
    with pytest.raises(ValueError, match=r"\[E, 2\]"):
        rti.light_scores(c3, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="finite"):
        rti.light_scores(c3, np.array([[0.1, np.nan]]))
    # no CPU path
    for call in (lambda: rti.light_scores(c3, luv), lambda: rti.light_scores(c1, luv, tile=8),
                 lambda: rti.light_field(scores, count, luv, 0.1, 0.2),
                 lambda: rti.relight_field(c3, field, tile=16), lambda: rti.relight_field(c1, torch.zeros((19, 37, 2))),
                 lambda: rti.relight_multilight(c3, 0.1, 0.2),
                 lambda: rti.relight_field_into(c3, field, torch.zeros((19, 37, 3)), tile=16),
                 lambda: rti.light_scores_into(c3, luv, scores)):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="layout"):
        rti.light_scores(c3, luv, layout="rows")
    with pytest.raises(ValueError, match="basis"):
        rti.relight_multilight(c3, 0.1, 0.2, basis="rbf")
    for kw in (dict(ws=-1.0), dict(wb=np.nan), dict(smooth=9), dict(smooth=-1), dict(smooth=1.5)):
        with pytest.raises(ValueError, match="ws|smooth"):
            rti.light_field(scores, count, luv, 0.1, 0.2, **kw)
    with pytest.raises(ValueError, match="main light"):
        rti.light_field(scores, count, luv, np.nan, 0.2)


# ---- the reference alone -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("basis", BASES)
def test_a_constant_field_reproduces_relight_ref(basis):
    H, W, T, k = 19, 37, 8, TERMS[basis]
    m = image_maps(H, W, k, 3)
    Ty, Tx = tile_grid(H, W, T)
    for lu, lv in ((0.3, -0.45), (0.0, 0.0), (0.8, 0.75)):
        field = np.empty((Ty, Tx, 2), np.float32)
        field[...] = (lu, lv)
        fu, fv = bilinear_ref(field, H, W, T)
        assert same_bits(fu, np.full(H * W, np.float64(np.float32(lu)))) and same_bits(fv, np.full(H * W, np.float64(np.float32(lv))))
        got = relight_field_ref(m, fu, fv, basis)
        for c in range(3):
            want = relight_ref(m[c], [float(np.float32(lu))], [float(np.float32(lv))], basis)[0]
            assert same_bits(got[:, c], want), (basis, lu, lv, c)
        assert np.isnan(got).any() and np.isfinite(got).any()
    # a light that is not finite gives NaN, INT32_MIN and 0
    fu[3], fv[5] = np.nan, np.inf
    for name, want in (("float32", np.nan), ("int32", -2 ** 31), ("uint8", 0)):
        got = relight_field_ref(m, fu, fv, basis, name)
        assert got.dtype == np.dtype(name) and got.shape == (H * W, 3)
        for p in (3, 5):
            assert (np.isnan(got[p]) if name == "float32" else got[p] == want).all(), (name, p)


def test_bilinear_interpolates_between_tile_centres():
    H, W, T = 17, 33, 8
    Ty, Tx = tile_grid(H, W, T)
    field = np.zeros((Ty, Tx, 2), np.float32)
    field[..., 0] = np.arange(Tx, dtype=np.float32)[None, :]
    field[..., 1] = np.arange(Ty, dtype=np.float32)[:, None]
    fu, fv = (x.reshape(H, W) for x in bilinear_ref(field, H, W, T))
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    assert np.array_equal(fu[0], np.clip((x - 3.5) / 8.0, 0.0, Tx - 1)) and (fu == fu[0]).all()
    assert np.array_equal(fv[:, 0], np.clip((y - 3.5) / 8.0, 0.0, Ty - 1)) and (fv.T == fv[:, 0]).all()


@pytest.mark.parametrize("basis", BASES)
def test_a_constant_term_map_scores_every_candidate_alike(basis):
    H, W, T, k = 17, 33, 16, TERMS[basis]
    m = constant_term_maps(H, W, k)
    luv = candidates(17)
    r = scores_ref(m, H, W, T, luv, basis)
    assert (r["scores"] == r["scores"][:, :, :1]).all() and (r["scores"][..., 1] > 0).all()
    assert r["pairs"].tolist() == [[2 * 16 * 15, 2 * 16 * 15, 15], [15, 15, 0]]  # the corner tile is one pixel
    assert (r["scores"][1, 2, :, 0] == 0).all() and (r["scores"][0, 0, :, 0] > 0).all()
    assert r["count"].tolist() == [[256, 256, 16], [16, 16, 1]]
    field, choice = field_ref(r["scores"], r["count"], luv, 1.0, 0.5, 0.9, 0.1, 0)
    assert (choice == 0).all() and same_bits(field, np.broadcast_to(luv[0].astype(np.float32), field.shape))


def test_field_reference_semantics():
    luv = candidates(5)
    scores = np.zeros((2, 3, 5, 2))
    count = np.ones((2, 3), np.int32)
    scores[0, 0, :, 0] = [1.0, 4.0, 2.0, 4.0, 0.5]        # a tie between 1 and 3 -> 1
    scores[0, 1, :, 1] = [-3.0, -1.0, -2.0, -5.0, -4.0]   # no positive brightness: all scores 0 -> 0
    scores[0, 2, :, 0] = [np.nan, 1.0, np.nan, 3.0, 2.0]  # NaN never wins and never becomes the maximum
    scores[1, 0, :, 0] = [np.nan, np.nan, 2.0, np.nan, np.nan]
    scores[1, 1, :, 0] = [9.0, 1.0, 1.0, 1.0, 1.0]
    count[1, 1] = 0                                        # an empty tile -> the main light
    scores[1, 2, :, 0], scores[1, 2, :, 1] = [1.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 4.0]  # wb decides
    field, choice = field_ref(scores, count, luv, 1.0, 0.5, 0.9, 0.1, 0)
    assert choice.tolist() == [[1, 0, 3], [2, -1, 0]]
    assert field_ref(scores, count, luv, 1.0, 2.0, 0.9, 0.1, 0)[1][1, 2] == 4
    assert same_bits(field[1, 1], np.float32([0.9, 0.1])) and same_bits(field[0, 2], luv[3].astype(np.float32))
    # smoothing: a constant field stays, the mean of the binomial weights is kept, 8 passes flatten
    flat = field_ref(np.ones((4, 5, 5, 2)), np.ones((4, 5), np.int32), luv, 1.0, 0.5, 0.9, 0.1, 8)[0]
    assert same_bits(flat, np.broadcast_to(luv[0].astype(np.float32), flat.shape))
    one = field_ref(scores, count, luv, 1.0, 0.5, 0.9, 0.1, 1)[0].astype(np.float64)
    f0 = field.astype(np.float64)
    corner = (4 * f0[0, 0] + 2 * f0[0, 1] + 2 * f0[1, 0] + f0[1, 1]) / 9.0
    assert np.allclose(one[0, 0], corner, rtol=1e-6, atol=1e-6)
    spread = [np.ptp(field_ref(scores, count, luv, 1.0, 0.5, 0.9, 0.1, s)[0][..., 0]) for s in (0, 1, 8)]
    assert spread[0] > spread[1] > spread[2] > 0
