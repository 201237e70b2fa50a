"""Multi-light detail enhancement on the GPU (rti_multilight.hip) against tests/multilight_ref.py and, bit for bit,
against rti.relight.

Shapes (multilight_ref.SHAPES): one pixel; exactly one tile; partial tiles in both axes at T = 8 and 16; an image lower
than a tile; a last tile one pixel wide and one pixel high, which has no pairs; T = 32, four pixels per lane, with
partial tiles.  Every map carries relight_ref's planted pixels (NaN, ±inf, the int32 edges), which the search leaves out
when they are not finite.

The scores are held to the header's bound, which is derived: a candidate's values are bit-exact, a difference of two of
them is exact in fp64, each square is rounded once, the n terms are summed in some order (at most n − 1 roundings on any
path) and divided once, against a reference that is the correctly rounded sum of the same squares.  The field and the
relight have no sum whose order could differ: they are compared for equality."""
import numpy as np
import pytest
import torch

import rti
from multilight_ref import (BASES, CANDIDATE_COUNTS, SHAPES, bilinear_ref, candidates, constant_term_maps, field_ref,
                            image_maps, relight_field_ref, same_bits, scores_ref, scores_within_bound, tile_grid)
from relight_ref import TERMS

pytestmark = pytest.mark.gpu

LAYOUTS = ["pixel", "planar"]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]
MAIN = (0.25, -0.4)


def name_of(dt):
    return str(dt).replace("torch.", "")


def on_device(cuda, m, H, W, layout, offset=False):
    """m fp32 [C, P, k] -> the device maps [H, W, k] / [3, H, W, k] (planar: [k, H, W] / [3, k, H, W]); offset: they start
    one element into a 16-byte aligned buffer."""
    C, P, k = m.shape
    a = m.reshape(C, H, W, k) if layout == "pixel" else np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(C, k, H, W)
    a = a if C == 3 else a[0]
    t = torch.as_tensor(np.array(a, order="C"), device=cuda)  # a copy: the cached maps are read-only
    if not offset:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=cuda)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def bits(t):
    t = t.contiguous()
    return t if t.dtype in (torch.uint8, torch.int32) else t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def random_field(H, W, T, seed=3):
    """A tile field with lights inside and outside the unit disc."""
    Ty, Tx = tile_grid(H, W, T)
    return np.random.default_rng(seed).uniform(-0.8, 0.8, (Ty, Tx, 2)).astype(np.float32)


# ---- rti_light_scores ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_T%d" % s)
def test_scores_against_the_reference(cuda, shape, basis):
    H, W, T = shape
    luv = candidates(17)
    worst = 0.0
    for C in (1, 3):
        m = image_maps(H, W, TERMS[basis], C)
        ref = scores_ref(m, H, W, T, luv, basis)
        first = None
        for layout in LAYOUTS:
            for offset in (False, True):
                coef = on_device(cuda, m, H, W, layout, offset)
                scores, count = rti.light_scores(coef, luv, basis, tile=T, layout=layout)
                assert scores.shape == ref["scores"].shape and scores.dtype == torch.float64
                assert np.array_equal(count.cpu().numpy(), ref["count"]), (C, layout, offset)
                ok, w = scores_within_bound(scores.cpu().numpy(), ref)
                worst = max(worst, w)
                print(f"{shape} {basis} C={C} {layout} offset={offset}: worst error {w:.3f} of its bound")
                assert ok, (C, layout, offset, w)
                again, _ = rti.light_scores(coef, luv, basis, tile=T, layout=layout)
                assert torch.equal(bits(scores), bits(again)), "two calls differ"
                first = scores if first is None else first
                assert torch.equal(bits(scores), bits(first)), "the layout or the alignment changed the bits"
        assert H * W < 26 or int(ref["count"].sum()) < H * W  # the planted non-finite pixels are left out
    print(f"{shape} {basis}: worst error {worst:.3f} of its bound")


@pytest.mark.parametrize("E", CANDIDATE_COUNTS)
def test_scores_candidate_counts(cuda, E):
    H, W, T = 19, 37, 8
    luv = candidates(E)
    for basis, C in (("ptm", 3), ("hsh16", 1), ("hsh9", 3)):
        m = image_maps(H, W, TERMS[basis], C)
        ref = scores_ref(m, H, W, T, luv, basis)
        scores, count = rti.light_scores(on_device(cuda, m, H, W, "pixel"), luv, basis, tile=T)
        assert scores.shape == (3, 5, E, 2) and np.array_equal(count.cpu().numpy(), ref["count"])
        ok, w = scores_within_bound(scores.cpu().numpy(), ref)
        print(f"E={E} {basis} C={C}: worst error {w:.3f} of its bound")
        assert ok, (basis, C, w)
    with pytest.raises(ValueError, match="64 candidates"):
        rti.light_scores(on_device(cuda, m, H, W, "pixel"), np.zeros((65, 2)), basis, tile=T)


def test_luminance_weights(cuda):
    H, W, T, basis = 19, 37, 16, "hsh9"
    luv, w = candidates(5), (0.2, 0.7, 0.1)
    m = image_maps(H, W, 9, 3)
    ref = scores_ref(m, H, W, T, luv, basis, w)
    scores, _ = rti.light_scores(on_device(cuda, m, H, W, "planar"), luv, basis, tile=T, layout="planar", weights=w)
    assert scores_within_bound(scores.cpu().numpy(), ref)[0]
    assert not scores_within_bound(scores.cpu().numpy(), scores_ref(m, H, W, T, luv, basis))[0]


def test_an_all_nan_tile_scores_zero_and_takes_the_main_light(cuda):
    H, W, T, basis = 19, 37, 8, "ptm"
    luv = candidates(17)
    m = image_maps(H, W, 6, 1).copy().reshape(1, H, W, 6)
    m[0, 8:16, 16:24] = np.nan  # tile (1, 2)
    m = m.reshape(1, H * W, 6)
    ref = scores_ref(m, H, W, T, luv, basis)
    assert ref["count"][1, 2] == 0
    scores, count = rti.light_scores(on_device(cuda, m, H, W, "pixel"), luv, basis, tile=T)
    assert int(count[1, 2]) == 0 and bool((scores[1, 2] == 0).all()) and np.array_equal(count.cpu().numpy(), ref["count"])
    assert scores_within_bound(scores.cpu().numpy(), ref)[0]
    field, choice = rti.light_field(scores, count, luv, *MAIN, smooth=0, return_choice=True)
    assert int(choice[1, 2]) == -1 and bool((choice.flatten()[choice.flatten() != -1] >= 0).all())
    assert same_bits(field[1, 2].cpu().numpy(), np.float32(MAIN))


# ---- rti_light_field -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(8, 8, 8), (19, 37, 8), (33, 70, 32), (17, 33, 16)], ids=lambda s: "%dx%d_T%d" % s)
def test_field_equals_the_restatement_on_the_kernels_scores(cuda, shape):
    H, W, T = shape
    for basis, E in (("ptm", 17), ("hsh16", 64)):
        luv = candidates(E)
        scores, count = rti.light_scores(on_device(cuda, image_maps(H, W, TERMS[basis], 3), H, W, "pixel"), luv, basis, tile=T)
        s, c = scores.cpu().numpy(), count.cpu().numpy()
        for smooth in (0, 1, 8):
            for ws, wb in ((1.0, 0.5), (0.0, 1.0), (2.5, 0.0)):
                field, choice = rti.light_field(scores, count, luv, *MAIN, ws=ws, wb=wb, smooth=smooth, return_choice=True)
                want_field, want_choice = field_ref(s, c, luv, ws, wb, *MAIN, smooth)
                assert np.array_equal(choice.cpu().numpy(), want_choice), (basis, smooth, ws, wb)
                assert same_bits(field.cpu().numpy(), want_field), (basis, smooth, ws, wb)
        assert field.shape == tile_grid(H, W, T) + (2,) and field.dtype == torch.float32


@pytest.mark.parametrize("basis", BASES)
def test_equal_scores_choose_the_first_candidate(cuda, basis):
    H, W, T = 17, 33, 16
    luv = candidates(17)
    m = constant_term_maps(H, W, TERMS[basis])
    scores, count = rti.light_scores(on_device(cuda, m, H, W, "pixel"), luv, basis, tile=T)
    assert bool((scores == scores[:, :, :1]).all()) and bool((scores[1, 2, :, 0] == 0).all())
    assert scores_within_bound(scores.cpu().numpy(), scores_ref(m, H, W, T, luv, basis))[0]
    field, choice = rti.light_field(scores, count, luv, *MAIN, smooth=0, return_choice=True)
    assert bool((choice == 0).all())
    assert same_bits(field.cpu().numpy(), np.broadcast_to(luv[0].astype(np.float32), (2, 3, 2)))


# ---- rti_relight_field -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_T%d" % s)
def test_relight_under_a_tile_field(cuda, shape, basis):
    """Every output type equals the restatement (bilinear in fp64, then relight_ref's chain per pixel); layouts, an odd
    base pointer and C = 3 against C = 1 give the same bits."""
    H, W, T = shape
    k = TERMS[basis]
    m = image_maps(H, W, k, 3)
    f = random_field(H, W, T)
    field = torch.as_tensor(f, device=cuda)
    lu, lv = bilinear_ref(f, H, W, T)
    for dt in OUT_DTYPES:
        want = relight_field_ref(m, lu, lv, basis, name_of(dt)).reshape(H, W, 3)
        for layout in LAYOUTS:
            for offset in (False, True):
                got = rti.relight_field(on_device(cuda, m, H, W, layout, offset), field, basis, tile=T, layout=layout,
                                        out_dtype=dt)
                assert got.dtype == dt and same_bits(got.cpu().numpy(), want), (dt, layout, offset)
            for c in range(3):
                one = rti.relight_field(on_device(cuda, m[c:c + 1], H, W, layout), field, basis, tile=T, layout=layout,
                                        out_dtype=dt)
                assert one.shape == (H, W) and same_bits(one.cpu().numpy(), want[..., c]), (dt, layout, c)


@pytest.mark.parametrize("basis", BASES)
def test_a_constant_field_is_the_plain_relight(cuda, basis):
    H, W, T = 19, 37, 16
    m = image_maps(H, W, TERMS[basis], 3)
    coef = on_device(cuda, m, H, W, "pixel")
    for lu, lv in ((0.3, -0.45), (0.0, 0.0), (0.8, 0.75)):
        field = torch.empty(tile_grid(H, W, T) + (2,), dtype=torch.float32, device=cuda)
        field[..., 0], field[..., 1] = lu, lv
        f32 = field[0, 0].cpu().numpy()
        for dt in OUT_DTYPES:
            got = rti.relight_field(coef, field, basis, tile=T, out_dtype=dt)
            for c in range(3):
                want = rti.relight(coef[c], float(f32[0]), float(f32[1]), basis, out_dtype=dt)
                assert same_bits(got[..., c].cpu().numpy(), want.cpu().numpy()), (lu, lv, dt, c)


@pytest.mark.parametrize("basis", BASES)
def test_lights_per_pixel_are_the_diagonal_of_relight(cuda, basis):
    """The PIXELS form with P lights equals the diagonal of rti.relight called with those P directions; a light that is
    not finite gives NaN, INT32_MIN and 0."""
    H, W = 19, 37
    P = H * W
    m = image_maps(H, W, TERMS[basis], 3)
    light = np.random.default_rng(8).uniform(-0.9, 0.9, (H, W, 2)).astype(np.float32)
    light[2, 3], light[4, 5, 1], light[6, 7, 0] = (0.0, 0.0), np.nan, -np.inf
    bad = ~np.isfinite(light).all(-1)
    lu, lv = light[..., 0].reshape(-1).astype(np.float64), light[..., 1].reshape(-1).astype(np.float64)
    finite_lu, finite_lv = np.where(bad.reshape(-1), 0.0, lu), np.where(bad.reshape(-1), 0.0, lv)
    dev_light = torch.as_tensor(light, device=cuda)
    for layout in LAYOUTS:
        coef = on_device(cuda, m, H, W, layout)
        for dt in OUT_DTYPES:
            got = rti.relight_field(coef, dev_light, basis, layout=layout, out_dtype=dt).cpu().numpy()
            assert same_bits(got, relight_field_ref(m, lu, lv, basis, name_of(dt)).reshape(H, W, 3)), (layout, dt)
            for c in range(3):
                full = rti.relight(coef[c], finite_lu, finite_lv, basis, layout=layout, out_dtype=dt)  # [P, H, W]
                diag = full.reshape(P, P).diagonal().reshape(H, W).cpu().numpy()
                assert same_bits(got[..., c][~bad], diag[~bad]), (layout, dt, c)
            blank = {torch.float32: np.nan, torch.int32: -2 ** 31, torch.uint8: 0}[dt]
            assert (np.isnan(got[bad]) if dt == torch.float32 else got[bad] == blank).all(), (layout, dt)


def test_a_padded_channel_stride_gives_the_same_bits(cuda):
    H, W, T, basis = 19, 37, 8, "hsh9"
    P, k = H * W, 9
    m = image_maps(H, W, k, 3)
    luv = candidates(17)
    dense = on_device(cuda, m, H, W, "pixel")
    field = torch.as_tensor(random_field(H, W, T), device=cuda)
    for pad in (1, 6):  # a stride that is a multiple of 4 elements (the 16-byte pieces stay), and one that is not
        buf = torch.full((3, P * k + pad), float("nan"), device=cuda)
        far = buf[:, :P * k].view(3, H, W, k)
        far.copy_(dense)
        assert not far.is_contiguous() and far.stride(0) == P * k + pad
        s0, c0 = torch.empty((3, 5, 17, 2), dtype=torch.float64, device=cuda), torch.empty((3, 5), dtype=torch.int32, device=cuda)
        s1, c1 = torch.empty_like(s0), torch.empty_like(c0)
        rti.light_scores_into(dense, luv, s0, c0, basis=basis, tile=T)
        rti.light_scores_into(far, luv, s1, c1, basis=basis, tile=T)
        assert torch.equal(bits(s0), bits(s1)) and torch.equal(c0, c1), pad
        for dt in OUT_DTYPES:
            o0, o1 = (torch.empty((H, W, 3), dtype=dt, device=cuda) for _ in range(2))
            rti.relight_field_into(dense, field, o0, basis=basis, tile=T)
            rti.relight_field_into(far, field, o1, basis=basis, tile=T)
            assert same_bits(o0.cpu().numpy(), o1.cpu().numpy()), (pad, dt)


# ---- end to end and the ops ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("basis", BASES)
def test_relight_multilight_is_the_three_calls_composed(cuda, basis):
    H, W, T = 33, 70, 16
    m = image_maps(H, W, TERMS[basis], 3)
    for layout in LAYOUTS:
        coef = on_device(cuda, m, H, W, layout)
        for maps_ in (coef, coef[1].contiguous()):
            luv = rti.light_candidates(*MAIN, radius=0.25, rings=3, per_ring=6)
            scores, count = rti.light_scores(maps_, luv, basis, tile=T, layout=layout)
            field = rti.light_field(scores, count, luv, *MAIN, ws=1.0, wb=0.25, smooth=1)
            want = rti.relight_field(maps_, field, basis, tile=T, layout=layout, out_dtype=torch.uint8)
            got, used = rti.relight_multilight(maps_, *MAIN, basis, tile=T, radius=0.25, rings=3, per_ring=6, wb=0.25,
                                               smooth=1, layout=layout, out_dtype=torch.uint8, return_field=True)
            assert torch.equal(got, want) and torch.equal(bits(used), bits(field))
            assert got.shape == ((H, W, 3) if maps_.dim() == 4 else (H, W)) and int(got.max()) > int(got.min())
            plain = rti.relight_multilight(maps_, *MAIN, basis, tile=T, layout=layout)
            assert plain.dtype == torch.float32 and plain.shape == got.shape
    with pytest.raises(ValueError, match="tile"):
        rti.relight_multilight(coef, *MAIN, basis, tile=12, layout=layout)
    with pytest.raises(ValueError, match="light must be"):
        rti.relight_field(coef, field[:, :-1], basis, tile=T, layout=layout)
    with pytest.raises(ValueError):
        rti.relight_field(coef, field, basis, tile=T, layout=layout, out_dtype=torch.float64)


@pytest.mark.parametrize("basis", BASES)
def test_torch_ops(cuda, basis):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    H, W, T = 19, 37, 8
    b = rti.basis_id(basis)
    m = image_maps(H, W, TERMS[basis], 3)
    luv = rti.light_candidates(*MAIN)
    luv_t = torch.as_tensor(luv)
    checks = ("test_schema", "test_faketensor")
    for planar in (False, True):
        layout = "planar" if planar else "pixel"
        for coef in (on_device(cuda, m, H, W, layout), on_device(cuda, m[:1], H, W, layout)):
            args = (coef, luv_t, b, T, planar)
            scores, count = torch.ops.rti.light_scores(*args)
            want_s, want_c = rti.light_scores(coef, luv, basis, tile=T, layout=layout)
            assert torch.equal(bits(scores), bits(want_s)) and torch.equal(count, want_c)
            torch.library.opcheck(torch.ops.rti.light_scores.default, args, test_utils=checks)
            args = (scores, count, luv_t, *MAIN, 1.0, 0.5, 2)
            field = torch.ops.rti.light_field(*args)
            assert torch.equal(bits(field), bits(rti.light_field(scores, count, luv, *MAIN)))
            torch.library.opcheck(torch.ops.rti.light_field.default, args, test_utils=checks)
            light = torch.as_tensor(np.random.default_rng(1).uniform(-0.7, 0.7, (H, W, 2)).astype(np.float32), device=cuda)
            for dt in OUT_DTYPES:
                for l, tile in ((field, T), (light, 0)):
                    args = (coef, l, b, tile, planar, dt)
                    got = torch.ops.rti.relight_field(*args)
                    want = rti.relight_field(coef, l, basis, tile=tile or None, layout=layout, out_dtype=dt)
                    assert got.dtype == dt and got.shape == want.shape and torch.equal(bits(got), bits(want))
                    torch.library.opcheck(torch.ops.rti.relight_field.default, args, test_utils=checks)
    with pytest.raises(ValueError):
        torch.ops.rti.light_scores(coef, luv_t, b, 12)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_field(coef, field.cpu(), b, T)
