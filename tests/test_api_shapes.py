"""The Python layer's argument handling, without a GPU: the stack parse, the coefficient shaping, the
torch ops' fake shapes (literal tables, not the helpers that produce them) and the messages of the checks
that run before any kernel.  The last two groups call the host half of librti.so as tests/test_abi.py does."""
import re

import numpy as np
import pytest
import torch

import rti
import rti.ops  # noqa: F401  registers torch.ops.rti.*
from rti import _lib as L
from rti import api

N, P, C, K = 7, 33, 2, 6
F32, F64, I32 = torch.float32, torch.float64, torch.int32


# ---- no library needed -------------------------------------------------------------------------

@pytest.mark.parametrize("shape,want", [((7, 33), (1, 7, 33, (33,))), ((7, 3, 11), (1, 7, 33, (3, 11))),
                                        ((2, 7, 3, 11), (2, 7, 33, (3, 11)))])
def test_stack_shape(shape, want):
    assert api._stack_shape(torch.empty(shape)) == want


@pytest.mark.parametrize("shape", [(7,), (2, 2, 7, 3, 11)])
def test_stack_shape_rejects_other_ranks(shape):
    with pytest.raises(ValueError, match=re.escape("I must be [N, P], [N, H, W] or [C, N, H, W]")):
        api._stack_shape(torch.empty(shape))


def meta(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="meta")


def stack(batched):
    return meta(C, N, P) if batched else meta(N, P)


def state(batched):
    return meta(C, K + 1, P, dtype=F64) if batched else meta(K + 1, P, dtype=F64)


def coef_shape(batched, planar):
    return ((C,) if batched else ()) + ((K, P) if planar else (P, K))


def described(out):
    return [(tuple(t.shape), t.dtype) for t in (out if isinstance(out, tuple) else (out,))]


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("batched", [False, True])
def test_fake_shapes(batched, planar):
    lead = (C,) if batched else ()
    coef = (coef_shape(batched, planar), F32)
    got = torch.ops.rti.fit_shared(meta(K, N), stack(batched), planar)
    assert described(got) == [coef]
    got = torch.ops.rti.fit_shared_residual(meta(N, K, dtype=F64), meta(K, K, dtype=F64), stack(batched), planar)
    assert described(got) == [coef, (lead + (P,), F32), (lead + (1,), F64)]
    got = torch.ops.rti.fit_robust(meta(N, K, dtype=F64), stack(batched), 1.0, 254.0, K, 0, 0.0, planar)
    assert described(got) == [coef, (lead + (P,), F32), (lead + (P,), I32), ((1,), I32)]
    got = torch.ops.rti.fit_accum_solve(meta(K, K, dtype=F64), state(batched), N, False, planar)
    assert described(got) == [coef, (lead + (P,), F32)]


def test_fake_shapes_spelled_out():
    """The coefficient shapes of the table above as plain numbers, and two residual cases with other sizes."""
    assert described(torch.ops.rti.fit_shared(meta(6, 7), meta(7, 33), False)) == [((33, 6), F32)]
    assert described(torch.ops.rti.fit_shared(meta(6, 7), meta(2, 7, 33), False)) == [((2, 33, 6), F32)]
    assert described(torch.ops.rti.fit_shared(meta(6, 7), meta(7, 33), True)) == [((6, 33), F32)]
    assert described(torch.ops.rti.fit_shared(meta(6, 7), meta(2, 7, 33), True)) == [((2, 6, 33), F32)]
    got = torch.ops.rti.fit_shared_residual(meta(10, 6, dtype=F64), meta(6, 6, dtype=F64), meta(3, 10, 32), True)
    assert described(got) == [((3, 6, 32), F32), ((3, 32), F32), ((3, 1), F64)]
    got = torch.ops.rti.fit_shared_residual(meta(10, 6, dtype=F64), meta(6, 6, dtype=F64), meta(10, 257), False)
    assert described(got) == [((257, 6), F32), ((257,), F32), ((2,), F64)]  # one slot per 256-pixel span


@pytest.mark.parametrize("batched", [False, True])
def test_fake_shape_fit_residual(batched):
    """The op takes [N, P] only; its fake does not validate and reads P off the last axis either way."""
    got = torch.ops.rti.fit_residual(meta(N, K), stack(batched), meta(P, K))
    assert described(got) == [((33,), F32)]


@pytest.mark.parametrize("C_", [1, 2])
def test_coef_helpers(C_):
    sp, k = (2, 3), 6  # P = 6; pixel (1, 2) is p = 5
    pix = api._coef_empty(C_, 6, k, "pixel", F32, "cpu")
    pla = api._coef_empty(C_, 6, k, "planar", F64, "cpu")
    assert (tuple(pix.shape), pix.dtype) == ((C_, 6, 6), F32) and (tuple(pla.shape), pla.dtype) == ((C_, 6, 6), F64)
    pla = api._coef_empty(C_, 6, 4, L.RTI_COEF_PLANAR, F32, "cpu")
    pix = api._coef_empty(C_, 6, 4, L.RTI_COEF_PIXEL_MAJOR, F32, "cpu")
    assert tuple(pix.shape) == (C_, 6, 4) and tuple(pla.shape) == (C_, 4, 6)
    pix.copy_(torch.arange(C_ * 24).reshape(pix.shape))
    pla.copy_(torch.arange(C_ * 24).reshape(pla.shape))
    res = torch.arange(C_ * 6).reshape(C_, 6)
    c = C_ - 1
    out = api._unflatten(pix, sp, True, "pixel")
    assert tuple(out.shape) == (C_, 2, 3, 4) and out[c, 1, 2, 3] == c * 24 + 5 * 4 + 3
    out = api._unflatten(pla, sp, True, "planar")
    assert tuple(out.shape) == (C_, 4, 2, 3) and out[c, 3, 1, 2] == c * 24 + 3 * 6 + 5
    out = api._unflatten(res, sp, True)
    assert tuple(out.shape) == (C_, 2, 3) and out[c, 1, 2] == c * 6 + 5
    # no leading channel axis on the input: channel 0's maps, without it
    out = api._unflatten(pix, sp, False, L.RTI_COEF_PIXEL_MAJOR)
    assert tuple(out.shape) == (2, 3, 4) and out[1, 2, 3] == 23
    out = api._unflatten(pla, sp, False, L.RTI_COEF_PLANAR)
    assert tuple(out.shape) == (4, 2, 3) and out[3, 1, 2] == 23
    out = api._unflatten(res, (6,), False)
    assert tuple(out.shape) == (6,) and out[5] == 5


def raises(text):
    return pytest.raises(ValueError, match=re.escape(text))


def test_messages_before_any_library_call():
    with raises("unknown coefficient layout 'rows' (expected 'pixel' or 'planar')"):
        api._layout_id("rows")
    with raises("unknown basis 'xyz'; expected one of ['hsh', 'hsh16', 'hsh2', 'hsh3', 'hsh9', 'ptm', 'ptm6']"):
        rti.basis_id("xyz")
    with raises("h16 operator of 5 torch.uint8 elements, expected 8 uint8 bytes for k=6, N=8: build it with "
                "rti.h16_operator(pinv) for this light set"):
        api._check_operator(torch.zeros(5, dtype=torch.uint8), 8, "h16", 6, 8)
    with raises("q8 operator of 8 torch.int8 elements, expected 8 uint8 bytes for k=6, N=8: build it with "
                "rti.q8_operator(pinv) for this light set"):
        api._check_operator(torch.zeros(8, dtype=torch.int8), 8, "q8", 6, 8)
    with raises("pixel-major stack needs unit light stride (I[..., p, n] with n contiguous)"):
        api.fit_shared_pm_into(None, torch.zeros(6, 4).t(), None, k=6)
    with raises("I must be a CUDA (HIP) tensor: librti runs only on the GPU, there is no CPU path"):
        rti.fit(torch.zeros(7, 3, 3), np.zeros(7), np.zeros(7))


def test_accumulate_messages():
    I3 = torch.zeros(1, 2, 5)
    R = torch.zeros(2, 6, dtype=F64)
    st = torch.zeros(1, 7, 5, dtype=F64)
    with raises("state must be contiguous float64 [1, 7, 5]; got torch.float64 (1, 6, 5)"):
        api.fit_accumulate_into(R, I3, torch.zeros(1, 6, 5, dtype=F64), k=6)
    with raises("state must be contiguous float64 [1, 7, 5]; got torch.float64 (1, 7, 5)"):
        api.fit_accumulate_into(R, I3, torch.zeros(1, 5, 7, dtype=F64).transpose(1, 2), k=6)
    with raises("R must be contiguous float64 [2, 6]; got torch.float64 (3, 6)"):
        api.fit_accumulate_into(torch.zeros(3, 6, dtype=F64), I3, st, k=6)
    with raises("I3 strides (10, 5, 1) are not light-major planes of stride 3"):
        api.fit_accumulate_into(R, I3, st, k=6, light_stride=3)
    M = torch.zeros(6, 6, dtype=F64)
    with raises("state must be contiguous float64 [C, 7, P]; got torch.float64 (1, 6, 5)"):
        api.fit_accum_solve_into(M, torch.zeros(1, 6, 5, dtype=F64), None, None, k=6, n_lights=8)
    with raises("state must be contiguous float64 [C, 7, P]; got torch.float64 (1, 7, 5)"):
        api.fit_accum_solve_into(M, torch.zeros(1, 5, 7, dtype=F64).transpose(1, 2), None, None, k=6, n_lights=8)
    with raises("M must be contiguous float64 [6, 6]; got torch.float64 (6, 5)"):
        api.fit_accum_solve_into(torch.zeros(6, 5, dtype=F64), st, None, None, k=6, n_lights=8)


# ---- the host half of the library ----------------------------------------------------------------

Q = (np.array([0.1, 0.2]), np.array([0.0, 0.3]))
DIRECTION_TAKERS = [rti.pinv, rti.design_matrix, rti.gram_inverse, rti.lsq_factors,
                    lambda lu, lv: rti.rbf_operator(lu, lv, *Q), lambda lu, lv: rti.basis_operator(lu, lv, *Q)]


@pytest.mark.parametrize("fn", DIRECTION_TAKERS, ids=["pinv", "design_matrix", "gram_inverse", "lsq_factors",
                                                      "rbf_operator", "basis_operator"])
def test_direction_errors(fn):
    rti.load()
    with raises("lu is empty"):
        fn([], [])
    with raises("lu and lv differ in length"):
        fn([0.1, 0.2, 0.3], [0.1, 0.2, 0.3, 0.4])


@pytest.mark.parametrize("form", ["h16", "q8"])
def test_u8_operators(form):
    lib = rti.load()
    build = getattr(rti, f"{form}_operator")
    pv = np.random.default_rng(3).normal(size=(6, 8))
    op = build(pv)
    assert op.dtype == np.uint8 and op.shape == (int(getattr(lib, f"rti_{form}_operator_bytes")(6, 8)),)
    assert op.size > 0 and op.any()
    pv[2, 5] = np.nan
    with pytest.raises(ValueError):
        build(pv)
