"""rti.FitAccumulator / rti_fit_accumulate / rti_fit_accum_solve on the GPU: the shared fit fed in chunks of light
planes.  The state after N lights must not depend on the chunking, to the bit; the fit read from it must meet the
fp64 NumPy least squares (conftest.coef_close at the project criterion 1e-4, res at rtol 1e-4 + atol 1e-3) and
the one-pass rti.fit_with_residual on the whole stack (coef_close at 1e-5, res at rtol 1e-5 + atol 1e-5: both
sides are fp64 sums rounded once to fp32, so they differ by about one fp32 ulp of the largest coefficient).

Stacks as tests/test_gpu_robust.py builds them: light directions with radius² uniform in [0.02, 0.8], seeded;
clean I = A·c_true in about [60, 170]; the noisy variant adds σ = 1 noise (so the residual is about 1 and the
cancellation in q − cᵀy is harmless).  cond(A) = 9.2 / 7.8 for PTM-6 at N = 24 / 100 and 96 for HSH-16 at N = 40.
P = 549: odd, so the fp64 planes are unaligned (one pixel per lane), two full 256-pixel spans plus 37 pixels;
P = 576: aligned planes (four pixels per lane; two staged 256-pixel coefficient rows and a 64-pixel tail wave);
P = 2052: the vector path over more than one workgroup; P = 1."""
import functools

import numpy as np
import pytest
import torch

import rti
from conftest import coef_close

pytestmark = pytest.mark.gpu

P0 = 549


def dirs(N, seed=0):
    rng = np.random.default_rng(1000 + seed)
    r, a = np.sqrt(rng.uniform(0.02, 0.8, N)), rng.uniform(0.0, 2.0 * np.pi, N)
    return (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clean(N, P=P0, basis="ptm", seed=0):
    """(lu, lv, A fp64 [N, k], c_true [P, k], I fp32 [N, P])"""
    lu, lv = dirs(N, seed)
    A = rti.design_matrix(lu, lv, basis)
    rng = np.random.default_rng(2000 + seed)
    c = rng.uniform(-15.0, 15.0, (P, A.shape[1]))
    const = 5 if basis == "ptm" else 0  # the basis' constant term
    c[:, const] = rng.uniform(105.0, 125.0, P) / A[0, const]
    return lu, lv, A, c, (A @ c.T).astype(np.float32)


@functools.lru_cache(maxsize=None)
def noisy(N, P=P0, basis="ptm", integer=False):
    """(lu, lv, A, I fp32 [N, P]): the clean stack plus σ = 1 noise, rounded to integers on request"""
    lu, lv, A, c, I = clean(N, P, basis)
    I = I + np.random.default_rng(5000 + N).normal(0.0, 1.0, I.shape).astype(np.float32)
    return lu, lv, A, (np.rint(I) if integer else I).astype(np.float32)


def lstsq_ref(A, I):
    """fp64 NumPy: (coef [P, k], res [P])"""
    I = I.astype(np.float64)
    c = np.linalg.lstsq(A, I, rcond=None)[0]
    return c.T, np.sqrt(((I - A @ c) ** 2).mean(0))


@functools.lru_cache(maxsize=None)
def ref(N, P=P0, basis="ptm", first=None):
    lu, lv, A, I = noisy(N, P, basis)
    return lstsq_ref(A[:first], I[:first])


def check(coef, res, want, onepass=None):
    """both gates: the fp64 reference and (if given) rti.fit_with_residual's (coef, res, rms)"""
    coef, res = coef.cpu().numpy(), res.cpu().numpy()
    err, ok = coef_close(coef, want[0])
    assert ok, err
    assert np.allclose(res, want[1], rtol=1e-4, atol=1e-3), np.abs(res - want[1]).max()
    if onepass is not None:
        c0, r0 = onepass[0].cpu().numpy(), onepass[1].cpu().numpy()
        err, ok = coef_close(coef, c0, rtol=1e-5)
        assert ok, err
        assert np.allclose(res, r0, rtol=1e-5, atol=1e-5), np.abs(res - r0).max()


def splits(sizes):
    edges = np.cumsum([0] + list(sizes))
    return list(zip(edges[:-1], edges[1:]))


def chunks_of(N, B):
    return [min(B, N - n) for n in range(0, N, B)]


def accumulate(cuda, I, lu, lv, sizes, basis="ptm", dtypes=None, **kw):
    """a FitAccumulator fed I [N, P] (or [C, N, ...]) in chunks of the given sizes"""
    It = torch.as_tensor(I, device=cuda)
    acc = rti.FitAccumulator(kw.pop("shape", (I.shape[-1],)), basis, device=cuda, **kw)
    for i, (a, b) in enumerate(splits(sizes)):
        chunk = It[..., a:b, :] if acc.channels is None or It.dim() == 3 else It[:, a:b]
        if dtypes is not None:
            chunk = chunk.to(dtypes[i])
        if kw.get("directions") is not None:
            acc.add(chunk)
        else:
            acc.add(chunk, lu[a:b], lv[a:b])
    assert acc.n_lights == sum(sizes)
    return acc


@functools.lru_cache(maxsize=None)
def state24(P=P0):
    """case 1's state for N = 24 in one chunk (the reference the other cases compare bits with)"""
    lu, lv, A, I = noisy(24, P)
    acc = accumulate(torch.device("cuda", 0), I, lu, lv, [24])
    return acc.state.clone(), acc.solve()


# ---- 1. chunking does not change a bit ------------------------------------------------------------------------
@pytest.mark.parametrize("P", [P0, 576, 2052])
def test_chunking_does_not_change_a_bit(cuda, P):
    lu, lv, A, I = noisy(24, P)
    state, (coef, res) = state24(P)
    assert state.shape == (1, 7, P) and state.dtype == torch.float64
    # the state is what it says: y = Aᵀ I and q = ‖I‖² (fp64 sums of exact products: 1e-15 relative)
    want = np.concatenate([A.T @ I.astype(np.float64), (I.astype(np.float64) ** 2).sum(0)[None]])
    assert np.allclose(state[0].cpu().numpy(), want, rtol=1e-12, atol=1e-9)
    for sizes in ([1] * 24, [1, 7, 16], [5, 19]):
        acc = accumulate(cuda, I, lu, lv, sizes)
        assert torch.equal(acc.state, state), sizes
        c, r = acc.solve()
        assert torch.equal(c, coef) and torch.equal(r, res), sizes
    check(coef, res, ref(24, P))


def test_vector_and_scalar_paths_agree_to_the_bit(cuda):
    """The same P = 576 planes from a base 4 bytes off 16-byte alignment take one pixel per lane."""
    P = 576
    lu, lv, A, I = noisy(24, P)
    state, _ = state24(P)
    buf = torch.empty(24 * P + 4, dtype=torch.float32, device=cuda)
    I3 = buf[1:1 + 24 * P].view(1, 24, P)
    assert I3.data_ptr() % 16 == 4
    I3.copy_(torch.as_tensor(I, device=cuda))
    got = torch.empty_like(state)
    rti.fit_accumulate_into(torch.as_tensor(A, device=cuda), I3, got, k=6, init=True)
    assert torch.equal(got, state)


# ---- 2. equals the one-pass fit and the fp64 reference --------------------------------------------------------
@pytest.mark.parametrize("orth", [False, True])
@pytest.mark.parametrize("N", [24, 100])
def test_equals_one_pass_fit_and_reference(cuda, N, orth):
    lu, lv, A, I = noisy(N)
    acc = accumulate(cuda, I, lu, lv, chunks_of(N, 7), **(dict(directions=(lu, lv)) if orth else {}))
    coef, res = acc.solve()
    assert coef.shape == (P0, 6) and res.shape == (P0,) and coef.dtype == res.dtype == torch.float32
    check(coef, res, ref(N), rti.fit_with_residual(torch.as_tensor(I, device=cuda), lu, lv))
    assert acc.lu == [float(x) for x in lu] and acc.lv == [float(x) for x in lv]


# ---- 3. preview -----------------------------------------------------------------------------------------------
def test_preview(cuda):
    lu, lv, A, I = noisy(24)
    It = torch.as_tensor(I, device=cuda)
    acc = rti.FitAccumulator((P0,), device=cuda)
    acc.add(It[:12], lu[:12], lv[:12])
    coef, res = acc.solve()
    check(coef, res, ref(24, first=12), rti.fit_with_residual(It[:12], lu[:12], lv[:12]))
    before = acc.state.clone()
    acc.solve()
    assert torch.equal(acc.state, before)  # solve leaves the state as it is
    acc.add(It[12:], lu[12:], lv[12:])
    state, (c24, r24) = state24()
    assert torch.equal(acc.state, state)
    coef, res = acc.solve()
    check(coef, res, ref(24), rti.fit_with_residual(It, lu, lv))
    assert torch.equal(coef, c24) and torch.equal(res, r24)
    again = acc.solve()
    assert torch.equal(again[0], coef) and torch.equal(again[1], res)


# ---- 4. init --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [P0, 576])
def test_init_overwrites_without_reading(cuda, P):
    lu, lv, A, I = noisy(24, P)
    I3 = torch.as_tensor(I, device=cuda).unsqueeze(0)
    Ad = torch.as_tensor(A, device=cuda)
    out = {}
    for fill in (float("nan"), 0.0):
        st = torch.full((1, 7, P), fill, dtype=torch.float64, device=cuda)
        rti.fit_accumulate_into(Ad[:5].contiguous(), I3[:, :5].contiguous(), st, k=6, init=True)
        rti.fit_accumulate_into(Ad[5:].contiguous(), I3[:, 5:].contiguous(), st, k=6)
        out[fill == 0.0] = st
    assert torch.equal(out[True], out[False]) and torch.equal(out[True], state24(P)[0])
    st = torch.zeros((1, 7, P), dtype=torch.float64, device=cuda)  # adding to zeros = init
    rti.fit_accumulate_into(Ad, I3, st, k=6)
    assert torch.equal(st, out[True])


def test_reset(cuda):
    lu, lv, A, I = noisy(24)
    It = torch.as_tensor(I, device=cuda)
    acc = accumulate(cuda, I, lu, lv, [5, 19])
    first = acc.state.clone()
    assert acc.reset() is acc and acc.n_lights == 0 and acc.lu == [] and acc.lv == []
    with pytest.raises(ValueError):
        acc.solve()
    acc.add(It[:5], lu[:5], lv[:5]).add(It[5:], lu[5:], lv[5:])
    assert torch.equal(acc.state, first) and acc.n_lights == 24


# ---- 5. dtypes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [P0, 576])
def test_dtypes_and_mixed_chunks(cuda, P):
    lu, lv, A, I = noisy(24, P, integer=True)
    assert I.min() >= 0 and I.max() <= 255 and np.array_equal(I, np.rint(I))
    u8, i32, f32 = torch.uint8, torch.int32, torch.float32
    states = [accumulate(cuda, I, lu, lv, [8, 8, 8], dtypes=d).state
              for d in ((u8, u8, u8), (i32, i32, i32), (f32, f32, f32), (u8, f32, i32))]
    for s in states[1:]:
        assert torch.equal(s, states[0])
    want = np.concatenate([A.T @ I.astype(np.float64), (I.astype(np.float64) ** 2).sum(0)[None]])
    assert np.allclose(states[0][0].cpu().numpy(), want, rtol=1e-12, atol=1e-9)


# ---- 6. bases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis,k,N,B,P", [("hsh9", 9, 24, 7, P0), ("hsh16", 16, 40, 13, P0), ("hsh9", 9, 24, 7, 576),
                                           ("hsh16", 16, 40, 13, 576)])
def test_hsh(cuda, basis, k, N, B, P):
    lu, lv, A, I = noisy(N, P, basis)
    acc = accumulate(cuda, I, lu, lv, chunks_of(N, B), basis)
    assert acc.state.shape == (1, k + 1, P)
    coef, res = acc.solve()
    assert coef.shape == (P, k)
    onepass = rti.fit_with_residual(torch.as_tensor(I, device=cuda), lu, lv, basis)
    check(coef, res, ref(N, P, basis), onepass)
    whole = accumulate(cuda, I, lu, lv, [N], basis)
    assert torch.equal(whole.state, acc.state)
    cp, rp = acc.solve(layout="planar")
    assert cp.shape == (k, P) and torch.equal(cp.T, coef) and torch.equal(rp, res)
    orth = accumulate(cuda, I, lu, lv, chunks_of(N, B), basis, directions=(lu, lv))
    check(*orth.solve(), ref(N, P, basis), onepass)


# ---- 7. shapes ------------------------------------------------------------------------------------------------
def test_channels_and_planar(cuda):
    lu, lv, A, I = noisy(24)
    want = ref(24)
    I4 = np.stack([I, I[:, ::-1], I]).reshape(3, 24, 9, 61)  # the stack, its pixel-reversed copy and the stack again
    acc = accumulate(cuda, I4, lu, lv, chunks_of(24, 7), shape=(9, 61), channels=3)
    assert acc.state.shape == (3, 7, P0)
    state, (c24, r24) = state24()
    assert torch.equal(acc.state[0], state[0]) and torch.equal(acc.state[2], state[0])
    assert torch.equal(acc.state[1], state[0].flip(-1))
    coef, res = acc.solve()
    assert coef.shape == (3, 9, 61, 6) and res.shape == (3, 9, 61)
    cp, rp = acc.solve(layout="planar")
    assert cp.shape == (3, 6, 9, 61) and torch.equal(cp.permute(0, 2, 3, 1), coef) and torch.equal(rp, res)
    for c, flip in enumerate((False, True, False)):
        cc, rr = coef[c].reshape(P0, 6), res[c].reshape(P0)
        if flip:
            cc, rr = cc.flip(0), rr.flip(0)
        check(cc, rr, want)
        assert torch.equal(cc, c24) and torch.equal(rr, r24)
    # [C, B, P] frames are the same chunk
    flat = accumulate(cuda, I4.reshape(3, 24, P0), lu, lv, [24], shape=(9, 61), channels=3)
    assert torch.equal(flat.state, acc.state)


def test_single_frames_and_flat_planes(cuda):
    lu, lv, A, I = noisy(24)
    It = torch.as_tensor(I, device=cuda)
    state, (c24, r24) = state24()
    acc = rti.FitAccumulator((9, 61), device=cuda)
    for n in range(24):  # the live-frame case: one [H, W] plane and scalar directions per call
        acc.add(It[n].reshape(9, 61), float(lu[n]), float(lv[n]))
    assert acc.n_lights == 24 and torch.equal(acc.state, state)
    coef, res = acc.solve()
    assert coef.shape == (9, 61, 6) and res.shape == (9, 61)
    assert torch.equal(coef.reshape(P0, 6), c24) and torch.equal(res.reshape(P0), r24)
    acc.reset()
    acc.add(It[:10].reshape(10, 9, 61), lu[:10], lv[:10]).add(It[10:], lu[10:], lv[10:])  # [B, H, W], then [B, P]
    assert torch.equal(acc.state, state)


def test_single_pixel(cuda):
    lu, lv, A, I = noisy(24)
    one = accumulate(cuda, I[:, 5:6], lu, lv, [7, 17])
    assert torch.equal(one.state[0, :, 0], state24()[0][0, :, 5])
    coef, res = one.solve()
    assert coef.shape == (1, 6) and res.shape == (1,)
    want = ref(24)
    check(coef, res, (want[0][5:6], want[1][5:6]))


@pytest.mark.parametrize("P,pad", [(P0, 3), (576, 3), (576, 4)])
def test_padded_planes(cuda, P, pad):
    """light_stride = P + pad on a buffer whose padding holds NaN (P = 576, pad 4: the 16-byte path)"""
    lu, lv, A, I = noisy(24, P)
    buf = torch.full((1, 24, P + pad), float("nan"), dtype=torch.float32, device=cuda)
    buf[0, :, :P] = torch.as_tensor(I, device=cuda)
    st = torch.empty((1, 7, P), dtype=torch.float64, device=cuda)
    Ad = torch.as_tensor(A, device=cuda)
    rti.fit_accumulate_into(Ad, buf[:, :, :P], st, k=6, init=True, light_stride=P + pad)
    assert torch.equal(st, state24(P)[0])
    with pytest.raises(ValueError):
        rti.fit_accumulate_into(Ad, buf[:, :, :P], st, k=6, init=True)  # the view is not dense planes
    with pytest.raises(ValueError):
        rti.fit_accumulate_into(Ad, buf[:, :, :P], st[:, :6], k=6, init=True)


def test_solve_into_planar_and_no_residual(cuda):
    state, (c24, r24) = state24(576)
    lu, lv, A, I = noisy(24, 576)
    M = torch.as_tensor(rti.gram_inverse(lu, lv), device=cuda)
    coef = torch.empty((1, 6, 576), dtype=torch.float32, device=cuda)
    rti.fit_accum_solve_into(M, state, coef, None, k=6, n_lights=24, layout="planar")
    assert torch.equal(coef[0].T, c24)


# ---- 8. fit_chunked -------------------------------------------------------------------------------------------
def test_fit_chunked(cuda):
    lu, lv, A, I = noisy(24)
    host = torch.as_tensor(I)

    def chunks():
        for i, (a, b) in enumerate(splits(chunks_of(24, 7))):
            frames = host[a:b]
            yield (frames.to(cuda) if i == 2 else frames), lu[a:b], lv[a:b]

    coef, res = rti.fit_chunked(chunks(), (P0,))
    _, (c24, r24) = state24()
    assert coef.is_cuda and torch.equal(coef, c24) and torch.equal(res, r24)
    ref_acc = accumulate(cuda, I, lu, lv, chunks_of(24, 7), directions=(lu, lv))
    c2, r2 = rti.fit_chunked((host[a:b] for a, b in splits(chunks_of(24, 7))), (P0,), directions=(lu, lv))
    co, ro = ref_acc.solve()
    assert torch.equal(c2, co) and torch.equal(r2, ro)


# ---- 9. errors ------------------------------------------------------------------------------------------------
def test_errors(cuda):
    lu, lv, A, I = noisy(24)
    It = torch.as_tensor(I, device=cuda)
    acc = rti.FitAccumulator((9, 61), device=cuda)
    acc.add(It[:5], lu[:5], lv[:5])
    with pytest.raises(ValueError, match="5 lights < 6 basis terms"):
        acc.solve()
    with pytest.raises(ValueError):
        acc.add(It[5:8], lu[5:7], lv[5:7])  # 2 directions for 3 planes
    with pytest.raises(ValueError):
        acc.add(It[5:8].reshape(3, 61, 9), lu[5:8], lv[5:8])  # wrong (H, W)
    with pytest.raises(ValueError):
        acc.add(It[5:8, :500], lu[5:8], lv[5:8])
    with pytest.raises(ValueError, match="CUDA"):
        acc.add(torch.as_tensor(I[5:8]), lu[5:8], lv[5:8])
    with pytest.raises(ValueError):
        acc.add(It[5:8].double(), lu[5:8], lv[5:8])
    with pytest.raises(ValueError):
        acc.add(It[5:8])  # no directions
    assert acc.n_lights == 5  # a refused chunk leaves the accumulator as it was
    with pytest.raises(ValueError):
        rti.FitAccumulator((9, 61), channels=3, device=cuda).add(It[:5].reshape(5, 9, 61), lu[:5], lv[:5])
    with pytest.raises(ValueError):
        rti.FitAccumulator((9, 61), "nope", device=cuda)
    known = rti.FitAccumulator((P0,), device=cuda, directions=(lu, lv))
    with pytest.raises(ValueError):
        known.add(It[:5], lu[:5], lv[:5])  # lu together with directions=
    known.add(It[:23])
    with pytest.raises(ValueError, match="orthonormal"):
        known.solve()  # before the last plane
    with pytest.raises(ValueError):
        known.add(It[22:])  # more planes than directions
    known.add(It[23:])
    check(*known.solve(), ref(24))


# ---- 10. torch ops --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    lu, lv, A, I = noisy(24)
    It = torch.as_tensor(I, device=cuda)
    Ad = torch.as_tensor(A, device=cuda)
    state, (c24, r24) = state24()
    st = torch.full((7, P0), float("nan"), dtype=torch.float64, device=cuda)
    assert torch.ops.rti.fit_accumulate(Ad[:9].contiguous(), It[:9], st, True) is None
    torch.ops.rti.fit_accumulate(Ad[9:].contiguous(), It[9:], st, False)
    assert torch.equal(st, state[0])
    M = torch.as_tensor(rti.gram_inverse(lu, lv), device=cuda)
    coef, res = torch.ops.rti.fit_accum_solve(M, st, 24, False, planar)
    assert torch.equal(coef.T if planar else coef, c24) and torch.equal(res, r24)
    # channels, and the orthonormal form
    U, W = rti.lsq_factors(lu, lv)
    Ud, Wd = torch.as_tensor(U, device=cuda), torch.as_tensor(W, device=cuda)
    I3 = torch.stack([It, It.flip(1)])
    st3 = torch.empty((2, 7, P0), dtype=torch.float64, device=cuda)
    torch.ops.rti.fit_accumulate(Ud, I3, st3, True)
    coef3, res3 = torch.ops.rti.fit_accum_solve(Wd, st3, 24, True, planar)
    known = accumulate(cuda, I, lu, lv, [24], directions=(lu, lv))
    ck, rk = known.solve(layout="planar" if planar else "pixel")
    assert torch.equal(coef3[0], ck) and torch.equal(res3[0], rk)
    assert coef3.shape == ((2, 6, P0) if planar else (2, P0, 6)) and res3.shape == (2, P0)
    torch.library.opcheck(torch.ops.rti.fit_accumulate.default, (Ad, It, st.clone(), True),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.rti.fit_accumulate.default, (Ud, I3, st3.clone(), False),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.rti.fit_accum_solve.default, (M, st, 24, False, planar),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.rti.fit_accum_solve.default, (Wd, st3, 24, True, planar),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.fit_accumulate(Ad.float(), It, st, True)
    with pytest.raises(ValueError):
        torch.ops.rti.fit_accum_solve(M, st[:6], 24, False, planar)


# ---- 11. the same fit as the one-pass kernel, to the bit ------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("P", [3080, P0])
@pytest.mark.parametrize("basis,N", [("ptm", 9), ("hsh9", 12), ("hsh16", 19)])
def test_same_bits_as_one_pass_fit(cuda, basis, N, P, C, dtype):
    """rti.FitAccumulator(directions=) fed the whole stack in one add, then solve, against rti.fit_with_residual:
    both run the same fma chains over U's rows in light order and the same steps from those sums to coefficients
    and residuals (the tail of fitres_body, restated in fit_accum_solve_k), so every value has the same bits.  P = 3080 is a multiple of 4
    but not of 256 (one launch holds whole staged waves, a partial wave and the unstaged rows), P = 549 takes one
    pixel per lane.  int32 stacks are left out: the one-pass kernel widens them through float, accumulate converts
    them to double directly, and above 2^24 the two legitimately differ."""
    lu, lv, A, I = noisy(N, P, basis, integer=dtype == torch.uint8)
    if dtype == torch.uint8:
        I = np.clip(I, 0, 255)
    if C == 1:
        It, shape, kw = torch.as_tensor(I, device=cuda).to(dtype), (P,), {}
    else:  # the stack and its pixel-reversed copy as [C, N, 1, P]
        It = torch.as_tensor(np.stack([I, I[:, ::-1]])[:, :, None, :].copy(), device=cuda).to(dtype)
        shape, kw = (1, P), dict(channels=2)
    acc = rti.FitAccumulator(shape, basis, device=cuda, directions=(lu, lv), **kw).add(It)
    for layout in ("pixel", "planar"):
        coef, res = acc.solve(layout=layout)
        c0, r0, _ = rti.fit_with_residual(It, lu, lv, basis, layout=layout)
        assert coef.shape == c0.shape and res.shape == r0.shape
        assert torch.equal(coef, c0), (layout, int((coef != c0).sum()))
        assert torch.equal(res, r0), (layout, int((res != r0).sum()))
