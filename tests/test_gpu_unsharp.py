"""rti_map_unsharp / rti_shade_normals on the GPU against their fp64 NumPy restatement (tests/unsharp_ref.py).

Map tolerance (derived, not tuned): |got − ref| <= 2^-23·|ref| + 1e-10·(1 + |amount|)·M with M = max|src| over the
valid pixels: the single fp32 rounding of the result, plus the fp64 error of the at most (2R+1)² products in each of
the numerator and denominator sums (fma on the GPU against rounded products in NumPy) with a wide margin.  Invalid
pixels must be bit-equal to src and no valid pixel may be NaN.

Shapes, with the kernel's 32×64 tile: maps smaller than the radius (1×1, 1×7, 5×1, 3×3 at R = 4), exactly one tile,
a tile ± 1 in each axis (W = 63 and 65 are no multiples of 4), and 70×140 = 3×3 tiles, whose middle tile has halo on
all four sides."""
import functools

import numpy as np
import pytest
import torch

import rti
import unsharp_ref as ur
from normals_ref import mixed_coef, peaked_coef, to_int32, to_uint8

pytestmark = pytest.mark.gpu

TH, TW = 32, 64
SIGMA_OF_R = {1: 0.3, 6: 2.0, 32: 10.6}  # the default radius of each sigma

# (H, W, channels, R, sigma, amount, invalid pixels)
CASES = [
    (1, 1, 3, 4, 1.5, 1.5, False), (1, 7, 1, 4, 1.5, -1.0, False), (5, 1, 6, 4, 1.5, 1.5, False),
    (3, 3, 3, 4, 1.5, 1.5, True), (5, 7, 16, 4, 1.5, 0.0, True),
    (TH, TW, 6, 6, 2.0, 1.5, True), (TH, TW, 1, 32, 10.6, -1.0, True), (TH, TW, 9, 1, 0.3, 1.5, True),
    (TH - 1, TW - 1, 3, 6, 2.0, 1.5, True), (TH + 1, TW + 1, 6, 6, 2.0, -1.0, True),
    (TH - 1, TW + 1, 9, 32, 10.6, 1.5, True), (TH + 1, TW - 1, 16, 1, 0.3, 0.0, True),
    (70, 140, 6, 6, 2.0, 1.5, True), (70, 140, 3, 32, 10.6, 1.5, True), (70, 140, 16, 6, 2.0, -1.0, True),
    (70, 140, 1, 1, 0.3, 1.5, True), (70, 140, 9, 6, 2.0, 0.0, True), (70, 138, 6, 32, 10.6, -1.0, True),
]


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def map_case(H, W, C, R, sigma, amount, bad):
    """(src [H, W, C] host fp32, reference fp64, valid mask) -- computed once, shared and never written."""
    src = ur.map_input(H, W, C, 100 * H + W + C, bad)
    ref, valid = ur.unsharp_ref(src, sigma, amount, R)
    for a in (src, ref, valid):
        a.setflags(write=False)
    return src, ref, valid


def offset_tensor(t, offset):
    """t, or a copy that starts 8 bytes into a 16-byte aligned buffer."""
    if not offset:
        return t
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=t.device)
    v = buf[2:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def run_map(cuda, src, layout, sigma, amount, R, *, renorm=False, offset=False):
    """The map through rti.map_unsharp_into in `layout`; with offset both src and dst start 8 bytes into an aligned
    buffer (the one-float load path).  dst sits between guard elements a stray store would overwrite.  Returns the
    result as [H, W, C] on the host."""
    t = torch.as_tensor(np.array(src.transpose(2, 0, 1) if layout == "planar" else src, order="C"), device=cuda)
    t = offset_tensor(t, offset)
    pad = 6 if offset else 8
    guard = torch.full((t.numel() + 2 * pad,), -7.0, dtype=torch.float32, device=cuda)
    dst = guard[pad:pad + t.numel()].view(t.shape)
    assert dst.data_ptr() % 16 == (8 if offset else 0)
    rti.map_unsharp_into(t, dst, sigma=sigma, amount=amount, radius=R, layout=layout, renorm=renorm)
    assert (guard[:pad] == -7).all() and (guard[pad + t.numel():] == -7).all()
    out = dst.cpu().numpy()
    return out.transpose(1, 2, 0) if layout == "planar" else out


def check_map(got, src, ref, valid, amount):
    assert np.array_equal(got[~valid].view(np.uint32), src[~valid].view(np.uint32))  # copied bit for bit
    assert not np.isnan(got[valid]).any()
    err = np.abs(got.astype(np.float64)[valid] - ref[valid])
    tol = ur.map_tolerance(ref, valid, src, amount)[valid]
    if err.size:
        print(f"worst error / tolerance {np.max(err / tol):.3g}")
    assert (err <= tol).all()


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_map_against_reference(cuda, case, layout, offset):
    H, W, C, R, sigma, amount, bad = case
    src, ref, valid = map_case(*case)
    got = run_map(cuda, src, layout, sigma, amount, R, offset=offset)
    check_map(got, src, ref, valid, amount)
    if amount == 0.0:
        assert np.array_equal(got.view(np.uint32), src.view(np.uint32))  # amount = 0 returns src bit for bit


@pytest.mark.parametrize("R", [1, 6, 32])
def test_default_radius_and_public_shapes(cuda, R):
    """rti.unsharp with the default radius of sigma, on [H, W, k], [k, H, W] and [H, W] maps."""
    sigma = SIGMA_OF_R[R]
    src, ref, valid = map_case(TH + 1, TW + 1, 6, R, sigma, 1.5, True)
    t = torch.as_tensor(src, device=cuda)
    got = rti.unsharp(t, sigma, 1.5)
    assert got.shape == t.shape and got.dtype == torch.float32
    check_map(got.cpu().numpy(), src, ref, valid, 1.5)
    pl = rti.unsharp(t.permute(2, 0, 1).contiguous(), sigma, 1.5, layout="planar")
    assert pl.shape == (6, TH + 1, TW + 1) and torch.equal(bits(pl.permute(1, 2, 0)), bits(got))
    one = src[..., :1].copy()
    r1, v1 = ur.unsharp_ref(one, sigma, 1.5, R)
    g1 = rti.unsharp(torch.as_tensor(one[..., 0], device=cuda), sigma, 1.5)
    assert g1.shape == (TH + 1, TW + 1)
    check_map(g1.cpu().numpy()[..., None], one, r1, v1, 1.5)


@pytest.mark.parametrize("case", [CASES[5], CASES[10], CASES[12], CASES[13]], ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_exact_properties(cuda, case):
    """Pixel-major and planar, the vector and the one-float load paths, and two runs give the same bits."""
    H, W, C, R, sigma, amount, bad = case
    src = map_case(*case)[0]
    base = run_map(cuda, src, "pixel", sigma, amount, R)
    for layout, offset in (("pixel", False), ("planar", False), ("pixel", True), ("planar", True)):
        again = run_map(cuda, src, layout, sigma, amount, R, offset=offset)
        assert np.array_equal(again.view(np.uint32), base.view(np.uint32)), (layout, offset)
    zero = run_map(cuda, src, "planar", sigma, 0.0, R)
    assert np.array_equal(zero.view(np.uint32), src.view(np.uint32))


@pytest.mark.parametrize("R", [1, 6, 32])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
def test_constant_and_ramp(cuda, layout, R):
    """A constant map stays constant; a linear ramp is unchanged at pixels at least R from every border and from
    every invalid pixel (the taps are symmetric and the denominator is their whole sum there)."""
    sigma, amount, H, W = SIGMA_OF_R[R], 1.5, 70, 140
    const = np.full((H, W, 3), 42.5, np.float32)
    got = run_map(cuda, const, layout, sigma, amount, R)
    assert (np.abs(got.astype(np.float64) - 42.5) <= 2.0 ** -23 * 42.5 + 1e-10 * (1 + amount) * 42.5).all()
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([3.0 * xx - 2.0 * yy + 11.0, 0.5 * yy + 1.0, -1.25 * xx], -1).astype(np.float32)  # exact in fp32
    ramp[40, 100, 1] = np.nan
    got = run_map(cuda, ramp, layout, sigma, amount, R)
    far = np.zeros((H, W), bool)
    far[R:H - R, R:W - R] = True
    far[40 - R:40 + R + 1, 100 - R:100 + R + 1] = False
    assert far.any()
    M = np.abs(ramp[np.isfinite(ramp).all(-1)]).max()
    tol = 2.0 ** -23 * np.abs(ramp.astype(np.float64)) + 1e-10 * (1 + amount) * M
    assert (np.abs(got.astype(np.float64) - ramp)[far] <= tol[far]).all()
    assert np.isnan(got[40, 100, 1]) and np.array_equal(got[40, 100, [0, 2]], ramp[40, 100, [0, 2]])


@pytest.mark.parametrize("nl", ["pixel", "planar"])
def test_renormalised_normals(cuda, nl):
    """rti.normals of a map of every class of pixel -> rti.normals_unsharp: unit length and the reference to 1e-6,
    kind-4 pixels stay NaN."""
    H, W = 45, 83
    coef = torch.as_tensor(mixed_coef(H * W, 77).reshape(H, W, 6), device=cuda)
    n, kind = rti.normals(coef, normal_layout=nl, return_kind=True)
    got = rti.normals_unsharp(n, 2.0, 1.5, layout=nl)
    assert got.shape == n.shape
    to_hwc = (lambda a: a.transpose(1, 2, 0)) if nl == "planar" else (lambda a: a)
    src = np.ascontiguousarray(to_hwc(n.cpu().numpy()))
    g = np.ascontiguousarray(to_hwc(got.cpu().numpy())).astype(np.float64)
    ref, valid = ur.unsharp_ref(src, 2.0, 1.5, renorm=True)
    bad = kind.cpu().numpy() == 4
    assert bad.any() and np.array_equal(~valid, bad) and np.isnan(g[bad]).all() and not np.isnan(g[valid]).any()
    assert np.abs(np.linalg.norm(g[valid], axis=-1) - 1.0).max() <= 1e-6
    err = np.abs(g - ref)[valid].max()
    print(f"renormalised normal error {err:.3g}")
    assert err <= 1e-6
    # a zero result renormalises to (0, 0, 1): the plain blur between two opposite normals, fma(w1, −1, w1) = 0
    z = np.zeros((1, 3, 3), np.float32)
    z[0, 0, 0], z[0, 2, 0] = 1.0, -1.0
    flat = rti.unsharp(torch.as_tensor(z, device=cuda), 50.0, -1.0, radius=1, renorm=True).cpu().numpy()
    assert np.array_equal(flat[0, 1], [0.0, 0.0, 1.0])
    assert np.abs(flat - ur.unsharp_ref(z, 50.0, -1.0, 1, renorm=True)[0]).max() <= 1e-6


@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("amount", [-1.0, 1.5])
def test_unsharp_commutes_with_relight(cuda, layout, amount):
    """Relighting is linear in the coefficients: relight(unsharp(coef)) and unsharp(relight(coef)) agree within
    8·2^-24·(1 + 2|a|)·max_p Σ_i |coef_i·b_i| (two fp32 roundings on each path)."""
    H, W, sigma = 70, 140, 2.0
    c = peaked_coef(np.random.default_rng(9), H * W, 0.0, 0.9)[0].astype(np.float32).reshape(H, W, 6)
    t = torch.as_tensor(np.ascontiguousarray(c.transpose(2, 0, 1)) if layout == "planar" else c, device=cuda)
    for lu, lv in ((0.3, -0.45), (0.0, 0.0)):
        a = rti.relight(rti.unsharp(t, sigma, amount, layout=layout), lu, lv, layout=layout)
        b = rti.unsharp(rti.relight(t, lu, lv, layout=layout), sigma, amount)
        assert a.shape == b.shape == (H, W)
        basis = np.array([lu * lu, lv * lv, lu * lv, lu, lv, 1.0])
        bound = 8 * 2.0 ** -24 * (1 + 2 * abs(amount)) * np.abs(c.astype(np.float64) * basis).sum(-1).max()
        err = (a.double() - b.double()).abs().max().item()
        print(f"commutation error {err:.3g}, bound {bound:.3g}")
        assert err <= bound


# ---- rti_shade_normals ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shade_case(P, with_albedo, lu, lv, kd, ks, e):
    n, a = ur.shade_inputs(P)
    ref = ur.shade_ref(n, lu, lv, a if with_albedo else None, kd, ks, e)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("with_albedo", [False, True])
@pytest.mark.parametrize("nl", ["pixel", "planar"])
@pytest.mark.parametrize("P", ur.SHADE_SIZES)
def test_shade_normals(cuda, P, nl, with_albedo, offset):
    n, a = ur.shade_inputs(P)
    nt = offset_tensor(torch.as_tensor(np.ascontiguousarray(n.T) if nl == "planar" else n, device=cuda), offset)
    at = offset_tensor(torch.as_tensor(a, device=cuda), offset) if with_albedo else None
    worst, excluded = 0.0, 0.0
    for lu, lv in ur.SHADE_DIRS:
        for kd, ks, e in ur.SHADE_PARAMS:
            ref = shade_case(P, with_albedo, lu, lv, kd, ks, e)
            nan = np.isnan(ref)
            kw = dict(albedo=at, kd=kd, ks=ks, exp=e, normal_layout=nl)
            got = rti.shade_normals(nt, lu, lv, **kw)
            assert got.shape == (P,) and got.dtype == torch.float32
            g = got.cpu().numpy().astype(np.float64)
            assert np.array_equal(np.isnan(g), nan)
            if (~nan).any():
                err = (np.abs(g - ref) / np.maximum(np.abs(ref), 1.0))[~nan].max()
                worst = max(worst, err)
                assert err <= 1e-6, (lu, lv, kd, ks, e, err)
            near = ur.near_integer(ref)
            excluded = max(excluded, near.mean())
            assert near.mean() <= 0.01
            for dt, conv in ((torch.int32, to_int32), (torch.uint8, to_uint8)):
                gi = rti.shade_normals(nt, lu, lv, out_dtype=dt, **kw)
                assert gi.dtype == dt and gi.shape == (P,)
                assert np.array_equal(gi.cpu().numpy()[~near], conv(ref)[~near]), (lu, lv, kd, ks, e, dt)
    print(f"shade fp32 worst err {worst:.3g}, near-integer share {excluded:.3%}")


def test_shade_normals_spatial_shapes_and_guards(cuda):
    n, a = ur.shade_inputs(1279)
    nt = torch.as_tensor(n[:1278].reshape(18, 71, 3), device=cuda)
    at = torch.as_tensor(a[:1278].reshape(18, 71), device=cuda)
    img = rti.shade_normals(nt, 0.3, -0.45, albedo=at, kd=0.4, ks=150.0, exp=75)
    assert img.shape == (18, 71)
    pl = rti.shade_normals(nt.permute(2, 0, 1).contiguous(), 0.3, -0.45, albedo=at, kd=0.4, ks=150.0, exp=75,
                           normal_layout="planar")
    assert torch.equal(bits(pl), bits(img))
    guard = torch.full((1278 + 16,), -7.0, device=cuda)
    out = guard[8:8 + 1278]
    rti.shade_normals_into(nt, 0.3, -0.45, out, albedo=at.reshape(-1), kd=0.4, ks=150.0, exp=75)
    assert torch.equal(bits(out), bits(img.reshape(-1))) and (guard[:8] == -7).all() and (guard[8 + 1278:] == -7).all()
    with pytest.raises(ValueError):
        rti.shade_normals(nt, 0.3, -0.45, albedo=at[:, :70])
    with pytest.raises(ValueError):
        rti.shade_normals(nt, 0.3, -0.45, exp=0)
    with pytest.raises(ValueError):
        rti.shade_normals(nt, 0.3, -0.45, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        rti.unsharp(nt, 2.0, renorm=True, layout="planar")
    with pytest.raises(ValueError):
        rti.unsharp(nt, 11.0)
    with pytest.raises(ValueError):
        rti.map_unsharp_into(nt, nt, sigma=2.0)
    with pytest.raises(ValueError, match="contiguous"):
        rti.map_unsharp_into(nt[:, ::2], torch.empty_like(nt[:, ::2]), sigma=2.0)


@pytest.mark.parametrize("planar", [False, True])
def test_torch_ops(cuda, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    layout = "planar" if planar else "pixel"
    src = map_case(TH + 1, TW + 1, 6, 6, 2.0, -1.0, True)[0]
    t = torch.as_tensor(np.ascontiguousarray(src.transpose(2, 0, 1)) if planar else src, device=cuda)
    got = torch.ops.rti.map_unsharp(t, 2.0, 1.5, 0, planar, False)
    want = rti.unsharp(t, 2.0, 1.5, layout=layout)
    assert got.shape == want.shape and torch.equal(bits(got), bits(want))
    torch.library.opcheck(torch.ops.rti.map_unsharp.default, (t, 2.0, 1.5, 0, planar, False),
                          test_utils=("test_schema", "test_faketensor"))
    n, a = ur.shade_inputs(1279)
    nt = torch.as_tensor(np.ascontiguousarray(n.T) if planar else n, device=cuda)
    at = torch.as_tensor(a, device=cuda)
    gr = torch.ops.rti.map_unsharp(nt.reshape((3, 1, 1279) if planar else (1, 1279, 3)), 2.0, 1.5, 0, planar, True)
    wr = rti.normals_unsharp(nt.reshape((3, 1, 1279) if planar else (1, 1279, 3)), 2.0, 1.5, layout=layout)
    assert torch.equal(bits(gr), bits(wr))
    for alb in (None, at):
        for dt in (torch.float32, torch.int32, torch.uint8):
            args = (nt, 0.3, -0.45, alb, 0.4, 150.0, 75, planar, dt)
            got = torch.ops.rti.shade_normals(*args)
            want = rti.shade_normals(nt, 0.3, -0.45, albedo=alb, kd=0.4, ks=150.0, exp=75, normal_layout=layout,
                                     out_dtype=dt)
            assert got.shape == want.shape and got.dtype == dt and torch.equal(bits(got), bits(want))
            torch.library.opcheck(torch.ops.rti.shade_normals.default, args, test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.shade_normals(nt.t().contiguous(), 0.3, -0.45, None, 1.0, 0.0, 1, planar, torch.float32)
