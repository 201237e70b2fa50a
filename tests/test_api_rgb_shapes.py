"""The Python layer over rti_relight_rgb / rti_relight_rgb_enhanced / rti_rgb_normals: spatial shapes round-trip,
scalar directions are squeezed, a non-contiguous input is made contiguous by the user-facing function and refused
by the graph-capturable launcher, and wrong dtypes, shapes and bases raise what the rgb8 siblings raise."""
import numpy as np
import pytest
import torch

import rti
from enhance_rgb_ref import peaked_rgb
from hsh8_ref import finite_hsh
from test_gpu_rgb8 import bits, dirs

pytestmark = pytest.mark.gpu

H, W = 12, 21
TERMS = {"ptm": 6, "hsh9": 9, "hsh16": 16}


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("basis", sorted(TERMS))
def test_relight_rgb_shapes(cuda, basis):
    k = TERMS[basis]
    host = peaked_rgb(H * W) if k == 6 else finite_hsh(H * W, k, 5)
    m = torch.as_tensor(host.reshape(3, H, W, k), device=cuda)
    flat = m.reshape(3, H * W, k)
    planar = m.permute(0, 3, 1, 2).contiguous()
    lu, lv = dirs(2)
    out = rti.relight_rgb(m, lu, lv, basis)
    assert out.shape == (2, H, W, 3) and out.dtype == torch.float32
    for c in range(3):
        assert same(out[..., c].contiguous(), rti.relight(m[c], lu, lv, basis))
    one = rti.relight_rgb(m, 0.3, -0.45, basis, out_dtype=torch.uint8)
    assert one.shape == (H, W, 3) and one.dtype == torch.uint8
    assert same(one, rti.relight_rgb(m, lu, lv, basis, out_dtype=torch.uint8)[0])  # dirs starts at (0.3, -0.45)
    assert same(rti.relight_rgb(flat, lu, lv, basis), out.reshape(2, H * W, 3))
    assert rti.relight_rgb(flat, 0.3, -0.45, basis).shape == (H * W, 3)
    assert same(rti.relight_rgb(planar, lu, lv, basis, layout="planar"), out)
    assert same(rti.relight_rgb(planar.reshape(3, k, H * W), lu, lv, basis, layout="planar"), out.reshape(2, H * W, 3))
    # a non-contiguous view: the user-facing function copies it, the launcher refuses it
    wide = torch.zeros((3, H, W, 2 * k), device=cuda)
    wide[..., ::2] = m
    view = wide[..., ::2]
    assert not view.is_contiguous() and same(rti.relight_rgb(view, lu, lv, basis), out)
    luv = torch.as_tensor(np.stack([lu, lv], -1), device=cuda)
    buf = torch.empty((2, H * W, 3), device=cuda)
    with pytest.raises(ValueError, match="contiguous"):
        rti.relight_rgb_into(view, luv, buf, basis=basis)
    assert same(rti.relight_rgb_into(m, luv, buf, basis=basis), out.reshape(2, H * W, 3))
    with pytest.raises(ValueError, match="terms"):
        rti.relight_rgb(m[..., :k - 1].contiguous(), lu, lv, basis)
    with pytest.raises(ValueError):
        rti.relight_rgb(m[:2], lu, lv, basis)
    with pytest.raises(ValueError):
        rti.relight_rgb(m[0], lu, lv, basis)
    with pytest.raises(ValueError, match="float32"):
        rti.relight_rgb(m.double(), lu, lv, basis)
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_rgb(m.cpu(), lu, lv, basis)
    with pytest.raises(ValueError, match="out_dtype"):
        rti.relight_rgb(m, lu, lv, basis, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="luv"):
        rti.relight_rgb_into(m, luv.float(), buf, basis=basis)
    with pytest.raises(ValueError, match="out"):
        rti.relight_rgb_into(m, luv, buf[:1], basis=basis)
    with pytest.raises(ValueError, match="out"):
        rti.relight_rgb_into(m, luv, buf.double(), basis=basis)


def test_enhanced_and_normals_shapes(cuda):
    m = torch.as_tensor(peaked_rgb(H * W).reshape(3, H, W, 6), device=cuda)
    flat = m.reshape(3, H * W, 6)
    planar = m.permute(0, 3, 1, 2).contiguous()
    kw = dict(gain=2.5, kd=0.4, ks=150.0, exp=20)
    for mode in ("diffuse_gain", "specular"):
        out = rti.relight_rgb_enhanced(m, 0.3, -0.45, mode, **kw)
        assert out.shape == (H, W, 3) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        assert same(rti.relight_rgb_enhanced(flat, 0.3, -0.45, mode, **kw), out.reshape(H * W, 3))
        assert same(rti.relight_rgb_enhanced(planar, 0.3, -0.45, mode, layout="planar", **kw), out)
        u8 = rti.relight_rgb_enhanced(m, 0.3, -0.45, mode, out_dtype=torch.uint8, **kw)
        assert u8.shape == (H, W, 3) and u8.dtype == torch.uint8 and bool(u8.any())
        wide = torch.zeros((3, H, W, 12), device=cuda)
        wide[..., ::2] = m
        assert same(rti.relight_rgb_enhanced(wide[..., ::2], 0.3, -0.45, mode, **kw), out)
        buf = torch.empty((H * W, 3), device=cuda)
        with pytest.raises(ValueError, match="contiguous"):
            rti.relight_rgb_enhanced_into(wide[..., ::2], 0.3, -0.45, mode, buf, **kw)
        assert same(rti.relight_rgb_enhanced_into(m, 0.3, -0.45, mode, buf, **kw), out.reshape(H * W, 3))
    n, kind, peak = rti.rgb_normals(m, return_kind=True, return_peak=True)
    assert n.shape == (H, W, 3) and kind.shape == peak.shape == (H, W) and kind.dtype == torch.uint8
    assert rti.rgb_normals(m).shape == (H, W, 3) and same(rti.rgb_normals(m), n)
    assert same(rti.rgb_normals(m, normal_layout="planar"), n.permute(2, 0, 1).contiguous())
    assert same(rti.rgb_normals(flat), n.reshape(H * W, 3))
    assert same(rti.rgb_normals(planar, layout="planar"), n)
    assert rti.rgb_normals(flat, return_peak=True)[1].shape == (H * W,)
    wide = torch.zeros((3, H, W, 12), device=cuda)
    wide[..., ::2] = m
    assert same(rti.rgb_normals(wide[..., ::2]), n)
    with pytest.raises(ValueError, match="contiguous"):
        rti.rgb_normals_into(wide[..., ::2], torch.empty((H * W, 3), device=cuda))
    with pytest.raises(ValueError, match="normals"):
        rti.rgb_normals_into(m, torch.empty((H * W, 2), device=cuda))
    with pytest.raises(ValueError, match="kind"):
        rti.rgb_normals_into(m, torch.empty((H * W, 3), device=cuda), torch.empty(H * W, device=cuda))
    for fn in (lambda x, **k: rti.relight_rgb_enhanced(x, 0.3, -0.45, "specular", **k), rti.rgb_normals):
        with pytest.raises(ValueError, match="terms"):
            fn(m[..., :5].contiguous())
        with pytest.raises(ValueError):
            fn(m[:2])
        with pytest.raises(ValueError, match="float32"):
            fn(m.half())
        with pytest.raises(ValueError, match="CUDA"):
            fn(m.cpu())
        with pytest.raises(ValueError, match="layout"):
            fn(m, layout="rows")
        with pytest.raises(ValueError, match="weights"):
            fn(m, weights=(1.0, 2.0))
        with pytest.raises(ValueError, match="weight"):
            fn(m, weights=(1.0, float("nan"), 0.0))
        with pytest.raises(NotImplementedError, match="PTM-6"):
            fn(m, basis="hsh9")
    with pytest.raises(ValueError, match="mode"):
        rti.relight_rgb_enhanced(m, 0.3, -0.45, "glossy")
    with pytest.raises(ValueError, match="out_dtype"):
        rti.relight_rgb_enhanced(m, 0.3, -0.45, "specular", out_dtype=torch.float64)
    with pytest.raises(ValueError, match="gain"):
        rti.relight_rgb_enhanced(m, 0.3, -0.45, "diffuse_gain", gain=-1.0)
    with pytest.raises(ValueError, match="spec_exp"):
        rti.relight_rgb_enhanced(m, 0.3, -0.45, "specular", exp=0)
    with pytest.raises(ValueError, match="layout"):
        rti.rgb_normals(m, normal_layout="rows")
