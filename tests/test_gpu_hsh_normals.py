"""HSH surface normals on the GPU (rti_hsh_normals.hip) against tests/hsh_normals_ref.py applied to the grid values
that rti.relight gives for the luminance map: the kernel never writes those values, so equal kinds, a bit-equal peak
and normals within 1e-6 (test_gpu_normals.py's bound for the PTM normals: two roundings of an fp64 result) show that
it formed the same bits and refined them the same way.

Sizes: a lane owns two pixels, a wave two runs of 64, a workgroup 512.  1 and 63 are a partial run, 64 one full run,
65 a full run and one pixel, 257 two waves and a one-pixel run, 1000 two workgroups (the second with a 40-pixel
run), 4099 nine workgroups and a 3-pixel tail.  Maps are oracle.synth_coef_fields plus hand-made pixels."""
import functools

import numpy as np
import pytest
import torch

import rti
from hsh_normals_ref import grid_dirs, grid_points, luminance, peak_normals

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 1000, 4099]
KS = [9, 16]
GRIDS = [4, 10, 16]
ACCURACY_BOUND_DEG = 1.5  # pinned on the CPU: test_hsh_normals_abi.py::test_reference_accuracy_on_a_lambertian_fit

# the normalisation constants of rti_basis.h: columns 0, 2 and 6 are K00, K10·t and K20·(3t² − 1)/2, t = 2·lw − 1
K00, K10, K20 = 0.39894228040143267794, 0.69098829894267095853, 0.89206205807638555727


def hand_made(k):
    """Pixels with a known answer, [n, k] fp32, and their names."""
    px = {}
    px["zero"] = np.zeros(k)                                  # flat: kind 2, (0, 0, 1)
    c = np.zeros(k); c[0] = 7.0; px["constant"] = c           # a constant function is flat too
    c = np.zeros(k); c[2] = -50.0; px["rim"] = c              # −t rises to the rim, where every point is equal
    c = np.zeros(k)                                           # −(t − ½)² = −⅔·P2(t) + t − 7/12: a ring of maxima
    c[6], c[2], c[0] = -(2.0 / 3.0) / K20 * 100, 1.0 / K10 * 100, -(7.0 / 12.0) / K00 * 100
    px["ring"] = c
    c = np.full(k, 3.0); c[1] = np.nan; px["nan"] = c
    c = np.full(k, 3.0); c[k - 1] = np.inf; px["inf"] = c
    names = list(px)
    return names, np.stack([px[n] for n in names]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def maps_of(P, k, C):
    """fp32 maps [C, P, k]: hand-made pixels first (as many as fit), then smooth random fields; never written."""
    import rti_oracle as o

    names, hm = hand_made(k)
    m = np.stack([o.synth_coef_fields(1, P, 50 + 7 * c + P, basis="hsh")[0, :, :k] for c in range(C)]).astype(np.float32)
    n = min(P, len(names))
    m[:, :n] = hm[:n]
    m.setflags(write=False)
    return m


def lum_of(m, weights=None):
    return m[0] if m.shape[0] == 1 else luminance(m, weights)


@functools.lru_cache(maxsize=None)
def reference(P, k, C, G):
    """(normals [P, 3], kind [P], peak [P], V [E, P]) from rti.relight's values of the luminance map."""
    lum = lum_of(maps_of(P, k, C))
    u, v = grid_dirs(G)
    V = rti.relight(torch.tensor(lum, device="cuda"), u, v, basis=f"hsh{k}").cpu().numpy()
    assert V.shape == (len(u), P) and V.dtype == np.float32
    return peak_normals(V, G, lum) + (V,)


def laid_out(m, layout):
    return np.ascontiguousarray(m.transpose(0, 2, 1)) if layout == "planar" else m


def squeeze1(t):
    return t[0] if t.shape[0] == 1 else t


def bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_against_reference(got, want, normal_layout):
    n, kind, peak = (t.cpu().numpy() for t in got)
    wn, wkind, wpeak, _ = want
    if normal_layout == "planar":
        n = n.T
    assert np.array_equal(kind, wkind), np.flatnonzero(kind != wkind)[:8]
    bad = wkind == 4
    assert np.isnan(n[bad]).all() and np.isnan(peak[bad]).all()
    assert not np.isnan(n[~bad]).any() and not np.isnan(peak[~bad]).any()
    assert np.array_equal(peak[~bad].view(np.uint32), wpeak[~bad].view(np.uint32))
    err = np.abs(n[~bad].astype(np.float64) - wn[~bad]).max() if (~bad).any() else 0.0
    assert err <= 1e-6, err


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("k", KS)
def test_values_are_the_relights_bits(cuda, k, C, layout, G):
    for P in SIZES:
        want = reference(P, k, C, G)
        md = squeeze1(torch.tensor(laid_out(maps_of(P, k, C), layout), device=cuda))
        for nl in ("pixel", "planar"):
            got = rti.hsh_normals(md, f"hsh{k}", layout=layout, normal_layout=nl, grid=G, return_kind=True,
                                  return_peak=True)
            assert got[0].shape == ((P, 3) if nl == "pixel" else (3, P)) and got[1].shape == got[2].shape == (P,)
            check_against_reference(got, want, nl)


@pytest.mark.parametrize("k", KS)
def test_hand_made_pixels(cuda, k):
    G, P = 10, 64
    names, _ = hand_made(k)
    n, kind, peak, V = reference(P, k, 1, G)
    got_n, got_kind, got_peak = rti.hsh_normals(torch.tensor(maps_of(P, k, 1)[0], device=cuda), f"hsh{k}", grid=G,
                                                return_kind=True, return_peak=True)
    got_n, got_kind = got_n.cpu().numpy(), got_kind.cpu().numpy()
    at = {name: i for i, name in enumerate(names)}
    pts = grid_points(G)
    for name in ("zero", "constant"):
        assert got_kind[at[name]] == 2 and got_n[at[name]].tolist() == [0.0, 0.0, 1.0]
    assert float(got_peak[at["zero"]]) == 0.0
    for name in ("nan", "inf"):
        assert got_kind[at[name]] == 4 and np.isnan(got_n[at[name]]).all() and np.isnan(float(got_peak[at[name]]))
    # the rim: every point with i² + j² = G² has lw = 0 and the same value, the largest; the first of them, (0, −G),
    # has no neighbour along u and none below: both steps are 0 and the normal lies in the plane.  r² is exactly 1,
    # so the kind is 0: a refined point is a convex combination of mask points and cannot leave the disc
    # (DESIGN.md §4.10), kind 1 is reachable by rounding only (test_hsh_normals_abi.py shows it on made-up values).
    rim = V[:, at["rim"]]
    on_rim = [e for e, (i, j) in enumerate(pts) if i * i + j * j == G * G and i * j == 0]  # (i/G)² + 0 is exactly 1
    assert len(on_rim) == 4 and (rim[on_rim] == rim.max()).all() and int(np.argmax(rim)) == 0 == on_rim[0]
    assert got_kind[at["rim"]] == kind[at["rim"]] == 0 and got_n[at["rim"]].tolist() == [0.0, -1.0, 0.0]
    # the ring: the maximum is shared by points (±a, ±b), (±b, ±a); the smallest index wins
    ring = V[:, at["ring"]]
    ties = np.flatnonzero(ring == ring.max())
    assert len(ties) >= 2, ties
    i, j = pts[ties[0]]
    assert j < 0 and got_kind[at["ring"]] == 0
    assert np.abs(got_n[at["ring"]] - n[at["ring"]]).max() <= 1e-6
    assert abs(got_n[at["ring"]][0] - i / G) <= 0.5 / G + 1e-6 and abs(got_n[at["ring"]][1] - j / G) <= 0.5 / G + 1e-6


def off_boundary(cuda, a, pad):
    """The array in a buffer that starts `pad` elements past a 16-byte boundary."""
    t = torch.tensor(np.ascontiguousarray(a), device=cuda)
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=cuda)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (pad * t.element_size()) % 16
    return v


def run_into(cuda, coef, k, P, layout="pixel", nl="pixel", G=10, weights=None):
    n = torch.empty((P, 3) if nl == "pixel" else (3, P), device=cuda)
    kind = torch.empty(P, dtype=torch.uint8, device=cuda)
    peak = torch.empty(P, device=cuda)
    rti.hsh_normals_into(coef, rti.peak_table(f"hsh{k}", G, cuda), n, kind, peak, basis=f"hsh{k}", layout=layout,
                         normal_layout=nl, grid=G, weights=weights)
    return n, kind, peak


@pytest.mark.parametrize("P", [257, 1000])
@pytest.mark.parametrize("k", KS)
def test_paths_agree_to_the_bit(cuda, k, P):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    m = maps_of(P, k, 3)
    md = torch.tensor(m, device=cuda)
    base = rti.hsh_normals(md, f"hsh{k}", return_kind=True, return_peak=True)
    assert same_bits(run_into(cuda, md, k, P), base)
    assert same_bits(torch.ops.rti.hsh_normals(md, k), base)
    assert same_bits(run_into(cuda, off_boundary(cuda, m, 2), k, P), base)  # 8 bytes off: per lane
    # a channel stride that is no multiple of 4: channel 1 starts off a 16-byte boundary
    cs = P * k + (1 if (P * k + 1) % 4 else 2)
    buf = torch.zeros(3 * cs, device=cuda)
    strided = torch.as_strided(buf, (3, P, k), (cs, k, 1))
    strided.copy_(md)
    assert strided.stride(0) % 4 != 0 and same_bits(run_into(cuda, strided, k, P), base)
    # planar maps, planar normals
    pl = torch.tensor(laid_out(m, "planar"), device=cuda)
    n_pl, kind_pl, peak_pl = run_into(cuda, pl, k, P, layout="planar", nl="planar")
    assert same_bits((n_pl.T, kind_pl, peak_pl), base)
    assert same_bits(torch.ops.rti.hsh_normals(pl, k, True, True), (base[0].T, base[1], base[2]))
    # one map, 8 bytes off
    one = rti.hsh_normals(md[1], f"hsh{k}", return_kind=True, return_peak=True)
    assert same_bits(run_into(cuda, off_boundary(cuda, m[1], 2), k, P), one)
    torch.library.opcheck(torch.ops.rti.hsh_normals.default, (md, k), test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("G", [4, 10])
@pytest.mark.parametrize("P", [63, 257, 1000])
@pytest.mark.parametrize("k", KS)
def test_bytes_and_fp32_agree(cuda, k, P, G):
    from rti import ops  # noqa: F401

    q = rti.quantise_hsh(torch.tensor(maps_of(P, k, 3), device=cuda).nan_to_num(0.0, 1e3, -1e3), f"hsh{k}")
    want = rti.hsh_normals(rti.dequantise_hsh(q), q.basis, grid=G, return_kind=True, return_peak=True)
    got = rti.hsh8_normals(q, grid=G, return_kind=True, return_peak=True)
    assert same_bits(got, want) and int((want[1] == 0).sum()) > P // 2
    assert same_bits(torch.ops.rti.hsh8_normals(q.coef, q.qparams, False, G), want)
    off = rti.QuantisedHSH(off_boundary(cuda, q.coef.cpu().numpy(), 1), q.qparams, q.basis)  # per lane
    assert same_bits(rti.hsh8_normals(off, grid=G, return_kind=True, return_peak=True), want)
    planar = rti.hsh8_normals(q, grid=G, normal_layout="planar")
    assert torch.equal(bits(planar.T), bits(want[0]))
    n = torch.empty((P, 3), device=cuda)
    rti.hsh8_normals_into(q.coef, q.qparams, rti.peak_table(q.basis, G, cuda), n, basis=q.basis, grid=G)
    assert torch.equal(bits(n), bits(want[0]))
    if G == 10 and P == 257:
        torch.library.opcheck(torch.ops.rti.hsh8_normals.default, (q.coef, q.qparams),
                              test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("k", KS)
def test_weights(cuda, k):
    P = 257
    md = torch.tensor(maps_of(P, k, 3), device=cuda)
    red = rti.hsh_normals(md[0].contiguous(), f"hsh{k}", return_kind=True, return_peak=True)
    got = rti.hsh_normals(md, f"hsh{k}", weights=(1, 0, 0), return_kind=True, return_peak=True)
    finite = torch.isfinite(md).all(dim=-1).all(dim=0)  # 0·inf is NaN: the hand-made inf pixel of another channel
    assert same_bits([t[finite] for t in got], [t[finite] for t in red])
    other = rti.hsh_normals(md, f"hsh{k}", weights=(0.2, 0.3, 0.5))
    want = peak_normals(rti.relight(torch.tensor(luminance(maps_of(P, k, 3), (0.2, 0.3, 0.5)), device=cuda),
                                    *grid_dirs(10), basis=f"hsh{k}").cpu().numpy(), 10,
                        luminance(maps_of(P, k, 3), (0.2, 0.3, 0.5)))
    ok = want[1] != 4
    assert np.abs(other.cpu().numpy()[ok].astype(np.float64) - want[0][ok]).max() <= 1e-6
    with pytest.raises(ValueError):
        rti.hsh_normals(md, f"hsh{k}", weights=(1, 0))
    with pytest.raises(ValueError, match="weight"):
        rti.hsh_normals(md, f"hsh{k}", weights=(1, float("nan"), 0))


def angles_deg(n, truth):
    c = (n.double() * truth.double()).sum(-1).clamp(-1, 1)
    return torch.rad2deg(torch.acos(c))


def test_end_to_end_from_a_fit(cuda):
    """A Lambertian RGB stack of 32×32 pixels, tilts <= 30°, under synth_dirs(40, 1), fitted with HSH-16: the
    normals of the fp32 fit lie within the bound pinned on the CPU.  Those from the bytes lie within that bound plus
    the quantisation's effect, which is bounded from the header: a grid value moves by at most eps = max over the
    grid of Σ_j |b_j|·step_j/2 (the luminance weights sum to 1), so the byte map's peak lies where the fp32 function
    is within 2·eps of its maximum A; for A·cos θ that is θ <= arccos(1 − 2·eps/A), and the argmax may also land one
    grid cell away, (1/G)/cos 30° radians.  The measured distance is printed."""
    import rti_oracle as o

    H = W = 32
    lu, lv = o.synth_dirs(40, 1)
    lw = np.sqrt(np.maximum(0.0, 1.0 - lu.astype(np.float64) ** 2 - lv.astype(np.float64) ** 2))
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    tilt, az = np.radians(30.0 * np.sqrt(yy)), 2 * np.pi * xx + 0.1
    truth = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], -1)
    shade = np.maximum(0.0, np.einsum("nc,hwc->nhw", np.stack([lu, lv, lw], 1), truth))
    I = np.stack([a * shade for a in (200.0, 150.0, 100.0)]).astype(np.float32)
    coef = rti.fit(torch.tensor(I, device=cuda), lu, lv, basis="hsh16")
    assert coef.shape == (3, H, W, 16)
    n, kind, albedo = rti.hsh_normals(coef, "hsh16", return_kind=True, return_peak=True)
    t = torch.tensor(truth, device=cuda)
    err = float(angles_deg(n, t).max())
    q = rti.quantise_hsh(coef, "hsh16")
    n8, albedo8 = rti.hsh8_normals(q, return_peak=True)
    err8, shift = float(angles_deg(n8, t).max()), float(angles_deg(n8, n).max())
    G = 10
    eps = float((np.abs(rti.basis_eval(*grid_dirs(G), "hsh16")) @ (q.scale.astype(np.float64) / 255.0 / 2)).max())
    A = float(albedo.min())
    shift_bound = float(np.degrees(np.arccos(max(-1.0, 1.0 - 2.0 * eps / A)) + (1.0 / G) / np.cos(np.radians(30.0))))
    print(f"worst angular error: fp32 fit {err:.3f} deg, bytes {err8:.3f} deg; bytes against fp32 {shift:.3f} deg "
          f"(eps {eps:.3f}, A {A:.1f}, bound {shift_bound:.2f} deg)")
    assert n.shape == (H, W, 3) and bool((kind == 0).all()) and err <= ACCURACY_BOUND_DEG
    assert shift <= shift_bound and err8 <= ACCURACY_BOUND_DEG + shift_bound
    img = rti.shade_normals(rti.normals_unsharp(n8, 2.0, 1.5), 0.3, -0.2, albedo=albedo8, ks=150, exp=75)
    assert img.shape == (H, W) and bool(torch.isfinite(img).all()) and float(img.max()) > 0
    assert rti.shade_normals(n, 0.3, -0.2, albedo=albedo).shape == (H, W)


def test_graph_capture_replays_the_eager_bits(cuda):
    """hsh_normals_into then hsh8_normals_into, captured once (a single chain, no parallel branches) and replayed on
    other data."""
    P, k = 1000, 16
    first, second = maps_of(P, k, 3), maps_of(1000, 16, 3)[:, ::-1].copy()
    md = torch.tensor(first, device=cuda)
    q = rti.quantise_hsh(torch.tensor(second, device=cuda).nan_to_num(0.0, 1e3, -1e3))
    c8 = q.coef.clone()
    table = rti.peak_table("hsh16", 10, cuda)  # built before the capture
    outs = [torch.empty((P, 3), device=cuda), torch.empty(P, dtype=torch.uint8, device=cuda), torch.empty(P, device=cuda)]
    outs8 = [torch.empty_like(t) for t in outs]

    def chain():
        rti.hsh_normals_into(md, table, *outs)
        rti.hsh8_normals_into(c8, q.qparams, table, *outs8)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    md.copy_(torch.tensor(second, device=cuda))
    graph.replay()
    torch.cuda.synchronize(cuda)
    assert same_bits(outs, rti.hsh_normals(md, return_kind=True, return_peak=True))
    assert same_bits(outs8, rti.hsh8_normals(q, return_kind=True, return_peak=True))
    assert int((outs[1] == 0).sum()) > P // 2


def test_api_shapes_and_refusals(cuda):
    H, W, k = 6, 11, 16
    m = torch.tensor(maps_of(H * W, k, 3).reshape(3, H, W, k), device=cuda)
    n, kind, peak = rti.hsh_normals(m, return_kind=True, return_peak=True)
    assert n.shape == (H, W, 3) and kind.shape == peak.shape == (H, W) and kind.dtype == torch.uint8
    assert rti.hsh_normals(m[0]).shape == (H, W, 3) and rti.hsh_normals(m[0].reshape(-1, k)).shape == (H * W, 3)
    flat = rti.hsh_normals(m.reshape(3, H * W, k))
    assert flat.shape == (H * W, 3) and torch.equal(bits(flat), bits(n.reshape(-1, 3)))
    pl = rti.hsh_normals(m.permute(0, 3, 1, 2).contiguous(), layout="planar", normal_layout="planar")
    assert pl.shape == (3, H, W) and torch.equal(bits(pl.permute(1, 2, 0)), bits(n))
    assert rti.hsh_normals(m[1].permute(2, 0, 1).contiguous(), layout="planar").shape == (H, W, 3)
    assert rti.hsh_normals(m[..., :9].contiguous(), "hsh9", grid=4).shape == (H, W, 3)
    assert rti.peak_table("hsh16", 10, cuda) is rti.peak_table("hsh16", 10, cuda)
    with pytest.raises(NotImplementedError):
        rti.hsh_normals(m[..., :6].contiguous(), "ptm")
    with pytest.raises(NotImplementedError):
        rti.normals(m[0], basis="hsh16")  # the PTM entry keeps refusing HSH
    with pytest.raises(ValueError, match="terms"):
        rti.hsh_normals(m, "hsh9")
    with pytest.raises(ValueError, match="grid"):
        rti.hsh_normals(m, grid=3)
    with pytest.raises(ValueError):
        rti.hsh_normals(m.double())
    with pytest.raises(ValueError, match="table"):
        rti.hsh_normals_into(m, rti.peak_table("hsh16", 4, cuda), torch.empty((H * W, 3), device=cuda))
