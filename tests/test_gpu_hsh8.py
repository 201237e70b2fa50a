"""8-bit RGB HSH maps on the GPU (rti_hsh8.hip) against tests/hsh8_ref.py (the header's arithmetic op by op in NumPy)
for the 2k header floats, the bytes and the dequantised maps, and against rti.relight of the dequantised maps for
the images.  Every comparison but the accuracy bound is exact: bytes, and bit patterns of fp32 / int32 values.

Sizes: one pixel per lane throughout, so 1 and 7 are a partial wave, 255 is one pixel short of a workgroup (three
full waves and a 63-pixel one), 256 one workgroup of full waves, 1073 and 1076 four workgroups and a 49 / 52-pixel
tail (1076 % 4 == 0: the uint8 images go out as dwords), 3077 thirteen workgroups.  BIG = 768·256 + 2·256 + 77 =
197197: the extremes' grid is capped at 768 workgroups of 256 pixels, so the 771 chunks make workgroups 0, 1 and 2
fold a second chunk (the last a 77-pixel one) and the tail kernel folds 768 partials with 256 lanes, three per
lane.  BIG runs once per k.  Maps run in both layouts, 16-byte aligned and 8 bytes off; the bytes 16-byte aligned
and 1 byte off a dword; every output between guard elements."""
import functools

import numpy as np
import pytest
import torch

import rti
from hsh8_ref import finite_hsh, host_dequantise, host_qparams, host_quantise, mixed_hsh

pytestmark = pytest.mark.gpu

BIG = 768 * 256 + 2 * 256 + 77
SIZES = [1, 7, 255, 256, 1073, 1076, 3077]
KS = [9, 16]
ES = [1, 2, 65]
OUT_DTYPES = [torch.float32, torch.int32, torch.uint8]


@functools.lru_cache(maxsize=None)
def dirs(E):
    """(0.3, -0.45), then (0.8, 0.75) with lu² + lv² > 1, then the pole, then seeded ones."""
    rng = np.random.default_rng(65)
    lu = np.concatenate([[0.3, 0.8, 0.0], rng.uniform(-0.7, 0.7, 62)])[:E]
    lv = np.concatenate([[-0.45, 0.75, 0.0], rng.uniform(-0.7, 0.7, 62)])[:E]
    return lu, lv


@functools.lru_cache(maxsize=None)
def case(P, k):
    """(maps [3, P, k] fp32, qparams [2k], raw [P, 3, k], dequantised [3, P, k]) of the host -- computed once,
    shared and never written."""
    m = mixed_hsh(P, k, 7000 + P + k)
    qp = host_qparams(m)
    raw = host_quantise(m, qp)
    deq = host_dequantise(raw, qp)
    for a in (m, qp, raw, deq):
        a.setflags(write=False)
    return m, qp, raw, deq


def on_device(cuda, a, offset):
    """The host array on the device as it is laid out; offset: it starts 8 bytes (uint8: 1 byte) into a 16-byte
    aligned buffer."""
    t = torch.as_tensor(np.array(a, order="C"), device=cuda)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    pad = 1 if t.dtype == torch.uint8 else 8 // t.element_size()
    buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=cuda)
    v = buf[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == pad * t.element_size() and v.is_contiguous()
    return v


def guarded(cuda, n, dtype, offset):
    """(buffer, view of n elements, lead, fill) with at least 16 guard elements on both sides; the view is 16-byte
    aligned, or with offset 1 byte (uint8) / 8 bytes (4-byte types) off."""
    fill = 77 if dtype == torch.uint8 else -7
    buf = torch.full((n + 48,), fill, dtype=dtype, device=cuda)
    lead = 16 + ((1 if dtype == torch.uint8 else 2) if offset else 0)
    return buf, buf[lead:lead + n], lead, fill


def guards_untouched(buf, lead, n, fill):
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + n:] == fill).all())


def laid_out(m, layout):
    return np.ascontiguousarray(m.transpose(0, 2, 1)) if layout == "planar" else m


def bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def run_quantiser(cuda, m, k, layout, offset):
    """rti_hsh_qparams + rti_hsh_quantise through the _into forms, outputs between guards, the workspace holding
    NaN bit patterns -> (qparams [2k], coef8 [P, 3, k]) on the host, guards checked."""
    P = m.shape[1]
    basis = f"hsh{k}"
    md = on_device(cuda, laid_out(m, layout), offset)
    ws = torch.full((rti.hsh_qparams_workspace(P, basis),), 0xFF, dtype=torch.uint8, device=cuda)
    qbuf, qp, qlead, qfill = guarded(cuda, 2 * k, torch.float32, False)
    cbuf, c8, clead, cfill = guarded(cuda, 3 * k * P, torch.uint8, offset)
    rti.hsh_qparams_into(md, ws, qp, basis=basis, layout=layout)
    rti.hsh_quantise_into(md, qp, c8, basis=basis, layout=layout)
    assert guards_untouched(qbuf, qlead, 2 * k, qfill) and guards_untouched(cbuf, clead, 3 * k * P, cfill)
    return qp.cpu().numpy(), c8.cpu().numpy().reshape(P, 3, k)


def check_quantiser(cuda, P, k, layout, offset):
    m, want_qp, want_raw, want_deq = case(P, k)
    qp, c8 = run_quantiser(cuda, m, k, layout, offset)
    print(f"P={P} k={k}: scale {qp[:k]} bias {qp[k:]}")
    assert same_bits(qp, want_qp)
    assert np.array_equal(c8, want_raw)
    if P >= 255:  # the comparison is of bytes inside the range, not of saturated terms
        live = [j for j in range(k) if j not in (5, 7)]
        inside = float(((want_raw[..., live] > 0) & (want_raw[..., live] < 255)).mean())
        print(f"P={P} k={k}: {inside:.3f} of the live terms' bytes strictly inside 1..254")
        assert inside > 0.9
        assert want_qp[5] == 1.0 and want_qp[k + 5] == 12.5 and not c8[..., 5].any()  # the constant term
    if P >= 256:
        assert want_qp[7] == 1.0 and want_qp[k + 7] == 0.0 and not c8[..., 7].any()   # the all-NaN term
    if P >= 8:  # the planted values: NaN -> 0, +inf -> 255, -inf -> 0
        assert c8[2, 0, 1] == 0 and c8[3, 1, 2] == 255 and c8[4, 2, 3] == 0
    q = rti.QuantisedHSH(torch.as_tensor(c8, device=cuda), torch.as_tensor(qp, device=cuda), f"hsh{k}")
    deq = rti.dequantise_hsh(q)
    assert deq.shape == (3, P, k) and deq.dtype == torch.float32
    assert same_bits(deq.cpu().numpy(), want_deq)


# ---- rti_hsh_qparams, rti_hsh_quantise, dequantise_hsh -----------------------------------------------------------

@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_quantiser_is_the_hosts(cuda, k, P, layout, offset):
    check_quantiser(cuda, P, k, layout, offset)


def planted(name, k):
    """A 2100-pixel map (eight workgroups and a 52-pixel tail) with the extremes of every term at chosen pixels,
    each in another channel."""
    P = 2100
    m = finite_hsh(P, k, 77).copy()
    lo_px, hi_px = {"0 and P-1": (0, P - 1), "P-1 and 0": (P - 1, 0), "63 and 64": (63, 64), "64 and 63": (64, 63),
                    "255 and 256": (255, 256), "256 and 255": (256, 255)}[name]
    for j in range(k):
        term = m[..., j]
        m[j % 3, lo_px, j] = term.min() - 100.0 - 7 * j
        m[(j + 1) % 3, hi_px, j] = term.max() + 100.0 + 11 * j
    return m


@pytest.mark.parametrize("name", ["0 and P-1", "P-1 and 0", "63 and 64", "64 and 63", "255 and 256", "256 and 255"])
@pytest.mark.parametrize("k", KS)
def test_extremes_at_the_seams(cuda, k, name):
    m = planted(name, k)
    want_qp = host_qparams(m)
    want_raw = host_quantise(m, want_qp)
    for layout in ("pixel", "planar"):
        for offset in (False, True):  # the staged path and the per-lane one
            qp, c8 = run_quantiser(cuda, m, k, layout, offset)
            assert same_bits(qp, want_qp), (layout, offset, qp, want_qp)
            assert np.array_equal(c8, want_raw), (layout, offset)


@pytest.mark.parametrize("k", KS)
def test_all_nan_maps(cuda, k):
    m = np.full((3, 300, k), np.nan, np.float32)
    qp, c8 = run_quantiser(cuda, m, k, "pixel", False)
    assert same_bits(qp, np.float32([1.0] * k + [0.0] * k)) and not c8.any()


# ---- rti_relight_hsh8 --------------------------------------------------------------------------------------------

def device_q(cuda, P, k, offset):
    """The host's quantised map of case(P, k) on the device (these tests do not lean on the device quantiser)."""
    _, qp, raw, _ = case(P, k)
    return on_device(cuda, raw, offset), on_device(cuda, qp, False)


def check_relight(cuda, P, k, offset, es):
    basis = f"hsh{k}"
    c8, qp = device_q(cuda, P, k, offset)
    fp32 = rti.dequantise_hsh(rti.QuantisedHSH(c8.clone(), qp, basis))
    assert fp32.shape == (3, P, k) and bool(torch.isfinite(fp32).all())
    for E in es:
        lu, lv = dirs(E)
        luv = torch.as_tensor(np.stack([lu, lv], -1), device=cuda)
        for dt in OUT_DTYPES:
            n = E * P * 3
            buf, view, lead, fill = guarded(cuda, n, dt, offset)
            got = rti.relight_hsh8_into(c8, qp, luv, view.view(E, P, 3), basis=basis)
            want = torch.stack([rti.relight(fp32[c], lu, lv, basis=basis, out_dtype=dt) for c in range(3)], -1)
            assert guards_untouched(buf, lead, n, fill), (E, dt)
            assert got.shape == want.shape == (E, P, 3)
            assert torch.equal(bits(got), bits(want)), (E, dt)
            assert P < 255 or bool(got.any()), (E, dt)  # images, not black frames


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k", KS)
def test_relight_hsh8_is_relight_of_the_dequantised_maps(cuda, k, P, offset):
    check_relight(cuda, P, k, offset, ES)


@pytest.mark.parametrize("k", KS)
def test_big(cuda, k):
    """Past the extremes' grid cap (see the module docstring): quantiser and relight, once per k."""
    check_quantiser(cuda, BIG, k, "pixel", False)
    check_relight(cuda, BIG, k, False, [2])


@pytest.mark.parametrize("P", [256, 1076])
@pytest.mark.parametrize("k", KS)
def test_paths_agree_to_the_bit(cuda, k, P):
    """The same pixels through the staged paths (aligned) and per lane (maps 8 bytes, bytes 1 byte off)."""
    m = case(P, k)[0]
    for layout in ("pixel", "planar"):
        a, b = run_quantiser(cuda, m, k, layout, False), run_quantiser(cuda, m, k, layout, True)
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    luv = torch.as_tensor(np.stack(dirs(65), -1), device=cuda)
    for dt in OUT_DTYPES:
        outs = []
        for offset in (False, True):
            c8, qp = device_q(cuda, P, k, offset)
            _, view, _, _ = guarded(cuda, 65 * P * 3, dt, offset)
            outs.append(bits(rti.relight_hsh8_into(c8, qp, luv, view.view(65, P, 3), basis=f"hsh{k}")))
        assert torch.equal(*outs), dt


@pytest.mark.parametrize("k", KS)
def test_accuracy_against_the_unquantised_maps(cuda, k):
    """|relight_hsh8 − rti.relight(fp32 maps)| <= Σ_j b_j·step_j/2 + 4·k·eps·Σ_j b_j·max|c_j| per direction, with
    b = |basis_eval(lu, lv)| in fp64 and eps = 2⁻²³: half a quantisation step per term, and slack for the two fp32
    chains.  Finite input, every pixel and channel counted."""
    P, basis = 3077, f"hsh{k}"
    m = finite_hsh(P, k, 31 + k)
    md = torch.as_tensor(m, device=cuda)
    q = rti.quantise_hsh(md, basis)
    lu, lv = dirs(8)
    got = rti.relight_hsh8(q, lu, lv).double()
    want = torch.stack([rti.relight(md[c], lu, lv, basis=basis) for c in range(3)], -1).double()
    b = np.abs(rti.basis_eval(lu, lv, basis))  # [E, k] fp64
    step = q.scale.astype(np.float64) / 255.0
    cmax = np.abs(m.astype(np.float64)).max(axis=(0, 1))
    bound = b @ (step / 2) + 4 * k * 2.0 ** -23 * (b @ cmax)
    err = (got - want).abs().amax(dim=(1, 2)).cpu().numpy()
    print(f"k={k}: max error / bound per direction {err / bound}")
    assert (err <= bound).all(), (err, bound)
    assert (err > 0).all()  # the comparison is of a quantised map


# ---- the Python layer, files, ops, graphs ------------------------------------------------------------------------

def test_api_shapes_and_refusals(cuda):
    H, W, k = 12, 21, 16
    m = torch.as_tensor(mixed_hsh(H * W, k, 5).reshape(3, H, W, k), device=cuda)
    q = rti.quantise_hsh(m)
    assert isinstance(q, rti.QuantisedHSH) and q.shape == (H, W) and q.device == m.device and q.basis == "hsh16"
    assert q.coef.shape == (H, W, 3, k) and q.qparams.shape == (2 * k,) and q.qparams.dtype == torch.float32
    qp = rti.quantise_hsh(m.permute(0, 3, 1, 2).contiguous(), layout="planar")
    assert torch.equal(qp.coef, q.coef) and torch.equal(bits(qp.qparams), bits(q.qparams))
    flat = rti.quantise_hsh(m.reshape(3, H * W, k), "hsh16")
    assert flat.shape == (H * W,) and torch.equal(flat.coef, q.coef.reshape(-1, 3, k))
    q9 = rti.quantise_hsh(m[..., :9].contiguous(), "hsh9")
    assert q9.k == 9 and q9.coef.shape == (H, W, 3, 9)
    out = rti.relight_hsh8(q, *dirs(2))
    assert out.shape == (2, H, W, 3) and out.dtype == torch.float32
    one = rti.relight_hsh8(q, 0.3, -0.45, out_dtype=torch.uint8)
    assert one.shape == (H, W, 3) and one.dtype == torch.uint8
    assert rti.relight_hsh8(flat, 0.3, -0.45).shape == (H * W, 3)
    d = rti.dequantise_hsh(q)
    assert d.shape == (3, H, W, k) and d.dtype == torch.float32 and d.device == m.device
    host = q.to("cpu")
    assert host.device.type == "cpu" and torch.equal(host.coef, q.coef.cpu())
    assert torch.equal(bits(rti.dequantise_hsh(host)), bits(d.cpu()))  # the same arithmetic on either device
    with pytest.raises(ValueError, match="CUDA"):
        rti.relight_hsh8(host, 0.1, 0.2)
    with pytest.raises(ValueError, match="terms"):
        rti.quantise_hsh(m, "hsh9")
    with pytest.raises(NotImplementedError):
        rti.quantise_hsh(m[..., :6].contiguous(), "ptm")
    with pytest.raises(ValueError):
        rti.quantise_hsh(m.half())
    with pytest.raises(ValueError):
        rti.relight_hsh8(q, 0.1, 0.2, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="workspace"):
        rti.hsh_qparams_into(m, torch.empty(8, dtype=torch.uint8, device=cuda), q.qparams)
    with pytest.raises(ValueError, match="qparams"):
        rti.hsh_quantise_into(m, q.qparams.double(), q.coef)
    with pytest.raises(ValueError, match="coef8"):
        rti.hsh_quantise_into(m, q.qparams, q.coef[:-1].contiguous())
    with pytest.raises(ValueError):
        rti.relight_hsh8_into(q.coef, q.qparams, torch.zeros((1, 2), device=cuda),
                              torch.empty((1, H * W, 3), device=cuda))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("H,W", [(24, 20), (5, 7)])
def test_device_and_host_write_the_same_file(cuda, tmp_path, H, W, k):
    """write_rti of the device-quantised map and of the fp32 maps (quantised on the host) are byte-identical, and
    a file round trip is exact: the loaded object is the written one."""
    basis = f"hsh{k}"
    m = mixed_hsh(H * W, k, 300 + H).reshape(3, H, W, k)
    q = rti.quantise_hsh(torch.as_tensor(m, device=cuda), basis)
    host_path = rti.write_rti(str(tmp_path / "host.rti"), m, basis)
    dev_path = rti.write_rti(str(tmp_path / "device.rti"), q)
    assert open(dev_path, "rb").read() == open(host_path, "rb").read()
    got_basis, back = rti.read_rti(dev_path)
    assert got_basis == basis and same_bits(rti.dequantise_hsh(q).cpu().numpy(), back)
    loaded = rti.read_rti(dev_path, quantised=True)[1].to(cuda)
    assert torch.equal(loaded.coef, q.coef) and torch.equal(bits(loaded.qparams), bits(q.qparams))
    lu, lv = dirs(2)
    assert torch.equal(rti.relight_hsh8(loaded, lu, lv, out_dtype=torch.uint8),
                       rti.relight_hsh8(q, lu, lv, out_dtype=torch.uint8))


def test_end_to_end_from_a_fit(cuda, tmp_path):
    """fit (HSH-9, colour stack) -> quantise_hsh -> file -> relight_hsh8 stays within the derived bound of
    test_accuracy_against_the_unquantised_maps of relighting the fp32 fit."""
    from rti_oracle import synth_dirs, synth_intensities

    k = 9
    lu, lv = synth_dirs(24, 0)
    I = np.stack([synth_intensities(20, 28, lu, lv, seed=s) for s in range(3)])
    coef = rti.fit(torch.as_tensor(I, device=cuda).float(), lu, lv, basis="hsh9")
    assert coef.shape == (3, 20, 28, k) and bool(torch.isfinite(coef).all())
    path = rti.write_rti(str(tmp_path / "object.rti"), rti.quantise_hsh(coef, "hsh9"))
    q = rti.read_rti(path, quantised=True)[1].to(cuda)
    got = rti.relight_hsh8(q, 0.25, -0.4)
    want = torch.stack([rti.relight(coef[c], 0.25, -0.4, basis="hsh9") for c in range(3)], -1)
    b = np.abs(rti.basis_eval(0.25, -0.4, "hsh9"))[0]
    cmax = coef.abs().amax(dim=(0, 1, 2)).cpu().numpy().astype(np.float64)
    bound = b @ (q.scale.astype(np.float64) / 255.0 / 2) + 4 * k * 2.0 ** -23 * (b @ cmax)
    err = float((got.double() - want.double()).abs().max())
    print(f"max |hsh8 - fp32| = {err:.3f} grey levels (bound {bound:.3f}), image max {float(want.max()):.1f}")
    assert got.shape == (20, 28, 3) and float(want.max()) > 50 and err <= bound


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("k", KS)
def test_torch_ops(cuda, k, planar):
    from rti import ops  # noqa: F401  registers torch.ops.rti.*

    P, basis = 1076, f"hsh{k}"
    m = case(P, k)[0]
    md = on_device(cuda, laid_out(m, "planar" if planar else "pixel"), False)
    q = rti.quantise_hsh(md, basis, layout="planar" if planar else "pixel")
    c8, qp = torch.ops.rti.hsh_quantise(md, k, planar)
    assert c8.shape == (P, 3, k) and qp.shape == (2 * k,) and c8.dtype == torch.uint8 and qp.dtype == torch.float32
    assert torch.equal(c8, q.coef) and torch.equal(bits(qp), bits(q.qparams))
    torch.library.opcheck(torch.ops.rti.hsh_quantise.default, (md, k, planar), test_utils=("test_schema", "test_faketensor"))
    lu, lv = dirs(2)
    luv = torch.as_tensor(np.stack([lu, lv], -1))
    for dt in OUT_DTYPES:
        got = torch.ops.rti.relight_hsh8(c8, qp, luv, dt)
        want = rti.relight_hsh8(q, lu, lv, out_dtype=dt)
        assert got.shape == want.shape == (2, P, 3) and got.dtype == dt and torch.equal(bits(got), bits(want))
        torch.library.opcheck(torch.ops.rti.relight_hsh8.default, (c8, qp, luv, dt),
                              test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError):
        torch.ops.rti.hsh_quantise(md.transpose(1, 2).contiguous(), k, planar)
    with pytest.raises(ValueError):
        torch.ops.rti.relight_hsh8(c8[:, :2], qp, luv, torch.float32)
    with pytest.raises(NotImplementedError):
        torch.ops.rti.hsh_quantise(md, 4, planar)


def test_graph_capture_replays_the_eager_bytes(cuda):
    """hsh_quantise_into then relight_hsh8_into, captured once (a single chain, no parallel branches) and replayed
    once on other data."""
    P, k, basis = 3077, 16, "hsh16"
    first, second = case(P, k)[0], mixed_hsh(P, k, 9)
    md = on_device(cuda, first, False)
    luv = torch.as_tensor(np.stack(dirs(2), -1), device=cuda)
    ws = torch.empty(rti.hsh_qparams_workspace(P, basis), dtype=torch.uint8, device=cuda)
    qp = torch.empty(2 * k, dtype=torch.float32, device=cuda)
    c8 = torch.empty((P, 3, k), dtype=torch.uint8, device=cuda)
    out = torch.empty((2, P, 3), dtype=torch.uint8, device=cuda)

    def chain():
        rti.hsh_qparams_into(md, ws, qp, basis=basis)
        rti.hsh_quantise_into(md, qp, c8, basis=basis)
        rti.relight_hsh8_into(c8, qp, luv, out, basis=basis)

    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        chain()  # loads the kernels before the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    md.copy_(torch.as_tensor(second, device=cuda))
    graph.replay()
    torch.cuda.synchronize(cuda)
    replayed = [t.clone() for t in (qp, c8, out)]
    q = rti.quantise_hsh(md, basis)
    assert torch.equal(bits(replayed[0]), bits(q.qparams)) and torch.equal(replayed[1], q.coef)
    assert torch.equal(replayed[2], rti.relight_hsh8(q, *dirs(2), out_dtype=torch.uint8))
    assert bool(replayed[2].any())
