"""The stride and offset arguments of the stack entries (include/rti.h), driven on the GPU through ctypes.

rti/api.py always passes dense strides, so this module calls rti._lib.lib() directly with views built by
tests/stride_ref.py: a dense stack [C, N, P] embedded in a poisoned allocation (plane n of channel c at
off + c·cs + n·ls; NaN / INT32_MIN / 255 everywhere else; uint8 data drawn from 0..100 so one padding byte read
as data moves a coefficient far beyond the tolerance) and outputs in NaN-filled buffers with 64-element guards.
Every call is held to three checks:

 (a) guards: every guard and gap element of every output keeps its NaN bit pattern (int32 views);
 (b) oracle: the written values match the fp64 oracle on the dense data at the tolerance of the entry's dense test;
 (c) bits: equal to the dense call on the same data, bit for bit, wherever the same arithmetic runs.

Forms (stride_ref.form_pads; vec = 4 elements, 16 for uint8 stacks):
  aligned   lpad = vec, cpad = 2·vec, opad = 4, offsets 0: every 16-byte predicate of rti_stack.h holds, the vector
            kernels run -> (c) always;
  oddlight  lpad = 1: one element per lane;
  offset    cpad = 3, opad = 2, input and output bases 1 element off a 16-byte boundary: one element per lane.
In the two misaligned forms (c) is asserted where reading the kernel shows the same per-pixel operation order in
the one-element-per-lane form: the VALU stream of rti_fit_shared (fit_valu_body: one fmaf chain per coefficient
over n = 0..N-1 whatever VEC and NC are), which is also where RTI_KERNEL_MFMA / RTI_KERNEL_TILE fall back to for
k in {6, 9, 16} (so their output must equal the dense RTI_KERNEL_VALU call), the one-pass fit + residual
(fitres_body: fp64 fma chains over ascending n) and the robust fit's kept counts.  rti_fit_residual, the operator
entries and the per-pixel entry assert (b) only there.

Shapes: P = 1024 + 256 + 36 (a whole 1024-pixel staged chunk, a whole 256-pixel wave span, a ragged tail that is a
multiple of 4), C = 2, N = 37 for the fp32 streams that step 8 planes at a time, else 20.  The q8 / h16 entries
refuse P % 16 != 0 by contract, so they run P = 1024 + 256 + 32."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rti
import rti_oracle as o
import stride_ref as sr
from conftest import coef_close, golden, relight_close
from rti import _lib as L
from robust_ref import fit_robust_ref

pytestmark = pytest.mark.gpu

P0 = 1024 + 256 + 36
C0 = 2
NP_DT = {"f32": np.float32, "i32": np.int32, "u8": np.uint8}
RTI_DT = {"f32": L.RTI_F32, "i32": L.RTI_I32, "u8": L.RTI_U8}
LAYOUTS = (("pixel", L.RTI_COEF_PIXEL_MAJOR), ("planar", L.RTI_COEF_PLANAR))
TILE8 = L.RTI_KERNEL_TILE | 0x100 | (4 << L.RTI_KERNEL_CHUNKS_SHIFT) | (2 << L.RTI_KERNEL_TILE_DEPTH_SHIFT) | \
    (8 << L.RTI_KERNEL_TILE_WAVES_SHIFT)  # an 8-wave setting of test_lds_tile_wide_workgroup: (rc, depth) = (4, 2)
SELECTORS = {"auto": L.RTI_KERNEL_AUTO, "valu": L.RTI_KERNEL_VALU, "mfma": L.RTI_KERNEL_MFMA,
             "tile": L.RTI_KERNEL_TILE, "tile8": TILE8}


# ---- plumbing ---------------------------------------------------------------------------------------------------
def vec_of(dt):
    return 16 if dt == "u8" else 4


def basis_of(k):
    return {6: "ptm", 9: "hsh9", 16: "hsh"}[k]


@functools.lru_cache(maxsize=None)
def lights(N):
    return o.synth_dirs(N, 100 + N)


@functools.lru_cache(maxsize=None)
def design64(k, N):
    lu, lv = lights(N)
    return o.design("ptm" if k <= 6 else "hsh", lu, lv)[:, :k]


@functools.lru_cache(maxsize=None)
def pinv64(k, N):
    return np.linalg.pinv(design64(k, N))


@functools.lru_cache(maxsize=None)
def stack(N, P=P0, C=C0):
    """integer samples 0..100 [C, N, P] (int64; cast per dtype), never changed"""
    a = np.random.default_rng(7 * N + P).integers(0, 101, (C, N, P))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def fit_ref(k, N, P=P0):
    """fp64 oracle coefficients [C, P, k] of stack(N, P)"""
    return np.stack([o.fit_shared(stack(N, P)[c].astype(np.float64), pinv64(k, N)) for c in range(C0)])


def dev(a, cuda):
    t = torch.as_tensor(np.ascontiguousarray(a), device=cuda)
    assert t.data_ptr() % 16 == 0  # the offsets below are element offsets from a 16-byte-aligned base
    return t


def ptr(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


class In:
    """a stack on the device: dense (form None) or embedded (stride_ref.embed_stack)"""

    def __init__(self, cuda, dense, form, dt, poison=None):
        dense = np.asarray(dense).astype(NP_DT[dt])
        self.C, self.N, self.P = dense.shape
        if form is None:
            self.t, self.ls, self.cs, self.off = dev(dense, cuda), self.P, self.N * self.P, 0
        else:
            pads = sr.form_pads(form, vec_of(dt))
            buf, b, self.ls, self.cs = sr.embed_stack(dense, pads["lpad"], pads["cpad"], pads["off"], poison)
            self.t, self.off = dev(buf, cuda), b.start
        self.ptr = ptr(self.t, self.off)
        self.dt = RTI_DT[dt]


class Out:
    """an output on the device: NaN-filled, the payload blocks between guards"""

    def __init__(self, cuda, blocks, dtype=np.float32):
        self.b = blocks
        self.t = dev(sr.nan_buffer(blocks, dtype), cuda)
        self.ptr = ptr(self.t, blocks.start)
        self._host = None

    def host(self):
        if self._host is None:
            self._host = self.t.cpu().numpy()
        return self._host

    def refresh(self):
        """forget the host copy: the next check reads the device buffer again (an Out used for more than one call)"""
        self._host = None

    def payload(self):
        return self.b.gather(self.host())

    def guards_ok(self, what):
        bad = sr.clobbered(self.host(), self.b)
        assert bad.size == 0, (what, "written outside the payload at", bad[:8].tolist(), "of", self.b.size)

    def untouched(self):
        return sr.untouched(self.host())


def coef_out(cuda, form, k, P=P0, C=C0):
    pads = sr.form_pads(form) if form else dict(opad=0, ooff=0)
    b, ocs = sr.out_blocks(C, P * k, pads["opad"], pads["ooff"])
    return Out(cuda, b), ocs


def map_out(cuda, form, P=P0, C=C0, dtype=np.float32):
    """res / kept [C][P]: dense by contract (no stride argument), so the form only moves the base"""
    b, _ = sr.out_blocks(1, C * P, 0, sr.form_pads(form)["ooff"] if form else 0)
    return Out(cuda, b, dtype)


def as_pk(payload, k, layout):
    """coefficient payload [C, P·k] -> [C, P, k]"""
    C = payload.shape[0]
    return payload.reshape(C, -1, k) if layout == "pixel" else payload.reshape(C, k, -1).transpose(0, 2, 1)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def assert_coef(got, ref, rtol, what):
    for c in range(got.shape[0]):
        err, ok = coef_close(got[c], ref[c], rtol=rtol)
        print(f"{what} channel {c}: max |Δ| / max|c_ref| = {err:.3g} (bound {rtol:g})")
        assert ok, (what, c, err)


# ---- rti_fit_shared ---------------------------------------------------------------------------------------------
def fit_shared(cuda, k, N, dt, form, layout_id, kernel, P=P0):
    pv = dev(pinv64(k, N).astype(np.float32), cuda)
    i = In(cuda, stack(N, P), form, dt)
    out, ocs = coef_out(cuda, form, k, P)
    st = L.lib().rti_fit_shared(ptr(pv), k, N, i.ptr, i.dt, P, C0, i.ls, i.cs, out.ptr, layout_id, ocs, kernel,
                                stream(cuda))
    torch.cuda.synchronize()
    return st, out


FIT_CASES = [(k, dt, sel) for k in (6, 9, 16) for dt in ("f32", "i32", "u8") for sel in SELECTORS
             if sel != "tile8" or dt == "f32"]  # the 8-wave tile kernels take fp32 stacks only


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("k,dt,sel", FIT_CASES, ids=[f"k{k}-{dt}-{sel}" for k, dt, sel in FIT_CASES])
def test_fit_shared(cuda, k, dt, sel, form):
    """Every selector × dtype × basis × layout.  Bits: equal to the dense call of the same selector in the aligned
    form and, for AUTO / VALU, in the misaligned forms too (same fmaf chain per pixel).  MFMA / TILE in a
    misaligned form take the documented way out for k in {6, 9, 16}, the one-chunk VALU stream (never a fault,
    never RTI_ERR_UNSUPPORTED): their output equals the dense RTI_KERNEL_VALU call bit for bit."""
    N = 37
    ref = fit_ref(k, N)
    for layout, lid in LAYOUTS:
        what = f"rti_fit_shared k={k} {dt} {sel} {layout} {form}"
        st, out = fit_shared(cuda, k, N, dt, form, lid, SELECTORS[sel])
        assert st == L.RTI_OK, (what, L.lib().rti_last_error())
        out.guards_ok(what)
        got = as_pk(out.payload(), k, layout)
        assert not np.isnan(got).any(), (what, "NaN in the output: poison was read or a pixel was not written")
        assert_coef(got, ref, 1e-4, what)
        same_path = form == "aligned" or sel in ("auto", "valu")
        st, dense = fit_shared(cuda, k, N, dt, None, lid, SELECTORS[sel if same_path else "valu"])
        assert st == L.RTI_OK
        assert bits_equal(got, as_pk(dense.payload(), k, layout)), (what, "differs from the dense call")


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("sel", ["mfma", "tile"])
def test_fit_shared_k5_matrix_core_only(cuda, sel, form):
    """k outside {6, 9, 16} has no VALU stream to fall back to: the matrix-core selectors fit it on 4-element
    aligned views and refuse a misaligned one with RTI_ERR_UNSUPPORTED before any launch (nothing written)."""
    k, N = 5, 37
    for layout, lid in LAYOUTS:
        st, out = fit_shared(cuda, k, N, "f32", form, lid, SELECTORS[sel])
        if form == "aligned":
            assert st == L.RTI_OK, L.lib().rti_last_error()
            out.guards_ok((sel, layout))
            assert_coef(as_pk(out.payload(), k, layout), fit_ref(k, N), 1e-4, f"k=5 {sel} {layout}")
        else:
            assert st == L.RTI_ERR_UNSUPPORTED, (sel, form, st)
            assert out.untouched()


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("sel", ["auto", "valu"])
def test_fit_shared_u8_16_pixel_lanes(cuda, sel, form):
    """PTM-6 on uint8 stacks loads 16 pixels per lane, which P = 1316 rules out even for a dense stack: the same
    checks at P = 1024 + 256 + 32, where the aligned form (pads of 16 and 32 bytes) keeps the 16-byte loads and
    AUTO's LDS-staged stores, and the misaligned forms drop to one pixel per lane with the same bits."""
    k, N = 6, 37
    for layout, lid in LAYOUTS:
        what = f"rti_fit_shared k=6 u8 {sel} {layout} {form} P={P16}"
        st, out = fit_shared(cuda, k, N, "u8", form, lid, SELECTORS[sel], P16)
        assert st == L.RTI_OK, (what, L.lib().rti_last_error())
        out.guards_ok(what)
        got = as_pk(out.payload(), k, layout)
        assert not np.isnan(got).any(), what
        assert_coef(got, fit_ref(k, N, P16), 1e-4, what)
        st, dense = fit_shared(cuda, k, N, "u8", None, lid, SELECTORS[sel], P16)
        assert st == L.RTI_OK
        assert bits_equal(got, as_pk(dense.payload(), k, layout)), (what, "differs from the dense call")


def gen_case(cuda, k, N, P, unit_px, per):
    """AUTO (launch generations) against RTI_KERNEL_ONE_LAUNCH on one padded view (cpad = 8, opad = 4) built on
    the device; `per`·`unit_px` pixels per part."""
    C, cpad, opad = 2, 8, 4
    cs, ocs = N * P + cpad, P * k + opad
    g = torch.Generator(device=cuda).manual_seed(k + N)
    I = torch.full((C * cs + sr.GUARD,), float("nan"), device=cuda)
    for c in range(C):
        I[c * cs:c * cs + N * P] = torch.randint(0, 101, (N * P,), generator=g, device=cuda, dtype=torch.uint8)
    pv = dev(pinv64(k, N).astype(np.float32), cuda)
    size = 2 * sr.GUARD + ocs + P * k
    outs = []
    for flags in (0, L.RTI_KERNEL_ONE_LAUNCH):
        coef = torch.full((size,), float("nan"), device=cuda)
        st = L.lib().rti_fit_shared(ptr(pv), k, N, ptr(I), L.RTI_F32, P, C, P, cs, ptr(coef, sr.GUARD),
                                    L.RTI_COEF_PIXEL_MAJOR, ocs, flags, stream(cuda))
        assert st == L.RTI_OK, L.lib().rti_last_error()
        outs.append((coef, int(L.lib().rti_last_launch_count())))
    torch.cuda.synchronize()
    (a, la), (b, lb) = outs
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert la > 1 and lb == 1, (la, lb)
    if cus == 256:
        assert la == 4, la  # 2 channels × 2 parts (valu_generations / tile_generations at 256 CUs)
    bits = torch.full((1,), float("nan"), device=cuda).view(torch.int32)
    ai = a.view(torch.int32)
    for lo, hi in ((0, sr.GUARD), (sr.GUARD + P * k, sr.GUARD + ocs), (sr.GUARD + ocs + P * k, size)):
        assert bool((ai[lo:hi] == bits).all()), ("guard or gap written", lo, hi)
    assert torch.equal(ai, b.view(torch.int32)), "launch generations differ from one launch"
    part = per * unit_px
    assert 0 < part < P
    px = np.unique(np.concatenate([np.random.default_rng(3).integers(0, P, 508), [0, part - 1, part, P - 1]]))
    assert px.size <= 512
    idx = torch.as_tensor(px, device=cuda)
    for c in range(C):
        got = a[sr.GUARD + c * ocs:sr.GUARD + c * ocs + P * k].reshape(P, k)[idx].cpu().numpy()
        assert not np.isnan(got).any()
        Ic = I[c * cs:c * cs + N * P].reshape(N, P)[:, idx].double().cpu().numpy()
        err, ok = coef_close(got, o.fit_shared(Ic, pinv64(k, N)), rtol=1e-4)
        print(f"generations k={k} channel {c}: {err:.3g}")
        assert ok, (c, err)


def test_fit_shared_generations_ptm6_padded_channels(cuda):
    """PTM-6 AUTO over padded channels.  valu_generations (256 CUs, 4 chunks per lane = 1024 pixels per wave)
    splits a channel once it has more than 2048 waves and keeps the split only when a part moves >= 256 MiB:
    P = 3480·1024 + 36 = 3 563 556 pixels (3481 waves -> 2 parts of 1741 and 1740 waves) and N = 38 planes
    (1741·1024·38·4 B = 258.4 MiB per part).  fp32 stack 2 × 38 × P × 4 B = 1.083 GB (1.009 GiB), coefficients
    2 × 171 MB; 4 launches."""
    gen_case(cuda, 6, 38, 3480 * 1024 + 36, 1024, 1741)


def test_fit_shared_generations_hsh16_padded_channels(cuda):
    """HSH-16 AUTO (the 8-wave 4096-pixel tile kernel) over padded channels.  tile_generations splits above
    4 × CUs = 1024 tiles in all and takes 2 parts per channel when 1 leaves a last round under 85 % full and 2 do
    not: 948 tiles per channel (948 % 256 = 180; 474 % 256 = 218), P = 947·4096 + 36 = 3 878 948, N = 20.
    fp32 stack 2 × 20 × P × 4 B = 621 MB, coefficients 2 × 248 MB; 4 launches."""
    gen_case(cuda, 16, 20, 947 * 4096 + 36, 4096, 474)


# ---- one-pass fit + residual, residual of given coefficients --------------------------------------------------------
def res_close(got, ref, atol, rtol):
    d = np.abs(np.asarray(got, np.float64) - ref)
    return float(d.max()), bool((d <= atol + rtol * ref).all())


def run_fitres(cuda, entry, k, N, dt, form, lid):
    lu, lv = lights(N)
    if entry == "svd":
        a, g = rti.lsq_factors(lu, lv, basis_of(k))
        fn = L.lib().rti_fit_shared_residual_svd
    else:
        a, g = rti.design_matrix(lu, lv, basis_of(k)), rti.gram_inverse(lu, lv, basis_of(k))
        fn = L.lib().rti_fit_shared_residual
    a, g = dev(np.asarray(a, np.float64), cuda), dev(np.asarray(g, np.float64), cuda)
    i = In(cuda, stack(N), form, dt)
    coef, ocs = coef_out(cuda, form, k)
    res = map_out(cuda, form)
    part = torch.zeros((C0, int(L.lib().rti_fit_shared_residual_blocks(P0))), dtype=torch.float64, device=cuda)
    st = fn(ptr(a), ptr(g), k, N, i.ptr, i.dt, P0, C0, i.ls, i.cs, coef.ptr, lid, ocs, res.ptr, ptr(part), 0,
            stream(cuda))
    torch.cuda.synchronize()
    assert st == L.RTI_OK, L.lib().rti_last_error()
    return coef, res, torch.sqrt(part.sum(dim=1) / (P0 * N)).cpu().numpy()


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("dt", ["f32", "u8"])
@pytest.mark.parametrize("k", [6, 16])
@pytest.mark.parametrize("entry", ["svd", "gram"])
def test_fit_shared_residual(cuda, entry, k, dt, form):
    """rti_fit_shared_residual_svd (coefficients to 1e-6, test_gpu_fitres.py) and rti_fit_shared_residual (Gram
    form, 1e-4, test_gpu_edge_solvers.py); residuals to 1e-4 + 1e-6·res_ref; the channel RMS from `partial` equals
    the dense call's to 1e-12, so no padding element was summed.  Bits equal the dense call in every form."""
    N = 37
    ref_c = fit_ref(k, N)
    for layout, lid in LAYOUTS:
        what = f"{entry} k={k} {dt} {layout} {form}"
        coef, res, rms = run_fitres(cuda, entry, k, N, dt, form, lid)
        coef.guards_ok(what + " coef")
        res.guards_ok(what + " res")
        got_c, got_r = as_pk(coef.payload(), k, layout), res.payload().reshape(C0, P0)
        assert not np.isnan(got_c).any() and not np.isnan(got_r).any(), what
        assert_coef(got_c, ref_c, 1e-6 if entry == "svd" else 1e-4, what)
        for c in range(C0):
            ref_r, _ = o.fit_residual(stack(N)[c].astype(np.float64), design64(k, N), ref_c[c])
            err, ok = res_close(got_r[c], ref_r, 1e-4, 1e-6)
            assert ok, (what, "res", c, err)
        dcoef, dres, drms = run_fitres(cuda, entry, k, N, dt, None, lid)
        assert np.isfinite(rms).all() and (np.abs(rms - drms) <= 1e-12 * drms).all(), (what, rms, drms)
        assert bits_equal(got_c, as_pk(dcoef.payload(), k, layout)), (what, "coef differs from the dense call")
        assert bits_equal(got_r, dres.payload().reshape(C0, P0)), (what, "res differs from the dense call")


def run_residual(cuda, k, N, dt, form, layout, lid):
    A = dev(design64(k, N).astype(np.float32), cuda)
    i = In(cuda, stack(N), form, dt)
    c32 = fit_ref(k, N).astype(np.float32)  # the coefficients the residual is taken of: [C, P, k]
    flat = (c32 if layout == "pixel" else c32.transpose(0, 2, 1)).reshape(C0, P0 * k)
    pads = sr.form_pads(form) if form else dict(opad=0, ooff=0)
    b, ocs = sr.out_blocks(C0, P0 * k, pads["opad"], pads["ooff"])
    cbuf = sr.nan_buffer(b)  # a coefficient INPUT here: NaN poison between the channels
    cbuf[b.index()] = flat
    cdev = dev(cbuf, cuda)
    res = map_out(cuda, form)
    part = torch.zeros((C0, int(L.lib().rti_fit_residual_blocks(P0))), dtype=torch.float64, device=cuda)
    st = L.lib().rti_fit_residual(ptr(A), k, N, i.ptr, i.dt, P0, C0, i.ls, i.cs, ptr(cdev, b.start), lid, ocs,
                                  res.ptr, ptr(part), stream(cuda))
    torch.cuda.synchronize()
    assert st == L.RTI_OK, L.lib().rti_last_error()
    return c32, res, torch.sqrt(part.sum(dim=1) / (P0 * N)).cpu().numpy()


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("dt", ["f32", "u8"])
@pytest.mark.parametrize("k", [6, 16])
def test_fit_residual(cuda, k, dt, form):
    """rti_fit_residual reads the stack AND a strided coefficient view: per pixel 1e-3 + 1e-4·res_ref on the given
    coefficients (test_gpu_residual.py), RMS equal to the dense call's to 1e-12, bits in the aligned form."""
    N = 20
    for layout, lid in LAYOUTS:
        what = f"rti_fit_residual k={k} {dt} {layout} {form}"
        c32, res, rms = run_residual(cuda, k, N, dt, form, layout, lid)
        res.guards_ok(what)
        got = res.payload().reshape(C0, P0)
        assert not np.isnan(got).any(), what
        for c in range(C0):
            ref_r, _ = o.fit_residual(stack(N)[c].astype(np.float64), design64(k, N), c32[c].astype(np.float64))
            err, ok = res_close(got[c], ref_r, 1e-3, 1e-4)
            assert ok, (what, c, err)
        _, dres, drms = run_residual(cuda, k, N, dt, None, layout, lid)
        assert np.isfinite(rms).all() and (np.abs(rms - drms) <= 1e-12 * drms).all(), (what, rms, drms)
        if form == "aligned":
            assert bits_equal(got, dres.payload().reshape(C0, P0)), (what, "differs from the dense call")


# ---- robust fit -----------------------------------------------------------------------------------------------------
ROBUST = dict(lo=1.0, hi=254.0, iters=3, delta=5.0)


@functools.lru_cache(maxsize=None)
def robust_ref(N):
    A = rti.design_matrix(*lights(N), "ptm")
    refs = [fit_robust_ref(A, stack(N)[c].astype(np.float64), **ROBUST) for c in range(C0)]
    for r in refs:  # no solve near a rank decision (robust_ref.check_inputs); the integer samples compare exactly
        assert (r["min_pivot"] >= 1e-6).all() and np.isnan(r["fail_pivot"]).all()
    return A, refs


def run_robust(cuda, N, dt, form, lid, poison):
    A, _ = robust_ref(N)
    i = In(cuda, stack(N), form, dt, poison)
    coef, ocs = coef_out(cuda, form, 6)
    res, kept = map_out(cuda, form), map_out(cuda, form, dtype=np.int32)
    fb = torch.zeros(1, dtype=torch.int32, device=cuda)
    st = L.lib().rti_fit_shared_robust(ptr(dev(A, cuda)), 6, N, i.ptr, i.dt, P0, C0, i.ls, i.cs, ROBUST["lo"],
                                       ROBUST["hi"], 6, ROBUST["iters"], ROBUST["delta"], coef.ptr, lid, ocs, res.ptr,
                                       kept.ptr, ptr(fb), 0, stream(cuda))
    torch.cuda.synchronize()
    assert st == L.RTI_OK, L.lib().rti_last_error()
    return coef, res, kept, int(fb.item())


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("dt,poison", [("u8", None), ("i32", 128), ("f32", None)])
def test_fit_shared_robust(cuda, dt, poison, form):
    """Window 1..254, 3 Huber passes.  The uint8 poison 255 lies outside the window, so the int32 run pads with
    128, inside it: a padding sample read as data changes `kept`.  kept equals the dense call's (and the
    reference's) exactly; coef (1e-4) and res (rtol 1e-4 + atol 1e-3) against tests/robust_ref.py."""
    N = 20
    _, refs = robust_ref(N)
    for layout, lid in LAYOUTS:
        what = f"rti_fit_shared_robust {dt} {layout} {form}"
        coef, res, kept, fb = run_robust(cuda, N, dt, form, lid, poison)
        for out, name in ((coef, "coef"), (res, "res"), (kept, "kept")):
            out.guards_ok(f"{what} {name}")
        got_c = as_pk(coef.payload(), 6, layout)
        got_r, got_k = res.payload().reshape(C0, P0), kept.payload().reshape(C0, P0)
        dcoef, dres, dkept, dfb = run_robust(cuda, N, dt, None, lid, None)
        assert np.array_equal(got_k, dkept.payload().reshape(C0, P0)), (what, "kept differs from the dense call")
        assert fb == dfb == sum(r["fallback_px"] for r in refs)
        assert_coef(got_c, np.stack([r["coef"] for r in refs]), 1e-4, what)
        for c in range(C0):
            assert np.array_equal(got_k[c], refs[c]["kept"]), (what, c)
            assert np.allclose(got_r[c], refs[c]["res"], rtol=1e-4, atol=1e-3), (what, c)
        if form == "aligned":
            assert bits_equal(got_c, as_pk(dcoef.payload(), 6, layout)), (what, "coef differs from the dense call")
            assert bits_equal(got_r, dres.payload().reshape(C0, P0)), (what, "res differs from the dense call")


# ---- 8-bit stacks on the matrix cores -----------------------------------------------------------------------------------
P16 = 1024 + 256 + 32  # the q8 / h16 entries refuse P % 16 != 0


def run_u8(cuda, entry, k, N, form, lid):
    op = dev(rti.api._u8_operator(entry, pinv64(k, N)), cuda)
    i = In(cuda, stack(N, P16), form, "u8")
    out, ocs = coef_out(cuda, form, k, P16)
    fn = L.lib().rti_fit_shared_q8 if entry == "q8" else L.lib().rti_fit_shared_h16
    st = fn(ptr(op), k, N, i.ptr, P16, C0, i.ls, i.cs, out.ptr, lid, ocs, 0, stream(cuda))
    torch.cuda.synchronize()
    return st, out, i


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("k", [6, 16])
@pytest.mark.parametrize("entry", ["q8", "h16"])
def test_fit_shared_u8_matrix_cores(cuda, entry, k, form):
    """rti_fit_shared_q8 / _h16 take 16-byte aligned views only: the aligned form (lpad 16, cpad 32) runs, matches
    the oracle (1e-6 for q8, 1e-4 for h16: their dense tests) and the dense call bit for bit; the two misaligned
    forms return RTI_ERR_UNSUPPORTED with nothing written, and rti.api.q8_supported is false for a base off 16 B."""
    N = 20
    for layout, lid in LAYOUTS:
        what = f"rti_fit_shared_{entry} k={k} {layout} {form}"
        st, out, i = run_u8(cuda, entry, k, N, form, lid)
        if form != "aligned":
            assert st == L.RTI_ERR_UNSUPPORTED, (what, st)
            assert out.untouched(), what
            continue
        assert st == L.RTI_OK, (what, L.lib().rti_last_error())
        out.guards_ok(what)
        got = as_pk(out.payload(), k, layout)
        assert not np.isnan(got).any(), what
        assert_coef(got, fit_ref(k, N, P16), 1e-6 if entry == "q8" else 1e-4, what)
        st, dense, _ = run_u8(cuda, entry, k, N, None, lid)
        assert st == L.RTI_OK
        assert bits_equal(got, as_pk(dense.payload(), k, layout)), (what, "differs from the dense call")
    t = torch.zeros(N * P16 + 16, dtype=torch.uint8, device=cuda)
    assert rti.api.q8_supported(t[:N * P16].view(N, P16), k, N, P16, entry)
    assert not rti.api.q8_supported(t[1:N * P16 + 1].view(N, P16), k, N, P16, entry)


# ---- light operators ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operator_case(N, E):
    lu, lv = lights(N)
    rng = np.random.default_rng(E)
    qu, qv = rng.uniform(-1, 1, E), rng.uniform(-1, 1, E)
    op = rti.basis_operator(lu, lv, qu, qv, "ptm")  # [N, E] fp64
    pv = o.pinv_shared("ptm", lu, lv)
    ref = np.stack([o.relight(o.fit_shared(stack(N)[c].astype(np.float64), pv), "ptm", qu, qv) for c in range(C0)])
    return op, ref  # ref [C, E, P]


def run_operator(cuda, precision, N, E, dt, form, rpad):
    op, _ = operator_case(N, E)
    i = In(cuda, stack(N), form, dt)
    pads = sr.form_pads(form) if form else dict(opad=0, ooff=0)
    b, orow, ocs = sr.out_rows(C0, E, P0, rpad, 2 * pads["opad"], pads["ooff"])
    out = Out(cuda, b)
    if precision == "split16":
        hi, lo, Kp, inv = rti.api.split_operator_f16(op, cuda)
        assert hi.data_ptr() % 16 == 0 and lo.data_ptr() % 16 == 0
        st = L.lib().rti_apply_operator_f16(ptr(hi), ptr(lo), Kp, inv, E, N, i.ptr, i.dt, P0, C0, i.ls, i.cs, out.ptr,
                                            L.RTI_F32, orow, ocs, stream(cuda))
    else:
        opd = dev(op.astype(np.float32), cuda)
        st = L.lib().rti_apply_operator(ptr(opd), E, N, E, i.ptr, i.dt, P0, C0, i.ls, i.cs, out.ptr, L.RTI_F32, orow,
                                        ocs, stream(cuda))
    torch.cuda.synchronize()
    assert st == L.RTI_OK, L.lib().rti_last_error()
    return out


@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("rpad", [4, 1])
@pytest.mark.parametrize("E", [3, 257])
@pytest.mark.parametrize("precision", ["fp32", "split16"])
def test_apply_operator(cuda, precision, E, rpad, form):
    """rti_apply_operator / _f16 on a padded input with out_row_stride = P + 4 / P + 1 and a padded
    out_channel_stride: guards between rows and between channels, the oracle at test_operator_ragged_vs_oracle's
    1e-5, bits against the dense call where every predicate holds (aligned form, row stride P + 4)."""
    N = 20
    _, ref = operator_case(N, E)
    for dt in ("f32", "u8"):
        what = f"apply_operator {precision} E={E} {dt} orow=P+{rpad} {form}"
        out = run_operator(cuda, precision, N, E, dt, form, rpad)
        out.guards_ok(what)
        got = out.payload()  # [C, E, P]
        assert not np.isnan(got).any(), what
        err, ok = relight_close(got, ref, rtol=1e-5)
        print(f"{what}: {err:.3g}")
        assert ok, (what, err)
        if form == "aligned" and rpad == 4:
            dense = run_operator(cuda, precision, N, E, dt, None, 0)
            assert bits_equal(got, dense.payload()), (what, "differs from the dense call")


# ---- per-pixel fit from camera positions (light_stride) -------------------------------------------------------------------
@pytest.mark.parametrize("lpad", [0, 16, 1], ids=["dense", "padded", "odd"])
def test_fit_perpixel_cam_light_stride(cuda, lpad):
    """rti_fit_perpixel_cam on [N][light_stride] uint8 planes (the golden of test_gpu_perpixel_relight.py, its 1e-6):
    a padded and an odd light stride, poison 255 between the planes, fp64 coefficients between guards (each NaN
    guard double is two NaN-pattern words); the padded form equals the dense call bit for bit."""
    d = golden("ptm_perpixel_32x32_N50.npz")
    frames = np.ascontiguousarray(d["frames"])
    N, H, W = frames.shape
    cams = dev(np.asarray(d["cams"], np.float64), cuda)

    def run(pad):
        buf, _, ls, _ = sr.embed_stack(frames.reshape(1, N, H * W), pad, 0, 0)
        b, _ = sr.out_blocks(1, 2 * H * W * 6)  # in 32-bit words
        out = Out(cuda, b)
        I = dev(buf, cuda)
        st = L.lib().rti_fit_perpixel_cam(ptr(cams), N, ptr(I), L.RTI_U8, H, W, ls, 0.0, 0.0, -1.0, out.ptr,
                                          L.RTI_F64, L.RTI_COEF_PIXEL_MAJOR, stream(cuda))
        torch.cuda.synchronize()
        assert st == L.RTI_OK, L.lib().rti_last_error()
        out.guards_ok(f"rti_fit_perpixel_cam lpad={pad}")
        return np.ascontiguousarray(out.payload()).view(np.float64).reshape(H, W, 6)

    got = run(lpad)
    err, ok = coef_close(got, d["coef"], rtol=1e-6)
    print(f"rti_fit_perpixel_cam lpad={lpad}: {err:.3g}")
    assert ok, err
    if lpad == 16:
        assert np.array_equal(got.view(np.int64), run(0).view(np.int64))
