"""The 64-bit offsets of the strided entries (include/rti.h): tiny stacks and coefficient maps placed by
tests/far_ref.py so that every address a kernel must form lies past 2^31 elements and past 2^32 bytes.

The data, oracles, tolerances and ctypes plumbing are those of tests/test_gpu_strides.py (imported, not restated);
only the buffers differ.  They are built on the device: an input is one allocation of far_ref.Plan.length elements
filled with the poison of stride_ref (NaN / INT32_MIN / 255) into which the dense [C, N, P] data (0..100) is copied
plane by plane; an output is one allocation filled with the NaN bit pattern.  The plan keeps every 32-bit
truncation of every offset inside the allocation and outside every payload, so a kernel that drops the high bits
reads poison (NaN coefficients, or bytes of 255 that move a coefficient far past the tolerance) or writes into the
NaN fill, and is caught by check (a) or (b) without touching memory the test does not own.

Every call is held to the three checks of test_gpu_strides.py: (a) every element outside the payload still holds
the NaN pattern (a device-side comparison of the whole allocation, in slices); (b) the fp64 oracle at the
tolerance of the entry's dense test; (c) bit equality with the dense call on the same data: always for the
`aligned` variant, and for the `odd` variant wherever test_gpu_strides.py asserts it for its misaligned forms.

Forms: farchan (far channel_stride), farlight (far light_stride; one channel for 4-byte stacks, see
far_ref._plans), farout (far coef_channel_stride / state_channel_stride / out_row_stride / out_channel_stride).
A test holds one far buffer at a time, drops it and empties torch's cache before it returns.

Left out on purpose: launch generations under far strides (they need millions of pixels; test_gpu_fullsize.py
and the padded-channel generation tests of test_gpu_strides.py stand for them), and anything that needs P·k
itself past 2^31.  farlight over fp32 / int32 stacks and the far pixel_stride of rti_fit_shared_pm hold one
channel (two go over the memory cap, far_ref._plans), so a second channel together with a far light stride is
driven on uint8 stacks only.

The entries added since (the last three sections) run on the helpers of tests/test_gpu_map_strides.py, which holds
their near forms: rti_relight_hsh_gain / rti_relight_hsh_specular and rti_light_scores / rti_relight_field over three
fp32 maps a far coef_channel_stride apart (channel 1 past 2^32 bytes, channel 2 past 2^31 elements), and
rti_photometric_stereo with a far channel_stride (three channels) or a far light_stride (one channel of fp32 / int32,
three of uint8), each under (a), (b) at the check of the entry's dense test and (c) in both variants: those entries
state the same bits on every path.  Their outputs are dense.  Left out there on purpose: outputs of these entries have
no stride arguments, so an output offset past 2^31 needs E·P·C or P·k itself past 2^31, the workload's own sizes,
which test_gpu_fullsize.py stands for; and the 8-bit payload entries (rti_relight_hsh8_gain, rti_relight_hsh8_specular)
take no strides at all."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import far_ref as fr
import rti
import rti_oracle as o
import stride_ref as sr
import test_gpu_map_strides as tn
import test_gpu_strides as ts
from conftest import coef_close, relight_close
from rti import _lib as L

pytestmark = pytest.mark.gpu

P0, P16 = ts.P0, ts.P16
assert (P0, P16) == (fr.P0, fr.P16)
BITS = int(sr.NAN_BITS)
TORCH_DT = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}
POISON = {"f32": float("nan"), "i32": -2**31, "u8": 255}
SLICE = 1 << 28  # elements per guard-scan slice (a 256 MiB boolean temporary)
FORMS = ("farchan", "farlight", "farout")
lib, ptr, stream = L.lib, ts.ptr, ts.stream


@pytest.fixture(autouse=True)
def release():
    yield
    torch.cuda.empty_cache()


# ---- far buffers ----------------------------------------------------------------------------------------------------
class FarIn:
    """dense [C, rows, inner] (NumPy) in a poisoned device allocation laid out by plan `name`"""

    def __init__(self, cuda, name, dense, dt, poison=None):
        p = fr.PLANS[name]
        d = torch.as_tensor(np.ascontiguousarray(np.asarray(dense).astype(ts.NP_DT[dt])), device=cuda)
        assert tuple(d.shape) == p.counts + (p.inner,) and d.element_size() == p.es, (name, d.shape)
        self.t = torch.full((p.length,), POISON[dt] if poison is None else poison, dtype=TORCH_DT[dt], device=cuda)
        assert self.t.data_ptr() % 16 == 0
        off = p.block_offsets()
        for c in range(p.counts[0]):
            for n in range(p.counts[1]):
                self.t.narrow(0, p.base + int(off[c, n]), p.inner).copy_(d[c, n])
        self.C, self.N, self.P = d.shape
        self.cs, self.ls = p.strides
        self.ptr, self.dt = ptr(self.t, p.base), ts.RTI_DT[dt]


class FarOut:
    """an output laid out by plan `name`: 32-bit words all holding the NaN pattern (8-byte elements: two each)"""

    def __init__(self, cuda, name):
        self.p = p = fr.PLANS[name]
        self.w = p.es // 4  # words per element
        self.t = torch.full((p.length * self.w,), BITS, dtype=torch.int32, device=cuda)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = ptr(self.t, p.base * self.w)
        self.strides = p.strides

    def _blocks(self):
        for e in self.p.block_offsets().ravel():
            yield (self.p.base + int(e)) * self.w, self.p.inner * self.w

    def fill(self, dense):
        """coefficients as a far INPUT: dense fp32 [counts.., inner] into the payload, NaN everywhere else"""
        d = torch.as_tensor(np.ascontiguousarray(dense, np.float32), device=self.t.device).reshape(-1, self.p.inner)
        for (lo, n), row in zip(self._blocks(), d):
            self.t.narrow(0, lo, n).copy_(row.view(torch.int32))

    def take(self, what, dtype=np.float32):
        """(a) + the payload [counts.., inner]: gathers it, puts the NaN pattern back and scans the allocation"""
        torch.cuda.synchronize()
        got = torch.stack([self.t.narrow(0, lo, n).clone() for lo, n in self._blocks()]).cpu().numpy()
        for lo, n in self._blocks():
            self.t.narrow(0, lo, n).fill_(BITS)
        self.untouched(what)
        return got.view(dtype).reshape(self.p.counts + (-1,))

    def untouched(self, what):
        bad = torch.zeros((), dtype=torch.bool, device=self.t.device)
        for lo in range(0, self.t.numel(), SLICE):
            bad |= (self.t[lo:lo + SLICE] != BITS).any()
        if bool(bad):
            where = [lo + int((self.t[lo:lo + SLICE] != BITS).nonzero()[0]) for lo in range(0, self.t.numel(), SLICE)
                     if bool((self.t[lo:lo + SLICE] != BITS).any())]
            raise AssertionError((what, "written outside the payload, first at words", where[:4], "payload base",
                                  self.p.base * self.w))


class DenseCoef:
    """the dense coefficient output of test_gpu_strides with FarOut's interface"""

    def __init__(self, cuda, k, P, C):
        self.o, ocs = ts.coef_out(cuda, None, k, P, C)
        self.ptr, self.strides = self.o.ptr, (ocs, P * k)

    def take(self, what, dtype=np.float32):
        """guards, the payload [C, 1, P·k], and the NaN fill put back for the next call"""
        torch.cuda.synchronize()
        self.o.refresh()
        self.o.guards_ok(what)
        got = self.o.payload()[:, None, :].copy()
        self.o.t.view(torch.int32).fill_(BITS)
        return got

    def untouched(self, what):
        torch.cuda.synchronize()
        self.o.refresh()
        assert self.o.untouched(), what


def stack_plan(form, dt, N, P, variant):
    """(plan name or None, channels) of the input of a case"""
    if form == "farout":
        return None, 2
    es = fr.ES[dt]
    return f"stack-{form}-es{es}-N{N}-P{P}-{variant}", 1 if form == "farlight" and es == 4 else 2


def make_in(cuda, form, dt, N, P, variant, poison=None):
    name, C = stack_plan(form, dt, N, P, variant)
    dense = ts.stack(N, P)[:C]
    return (FarIn(cuda, name, dense, dt, poison) if name else ts.In(cuda, dense, None, dt)), C


def make_coef(cuda, form, k, P, C, variant):
    return FarOut(cuda, f"coef-farchan-k{k}-P{P}-{variant}") if form == "farout" else DenseCoef(cuda, k, P, C)


def as_pk(payload, k, layout):
    return ts.as_pk(payload.reshape(payload.shape[0], -1), k, layout)


@functools.lru_cache(maxsize=None)
def dense_fit_shared(k, N, dt, lid, kernel, P):
    st, out = ts.fit_shared(torch.device("cuda", 0), k, N, dt, None, lid, kernel, P)
    assert st == L.RTI_OK, lib().rti_last_error()
    return out.payload()


# ---- rti_fit_shared -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", ["f32", "i32", "u8"])
def test_fit_shared(cuda, dt, form, variant):
    """Every selector × basis × layout on one far buffer.  Bits as test_gpu_strides.test_fit_shared: the dense call
    of the same selector in the aligned variant and for AUTO / VALU in the odd one; MFMA / TILE on an odd view fall
    back to the VALU stream and equal the dense RTI_KERNEL_VALU call.  uint8 PTM-6 also runs at P = 1312, where the
    aligned variant loads 16 pixels per lane."""
    N = 37
    for P in (P0, P16) if dt == "u8" else (P0,):
        i, C = make_in(cuda, form, dt, N, P, variant)
        for k in (6, 9, 16) if P == P0 else (6,):
            ref = ts.fit_ref(k, N, P)[:C]
            out = make_coef(cuda, form, k, P, C, variant)
            pv = ts.dev(ts.pinv64(k, N).astype(np.float32), cuda)
            for sel in ts.SELECTORS if P == P0 else ("auto", "valu"):
                if sel == "tile8" and dt != "f32":
                    continue
                for layout, lid in ts.LAYOUTS:
                    what = f"rti_fit_shared k={k} {dt} {sel} {layout} {form} {variant} P={P}"
                    st = lib().rti_fit_shared(ptr(pv), k, N, i.ptr, i.dt, P, C, i.ls, i.cs, out.ptr, lid,
                                              out.strides[0], ts.SELECTORS[sel], stream(cuda))
                    assert st == L.RTI_OK, (what, lib().rti_last_error())
                    got = as_pk(out.take(what), k, layout)
                    assert not np.isnan(got).any(), (what, "NaN in the output: poison read or a pixel not written")
                    ts.assert_coef(got, ref, 1e-4, what)
                    same = variant == "aligned" or sel in ("auto", "valu")
                    dense = dense_fit_shared(k, N, dt, lid, ts.SELECTORS[sel if same else "valu"], P)
                    assert ts.bits_equal(got, ts.as_pk(dense, k, layout)[:C]), (what, "differs from the dense call")
            del out
        del i
        torch.cuda.empty_cache()


# ---- 8-bit stacks on the matrix cores -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("entry", ["q8", "h16"])
def test_fit_shared_u8_matrix_cores(cuda, entry, form, variant):
    """rti_fit_shared_q8 / _h16: the aligned variant runs (oracle 1e-6 / 1e-4, bits of the dense call); an odd
    stride is refused with RTI_ERR_UNSUPPORTED and nothing is written."""
    N = 20
    fn = lib().rti_fit_shared_q8 if entry == "q8" else lib().rti_fit_shared_h16
    i, C = make_in(cuda, form, "u8", N, P16, variant)
    for k in (6, 16):
        op = ts.dev(rti.api._u8_operator(entry, ts.pinv64(k, N)), cuda)
        out = make_coef(cuda, form, k, P16, C, variant)
        for layout, lid in ts.LAYOUTS:
            what = f"rti_fit_shared_{entry} k={k} {layout} {form} {variant}"
            st = fn(ptr(op), k, N, i.ptr, P16, C, i.ls, i.cs, out.ptr, lid, out.strides[0], 0, stream(cuda))
            torch.cuda.synchronize()
            if variant == "odd":
                assert st == L.RTI_ERR_UNSUPPORTED, (what, st)
                out.untouched(what)
                continue
            assert st == L.RTI_OK, (what, lib().rti_last_error())
            got = as_pk(out.take(what), k, layout)
            assert not np.isnan(got).any(), what
            ts.assert_coef(got, ts.fit_ref(k, N, P16), 1e-6 if entry == "q8" else 1e-4, what)
            st, dense, _ = ts.run_u8(cuda, entry, k, N, None, lid)
            assert st == L.RTI_OK
            assert ts.bits_equal(got, ts.as_pk(dense.payload(), k, layout)), (what, "differs from the dense call")
        del out


# ---- pixel-major fit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", ["farchan", "farout"])
def test_fit_shared_pm(cuda, form, variant):
    """rti_fit_shared_pm AUTO on fp32 [C][P][N] with a far channel_stride, or into far coefficient channels: PTM-6
    (the VALU generations form) and HSH-16 (the direct form) when aligned, one lane per pixel when odd; oracle at
    1e-4 (test_gpu_pm.py), bits of the dense call in the aligned variant."""
    N, C = 20, 2
    pm = np.ascontiguousarray(ts.stack(N).transpose(0, 2, 1)).reshape(C, 1, P0 * N)  # [C][P·N]
    dense = ts.dev(pm.astype(np.float32), cuda)
    far = FarIn(cuda, f"pm-farchan-es4-N20-{variant}", pm, "f32") if form == "farchan" else None
    for k in (6, 16):
        pv = ts.dev(ts.pinv64(k, N).astype(np.float32), cuda)
        for layout, lid in ts.LAYOUTS:
            what = f"rti_fit_shared_pm k={k} {layout} {form} {variant}"
            got = []
            for is_far in (True, False):
                out = make_coef(cuda, form if is_far else None, k, P0, C, variant)
                src, cs = (far.ptr, far.cs) if is_far and far is not None else (ptr(dense), P0 * N)
                st = lib().rti_fit_shared_pm(ptr(pv), k, N, src, L.RTI_F32, P0, C, N, cs, out.ptr, lid, out.strides[0],
                                             0, stream(cuda))
                assert st == L.RTI_OK, (what, lib().rti_last_error())
                got.append(as_pk(out.take(what), k, layout))
                del out
            assert not np.isnan(got[0]).any(), what
            ts.assert_coef(got[0], ts.fit_ref(k, N), 1e-4, what)
            if variant == "aligned":
                assert ts.bits_equal(got[0], got[1]), (what, "differs from the dense call")


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_fit_shared_pm_far_pixel_stride(cuda, variant):
    """rti_fit_shared_pm with a far pixel_stride (one channel): pixel p's N samples at p·pixel_stride, the last
    pixels past both limits.  pixel_stride != N routes AUTO and RTI_KERNEL_VALU to one lane per pixel
    (fit_pm_lane), in either variant; oracle at 1e-4, and the bits of the same kernel on pixel_stride = N + 4."""
    N = 20
    rows = np.ascontiguousarray(ts.stack(N)[:1].transpose(0, 2, 1))  # [1][P][N]
    far = FarIn(cuda, f"pm-farpixel-es4-N20-{variant}", rows, "f32")
    near = ts.In(cuda, rows, "aligned", "f32")  # rows of N + 4 between NaN poison
    for k in (6, 9, 16):
        pv = ts.dev(ts.pinv64(k, N).astype(np.float32), cuda)
        for sel in ("auto", "valu"):
            for layout, lid in ts.LAYOUTS:
                what = f"rti_fit_shared_pm k={k} {sel} {layout} far pixel_stride {variant}"
                got = []
                for src in (far, near):
                    out = DenseCoef(cuda, k, P0, 1)
                    st = lib().rti_fit_shared_pm(ptr(pv), k, N, src.ptr, L.RTI_F32, P0, 1, src.ls, 0, out.ptr, lid, 0,
                                                 ts.SELECTORS[sel], stream(cuda))
                    assert st == L.RTI_OK, (what, lib().rti_last_error())
                    got.append(as_pk(out.take(what), k, layout))
                assert not np.isnan(got[0]).any(), (what, "NaN in the output: poison read or a pixel not written")
                ts.assert_coef(got[0], ts.fit_ref(k, N)[:1], 1e-4, what)
                assert ts.bits_equal(got[0], got[1]), (what, "differs from the call on pixel_stride = N + 4")


# ---- one-pass fit + residual, residual of given coefficients, robust fit --------------------------------------------
def fitres_call(cuda, entry, k, N, i, C, coef, lid):
    lu, lv = ts.lights(N)
    if entry == "svd":
        a, g = rti.lsq_factors(lu, lv, ts.basis_of(k))
        fn = lib().rti_fit_shared_residual_svd
    else:
        a, g = rti.design_matrix(lu, lv, ts.basis_of(k)), rti.gram_inverse(lu, lv, ts.basis_of(k))
        fn = lib().rti_fit_shared_residual
    a, g = ts.dev(np.asarray(a, np.float64), cuda), ts.dev(np.asarray(g, np.float64), cuda)
    res = ts.map_out(cuda, None, P0, C)
    part = torch.zeros((C, int(lib().rti_fit_shared_residual_blocks(P0))), dtype=torch.float64, device=cuda)
    st = fn(ptr(a), ptr(g), k, N, i.ptr, i.dt, P0, C, i.ls, i.cs, coef.ptr, lid, coef.strides[0], res.ptr, ptr(part),
            0, stream(cuda))
    torch.cuda.synchronize()
    assert st == L.RTI_OK, lib().rti_last_error()
    return res, torch.sqrt(part.sum(dim=1) / (P0 * N)).cpu().numpy()


@functools.lru_cache(maxsize=None)
def dense_fitres(entry, k, N, dt, lid):
    coef, res, rms = ts.run_fitres(torch.device("cuda", 0), entry, k, N, dt, None, lid)
    return coef.payload(), res.payload().reshape(ts.C0, P0), rms


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", ["f32", "i32", "u8"])
@pytest.mark.parametrize("entry", ["svd", "gram"])
def test_fit_shared_residual(cuda, entry, dt, form, variant):
    """Both forms of the one-pass fit + residual: coefficients 1e-6 (svd) / 1e-4 (gram), residuals 1e-4 + 1e-6·ref,
    channel RMS equal to the dense call's to 1e-12, bits of the dense call in both variants (fitres_body)."""
    N = 37
    i, C = make_in(cuda, form, dt, N, P0, variant)
    for k in (6, 16):
        ref_c = ts.fit_ref(k, N)[:C]
        coef = make_coef(cuda, form, k, P0, C, variant)
        for layout, lid in ts.LAYOUTS:
            what = f"{entry} k={k} {dt} {layout} {form} {variant}"
            res, rms = fitres_call(cuda, entry, k, N, i, C, coef, lid)
            res.guards_ok(what + " res")
            got_c, got_r = as_pk(coef.take(what), k, layout), res.payload().reshape(C, P0)
            assert not np.isnan(got_c).any() and not np.isnan(got_r).any(), what
            ts.assert_coef(got_c, ref_c, 1e-6 if entry == "svd" else 1e-4, what)
            for c in range(C):
                ref_r, _ = o.fit_residual(ts.stack(N)[c].astype(np.float64), ts.design64(k, N), ref_c[c])
                err, ok = ts.res_close(got_r[c], ref_r, 1e-4, 1e-6)
                assert ok, (what, "res", c, err)
            dcoef, dres, drms = dense_fitres(entry, k, N, dt, lid)
            assert np.isfinite(rms).all() and (np.abs(rms - drms[:C]) <= 1e-12 * drms[:C]).all(), (what, rms, drms)
            assert ts.bits_equal(got_c, ts.as_pk(dcoef, k, layout)[:C]), (what, "coef differs from the dense call")
            assert ts.bits_equal(got_r, dres[:C]), (what, "res differs from the dense call")
        del coef


@functools.lru_cache(maxsize=None)
def dense_residual(k, N, dt, layout, lid):
    _, res, rms = ts.run_residual(torch.device("cuda", 0), k, N, dt, None, layout, lid)
    return res.payload().reshape(ts.C0, P0), rms


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", ["f32", "i32", "u8"])
def test_fit_residual(cuda, dt, form, variant):
    """rti_fit_residual: the coefficients are a far INPUT in farout.  1e-3 + 1e-4·ref per pixel, RMS equal to the
    dense call's to 1e-12, bits in the aligned variant."""
    N = 20
    i, C = make_in(cuda, form, dt, N, P0, variant)
    for k in (6, 16):
        A = ts.dev(ts.design64(k, N).astype(np.float32), cuda)
        c32 = ts.fit_ref(k, N).astype(np.float32)[:C]
        for layout, lid in ts.LAYOUTS:
            what = f"rti_fit_residual k={k} {dt} {layout} {form} {variant}"
            flat = (c32 if layout == "pixel" else c32.transpose(0, 2, 1)).reshape(C, P0 * k)
            if form == "farout":
                cbuf = FarOut(cuda, f"coef-farchan-k{k}-P{P0}-{variant}")
                cbuf.fill(flat)
                cptr, ocs = cbuf.ptr, cbuf.strides[0]
            else:
                cbuf = ts.dev(flat, cuda)
                cptr, ocs = ptr(cbuf), P0 * k
            res = ts.map_out(cuda, None, P0, C)
            part = torch.zeros((C, int(lib().rti_fit_residual_blocks(P0))), dtype=torch.float64, device=cuda)
            st = lib().rti_fit_residual(ptr(A), k, N, i.ptr, i.dt, P0, C, i.ls, i.cs, cptr, lid, ocs, res.ptr,
                                        ptr(part), stream(cuda))
            torch.cuda.synchronize()
            assert st == L.RTI_OK, (what, lib().rti_last_error())
            del cbuf
            res.guards_ok(what)
            got = res.payload().reshape(C, P0)
            assert not np.isnan(got).any(), what
            for c in range(C):
                ref_r, _ = o.fit_residual(ts.stack(N)[c].astype(np.float64), ts.design64(k, N), c32[c].astype(np.float64))
                err, ok = ts.res_close(got[c], ref_r, 1e-3, 1e-4)
                assert ok, (what, c, err)
            dres, drms = dense_residual(k, N, dt, layout, lid)
            rms = torch.sqrt(part.sum(dim=1) / (P0 * N)).cpu().numpy()
            assert np.isfinite(rms).all() and (np.abs(rms - drms[:C]) <= 1e-12 * drms[:C]).all(), (what, rms, drms)
            if variant == "aligned":
                assert ts.bits_equal(got, dres[:C]), (what, "differs from the dense call")


@functools.lru_cache(maxsize=None)
def dense_robust(N, dt, lid):
    coef, res, kept, fb = ts.run_robust(torch.device("cuda", 0), N, dt, None, lid, None)
    return coef.payload(), res.payload().reshape(ts.C0, P0), kept.payload().reshape(ts.C0, P0), fb


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt,poison", [("u8", None), ("i32", 128), ("f32", None)])
def test_fit_shared_robust(cuda, dt, poison, form, variant):
    """As test_gpu_strides.test_fit_shared_robust (the int32 stack is padded with 128, inside the window, so a
    padding sample read as data changes `kept`): kept equals the dense call's and the reference's, coef 1e-4, res
    rtol 1e-4 + atol 1e-3, bits in the aligned variant."""
    N = 20
    _, refs = ts.robust_ref(N)
    A = ts.dev(ts.robust_ref(N)[0], cuda)
    i, C = make_in(cuda, form, dt, N, P0, variant, poison)
    coef = make_coef(cuda, form, 6, P0, C, variant)
    R = ts.ROBUST
    for layout, lid in ts.LAYOUTS:
        what = f"rti_fit_shared_robust {dt} {layout} {form} {variant}"
        res, kept = ts.map_out(cuda, None, P0, C), ts.map_out(cuda, None, P0, C, dtype=np.int32)
        fb = torch.zeros(1, dtype=torch.int32, device=cuda)
        st = lib().rti_fit_shared_robust(ptr(A), 6, N, i.ptr, i.dt, P0, C, i.ls, i.cs, R["lo"], R["hi"], 6, R["iters"],
                                         R["delta"], coef.ptr, lid, coef.strides[0], res.ptr, kept.ptr, ptr(fb), 0,
                                         stream(cuda))
        torch.cuda.synchronize()
        assert st == L.RTI_OK, (what, lib().rti_last_error())
        res.guards_ok(what + " res")
        kept.guards_ok(what + " kept")
        got_c = as_pk(coef.take(what), 6, layout)
        got_r, got_k = res.payload().reshape(C, P0), kept.payload().reshape(C, P0)
        dcoef, dres, dkept, dfb = dense_robust(N, dt, lid)
        assert np.array_equal(got_k, dkept[:C]), (what, "kept differs from the dense call")
        assert int(fb.item()) == sum(r["fallback_px"] for r in refs[:C])
        ts.assert_coef(got_c, np.stack([r["coef"] for r in refs[:C]]), 1e-4, what)
        for c in range(C):
            assert np.array_equal(got_k[c], refs[c]["kept"]), (what, c)
            assert np.allclose(got_r[c], refs[c]["res"], rtol=1e-4, atol=1e-3), (what, c)
        if variant == "aligned":
            assert ts.bits_equal(got_c, ts.as_pk(dcoef, 6, layout)[:C]), (what, "coef differs from the dense call")
            assert ts.bits_equal(got_r, dres[:C]), (what, "res differs from the dense call")


# ---- light operators ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_operator(precision, N, E, dt):
    return ts.run_operator(torch.device("cuda", 0), precision, N, E, dt, None, 0).payload()


OP_FORMS = ("farchan", "farlight", "farop", "faroutrow", "faroutchan")
OP_CASES = [(p, f, E) for p in ("fp32", "split16") for f in OP_FORMS if (p, f) != ("split16", "farop")
            for E in ((3, 257) if f in ("farchan", "farlight", "faroutchan") else (3,))]


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("precision,form,E", OP_CASES, ids=[f"{p}-{f}-E{E}" for p, f, E in OP_CASES])
def test_apply_operator(cuda, precision, form, E, variant):
    """rti_apply_operator / _f16 with one far argument: channel_stride, light_stride, op_stride (fp32 entry only:
    the split operator has no stride), out_row_stride (E = 3, one channel) or out_channel_stride (E = 3 and 257).
    The oracle at 1e-5 (test_operator_ragged_vs_oracle), bits of the dense call in the aligned variant."""
    N = 20
    op, ref = ts.operator_case(N, E)
    far_out = {"faroutrow": f"opout-farrow-E3-{variant}", "faroutchan": f"opout-farchan-E{E}-{variant}"}.get(form)
    out = FarOut(cuda, far_out) if far_out else None  # one far buffer serves both dtypes: take() restores its fill
    if precision == "split16":
        hi, lo, Kp, inv = rti.api.split_operator_f16(op, cuda)
    elif form == "farop":
        opd = FarIn(cuda, f"op-farrow-N20-E3-{variant}", op.astype(np.float32)[None], "f32")
        optr, ostride = opd.ptr, opd.ls
    else:
        opd = ts.dev(op.astype(np.float32), cuda)
        optr, ostride = ptr(opd), E
    for dt in ("f32", "u8"):
        what = f"apply_operator {precision} E={E} {dt} {form} {variant}"
        if form == "faroutrow":
            C, i = 1, ts.In(cuda, ts.stack(N)[:1], None, dt)
        else:
            i, C = make_in(cuda, form if form in ("farchan", "farlight") else "farout", dt, N, P0, variant)
        if far_out:
            ocs, orow = out.strides
        else:
            b, orow, ocs = sr.out_rows(C, E, P0)
            out = ts.Out(cuda, b)
        if precision == "split16":
            st = lib().rti_apply_operator_f16(ptr(hi), ptr(lo), Kp, inv, E, N, i.ptr, i.dt, P0, C, i.ls, i.cs, out.ptr,
                                              L.RTI_F32, orow, ocs, stream(cuda))
        else:
            st = lib().rti_apply_operator(optr, E, N, ostride, i.ptr, i.dt, P0, C, i.ls, i.cs, out.ptr, L.RTI_F32, orow,
                                          ocs, stream(cuda))
        torch.cuda.synchronize()
        assert st == L.RTI_OK, (what, lib().rti_last_error())
        if far_out:
            got = out.take(what)
        else:
            out.guards_ok(what)
            got = out.payload()
        del i
        torch.cuda.empty_cache()
        assert not np.isnan(got).any(), what
        err, ok = relight_close(got, ref[:C], rtol=1e-5)
        print(f"{what}: {err:.3g}")
        assert ok, (what, err)
        if variant == "aligned":
            assert ts.bits_equal(got, dense_operator(precision, N, E, dt)[:C]), (what, "differs from the dense call")


# ---- per-pixel fit from camera positions ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_fit_perpixel_cam_light_stride(cuda, variant):
    """rti_fit_perpixel_cam on uint8 planes a far light_stride apart (the golden of test_gpu_perpixel_relight.py at
    its 1e-6); the aligned variant equals the dense call bit for bit."""
    d = ts.golden("ptm_perpixel_32x32_N50.npz")
    frames = np.ascontiguousarray(d["frames"])
    N, H, W = frames.shape
    cams = ts.dev(np.asarray(d["cams"], np.float64), cuda)

    def run(i):
        b, _ = sr.out_blocks(1, 2 * H * W * 6)
        out = ts.Out(cuda, b)
        st = lib().rti_fit_perpixel_cam(ptr(cams), N, i.ptr, L.RTI_U8, H, W, i.ls, 0.0, 0.0, -1.0, out.ptr, L.RTI_F64,
                                        L.RTI_COEF_PIXEL_MAJOR, stream(cuda))
        torch.cuda.synchronize()
        assert st == L.RTI_OK, lib().rti_last_error()
        out.guards_ok("rti_fit_perpixel_cam")
        return np.ascontiguousarray(out.payload()).view(np.float64).reshape(H, W, 6)

    got = run(FarIn(cuda, f"cam-farlight-N50-P1024-{variant}", frames.reshape(1, N, H * W), "u8"))
    torch.cuda.empty_cache()
    err, ok = coef_close(got, d["coef"], rtol=1e-6)
    print(f"rti_fit_perpixel_cam far {variant}: {err:.3g}")
    assert ok, err
    if variant == "aligned":
        assert np.array_equal(got.view(np.int64), run(ts.In(cuda, frames.reshape(1, N, H * W), None, "u8")).view(np.int64))


# ---- the shared fit fed in chunks -------------------------------------------------------------------------------------
ACC_FORMS = ("farchan", "farlight", "farstate", "farcoef")


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("form", ACC_FORMS)
@pytest.mark.parametrize("dt", ["f32", "u8"])
def test_fit_accumulate_and_solve(cuda, dt, form, variant):
    """rti_fit_accumulate (one chunk of N planes, init) into an fp64 state and rti_fit_accum_solve from it, with a
    far light_stride, channel_stride, state_channel_stride (2^29 doubles: past 2^32 bytes) or coef_channel_stride.
    The state against y_j = Σ_n A[n][j]·I (fp64 NumPy; the data are integers, so only the order of the fp64 sums
    differs: 1e-12 relative to the largest |y|) and bit-equal to the dense call's in both variants (the entry
    documents the same bits on either path); coefficients at coef_close's default bound and residuals at
    rtol 1e-4 + atol 1e-3 (test_gpu_accum.check), both bit-equal to the dense call's."""
    N = 20
    i, C = make_in(cuda, form if form in ("farchan", "farlight") else "farout", dt, N, P0, variant)
    for k in (6, 16):
        A64 = ts.design64(k, N)
        R = ts.dev(A64, cuda)
        M = ts.dev(np.asarray(rti.gram_inverse(*ts.lights(N), ts.basis_of(k)), np.float64), cuda)
        what = f"accum k={k} {dt} {form} {variant}"
        results = []
        for far in (True, False):
            src = i if far else ts.In(cuda, ts.stack(N)[:C], None, dt)
            if far and form == "farstate":
                state = FarOut(cuda, f"state-farchan-k{k}-{variant}")
                sptr, scs = state.ptr, state.strides[0]
            else:
                state = torch.full((C * (k + 1) * P0,), float("nan"), dtype=torch.float64, device=cuda)
                sptr, scs = ptr(state), (k + 1) * P0
            st = lib().rti_fit_accumulate(ptr(R), k, N, src.ptr, src.dt, P0, C, src.ls, src.cs, sptr, scs, 1, stream(cuda))
            assert st == L.RTI_OK, (what, lib().rti_last_error())
            per_layout = []
            for layout, lid in ts.LAYOUTS:
                coef = make_coef(cuda, "farout" if far and form == "farcoef" else None, k, P0, C, variant)
                res = ts.map_out(cuda, None, P0, C)
                st = lib().rti_fit_accum_solve(ptr(M), k, 0, N, sptr, P0, C, scs, coef.ptr, lid, coef.strides[0], res.ptr,
                                               stream(cuda))
                assert st == L.RTI_OK, (what, lib().rti_last_error())
                torch.cuda.synchronize()
                res.guards_ok(what + " res")
                per_layout.append((as_pk(coef.take(what + " coef"), k, layout), res.payload().reshape(C, P0)))
                del coef
            if isinstance(state, FarOut):
                sv = np.ascontiguousarray(state.take(what + " state", np.int32)).view(np.float64).reshape(C, k + 1, P0)
            else:
                sv = state.cpu().numpy().reshape(C, k + 1, P0)
            del state
            torch.cuda.empty_cache()
            results.append((sv, per_layout))
        (sv, far_out), (dsv, dense_out) = results
        I64 = ts.stack(N)[:C].astype(np.float64)
        want = np.concatenate([np.einsum("nj,cnp->cjp", A64, I64), (I64 ** 2).sum(1, keepdims=True)], axis=1)
        assert not np.isnan(sv).any(), (what, "NaN in the state: poison read or an element not written")
        assert np.abs(sv - want).max() <= 1e-12 * np.abs(want).max(), (what, np.abs(sv - want).max())
        assert np.array_equal(sv.view(np.int64), dsv.view(np.int64)), (what, "state differs from the dense call")
        for (gc, gr), (dc, dr) in zip(far_out, dense_out):
            for c in range(C):
                err, ok = coef_close(gc[c], ts.fit_ref(k, N)[c])
                assert ok, (what, c, err)
                ref_r, _ = o.fit_residual(I64[c], A64, ts.fit_ref(k, N)[c])
                assert np.allclose(gr[c], ref_r, rtol=1e-4, atol=1e-3), (what, c)
            assert ts.bits_equal(gc, dc) and ts.bits_equal(gr, dr), (what, "solve differs from the dense call")


# ---- readers of three fp32 maps [3, P, k] ---------------------------------------------------------------------------
PM = 1024 + 52  # the ragged size of the map readers' path tests (test_gpu_lrgb.py, test_gpu_hsh8.py)


@functools.lru_cache(maxsize=None)
def maps(k):
    """three fp32 coefficient maps [3, PM·k] (either layout reads the same numbers), never changed"""
    a = np.random.default_rng(50 + k).uniform(-40.0, 90.0, (3, 1, PM * k)).astype(np.float32)
    a.setflags(write=False)
    return a


def map_sources(cuda, k, variant):
    """(pointer, coef_channel_stride, keep-alive) of the far maps, then of the dense ones"""
    far = FarIn(cuda, f"maps-farchan-k{k}-P{PM}-{variant}", maps(k), "f32")
    dense = ts.dev(maps(k), cuda)
    return (far.ptr, far.cs, far), (ptr(dense), 0, dense)


def same_bytes(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_lrgb_from_rgb(cuda, variant):
    """rti_lrgb_from_rgb over three far maps: bit-equal to the dense call (pinned to tests/lrgb_ref.py)."""
    g = np.ascontiguousarray(rti.gram(*ts.lights(20)), np.float64)
    for layout, lid in ts.LAYOUTS:
        for _, olid in ts.LAYOUTS:
            outs = []
            for cp, cs, keep in map_sources(cuda, 6, variant):
                out = torch.full((9 * PM,), float("nan"), device=cuda)
                st = lib().rti_lrgb_from_rgb(cp, lid, cs, PM, rti.api._dptr(g), None, ptr(out), olid, stream(cuda))
                torch.cuda.synchronize()
                assert st == L.RTI_OK, lib().rti_last_error()
                outs.append(out)
                del keep
            assert not torch.isnan(outs[1]).any()
            assert same_bytes(*outs), ("rti_lrgb_from_rgb", layout, olid, variant, "differs from the dense call")


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("k,basis", [(9, "hsh9"), (16, "hsh16")])
def test_hsh_qparams_quantise_normals(cuda, k, basis, variant):
    """rti_hsh_qparams + rti_hsh_quantise and rti_hsh_normals over three far maps: bit-equal to the dense calls
    (pinned to tests/hsh8_ref.py and tests/hsh_normals_ref.py)."""
    b = rti.api._hsh8_basis(basis)
    table = rti.api.peak_table(basis, 10, cuda)
    for layout, lid in ts.LAYOUTS:
        outs = []
        for cp, cs, keep in map_sources(cuda, k, variant):
            ws = torch.empty(rti.api.hsh_qparams_workspace(PM, basis), dtype=torch.uint8, device=cuda)
            qp = torch.full((2 * k,), float("nan"), device=cuda)
            c8 = torch.full((3 * k * PM,), 77, dtype=torch.uint8, device=cuda)
            nrm = torch.full((3 * PM,), float("nan"), device=cuda)
            kind = torch.full((PM,), 99, dtype=torch.uint8, device=cuda)
            st = lib().rti_hsh_qparams(cp, b, lid, cs, PM, ptr(ws), ptr(qp), stream(cuda))
            assert st == L.RTI_OK, lib().rti_last_error()
            st = lib().rti_hsh_quantise(cp, b, lid, cs, PM, ptr(qp), ptr(c8), stream(cuda))
            assert st == L.RTI_OK, lib().rti_last_error()
            st = lib().rti_hsh_normals(cp, b, lid, 3, cs, PM, None, 10, ptr(table), ptr(nrm), 0, ptr(kind), None,
                                       stream(cuda))
            assert st == L.RTI_OK, lib().rti_last_error()
            torch.cuda.synchronize()
            outs.append((qp, c8, nrm, kind))
            del keep
        assert not torch.isnan(outs[1][0]).any()
        for name, a, d in zip(("qparams", "coef8", "normals", "kind"), *outs):
            assert same_bytes(a, d), (f"hsh {name}", layout, variant, "differs from the dense call")


@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_rgb8_qparams_quantise(cuda, variant):
    """rti_rgb8_qparams + rti_rgb8_quantise over three far maps: bit-equal to the dense calls (tests/rgb8_ref.py)."""
    for layout, lid in ts.LAYOUTS:
        outs = []
        for cp, cs, keep in map_sources(cuda, 6, variant):
            ws = torch.empty(rti.api.rgb8_qparams_workspace(PM), dtype=torch.uint8, device=cuda)
            qp = torch.full((12,), float("nan"), dtype=torch.float64, device=cuda)
            c8 = torch.full((18 * PM,), 77, dtype=torch.uint8, device=cuda)
            st = lib().rti_rgb8_qparams(cp, lid, cs, PM, ptr(ws), ptr(qp), stream(cuda))
            assert st == L.RTI_OK, lib().rti_last_error()
            st = lib().rti_rgb8_quantise(cp, lid, cs, PM, ptr(qp), ptr(c8), stream(cuda))
            assert st == L.RTI_OK, lib().rti_last_error()
            torch.cuda.synchronize()
            outs.append((qp, c8))
            del keep
        assert not torch.isnan(outs[1][0]).any()
        for name, a, d in zip(("qparams", "coef8"), *outs):
            assert same_bytes(a, d), (f"rgb8 {name}", layout, variant, "differs from the dense call")


# ---- renderers under a normal map, multi-light and photometric stereo (helpers: tests/test_gpu_map_strides.py) ------
assert tn.PM == PM and tn.PS_P == P0
LAYOUT_IDS = [name for name, _ in ts.LAYOUTS]


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("layout,lid", ts.LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("k", [9, 16])
def test_render_far_channel_stride(cuda, k, layout, lid, variant):
    """rti_relight_hsh_gain and rti_relight_hsh_specular over three far maps (gain 2.5; kd 0.4, ks 150, exponent 75),
    pixel-major normals (the layout that stages), E = 3, F32 and U8: the restatements at their dense tests' check, and
    the bits of the dense call in both variants (the odd stride reads one element per lane)."""
    flat = tn.flat_maps(tn.G.maps(PM, k, "fp32"), layout)
    far = FarIn(cuda, f"maps-farchan-k{k}-P{PM}-{variant}", flat[:, None, :], "f32")
    dense = tn.Maps(cuda, flat, None)
    nid = L.RTI_NORMAL_PIXEL_MAJOR
    for entry in sorted(tn.RENDER):
        n = tn.normal_map(cuda, tn.RENDER[entry][0].normals(PM), "pixel", None)
        for dt in ("f32", "u8"):
            what = f"rti_relight_hsh_{entry} k={k} {layout} {dt} farchan {variant}"
            got = tn.render(cuda, entry, far.ptr, far.cs, lid, k, 3, PM, n.ptr, nid, dt, what)
            worst = tn.check_render(entry, got, PM, k, 3, dt, what)
            print(f"{what}: worst fp32 error {worst:.3g} of its bound")
            want = tn.render(cuda, entry, dense.ptr, 0, lid, k, 3, PM, n.ptr, nid, dt, what + " dense")
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, "differs from the dense call")
    del far


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("layout,lid", ts.LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("k", [6, 9, 16])
def test_multilight_far_channel_stride(cuda, k, layout, lid, variant):
    """rti_light_scores (scores within the header's bound of multilight_ref, count exact) and rti_relight_field under
    a tile field (F32 and U8, equal to the restatement) over three far maps of 19 x 37 pixels, T = 8; every output
    bit-equal to the dense call."""
    flat = tn.flat_maps(tn.M.image_maps(*tn.HW, k, 3), layout)
    far = FarIn(cuda, f"maps-farchan-k{k}-P{tn.HW[0] * tn.HW[1]}-{variant}", flat[:, None, :], "f32")
    dense = tn.Maps(cuda, flat, None)
    what = f"multi-light k={k} {layout} farchan {variant}"
    worst = tn.check_multilight(cuda, k, layout, lid, (far.ptr, far.cs), (dense.ptr, 0), what, field_forms=(True,))
    print(f"{what}: worst score error {worst:.3f} of its bound")
    del far


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("dt,poison", tn.PS_DTYPES, ids=[d for d, _ in tn.PS_DTYPES])
@pytest.mark.parametrize("form", ["farchan", "farlight"])
def test_photometric_stereo(cuda, form, dt, poison, variant):
    """rti_photometric_stereo, N = 20, P = 1316, with a far channel_stride (C = 3) or a far light_stride (C = 1 for
    fp32 / int32: two such channels go over the memory cap, far_ref._plans; C = 3 for uint8): iters 0 and 2, both
    normal layouts, the six outputs against ps_ref at test_gpu_ps.check's tolerances and bit-equal to the dense call,
    kept exact against both.  The streaming form and the resident form of 256 pixels both run; the aligned variant
    stages the tile by 16-byte loads, the odd one by elements."""
    es = fr.ES[dt]
    C = 1 if form == "farlight" and es == 4 else 3
    i = FarIn(cuda, f"ps-{form}-es{es}-N{tn.PS_N}-P{P0}-{variant}", tn.ps_stack(dt, C), dt, poison)
    assert tn.ps_vec(i.ptr.value, i.ls, i.cs, es, C) == (variant == "aligned")
    tiles = tn.check_ps(cuda, i.ptr, dt, C, i.ls, i.cs, f"rti_photometric_stereo {form} C={C} {dt} {variant}")
    assert tiles == {0, 256}, tiles
    del i
