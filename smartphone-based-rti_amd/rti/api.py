"""Native API: ``fit()`` / ``relight()`` on CUDA (HIP) tensors through librti.so.

Every compute call goes to a HIP kernel of ``librti.so`` on the caller's
current torch stream.  Host-side work is limited to the k×N pseudo-inverse
(``rti_pinv``, also native) and argument marshalling; there is no CPU path for
the fit or the relight, and CPU tensors are rejected.

Reference mapping (bara96/Smartphone-based-RTI @ v0):
  * ``fit(mode="shared")``   — analysis.py:321-363 + :280-298, one pseudo-inverse
    for every pixel (directional lights).
  * ``fit(mode="perpixel")`` — the reference's own geometry: each pixel's light
    list from compute_intensities (analysis.py:196-246), solved per pixel.
  * ``relight()``            — analysis.py:300-315 (grid evaluation),
    analysis.py:375-411 (int32 tables), interactive_relighting.py:25-36 (clip).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib as L

BASES = {
    "ptm": L.RTI_BASIS_PTM6, "ptm6": L.RTI_BASIS_PTM6,
    "hsh": L.RTI_BASIS_HSH16, "hsh3": L.RTI_BASIS_HSH16, "hsh16": L.RTI_BASIS_HSH16,
    "hsh2": L.RTI_BASIS_HSH9, "hsh9": L.RTI_BASIS_HSH9,
}
_KERNELS = {"auto": L.RTI_KERNEL_AUTO, "valu": L.RTI_KERNEL_VALU, "mfma": L.RTI_KERNEL_MFMA, "tile": L.RTI_KERNEL_TILE}
_IN_DTYPES = {torch.float32: L.RTI_F32, torch.uint8: L.RTI_U8, torch.int32: L.RTI_I32}
_COEF_DTYPES = {torch.float32: L.RTI_F32, torch.float64: L.RTI_F64}
_OUT_DTYPES = {torch.float32: L.RTI_F32, torch.float64: L.RTI_F64, torch.int32: L.RTI_I32, torch.uint8: L.RTI_U8}


def basis_id(basis):
    if isinstance(basis, int):
        return basis
    try:
        return BASES[basis.lower()]
    except (KeyError, AttributeError):
        raise ValueError(f"unknown basis {basis!r}; expected one of {sorted(BASES)}") from None


def basis_terms(basis):
    return L.lib().rti_basis_terms(basis_id(basis))


def _f32_host(x, name):
    a = np.ascontiguousarray(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float32).ravel())
    if a.size == 0:
        raise ValueError(f"{name} is empty")
    return a


def _dirs(lu, lv):
    """One light set's directions as two fp32 host arrays of equal length."""
    lu, lv = _f32_host(lu, "lu"), _f32_host(lv, "lv")
    if lu.size != lv.size:
        raise ValueError("lu and lv differ in length")
    return lu, lv


def _rcond(rcond):
    """The C ABI's SVD threshold: negative = none (the reference's semantics)."""
    return -1.0 if rcond is None else float(rcond)


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def design_matrix(lu, lv, basis="ptm"):
    """Host fp64 design matrix [N, k] (analysis.py:280-291 for PTM)."""
    lu, lv = _dirs(lu, lv)
    b = basis_id(basis)
    A = np.empty((lu.size, basis_terms(b)), dtype=np.float64)
    L.check(L.lib().rti_design_matrix(b, _fptr(lu), _fptr(lv), lu.size, _dptr(A)), "rti_design_matrix")
    return A


def pinv(lu, lv, basis="ptm", rcond=None):
    """Host fp64 pseudo-inverse [k, N] of the shared design (analysis.py:293-298).

    ``rcond=None`` keeps the reference's semantics (no threshold)."""
    lu, lv = _dirs(lu, lv)
    b = basis_id(basis)
    out = np.empty((basis_terms(b), lu.size), dtype=np.float64)
    L.check(L.lib().rti_pinv(b, _fptr(lu), _fptr(lv), lu.size, _rcond(rcond), _dptr(out)), "rti_pinv")
    return out


def gram_inverse(lu, lv, basis="ptm", rcond=None):
    """Host fp64 Gram (pseudo-)inverse (AᵀA)⁺ [k, k] of the shared design (pinv = ginv·Aᵀ; the
    same SVD and rcond semantics as ``pinv``)."""
    lu, lv = _dirs(lu, lv)
    b = basis_id(basis)
    k = basis_terms(b)
    out = np.empty((k, k), dtype=np.float64)
    L.check(L.lib().rti_gram_inverse(b, _fptr(lu), _fptr(lv), lu.size, _rcond(rcond), _dptr(out)),
            "rti_gram_inverse")
    return out


def lsq_factors(lu, lv, basis="ptm", rcond=None):
    """Host fp64 thin-SVD factors ``(U [N, k], W [k, k])`` of the shared design, split as the
    reference's solve is (analysis.py:295-298: ``c = uᵀL; w = c/s; a = vᵀw``): U = the orthonormal
    left singular vectors, W = V Σ⁻¹, so pinv = W·Uᵀ (rcond as ``pinv``)."""
    lu, lv = _dirs(lu, lv)
    b = basis_id(basis)
    k = basis_terms(b)
    U = np.empty((lu.size, k), dtype=np.float64)
    W = np.empty((k, k), dtype=np.float64)
    L.check(L.lib().rti_lsq_factors(b, _fptr(lu), _fptr(lv), lu.size, _rcond(rcond), _dptr(U), _dptr(W)),
            "rti_lsq_factors")
    return U, W


# the 8-bit matrix-core forms of the shared fit: form -> librti's (operator_bytes, operator builder, fit entry,
# max_lights), looked up when used (importing this module does not load the library)
_U8_FORMS = {
    "h16": ("rti_h16_operator_bytes", "rti_h16_operator", "rti_fit_shared_h16", "rti_fit_shared_h16_max_lights"),
    "q8": ("rti_q8_operator_bytes", "rti_q8_operator", "rti_fit_shared_q8", "rti_fit_shared_q8_max_lights"),
}


def _u8_form(form):
    return tuple(getattr(L.lib(), name) for name in _U8_FORMS[form])


def _u8_operator(form, pinv64):
    pv = np.ascontiguousarray(np.asarray(pinv64, np.float64))
    k, N = pv.shape
    nbytes, build = _u8_form(form)[:2]
    nb = int(nbytes(k, N))
    if nb <= 0:
        raise ValueError(f"no {form} operator for k={k}, N={N}")
    op = np.zeros(nb, dtype=np.uint8)
    L.check(build(_dptr(pv), k, N, ctypes.c_void_p(op.ctypes.data)), _U8_FORMS[form][1])
    return op


def q8_operator(pinv64):
    """Host: the fixed-point int8-digit form of an fp64 operator [k, N] for ``rti_fit_shared_q8`` (8-bit
    stacks on the int8 matrix cores; layout in csrc/rti_q8.h).  Raises ValueError for non-finite entries."""
    return _u8_operator("q8", pinv64)


def h16_operator(pinv64):
    """Host: the split-fp16 form of an fp64 operator [k, N] for ``rti_fit_shared_h16`` (8-bit stacks on the
    fp16 matrix cores; layout in csrc/rti_fit_h16.hip).  Raises ValueError for non-finite entries."""
    return _u8_operator("h16", pinv64)


def _check_operator(op_dev, nbytes, form, k, N):
    """The kernels copy exactly rti_*_operator_bytes(k, N) bytes of the operator into LDS: one built for
    another (k, N) would be read out of range or misread, so its size must match (the C ABI cannot check
    a device buffer it is not given the size of)."""
    if op_dev.dtype != torch.uint8 or op_dev.numel() != nbytes:
        raise ValueError(f"{form} operator of {op_dev.numel()} {op_dev.dtype} elements, expected {nbytes} uint8 "
                         f"bytes for k={k}, N={N}: build it with rti.{form}_operator(pinv) for this light set")


def _fit_u8_into(form, op_dev, I, coef, k, layout, flags):
    C, N, P = (1, *I.shape) if I.dim() == 2 else I.shape
    nbytes, _, entry, _ = _u8_form(form)
    _check_operator(op_dev, int(nbytes(k, N)), form, k, N)
    st = entry(_vp(op_dev), k, N, _vp(I), P, C, P, N * P, _vp(coef), _layout_id(layout), P * k, int(flags),
               _stream_of(I))
    L.check(st, _U8_FORMS[form][2])
    return coef


def fit_h16_into(op_dev, I, coef, *, k, layout="pixel", flags=0):
    """Launch ``rti_fit_shared_h16`` on preallocated tensors: op_dev = h16_operator(...) on the device
    (uint8), I a contiguous uint8 CUDA [N, P] or [C, N, P] stack, coef fp32 as fit_shared_into."""
    return _fit_u8_into("h16", op_dev, I, coef, k, layout, flags)


def _u8_max_lights(form):
    return int(_u8_form(form)[3]())


def q8_supported(I, k, N, P, kernel="q8"):
    """Whether ``rti_fit_shared_q8`` (kernel="q8") or ``rti_fit_shared_h16`` (kernel="h16") takes this contiguous
    stack of P-pixel planes (uint8, k in {6, 9, 16}, N within the kernel's LDS budget, 16-byte aligned planes)."""
    if I.dtype != torch.uint8 or k not in (6, 9, 16) or N > _u8_max_lights("h16" if kernel == "h16" else "q8"):
        return False
    return P % 16 == 0 and I.data_ptr() % 16 == 0


def fit_q8_into(op_dev, I, coef, *, k, layout="pixel", flags=0):
    """Launch ``rti_fit_shared_q8`` on preallocated tensors: op_dev = q8_operator(...) on the device (uint8),
    I a contiguous uint8 CUDA [N, P] or [C, N, P] stack, coef fp32 as fit_shared_into."""
    return _fit_u8_into("q8", op_dev, I, coef, k, layout, flags)


_PM_KERNELS = ("auto", "valu", "mfma", "tile")  # the selectors rti_fit_shared_pm honours


def _fit_shared_pixel_major(I, lu, lv, b, k, rcond, cl, kernel, given_pixel_major):
    """rti.fit(mode="shared") on a pixel-major stack: ``rti_fit_shared_pm`` on the tensor's own memory.
    Integer kernel words pass through unchanged (the C entry refuses bits it does not document)."""
    if isinstance(kernel, str) and kernel not in _PM_KERNELS:
        raise NotImplementedError(f"kernel={kernel!r} does not take pixel-major stacks (rti_fit_shared_pm: "
                                  f"{', '.join(_PM_KERNELS)}); pass stack='light' with a light-major stack")
    if given_pixel_major:
        if I.dim() == 2:
            spatial, C = (I.shape[0],), 1
        elif I.dim() == 3:
            spatial, C = tuple(I.shape[:2]), 1
        elif I.dim() == 4:
            spatial, C = tuple(I.shape[1:3]), I.shape[0]
        else:
            raise ValueError("pixel-major I must be [P, N], [H, W, N] or [C, H, W, N]")
        N = I.shape[-1]
        v = I if I.stride(-1) == 1 else I.contiguous()
        if v.dim() == 3 and C == 1:
            v = v.reshape(-1, N)
        v = v.reshape(C, -1, N)
    else:
        v = _pixel_major_of(I)
        C, N = v.shape[0], v.shape[2]
        spatial = tuple(I.shape[-2:]) if I.dim() >= 3 else (I.shape[-1],)
    P = v.shape[1]
    if N < k:
        raise ValueError(f"shapes not aligned: {N} lights < {k} basis terms (analysis.py:298)")
    pv = pinv(lu, lv, b, rcond)
    if pv.shape[1] != N:
        raise ValueError(f"{pv.shape[1]} light directions for {N} intensity values per pixel")
    if I.dtype not in _IN_DTYPES:
        raise ValueError(f"I dtype {I.dtype} unsupported (float32, uint8 or int32)")
    coef = _coef_empty(C, P, k, cl, torch.float32, I.device)
    fit_shared_pm_into(torch.as_tensor(pv.astype(np.float32), device=I.device), v, coef, k=k, layout=cl,
                       kernel=kernel)
    return _unflatten(coef, spatial, I.dim() == 4, cl)


def basis_eval(lu, lv, basis="ptm"):
    """Host fp64 basis values [E, k] at (lu, lv)."""
    lu = np.ascontiguousarray(np.asarray(lu, np.float64).ravel())
    lv = np.ascontiguousarray(np.asarray(lv, np.float64).ravel())
    b = basis_id(basis)
    out = np.empty((lu.size, basis_terms(b)), np.float64)
    L.check(L.lib().rti_basis_eval(b, _dptr(lu), _dptr(lv), lu.size, _dptr(out)), "rti_basis_eval")
    return out


def _require_cuda(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor: librti runs only on the GPU, there is no CPU path")


def _stream_of(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _layout_id(layout):
    if layout in ("pixel", "pixel_major", L.RTI_COEF_PIXEL_MAJOR):
        return L.RTI_COEF_PIXEL_MAJOR
    if layout in ("planar", L.RTI_COEF_PLANAR):
        return L.RTI_COEF_PLANAR
    raise ValueError(f"unknown coefficient layout {layout!r} (expected 'pixel' or 'planar')")


def _kernel_word(kernel):
    """A kernel selector by name, or an integer kernel word as it is (the C entries refuse bits they do not
    document)."""
    return _KERNELS[kernel] if isinstance(kernel, str) else int(kernel)


def _stack_shape(I):
    """A light-major stack [N, P], [N, H, W] or [C, N, H, W] -> (C, N, P, spatial)."""
    if I.dim() == 2:
        (N, P), C, spatial = I.shape, 1, (I.shape[1],)
    elif I.dim() == 3:
        N, H, W = I.shape
        C, P, spatial = 1, H * W, (H, W)
    elif I.dim() == 4:
        C, N, H, W = I.shape
        P, spatial = H * W, (H, W)
    else:
        raise ValueError("I must be [N, P], [N, H, W] or [C, N, H, W]")
    return C, N, P, spatial


def _stack3(I, C, N, P):
    """The stack as the launchers take it: contiguous [C, N, P] (a copy only if I is not contiguous)."""
    return I.contiguous().reshape(C, N, P)


def _coef_empty(C, P, k, layout, dtype, device):
    """The coefficient tensor a launcher fills: [C, P, k] (pixel-major) or [C, k, P] (planar)."""
    shape = (C, P, k) if _layout_id(layout) == L.RTI_COEF_PIXEL_MAJOR else (C, k, P)
    return torch.empty(shape, dtype=dtype, device=device)


def _unflatten(t, spatial, lead, layout=None):
    """A launcher's output back in the caller's shape: a per-pixel map [C, P] -> [C, *spatial] (a per-channel
    scalar [C] with spatial = ()), or with ``layout`` coefficients [C, P, k] -> [C, *spatial, k] / [C, k, P] ->
    [C, k, *spatial]; without ``lead`` (the input had no channel axis) the leading C is dropped."""
    if layout is None:
        out = t.reshape(t.shape[:1] + spatial)
    elif _layout_id(layout) == L.RTI_COEF_PIXEL_MAJOR:
        out = t.reshape(t.shape[:1] + spatial + t.shape[2:])
    else:
        out = t.reshape(t.shape[:2] + spatial)
    return out if lead else out[0]


def _coef_spatial(coef, k, cl):
    """The spatial shape of coefficient maps [..., k] (pixel-major) or [k, ...] (planar)."""
    if cl == L.RTI_COEF_PIXEL_MAJOR:
        if coef.shape[-1] != k:
            raise ValueError(f"coef last dim {coef.shape[-1]} != {k} terms")
        return tuple(coef.shape[:-1])
    if coef.shape[0] != k:
        raise ValueError(f"coef first dim {coef.shape[0]} != {k} terms")
    return tuple(coef.shape[1:])


def fit_shared_into(pinv_dev, I, coef, *, k, layout="pixel", kernel="auto", nontemporal=False, flags=0):
    """Launch ``rti_fit_shared`` on preallocated tensors (no allocation, graph-capturable).

    pinv_dev: CUDA fp32 [k, N]; I: CUDA [C, N, P] or [N, P] (contiguous
    light-major, fp32/u8/int32); coef: CUDA fp32 [C, P, k] / [C, k, P]."""
    C, N, P = (1, *I.shape) if I.dim() == 2 else I.shape
    kern = _kernel_word(kernel)
    if nontemporal:
        kern |= L.RTI_KERNEL_NONTEMPORAL
    kern |= int(flags)
    st = L.lib().rti_fit_shared(_vp(pinv_dev), k, N, _vp(I), _IN_DTYPES[I.dtype], P, C, P, N * P, _vp(coef),
                                _layout_id(layout), P * k, kern, _stream_of(I))
    L.check(st, "rti_fit_shared")
    return coef


def fit_shared_pm_into(pinv_dev, I, coef, *, k, layout="pixel", kernel="auto", flags=0):
    """Launch ``rti_fit_shared_pm`` (pixel-major stacks, the reference's (R, R, N) layout,
    analysis.py:217-219) on preallocated tensors: pinv_dev CUDA fp32 [k, N]; I CUDA [P, N] or [C, P, N]
    with unit light stride (any pixel / channel stride, e.g. a view of [H, W, N]); coef as
    fit_shared_into.  A broadcast (stride-0) pixel or channel dimension is materialised first: the C ABI
    reads a zero stride as "dense"."""
    I3 = I if I.dim() == 3 else I.unsqueeze(0)
    C, P, N = I3.shape
    if I3.stride(2) != 1 and N > 1:
        raise ValueError("pixel-major stack needs unit light stride (I[..., p, n] with n contiguous)")
    if (P > 1 and I3.stride(1) == 0) or (C > 1 and I3.stride(0) == 0):
        I3 = I3.contiguous()
    ps = I3.stride(1) if P > 1 else N
    cs = I3.stride(0) if C > 1 else P * ps
    kern = _kernel_word(kernel) | int(flags)
    st = L.lib().rti_fit_shared_pm(_vp(pinv_dev), k, N, _vp(I3), _IN_DTYPES[I.dtype], P, C, ps, cs, _vp(coef),
                                   _layout_id(layout), P * k, kern, _stream_of(I))
    L.check(st, "rti_fit_shared_pm")
    return coef


def _pixel_major_of(I):
    """A light-major-shaped stack ([N, P], [N, H, W], [C, N, H, W]) that is a view of a pixel-major one
    (I.permute of the reference's [H, W, N]) -> the same data as [C, P, N] with unit light stride, else None."""
    if I.dim() < 2 or I.dim() > 4 or I.stride(1 if I.dim() == 4 else 0) != 1:
        return None  # the light dimension must be the unit-stride one
    if any(st == 0 and n > 1 for st, n in zip(I.stride(), I.shape)):
        return None  # a broadcast (expanded) dimension: not a pixel-major stack in memory
    if I.dim() == 2:
        v = I.t().unsqueeze(0)
    elif I.dim() == 3:
        N, H, W = I.shape
        if I.stride(1) != W * I.stride(2):
            return None
        v = I.permute(1, 2, 0).reshape(1, H * W, N) if H * W > 0 else None
    else:
        C, N, H, W = I.shape
        if I.stride(2) != W * I.stride(3):
            return None
        v = I.permute(0, 2, 3, 1).reshape(C, H * W, N)
    if v is None or v.data_ptr() != I.data_ptr() or v.stride(2) != 1 or v.shape[2] < 2:
        return None  # reshape copied: not a view
    return v


def fit(I, lu=None, lv=None, basis="ptm", mode="shared", rcond=None, *, cams=None, origin=(0.0, 0.0),
        layout="pixel", kernel="auto", coef_dtype=torch.float32, nontemporal=False, stack="auto"):
    """Fit per-pixel reflectance coefficients on the GPU.

    mode="shared" (the north_star path; directional lights, one (lu, lv) per light):
        I: CUDA tensor [N, H, W], [N, P] or [C, N, H, W] (light-major), fp32/u8/int32;
        with stack="pixel" the reference's own pixel-major layout instead, [H, W, N], [P, N] or
        [C, H, W, N] (analysis.py:217-219), fitted in place by ``rti_fit_shared_pm`` (no transpose).
        stack="auto" also routes a light-major-shaped VIEW of an fp32 / int32 pixel-major stack
        (``Ipm.permute(2, 0, 1)``) to that kernel instead of copying it, when kernel is one it takes
        ("auto", "valu", "mfma", "tile") and nontemporal is off; 8-bit views keep the copy + h16 path.
        lu, lv: N light directions (host or device).  Returns fp32 coefficients
        [.., H, W, k] (layout="pixel") or [.., k, H, W] (layout="planar").
        uint8 light-major stacks run the split-fp16 MFMA kernel under kernel="auto" (``rti_fit_shared_h16``:
        the operator carried to 22 significant bits, fp32 sums; within ≈1e-6 of max|c| of the fp32 stream
        that ``fit_shared_into`` / ``torch.ops.rti.fit_shared`` run on the same stack).
    mode="perpixel" (the reference's geometry, PTM only):
        either cams=[N, 3] camera positions with I light-major [N, H, W]
        (directions generated in-kernel, pixel (x, y) at origin + (x, y, 0)),
        or lu, lv, I pixel-major [H, W, N] exactly as compute_intensities returns
        them (analysis.py:217-219).  Coefficients in coef_dtype (fp32 or fp64).
    """
    _require_cuda(I, "I")
    cl = _layout_id(layout)
    if mode == "shared":
        if lu is None or lv is None:
            raise ValueError("shared mode needs lu and lv (one direction per light)")
        b = basis_id(basis)
        k = basis_terms(b)
        if stack not in ("auto", "light", "pixel"):
            raise ValueError(f"unknown stack layout {stack!r} (expected 'auto', 'light' or 'pixel')")
        if stack == "pixel":
            if nontemporal:
                raise NotImplementedError("nontemporal loads apply to light-major stacks (rti_fit_shared)")
            return _fit_shared_pixel_major(I, lu, lv, b, k, rcond, cl, kernel, True)
        # AUTO routes a pixel-major VIEW to rti_fit_shared_pm only where that kernel honours the request: fp32 /
        # int32 stacks (8-bit stacks keep the transposing copy and the h16 matrix-core fit) and the selectors and
        # options rti_fit_shared_pm takes; everything else keeps the light-major path below
        if (stack == "auto" and not I.is_contiguous() and I.dtype in (torch.float32, torch.int32)
                and kernel in _PM_KERNELS and not nontemporal and _pixel_major_of(I) is not None):
            return _fit_shared_pixel_major(I, lu, lv, b, k, rcond, cl, kernel, False)
        C, N, P, spatial = _stack_shape(I)
        if N < k:
            raise ValueError(f"shapes not aligned: {N} lights < {k} basis terms (analysis.py:298)")
        pv = pinv(lu, lv, b, rcond)
        if pv.shape[1] != N:
            raise ValueError(f"{pv.shape[1]} light directions for {N} intensity planes")
        Ic = _stack3(I, C, N, P)
        coef = _coef_empty(C, P, k, cl, torch.float32, I.device)
        # 8-bit stacks (the reference's V channel): AUTO runs the split-fp16 fit on the fp16 matrix cores
        # (kernel="h16"); kernel="q8" the int8 fixed-point form (exact sums); both need a finite
        # operator (a rank-deficient light set without rcond keeps the fp32 path and the reference's NaN)
        mk = "h16" if kernel == "auto" else kernel
        if mk in ("h16", "q8") and q8_supported(Ic, k, N, P, mk) and np.isfinite(pv).all():
            _fit_u8_into(mk, torch.as_tensor(_u8_operator(mk, pv), device=I.device), Ic, coef, k, cl, 0)
        elif kernel in ("q8", "h16"):
            raise NotImplementedError(f"kernel={kernel!r} needs a uint8 stack, k in (6, 9, 16), "
                                      f"N <= {_u8_max_lights(kernel)}, 16-pixel-aligned planes and a finite "
                                      "pseudo-inverse")
        else:
            pinv_dev = torch.as_tensor(pv.astype(np.float32), device=I.device)
            fit_shared_into(pinv_dev, Ic, coef, k=k, layout=cl, kernel=kernel, nontemporal=nontemporal)
        return _unflatten(coef, spatial, I.dim() == 4, cl)
    if mode != "perpixel":
        raise ValueError(f"unknown mode {mode!r} (expected 'shared' or 'perpixel')")
    if basis_id(basis) != L.RTI_BASIS_PTM6:
        raise NotImplementedError("per-pixel mode is the reference's PTM-6 path")
    cdt = _COEF_DTYPES.get(coef_dtype)
    if cdt is None:
        raise ValueError("coef_dtype must be torch.float32 or torch.float64")
    rc = _rcond(rcond)
    if cams is not None:
        if I.dim() != 3:
            raise ValueError("per-pixel camera mode needs I light-major [N, H, W]")
        N, H, W = I.shape
        cams_d = torch.as_tensor(np.asarray(cams.detach().cpu() if torch.is_tensor(cams) else cams, np.float64),
                                 device=I.device).contiguous()
        if cams_d.shape != (N, 3):
            raise ValueError(f"cams must be [{N}, 3]")
        Ic = I.contiguous()
        shape = (H, W, 6) if cl == L.RTI_COEF_PIXEL_MAJOR else (6, H, W)
        coef = torch.empty(shape, dtype=coef_dtype, device=I.device)
        st = L.lib().rti_fit_perpixel_cam(_vp(cams_d), N, _vp(Ic), _IN_DTYPES[Ic.dtype], H, W, H * W,
                                          float(origin[0]), float(origin[1]), rc, _vp(coef), cdt, cl, _stream_of(I))
        L.check(st, "rti_fit_perpixel_cam")
        return coef
    if lu is None or lv is None:
        raise ValueError("per-pixel mode needs cams=[N,3] or per-pixel lu, lv [H, W, N]")
    lu_d = torch.as_tensor(lu, device=I.device).to(torch.float32).contiguous()
    lv_d = torch.as_tensor(lv, device=I.device).to(torch.float32).contiguous()
    if lu_d.shape != I.shape or lv_d.shape != I.shape:
        raise ValueError("per-pixel lu, lv and I must share the pixel-major shape [.., N]")
    N = I.shape[-1]
    spatial = tuple(I.shape[:-1])
    P = int(np.prod(spatial)) if spatial else 1
    Ic = I.contiguous()
    shape = spatial + (6,) if cl == L.RTI_COEF_PIXEL_MAJOR else (6,) + spatial
    coef = torch.empty(shape, dtype=coef_dtype, device=I.device)
    st = L.lib().rti_fit_perpixel_dirs(_vp(lu_d), _vp(lv_d), _vp(Ic), _IN_DTYPES[Ic.dtype], N, P, rc, _vp(coef), cdt,
                                       cl, _stream_of(I))
    L.check(st, "rti_fit_perpixel_dirs")
    return coef


def fit_residual_into(A_dev, I3, coef, res, partial, *, k, layout="pixel"):
    """Launch ``rti_fit_residual`` on preallocated tensors (no allocation, graph-capturable).

    A_dev fp32 [N, k] (``design_matrix`` rounded to fp32, on the device), I3 CUDA [C, N, P] light-major
    (fp32/u8/int32), coef fp32 [C, P, k] / [C, k, P] contiguous, res fp32 [C, P], partial fp64
    [C, rti_fit_residual_blocks(P)] zeroed (or None): each workgroup's residual energy."""
    C, N, P = I3.shape
    st = L.lib().rti_fit_residual(_vp(A_dev), k, N, _vp(I3), _IN_DTYPES[I3.dtype], P, C, P, N * P, _vp(coef),
                                  _layout_id(layout), P * k, _vp(res), None if partial is None else _vp(partial),
                                  _stream_of(I3))
    L.check(st, "rti_fit_residual")


def fit_residual(I, coef, lu, lv, basis="ptm", *, layout="pixel"):
    """Per-pixel RMS residual of a shared-direction fit (``rti_fit_residual``).

    I: the stack ``fit`` was given ([N, P], [N, H, W] or [C, N, H, W]); coef: its
    fp32 output (same layout).  Returns ``(res, rms)``: res fp32 with I's spatial
    shape (plus the leading C for 4-D stacks) = sqrt(Σ_n (I_n − A_n·coef)² / N), and
    rms fp64 [C] (or a 0-d tensor) = the RMS residual over all pixels of a channel,
    summed from per-workgroup wavefront reductions on the device."""
    _require_cuda(I, "I")
    _require_cuda(coef, "coef")
    cl = _layout_id(layout)
    b = basis_id(basis)
    k = basis_terms(b)
    C, N, P, spatial = _stack_shape(I)
    if coef.dtype != torch.float32 or coef.numel() != C * P * k:
        raise ValueError(f"coef must be fp32 with {C}x{P}x{k} elements (the output of fit)")
    A = design_matrix(lu, lv, b)
    if A.shape[0] != N:
        raise ValueError(f"{A.shape[0]} light directions for {N} intensity planes")
    A_dev = torch.as_tensor(A.astype(np.float32), device=I.device).contiguous()
    Ic = _stack3(I, C, N, P)
    cc = coef.contiguous()
    res = torch.empty((C, P), dtype=torch.float32, device=I.device)
    nb = int(L.lib().rti_fit_residual_blocks(P))
    partial = torch.zeros((C, nb), dtype=torch.float64, device=I.device)
    fit_residual_into(A_dev, Ic, cc, res, partial, k=k, layout=cl)
    rms = torch.sqrt(partial.sum(dim=1) / (P * N))
    return _unflatten(res, spatial, I.dim() == 4), _unflatten(rms, (), I.dim() == 4)


def fit_shared_residual_into(U_dev, W_dev, I3, coef, res, partial, *, k, layout="pixel", chunks=0):
    """Launch ``rti_fit_shared_residual_svd`` on preallocated tensors (no allocation, graph-capturable).

    U_dev fp64 [N, k], W_dev fp64 [k, k] (``lsq_factors``), I3 CUDA [C, N, P] light-major, coef fp32
    [C, P, k] / [C, k, P], res fp32 [C, P] (or None), partial fp64 [C, rti_fit_shared_residual_blocks(P)]
    zeroed (or None)."""
    C, N, P = I3.shape
    cl = _layout_id(layout)
    st = L.lib().rti_fit_shared_residual_svd(_vp(U_dev), _vp(W_dev), k, N, _vp(I3), _IN_DTYPES[I3.dtype], P, C, P,
                                             N * P, _vp(coef), cl, P * k, None if res is None else _vp(res),
                                             None if partial is None else _vp(partial),
                                             int(chunks) << L.RTI_KERNEL_CHUNKS_SHIFT, _stream_of(I3))
    L.check(st, "rti_fit_shared_residual_svd")


def fit_with_residual(I, lu, lv, basis="ptm", rcond=None, *, layout="pixel", chunks=0):
    """Shared-direction fit AND per-pixel residuals in ONE pass over the stack
    (``rti_fit_shared_residual_svd``: the reference's SVD solve, analysis.py:295-298, per pixel —
    y = Uᵀ I and ‖I‖² accumulated in fp64, coefficients = V Σ⁻¹ y, residual energy ‖I‖² − ‖y‖²).

    I: CUDA [N, P], [N, H, W] or [C, N, H, W] (light-major, fp32/u8/int32).  Returns
    ``(coef, res, rms)``: coef fp32 as ``fit`` returns it (layout), res fp32 with I's spatial shape
    (leading C for 4-D stacks) = sqrt(Σ_n (I_n − A_n·coef)² / N) for the least-squares solution, and
    rms fp64 [C] (0-d for 2/3-D stacks) = the RMS residual over all pixels, summed from per-workgroup
    wavefront reductions.  An exactly rank-deficient light set (rcond=None) gives NaN coefficients AND
    NaN residuals, like the reference's division by a zero singular value."""
    _require_cuda(I, "I")
    if I.dtype not in _IN_DTYPES:
        raise ValueError(f"I dtype {I.dtype} unsupported (float32, uint8 or int32)")
    cl = _layout_id(layout)
    b = basis_id(basis)
    k = basis_terms(b)
    C, N, P, spatial = _stack_shape(I)
    if N < k:
        raise ValueError(f"shapes not aligned: {N} lights < {k} basis terms (analysis.py:298)")
    U, W = lsq_factors(lu, lv, b, rcond)
    if U.shape[0] != N:
        raise ValueError(f"{U.shape[0]} light directions for {N} intensity planes")
    dev = I.device
    U_dev = torch.as_tensor(U, device=dev).contiguous()
    W_dev = torch.as_tensor(W, device=dev).contiguous()
    Ic = _stack3(I, C, N, P)
    coef = _coef_empty(C, P, k, cl, torch.float32, dev)
    res = torch.empty((C, P), dtype=torch.float32, device=dev)
    partial = torch.zeros((C, int(L.lib().rti_fit_shared_residual_blocks(P))), dtype=torch.float64, device=dev)
    fit_shared_residual_into(U_dev, W_dev, Ic, coef, res, partial, k=k, layout=cl, chunks=chunks)
    rms = torch.sqrt(partial.sum(dim=1) / (P * N))
    lead = I.dim() == 4
    return _unflatten(coef, spatial, lead, cl), _unflatten(res, spatial, lead), _unflatten(rms, (), lead)


def fit_robust_into(A_dev, I3, coef, res, kept, fallback, *, k, lo, hi, min_lights, iters=0, delta=0.0,
                    layout="pixel", kernel=0):
    """Launch ``rti_fit_shared_robust`` on preallocated tensors (no allocation, graph-capturable).

    A_dev fp64 [N, k] (``design_matrix`` on the device), I3 CUDA [C, N, P] light-major (fp32/u8/int32), coef
    fp32 [C, P, k] / [C, k, P], res fp32 [C, P] or None, kept int32 [C, P] or None, fallback int32 [1] zeroed
    (or None): the count of pixels that fell back to every light.  lo / hi: the intensity window (±inf = no
    bound); kernel: 0 or ``RTI_KERNEL_ONE_LAUNCH`` (the streaming form, for measurement)."""
    C, N, P = I3.shape
    st = L.lib().rti_fit_shared_robust(_vp(A_dev), k, N, _vp(I3), _IN_DTYPES[I3.dtype], P, C, P, N * P, float(lo),
                                       float(hi), int(min_lights), int(iters), float(delta), _vp(coef),
                                       _layout_id(layout), P * k, None if res is None else _vp(res),
                                       None if kept is None else _vp(kept),
                                       None if fallback is None else _vp(fallback), int(kernel), _stream_of(I3))
    L.check(st, "rti_fit_shared_robust")


def _robust_window(I, lo, hi):
    """fit_robust's default window: none, except 1..254 for a uint8 stack given neither bound."""
    if lo is None and hi is None and I.dtype == torch.uint8:
        return 1.0, 254.0
    return (-np.inf if lo is None else float(lo)), (np.inf if hi is None else float(hi))


def fit_robust(I, lu, lv, basis="ptm", *, lo=None, hi=None, min_lights=None, iters=0, delta=None, layout="pixel",
               stats=None, kernel=0):
    """Shared-direction fit that leaves out the samples the model cannot describe
    (``rti_fit_shared_robust``): per pixel, the samples outside the intensity window [lo, hi] (clipped
    highlights, self-shadow) are dropped and, with iters > 0, the rest are reweighted ``iters`` times by
    Huber's function of their residuals, w = min(1, delta/|r|) (delta in intensity units).

    I: CUDA [N, P], [N, H, W] or [C, N, H, W] (light-major, fp32/u8/int32); PTM-6 or HSH-9.  lo / hi:
    None = no bound; a uint8 stack given NEITHER bound uses lo = 1, hi = 254 (the 8-bit clip values are
    dropped).  min_lights (default k): a pixel with fewer samples in the window, or whose windowed system
    is rank-deficient, falls back to every light.  Returns ``(coef, res, kept)``: coef fp32 as ``fit``
    returns it (layout), res fp32 with I's spatial shape (leading C for 4-D stacks) = the RMS residual
    over the pixel's window, kept int32 of the same shape = the samples in its window (N on fallback
    pixels).  ``stats``, if a dict, receives ``fallback_px`` (this waits for the kernel)."""
    _require_cuda(I, "I")
    if I.dtype not in _IN_DTYPES:
        raise ValueError(f"I dtype {I.dtype} unsupported (float32, uint8 or int32)")
    cl = _layout_id(layout)
    b = basis_id(basis)
    k = basis_terms(b)
    C, N, P, spatial = _stack_shape(I)
    if N < k:
        raise ValueError(f"shapes not aligned: {N} lights < {k} basis terms (analysis.py:298)")
    A = design_matrix(lu, lv, b)
    if A.shape[0] != N:
        raise ValueError(f"{A.shape[0]} light directions for {N} intensity planes")
    lo, hi = _robust_window(I, lo, hi)
    dev = I.device
    A_dev = torch.as_tensor(A, device=dev).contiguous()
    Ic = _stack3(I, C, N, P)
    coef = _coef_empty(C, P, k, cl, torch.float32, dev)
    res = torch.empty((C, P), dtype=torch.float32, device=dev)
    kept = torch.empty((C, P), dtype=torch.int32, device=dev)
    fallback = torch.zeros(1, dtype=torch.int32, device=dev)
    fit_robust_into(A_dev, Ic, coef, res, kept, fallback, k=k, lo=lo, hi=hi,
                    min_lights=k if min_lights is None else min_lights, iters=iters,
                    delta=0.0 if delta is None else delta, layout=cl, kernel=kernel)
    if isinstance(stats, dict):
        stats["fallback_px"] = int(fallback.item())
    lead = I.dim() == 4
    return _unflatten(coef, spatial, lead, cl), _unflatten(res, spatial, lead), _unflatten(kept, spatial, lead)


def ps_design(lu, lv, lz=None):
    """Host fp64 design matrix [N, 3] of photometric stereo (``rti_ps_design``): the rows (lu, lv, lw) with
    lw = sqrt(max(0, 1 − lu² − lv²)), or with a measured third component ``lz`` in its place."""
    lu, lv = _dirs(lu, lv)
    A = np.empty((lu.size, 3), dtype=np.float64)
    L.check(L.lib().rti_ps_design(_fptr(lu), _fptr(lv), lu.size, _dptr(A)), "rti_ps_design")
    if lz is not None:
        lz = np.asarray(lz.detach().cpu() if torch.is_tensor(lz) else lz, dtype=np.float64).ravel()
        if lz.size != lu.size:
            raise ValueError("lz and lu differ in length")
        A[:, 2] = lz
    return A


def photometric_stereo_into(A_dev, I3, normals, albedo, kind, res, kept, fallback, *, lo, hi, min_lights, iters=0,
                            delta=0.0, weights=None, normal_layout="pixel", kernel=0, light_stride=None):
    """Launch ``rti_photometric_stereo`` on preallocated tensors (no allocation, graph-capturable).

    A_dev fp64 [N, 3] (``ps_design`` on the device), I3 CUDA [C, N, P] light-major (fp32/u8/int32), C = 1 or 3;
    with ``light_stride`` > P it is a view of planes padded to that many elements (channel stride
    N·light_stride).  normals fp32 [P, 3] (normal_layout="pixel") or [3, P], albedo fp32 [C, P], kind uint8 [P]
    or None, res fp32 [C, P] or None, kept int32 [C, P] or None, fallback int32 [1] zeroed (or None): the count
    of channel-pixels that fell back to every light.  lo / hi: the intensity window (±inf = no bound); weights:
    None or the three luminance weights that combine an RGB pixel's channels into its normal; kernel: 0 or
    ``RTI_KERNEL_ONE_LAUNCH`` (the streaming form, for measurement)."""
    C, N, P = I3.shape
    ls = P if light_stride is None else int(light_stride)
    if A_dev.dtype != torch.float64 or tuple(A_dev.shape) != (N, 3) or not A_dev.is_contiguous():
        raise ValueError(f"A must be contiguous float64 [{N}, 3]; got {A_dev.dtype} {tuple(A_dev.shape)}")
    if ls < P or any(n > 1 and s != w for n, s, w in zip(I3.shape, I3.stride(), (N * ls, ls, 1))):
        raise ValueError(f"I3 strides {tuple(I3.stride())} are not light-major planes of stride {ls}")

    def opt(t, name, dtype, n):
        return None if t is None else _map_out(t, name, dtype, n, I3)

    st = L.lib().rti_photometric_stereo(_vp(A_dev), N, _vp(I3), _IN_DTYPES[I3.dtype], P, C, ls, N * ls, float(lo),
                                        float(hi), int(min_lights), int(iters), float(delta), _luma_weights(weights),
                                        _map_out(normals, "normals", torch.float32, 3 * P, I3),
                                        _normal_layout_id(normal_layout),
                                        _map_out(albedo, "albedo", torch.float32, C * P, I3),
                                        opt(kind, "kind", torch.uint8, P), opt(res, "res", torch.float32, C * P),
                                        opt(kept, "kept", torch.int32, C * P), opt(fallback, "fallback", torch.int32, 1),
                                        int(kernel), _stream_of(I3))
    L.check(st, "rti_photometric_stereo")


def photometric_stereo(I, lu, lv, lz=None, *, lo=None, hi=None, min_lights=None, iters=0, delta=None, weights=None,
                       normal_layout="pixel", return_kind=False, return_res=False, return_kept=False, stats=None,
                       kernel=0):
    """Surface normals and albedo by photometric stereo on the GPU (``rti_photometric_stereo``): the Lambertian
    model I_n = g·l_n fitted per pixel to the stack itself, n = g/‖g‖ and albedo ‖g‖, the normal map of
    RTIBuilder and Relight.  The samples the model cannot describe are left out as ``fit_robust`` leaves them
    out: those outside the intensity window [lo, hi] (attached shadow, clipped highlight) are dropped and, with
    iters > 0, the rest are reweighted ``iters`` times by Huber's function of their residuals (delta in
    intensity units).

    I: CUDA [N, P], [N, H, W] or [3, N, H, W] (light-major, fp32/u8/int32); an RGB stack gives ONE normal per
    pixel, from the weighted sum of its channels' fits (weights, default 0.299, 0.587, 0.114), and an albedo per
    channel.  lz: the lights' measured third component (default sqrt(1 − lu² − lv²)).  lo / hi: None = no bound;
    a uint8 stack given NEITHER bound uses 1..254.  min_lights (default 3): a channel of a pixel with fewer
    samples in the window, or whose windowed system is rank-deficient, falls back to every light.

    Returns ``(normals, albedo)``: fp32 unit normals [H, W, 3] (or [3, H, W] with normal_layout="planar") and
    fp32 albedo [H, W], or [H, W, 3] for RGB (an image).  Then, as asked: with return_kind uint8 [H, W] (0 a
    normal facing the viewer, 1 one facing away, returned as fitted, 2 g = 0: (0, 0, 1), 4 non-finite: NaN);
    with return_res fp32 [H, W] ([3, H, W] for RGB), the RMS residual over the window; with return_kept int32 of
    that shape, the samples in the window (N after a fallback).  ``stats``, if a dict, receives ``fallback_px``
    (this waits for the kernel)."""
    _require_cuda(I, "I")
    if I.dtype not in _IN_DTYPES:
        raise ValueError(f"I dtype {I.dtype} unsupported (float32, uint8 or int32)")
    nl = _normal_layout_id(normal_layout)
    C, N, P, spatial = _stack_shape(I)
    if C not in (1, 3):
        raise ValueError(f"a 4-D stack must be RGB, [3, N, H, W]; got {C} channels")
    if N < 3:
        raise ValueError(f"shapes not aligned: {N} lights < 3 unknowns")
    A = ps_design(lu, lv, lz)
    if A.shape[0] != N:
        raise ValueError(f"{A.shape[0]} light directions for {N} intensity planes")
    lo, hi = _robust_window(I, lo, hi)
    dev = I.device
    lead = I.dim() == 4
    normals = _coef_empty(1, P, 3, nl, torch.float32, dev)
    albedo = torch.empty((C, P), dtype=torch.float32, device=dev)
    kind = torch.empty((1, P), dtype=torch.uint8, device=dev) if return_kind else None
    res = torch.empty((C, P), dtype=torch.float32, device=dev) if return_res else None
    kept = torch.empty((C, P), dtype=torch.int32, device=dev) if return_kept else None
    fallback = torch.zeros(1, dtype=torch.int32, device=dev) if isinstance(stats, dict) else None
    photometric_stereo_into(torch.as_tensor(A, device=dev).contiguous(), _stack3(I, C, N, P), normals, albedo, kind,
                            res, kept, fallback, lo=lo, hi=hi, min_lights=3 if min_lights is None else min_lights,
                            iters=iters, delta=0.0 if delta is None else delta, weights=weights, normal_layout=nl,
                            kernel=kernel)
    if fallback is not None:
        stats["fallback_px"] = int(fallback.item())
    alb = _unflatten(albedo, spatial, lead)
    out = [_unflatten(normals, spatial, False, nl), alb.movedim(0, -1).contiguous() if lead else alb]
    if return_kind:
        out.append(_unflatten(kind, spatial, False))
    out += [_unflatten(t, spatial, lead) for t in (res, kept) if t is not None]
    return tuple(out)


def ps_near_lights(light_pos, light_scale=None):
    """Host fp64 [N, 4] light table of near-light photometric stereo: the rows (x, y, z, scale) from positions
    [N, 3] in the frame of ``light_dirs``' ``cams`` and the lights' relative strengths (default 1)."""
    pos = np.asarray(light_pos.detach().cpu() if torch.is_tensor(light_pos) else light_pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"light_pos must be [N, 3]; got {pos.shape}")
    lights = np.ones((pos.shape[0], 4), dtype=np.float64)
    lights[:, :3] = pos
    if light_scale is not None:
        sc = np.asarray(light_scale.detach().cpu() if torch.is_tensor(light_scale) else light_scale, dtype=np.float64)
        if sc.shape != (pos.shape[0],):
            raise ValueError(f"light_scale must be [{pos.shape[0]}]; got {sc.shape}")
        lights[:, 3] = sc
    return lights


def photometric_stereo_near_into(lights_dev, I3, H, W, normals, albedo, kind, res, kept, fallback, *, lo, hi,
                                 min_lights, origin=(0.0, 0.0), height=None, z_offset=0.0, falloff=True, r0=1.0,
                                 iters=0, delta=0.0, weights=None, normal_layout="pixel", kernel=0, light_stride=None):
    """Launch ``rti_photometric_stereo_near`` on preallocated tensors (no allocation, graph-capturable).

    lights_dev fp64 [N, 4] (``ps_near_lights`` on the device), I3 CUDA [C, N, H·W] light-major as
    ``photometric_stereo_into`` takes it (``light_stride`` likewise); pixel p = y·W + x sits at (origin[0] + x,
    origin[1] + y, z_offset + height[p]).  height: fp32 [H·W] (any shape of that many elements) or None = the
    plane; a non-finite entry counts as 0.  falloff: inverse-square strength (r0/r)², r0 the distance at which a
    light's scale is its strength; False = direction only.  The outputs and the remaining arguments as
    ``photometric_stereo_into``."""
    C, N, P = I3.shape
    H, W = int(H), int(W)
    if H * W != P:
        raise ValueError(f"H·W = {H}·{W} is not the stack's {P} pixels")
    ls = P if light_stride is None else int(light_stride)
    if lights_dev.dtype != torch.float64 or tuple(lights_dev.shape) != (N, 4) or not lights_dev.is_contiguous():
        raise ValueError(f"lights must be contiguous float64 [{N}, 4]; got {lights_dev.dtype} {tuple(lights_dev.shape)}")
    _require_cuda(lights_dev, "lights")
    if ls < P or any(n > 1 and s != w for n, s, w in zip(I3.shape, I3.stride(), (N * ls, ls, 1))):
        raise ValueError(f"I3 strides {tuple(I3.stride())} are not light-major planes of stride {ls}")

    def opt(t, name, dtype, n):
        return None if t is None else _map_out(t, name, dtype, n, I3)

    st = L.lib().rti_photometric_stereo_near(
        _vp(lights_dev), N, _vp(I3), _IN_DTYPES[I3.dtype], H, W, C, ls, N * ls, float(origin[0]), float(origin[1]),
        opt(height, "height", torch.float32, P), float(z_offset), int(bool(falloff)), float(r0), float(lo), float(hi),
        int(min_lights), int(iters), float(delta), _luma_weights(weights),
        _map_out(normals, "normals", torch.float32, 3 * P, I3), _normal_layout_id(normal_layout),
        _map_out(albedo, "albedo", torch.float32, C * P, I3), opt(kind, "kind", torch.uint8, P),
        opt(res, "res", torch.float32, C * P), opt(kept, "kept", torch.int32, C * P),
        opt(fallback, "fallback", torch.int32, 1), int(kernel), _stream_of(I3))
    L.check(st, "rti_photometric_stereo_near")


def photometric_stereo_near(I, light_pos, *, light_scale=None, origin=(0.0, 0.0), height=None, z_offset=0.0,
                            falloff=True, r0=None, refine=0, height_kw=None, return_height=False, lo=None, hi=None,
                            min_lights=None, iters=0, delta=None, weights=None, normal_layout="pixel",
                            return_kind=False, return_res=False, return_kept=False, stats=None, kernel=0):
    """``photometric_stereo`` for lights near the object (``rti_photometric_stereo_near``): every pixel gets its own
    light vector and strength from the light's position, l = s_n·(r0/r)²·d/r with d = light_pos_n − (origin[0] + x,
    origin[1] + y, z_offset + height[y, x]) and r = ‖d‖, instead of one direction for the whole image.

    I: CUDA [N, H, W] or [3, N, H, W] ([N, P] is one row of P pixels).  light_pos: [N, 3] in pixel units, in the
    frame of ``light_dirs``' ``cams`` (the reference pipeline's camera positions feed it as they are); light_scale:
    None or [N] relative strengths.  height: None (the plane z = z_offset) or fp32 [H, W] above z_offset; NaN
    counts as 0.  falloff=False keeps the direction only.  r0: the distance at which a light's scale is its
    strength, so the albedo stays in intensity units; default the lights' mean distance from the image centre at z =
    z_offset.  refine=K runs K rounds of normals -> ``height_from_normals(n, **height_kw)`` -> the same launch with
    that height; the height it returns has zero mean, so z_offset is the gauge and the caller's.  The workspace and
    the outputs are allocated once.  The robust arguments and the returns are ``photometric_stereo``'s, then with
    return_height the last height map used, fp32 [H, W] (zeros if none was)."""
    _require_cuda(I, "I")
    if I.dtype not in _IN_DTYPES:
        raise ValueError(f"I dtype {I.dtype} unsupported (float32, uint8 or int32)")
    nl = _normal_layout_id(normal_layout)
    C, N, P, spatial = _stack_shape(I)
    H, W = (1, P) if len(spatial) == 1 else spatial
    if C not in (1, 3):
        raise ValueError(f"a 4-D stack must be RGB, [3, N, H, W]; got {C} channels")
    if N < 3:
        raise ValueError(f"shapes not aligned: {N} lights < 3 unknowns")
    lights = ps_near_lights(light_pos, light_scale)
    if lights.shape[0] != N:
        raise ValueError(f"{lights.shape[0]} light positions for {N} intensity planes")
    refine = int(refine)
    if refine < 0:
        raise ValueError("refine must be >= 0")
    x0, y0, z_offset = float(origin[0]), float(origin[1]), float(z_offset)
    if r0 is None:
        centre = np.array([x0 + 0.5 * (W - 1), y0 + 0.5 * (H - 1), z_offset])
        r0 = float(np.linalg.norm(lights[:, :3] - centre, axis=1).mean())
    lo, hi = _robust_window(I, lo, hi)
    dev = I.device
    lead = I.dim() == 4
    if height is not None:
        _require_cuda(height, "height")
        if height.dtype != torch.float32 or height.numel() != P:
            raise ValueError(f"height must be float32 with {P} elements; got {height.dtype} {tuple(height.shape)}")
        height = height.contiguous()
    normals = _coef_empty(1, P, 3, nl, torch.float32, dev)
    albedo = torch.empty((C, P), dtype=torch.float32, device=dev)
    kind = torch.empty((1, P), dtype=torch.uint8, device=dev) if return_kind else None
    res = torch.empty((C, P), dtype=torch.float32, device=dev) if return_res else None
    kept = torch.empty((C, P), dtype=torch.int32, device=dev) if return_kept else None
    fallback = torch.zeros(1, dtype=torch.int32, device=dev) if isinstance(stats, dict) else None
    lights_dev = torch.as_tensor(lights, device=dev).contiguous()
    I3 = _stack3(I, C, N, P)

    def launch(h):
        photometric_stereo_near_into(lights_dev, I3, H, W, normals, albedo, kind, res, kept, fallback, lo=lo, hi=hi,
                                     min_lights=3 if min_lights is None else min_lights, origin=(x0, y0), height=h,
                                     z_offset=z_offset, falloff=falloff, r0=r0, iters=iters,
                                     delta=0.0 if delta is None else delta, weights=weights, normal_layout=nl,
                                     kernel=kernel)

    launch(height)
    if refine:
        kw = dict(height_kw or {})
        ws = height_workspace(H, W, kw.get("precond", "multigrid"), dev)
        hbuf = torch.empty((H, W), dtype=torch.float32, device=dev)
        n_map = normals[0].reshape((H, W, 3) if nl == L.RTI_NORMAL_PIXEL_MAJOR else (3, H, W))
        for _ in range(refine):
            height_from_normals_into(n_map, ws, hbuf, layout=nl, **kw)
            if fallback is not None:
                fallback.zero_()
            launch(hbuf)
        height = hbuf
    if fallback is not None:
        stats["fallback_px"] = int(fallback.item())
    alb = _unflatten(albedo, spatial, lead)
    out = [_unflatten(normals, spatial, False, nl), alb.movedim(0, -1).contiguous() if lead else alb]
    if return_kind:
        out.append(_unflatten(kind, spatial, False))
    out += [_unflatten(t, spatial, lead) for t in (res, kept) if t is not None]
    if return_height:
        out.append(torch.zeros((H, W), dtype=torch.float32, device=dev) if height is None else height.reshape(H, W))
    return tuple(out)


def fit_accumulate_into(R_dev, I3, state, *, k, init=False, light_stride=None):
    """Launch ``rti_fit_accumulate`` on preallocated tensors (no allocation, graph-capturable): add the chunk's
    B light planes to the fit state.

    R_dev fp64 [B, k]: the chunk's rows of the design matrix (or of U from ``lsq_factors``).  I3 CUDA
    [C, B, P] light-major (fp32/u8/int32); with ``light_stride`` > P it is a view of planes padded to that
    many elements (channel stride B·light_stride).  state fp64 [C, k+1, P], contiguous.  ``init``: the
    state is overwritten (never read), else added to."""
    C, B, P = I3.shape
    ls = P if light_stride is None else int(light_stride)
    if state.dtype != torch.float64 or tuple(state.shape) != (C, k + 1, P) or not state.is_contiguous():
        raise ValueError(f"state must be contiguous float64 [{C}, {k + 1}, {P}]; got {state.dtype} {tuple(state.shape)}")
    if R_dev.dtype != torch.float64 or tuple(R_dev.shape) != (B, k) or not R_dev.is_contiguous():
        raise ValueError(f"R must be contiguous float64 [{B}, {k}]; got {R_dev.dtype} {tuple(R_dev.shape)}")
    want = (B * ls, ls, 1)
    if ls < P or any(n > 1 and s != w for n, s, w in zip(I3.shape, I3.stride(), want)):
        raise ValueError(f"I3 strides {tuple(I3.stride())} are not light-major planes of stride {ls}")
    st = L.lib().rti_fit_accumulate(_vp(R_dev), k, B, _vp(I3), _IN_DTYPES[I3.dtype], P, C, ls, B * ls, _vp(state),
                                    (k + 1) * P, 1 if init else 0, _stream_of(I3))
    L.check(st, "rti_fit_accumulate")


def fit_accum_solve_into(M_dev, state, coef, res, *, k, n_lights, orth=False, layout="pixel"):
    """Launch ``rti_fit_accum_solve`` on preallocated tensors (no allocation, graph-capturable): coefficients
    and residuals from a fit state, which stays as it is.

    M_dev fp64 [k, k]: ``gram_inverse`` over every direction accumulated (state built from design rows), or
    with ``orth`` W of ``lsq_factors`` (state built from all N rows of U).  state fp64 [C, k+1, P]; coef fp32
    [C, P, k] / [C, k, P]; res fp32 [C, P] or None; n_lights: the lights accumulated."""
    C, k1, P = state.shape
    if state.dtype != torch.float64 or k1 != k + 1 or not state.is_contiguous():
        raise ValueError(f"state must be contiguous float64 [C, {k + 1}, P]; got {state.dtype} {tuple(state.shape)}")
    if M_dev.dtype != torch.float64 or tuple(M_dev.shape) != (k, k) or not M_dev.is_contiguous():
        raise ValueError(f"M must be contiguous float64 [{k}, {k}]; got {M_dev.dtype} {tuple(M_dev.shape)}")
    st = L.lib().rti_fit_accum_solve(_vp(M_dev), k, 1 if orth else 0, int(n_lights), _vp(state), P, C, (k + 1) * P,
                                     _vp(coef), _layout_id(layout), P * k, None if res is None else _vp(res),
                                     _stream_of(state))
    L.check(st, "rti_fit_accum_solve")


class FitAccumulator:
    """The shared-direction fit fed in chunks of light planes (``rti_fit_accumulate`` /
    ``rti_fit_accum_solve``): for stacks that do not fit in device memory and for frames that arrive over
    time, as the reference's frame loop produces one intensity plane and one light direction per video frame.

        acc = rti.FitAccumulator((H, W))
        for frame, lu, lv in frames: acc.add(frame, lu, lv)      # CUDA [H, W] (or [B, H, W] with B directions)
        coef, res = acc.solve()                                  # any time n_lights >= k; add() may go on

    The device holds only ``state``: fp64 [C, k+1, P], per pixel y = Aᵀ I and ‖I‖² over the lights so far.
    It does not depend on how the lights were split into chunks, to the bit.  ``solve`` is the Gram form,
    coef = (AᵀA)⁺ y over every direction seen (cond(A)² in its rounding error).  With
    ``directions=(lu_all, lv_all)`` given up front (the out-of-core case) the state is fed the rows of U of
    the thin SVD instead and ``solve`` is the reference's SVD solve (cond(A), as ``fit_with_residual``);
    ``add(frames)`` then takes the next rows in order, and ``solve`` needs all N planes.

    shape: (H, W) or (P,).  channels=None: single-channel frames, outputs carry no leading C; channels=C:
    frames are [C, B, H, W].  rcond: the SVD threshold of ``lsq_factors`` for ``directions`` (``solve`` takes
    its own otherwise)."""

    def __init__(self, shape, basis="ptm", *, channels=None, device="cuda", directions=None, rcond=None):
        self.spatial = tuple(int(s) for s in shape)
        if len(self.spatial) not in (1, 2) or min(self.spatial) < 1:
            raise ValueError(f"shape must be (H, W) or (P,); got {shape!r}")
        self.P = int(np.prod(self.spatial))
        self.basis = basis_id(basis)
        self.k = basis_terms(self.basis)
        if channels is not None and int(channels) < 1:
            raise ValueError(f"channels must be None or >= 1; got {channels!r}")
        self.channels = None if channels is None else int(channels)
        C = 1 if channels is None else self.channels
        self.state = torch.empty((C, self.k + 1, self.P), dtype=torch.float64, device=device)  # the first add inits
        _require_cuda(self.state, "device")
        self._factors = None
        if directions is not None:
            lu, lv = directions
            U, W = lsq_factors(lu, lv, self.basis, rcond)
            if U.shape[0] < self.k:
                raise ValueError(f"shapes not aligned: {U.shape[0]} lights < {self.k} basis terms (analysis.py:298)")
            self._factors = (U, torch.as_tensor(W, device=self.state.device).contiguous())
            self._dirs = (_f32_host(lu, "lu"), _f32_host(lv, "lv"))
        self.reset()

    def reset(self):
        """Forget every light: the next ``add`` overwrites the state."""
        self.n_lights = 0
        self.lu, self.lv = [], []
        return self

    def _chunk(self, frames):
        """frames -> [C, B, P] contiguous"""
        _require_cuda(frames, "frames")
        if frames.device != self.state.device:
            raise ValueError(f"frames on {frames.device}, the accumulator on {self.state.device}")
        if frames.dtype not in _IN_DTYPES:
            raise ValueError(f"frames dtype {frames.dtype} unsupported (float32, uint8 or int32)")
        sp, shp = self.spatial, tuple(frames.shape)
        if self.channels is None:
            if shp == sp:  # one frame
                return frames.contiguous().reshape(1, 1, self.P)
            if len(shp) >= 2 and (shp[1:] == sp or shp[1:] == (self.P,)):
                return frames.contiguous().reshape(1, shp[0], self.P)
            raise ValueError(f"frames {shp} are not {sp} planes ([H, W], [B, H, W] or [B, P])")
        if len(shp) >= 3 and shp[0] == self.channels and (shp[2:] == sp or shp[2:] == (self.P,)):
            return frames.contiguous().reshape(shp[0], shp[1], self.P)
        raise ValueError(f"frames {shp} are not [C={self.channels}, B] + {sp} planes")

    def add(self, frames, lu=None, lv=None):
        """Add B light planes: CUDA [H, W] (one frame; lu, lv scalars), [B, H, W], [B, P] or, with channels,
        [C, B, H, W]; float32 / uint8 / int32, and chunks of different dtypes may be mixed.  lu, lv: the B
        directions (not with ``directions=``, where the planes take the next B rows in order)."""
        I3 = self._chunk(frames)
        B = I3.shape[1]
        if self._factors is not None:
            if lu is not None or lv is not None:
                raise ValueError("this accumulator was given every direction up front: add(frames) takes no lu / lv")
            U, (lu_all, lv_all) = self._factors[0], self._dirs
            if self.n_lights + B > U.shape[0]:
                raise ValueError(f"{self.n_lights + B} intensity planes for {U.shape[0]} light directions")
            rows = U[self.n_lights:self.n_lights + B]
            lu, lv = lu_all[self.n_lights:self.n_lights + B], lv_all[self.n_lights:self.n_lights + B]
        else:
            if lu is None or lv is None:
                raise ValueError("add(frames, lu, lv): the planes' light directions are missing")
            lu, lv = _f32_host(lu, "lu"), _f32_host(lv, "lv")
            if lu.size != B or lv.size != B:
                raise ValueError(f"{lu.size} / {lv.size} light directions for {B} intensity planes")
            rows = design_matrix(lu, lv, self.basis)  # a row of A depends on its own light only
        R_dev = torch.as_tensor(np.ascontiguousarray(rows), device=self.state.device)
        fit_accumulate_into(R_dev, I3, self.state, k=self.k, init=self.n_lights == 0)
        self.n_lights += B
        self.lu.extend(float(x) for x in lu)
        self.lv.extend(float(x) for x in lv)
        return self

    def solve(self, rcond=None, layout="pixel"):
        """``(coef, res)`` of the lights added so far, shaped as ``fit_with_residual`` returns its first two
        values; the state is left as it is (a preview: ``add`` may go on, ``solve`` may be repeated)."""
        cl = _layout_id(layout)
        k, P, N = self.k, self.P, self.n_lights
        if N < k:
            raise ValueError(f"shapes not aligned: {N} lights < {k} basis terms (analysis.py:298)")
        dev = self.state.device
        if self._factors is not None:
            if rcond is not None:
                raise ValueError("with directions= the SVD threshold is the constructor's rcond")
            if N != self._factors[0].shape[0]:
                raise ValueError(f"{N} of {self._factors[0].shape[0]} planes added: a prefix of U's rows is not an "
                                 "orthonormal basis, so this form has no preview (omit directions= for one)")
            M_dev, orth = self._factors[1], True
        else:
            ginv = gram_inverse(np.asarray(self.lu, np.float32), np.asarray(self.lv, np.float32), self.basis, rcond)
            M_dev, orth = torch.as_tensor(ginv, device=dev).contiguous(), False
        C = self.state.shape[0]
        coef = _coef_empty(C, P, k, cl, torch.float32, dev)
        res = torch.empty((C, P), dtype=torch.float32, device=dev)
        fit_accum_solve_into(M_dev, self.state, coef, res, k=k, n_lights=N, orth=orth, layout=cl)
        lead = self.channels is not None
        return _unflatten(coef, self.spatial, lead, cl), _unflatten(res, self.spatial, lead)


def fit_chunked(chunks, shape, basis="ptm", *, rcond=None, layout="pixel", **kw):
    """The out-of-core shared fit: consume an iterable of ``(frames, lu, lv)`` chunks (with
    ``directions=``: of ``frames``) through a ``FitAccumulator`` and return ``solve()``'s ``(coef, res)``.
    The stack may live in host memory or on disk: CPU chunks are moved with
    ``.to(device, non_blocking=True)`` (pinned chunks overlap the previous chunk's kernel; the producer
    must not rewrite a pinned buffer before its copy has run).  kw: channels, device, directions."""
    if kw.get("directions") is not None:
        kw["rcond"] = rcond
    acc = FitAccumulator(shape, basis, **kw)
    for chunk in chunks:
        frames, *d = chunk if isinstance(chunk, (tuple, list)) else (chunk,)
        if torch.is_tensor(frames) and not frames.is_cuda:
            frames = frames.to(acc.state.device, non_blocking=True)
        acc.add(frames, *d)
    return acc.solve(None if acc._factors is not None else rcond, layout)


def light_dirs(cams, H, W, origin=(0.0, 0.0), device="cuda"):
    """compute_intensities' light vectors on the GPU: (lu, lv) fp32 [H, W, N]."""
    cams_d = torch.as_tensor(np.asarray(cams.detach().cpu() if torch.is_tensor(cams) else cams, np.float64),
                             device=device).contiguous()
    _require_cuda(cams_d, "cams")
    N = cams_d.shape[0]
    lu = torch.empty((H, W, N), dtype=torch.float32, device=cams_d.device)
    lv = torch.empty_like(lu)
    st = L.lib().rti_light_dirs(_vp(cams_d), N, H, W, float(origin[0]), float(origin[1]), _vp(lu), _vp(lv),
                                _stream_of(cams_d))
    L.check(st, "rti_light_dirs")
    return lu, lv


def relight(coef, lu, lv, basis="ptm", *, layout="pixel", out_dtype=torch.float32, out_layout="eval"):
    """Evaluate coefficient maps at light directions on the GPU.

    coef: CUDA fp32/fp64, [H, W, k] / [P, k] (layout="pixel") or [k, H, W] /
    [k, P] (layout="planar").  lu, lv: scalars or E directions.
    Returns [E, H, W] (out_layout="eval") or [H, W, E] (out_layout="pixel"),
    squeezed to [H, W] for a single scalar direction.  out_dtype int32 gives
    the reference's truncated tables, uint8 its clipped display values."""
    _require_cuda(coef, "coef")
    b = basis_id(basis)
    k = basis_terms(b)
    cl = _layout_id(layout)
    cdt = _COEF_DTYPES.get(coef.dtype)
    if cdt is None:
        raise ValueError("coef must be float32 or float64")
    odt = _OUT_DTYPES.get(out_dtype)
    if odt is None:
        raise ValueError("out_dtype must be float32, float64, int32 or uint8")
    spatial = _coef_spatial(coef, k, cl)
    P = int(np.prod(spatial))
    scalar = np.ndim(lu) == 0 and np.ndim(lv) == 0
    luv = np.stack([np.asarray(lu, np.float64).ravel(), np.asarray(lv, np.float64).ravel()], -1)
    E = luv.shape[0]
    luv_d = torch.as_tensor(np.ascontiguousarray(luv), device=coef.device)
    ol = L.RTI_OUT_EVAL_MAJOR if out_layout == "eval" else L.RTI_OUT_PIXEL_MAJOR
    shape = (E,) + spatial if ol == L.RTI_OUT_EVAL_MAJOR else spatial + (E,)
    out = torch.empty(shape, dtype=out_dtype, device=coef.device)
    c = coef.contiguous()
    st = L.lib().rti_relight(_vp(c), cdt, b, P, cl, _vp(luv_d), E, _vp(out), odt, ol, _stream_of(c))
    L.check(st, "rti_relight")
    if scalar:
        return out[0] if ol == L.RTI_OUT_EVAL_MAJOR else out[..., 0]
    return out


def relight_frame(src, hsv, lu=None, lv=None, basis="ptm", *, layout="pixel", out=None):
    """One relighting_event image on the GPU (interactive_relighting.py:31-38):
    V = clip(value, 0, 255) written into the HSV ROI's V channel, then OpenCV's 8-bit
    HSV -> BGR conversion, in one launch.

    src: CUDA int32 [H, W] table image (the cursor's interpolation_results[ly][lx]), or
    fp32/fp64 coefficient maps ([H, W, k] layout="pixel" / [k, H, W] "planar") evaluated at
    (lu, lv) and truncated to int32 like the reference's tables.
    hsv: CUDA uint8 [H, W, 3].  Returns (or fills ``out``) CUDA uint8 [H, W, 3] BGR."""
    _require_cuda(src, "src")
    _require_cuda(hsv, "hsv")
    if hsv.dtype != torch.uint8 or hsv.shape[-1] != 3:
        raise ValueError("hsv must be uint8 [..., 3]")
    spatial = tuple(hsv.shape[:-1])
    P = int(np.prod(spatial))
    if src.dtype == torch.int32:
        if int(src.numel()) != P:
            raise ValueError(f"table image has {src.numel()} pixels, hsv has {P}")
        sdt, b, cl, u, v = L.RTI_I32, L.RTI_BASIS_PTM6, L.RTI_COEF_PIXEL_MAJOR, 0.0, 0.0
    else:
        sdt = _COEF_DTYPES.get(src.dtype)
        if sdt is None:
            raise ValueError("src must be an int32 table image or float32/float64 coefficients")
        if lu is None or lv is None:
            raise ValueError("coefficient maps need a light direction (lu, lv)")
        b = basis_id(basis)
        k = basis_terms(b)
        cl = _layout_id(layout)
        if int(src.numel()) != P * k:
            raise ValueError(f"coefficients {tuple(src.shape)} do not match {k} terms x {P} pixels")
        u, v = float(lu), float(lv)
    h = hsv.contiguous()
    c = src.contiguous()
    if out is None:
        out = torch.empty(spatial + (3,), dtype=torch.uint8, device=hsv.device)
    elif out.dtype != torch.uint8 or int(out.numel()) != 3 * P or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor with 3 bytes per pixel")
    if out.data_ptr() == h.data_ptr():
        raise ValueError("out may not alias hsv")
    st = L.lib().rti_relight_frame(_vp(c), sdt, b, cl, P, u, v, _vp(h), _vp(out), _stream_of(h))
    L.check(st, "rti_relight_frame")
    return out


# ---- PTM surface normals and enhanced relighting (rti_normals.hip) ------------

# the normal layouts carry the coefficient layouts' values ([p][·] = 0, [·][p] = 1; tests/test_normals_abi.py), so
# _coef_empty and _unflatten shape a normal map as they shape 3-term coefficients
_NORMAL_LAYOUTS = {"pixel": L.RTI_NORMAL_PIXEL_MAJOR, "pixel_major": L.RTI_NORMAL_PIXEL_MAJOR,
                   "planar": L.RTI_NORMAL_PLANAR, L.RTI_NORMAL_PIXEL_MAJOR: L.RTI_NORMAL_PIXEL_MAJOR,
                   L.RTI_NORMAL_PLANAR: L.RTI_NORMAL_PLANAR}
ENHANCE_MODES = {"diffuse_gain": L.RTI_ENHANCE_DIFFUSE_GAIN, "specular": L.RTI_ENHANCE_SPECULAR}
_ENHANCED_DTYPES = {torch.float32: L.RTI_F32, torch.int32: L.RTI_I32, torch.uint8: L.RTI_U8}


def _normal_layout_id(layout):
    try:
        return _NORMAL_LAYOUTS[layout]
    except (KeyError, TypeError):
        raise ValueError(f"unknown normal layout {layout!r} (expected 'pixel' or 'planar')") from None


def _enhance_mode_id(mode):
    if isinstance(mode, int):
        return mode
    try:
        return ENHANCE_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"unknown mode {mode!r} (expected one of {sorted(ENHANCE_MODES)})") from None


def _ptm_maps(coef, k):
    """Contiguous CUDA fp32 / fp64 coefficient maps of k terms per pixel -> (dtype id, P)."""
    _require_cuda(coef, "coef")
    cdt = _COEF_DTYPES.get(coef.dtype)
    if cdt is None:
        raise ValueError("coef must be float32 or float64")
    if not coef.is_contiguous() or coef.numel() == 0 or coef.numel() % k:
        raise ValueError(f"coef must be contiguous maps of {k} terms per pixel; got {tuple(coef.shape)}")
    return cdt, coef.numel() // k


def _map_out(t, name, dtype, n, like):
    """A caller-allocated output: contiguous, ``dtype``, n elements, on the coefficients' device."""
    _require_cuda(t, name)
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of {n} elements on {like.device}; got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return _vp(t)


def ptm_normals_into(coef, normals, kind=None, peak=None, *, layout="pixel", normal_layout="pixel", basis="ptm"):
    """Launch ``rti_ptm_normals`` on preallocated tensors (no allocation, graph-capturable).

    coef: contiguous CUDA fp32 / fp64 maps, [P, 6] (layout="pixel") or [6, P] ("planar"), any spatial shape in
    place of P; normals: fp32 with 3 values per pixel, [P, 3] (normal_layout="pixel") or [3, P]; kind: uint8
    [P] or None; peak: fp32 [P] or None."""
    b = basis_id(basis)
    cdt, P = _ptm_maps(coef, basis_terms(b))
    st = L.lib().rti_ptm_normals(_vp(coef), cdt, b, _layout_id(layout), P,
                                 _map_out(normals, "normals", torch.float32, 3 * P, coef),
                                 _normal_layout_id(normal_layout),
                                 None if kind is None else _map_out(kind, "kind", torch.uint8, P, coef),
                                 None if peak is None else _map_out(peak, "peak", torch.float32, P, coef),
                                 _stream_of(coef))
    L.check(st, "rti_ptm_normals")
    return normals


def relight_enhanced_into(coef, lu, lv, mode, out, *, gain=1.0, kd=1.0, ks=0.0, exp=1, layout="pixel", basis="ptm"):
    """Launch ``rti_relight_enhanced`` on preallocated tensors (no allocation, graph-capturable).

    coef as ``ptm_normals_into``; out: fp32, int32 or uint8 with one element per pixel; mode "diffuse_gain"
    or "specular" (or the RTI_ENHANCE_* value)."""
    b = basis_id(basis)
    cdt, P = _ptm_maps(coef, basis_terms(b))
    odt = _ENHANCED_DTYPES.get(out.dtype) if torch.is_tensor(out) else None
    if odt is None:
        raise ValueError("out must be a float32, int32 or uint8 tensor")
    st = L.lib().rti_relight_enhanced(_vp(coef), cdt, b, _layout_id(layout), P, _enhance_mode_id(mode), float(gain),
                                      float(kd), float(ks), int(exp), float(lu), float(lv),
                                      _map_out(out, "out", out.dtype, P, coef), odt, _stream_of(coef))
    L.check(st, "rti_relight_enhanced")
    return out


def normals(coef, *, layout="pixel", normal_layout="pixel", return_kind=False, return_peak=False, basis="ptm"):
    """Per-pixel surface normals of PTM-6 coefficient maps on the GPU (``rti_ptm_normals``): the light
    direction at which each pixel's fitted biquadratic peaks (Malzbender et al. 2001), in fp64 per pixel.

    coef: CUDA fp32/fp64, [H, W, 6] / [P, 6] (layout="pixel") or [6, H, W] / [6, P] ("planar").  Returns
    fp32 unit normals [H, W, 3] (normal_layout="pixel") or [3, H, W] ("planar"); with return_kind also
    uint8 [H, W] (0 interior maximum, 1 maximum outside the unit disc, projected onto its edge, 2 no
    maximum: the Lambertian reading of the linear terms, 4 non-finite coefficients: NaN normal); with
    return_peak also fp32 [H, W], the PTM's value at the normal (an albedo proxy).  Only PTM-6 has a
    closed-form maximum: any other basis raises NotImplementedError."""
    _require_cuda(coef, "coef")
    b = basis_id(basis)
    cl, nl = _layout_id(layout), _normal_layout_id(normal_layout)
    spatial = _coef_spatial(coef, basis_terms(b), cl)
    P = int(np.prod(spatial))
    n = _coef_empty(1, P, 3, nl, torch.float32, coef.device)
    kind = torch.empty((1, P), dtype=torch.uint8, device=coef.device) if return_kind else None
    peak = torch.empty((1, P), dtype=torch.float32, device=coef.device) if return_peak else None
    ptm_normals_into(coef.contiguous(), n, kind, peak, layout=cl, normal_layout=normal_layout, basis=b)
    out = (_unflatten(n, spatial, False, nl),) + tuple(_unflatten(t, spatial, False) for t in (kind, peak)
                                                       if t is not None)
    return out if len(out) > 1 else out[0]


def relight_enhanced(coef, lu, lv, mode, *, gain=1.0, kd=1.0, ks=0.0, exp=1, layout="pixel",
                     out_dtype=torch.float32, basis="ptm"):
    """One enhanced rendering of PTM-6 coefficient maps at the light direction (lu, lv) on the GPU
    (``rti_relight_enhanced``; Malzbender et al. 2001), computed from the coefficients alone.

    mode="diffuse_gain": each pixel's curvature scaled by ``gain`` (>= 0) about its peak, whose location and
    height stay (gain=1 is ``relight``).  mode="specular": kd·L(lu, lv) + ks·max(0, n·H)^exp with n the pixel's
    normal (``normals``), H the half vector between the light and the viewer and exp an integer in [1, 255]
    (kd=1, ks=0 is ``relight``).  coef as ``normals``.  Returns the spatial shape in out_dtype: float32, or
    int32 / uint8 converted as ``relight`` does; an int32 result is a valid ``src`` of ``relight_frame``."""
    _require_cuda(coef, "coef")
    b = basis_id(basis)
    cl = _layout_id(layout)
    spatial = _coef_spatial(coef, basis_terms(b), cl)
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    out = torch.empty((1, int(np.prod(spatial))), dtype=out_dtype, device=coef.device)
    relight_enhanced_into(coef.contiguous(), lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp, layout=cl, basis=b)
    return _unflatten(out, spatial, False)


# ---- unsharp masking of maps, shading from a normal map (rti_unsharp.hip) ------------

def gauss_taps(sigma, radius=None):
    """The normalised Gaussian taps w[0..R] ``rti_map_unsharp`` convolves with (host, fp64): w0 + 2·Σ w = 1.
    radius None = max(1, ceil(3·sigma))."""
    lib = L.lib()
    R = lib.rti_gauss_radius(float(sigma)) if radius is None else int(radius)
    if R < 0:
        raise ValueError(f"rti_gauss_radius: sigma {sigma!r} must be finite and positive")
    taps = np.zeros(max(R, 0) + 1, np.float64)
    L.check(lib.rti_gauss_taps(float(sigma), R, _dptr(taps)), "rti_gauss_taps")
    return taps


def _map_dims(src, layout, renorm=False):
    """A dense fp32 map [H, W], [H, W, k] (pixel-major) or [k, H, W] (planar) on the GPU -> (channels, H, W).  The
    dtype and the shape are judged before the device, so a wrong map is named as such wherever it lives."""
    if not torch.is_tensor(src):
        raise ValueError("map must be a CUDA (HIP) tensor")
    if src.dtype != torch.float32:
        raise ValueError(f"map must be float32 (fp64 maps are not built); got {src.dtype}")
    if src.dim() == 2:
        k, (H, W) = 1, src.shape
    elif src.dim() == 3:
        k, H, W = (src.shape[2], src.shape[0], src.shape[1]) if layout == L.RTI_COEF_PIXEL_MAJOR else tuple(src.shape)
    else:
        raise ValueError(f"map must be [H, W], [H, W, k] (pixel) or [k, H, W] (planar); got {tuple(src.shape)}")
    if renorm and k != 3:
        raise ValueError(f"renorm needs 3 channels (a normal map); got {k}")
    if not src.is_contiguous():
        raise ValueError("map must be contiguous (strided maps are not built)")
    _require_cuda(src, "map")
    return int(k), int(H), int(W)


def map_unsharp_into(src, dst, *, sigma, amount=1.0, radius=0, layout="pixel", renorm=False):
    """Launch ``rti_map_unsharp`` on preallocated tensors (no allocation, graph-capturable).

    src: contiguous CUDA fp32 [H, W], [H, W, k] (layout="pixel") or [k, H, W] ("planar"), k <= 16; dst: the
    same shape, not overlapping src.  dst = src + amount·(src − blur) with blur the Gaussian of ``sigma``
    cut at ``radius`` (0 = max(1, ceil(3·sigma)), at most 32), normalised over the finite pixels inside the
    image; a pixel with a non-finite channel is copied.  renorm (k = 3): the result scaled to unit length."""
    cl = _layout_id(layout)
    k, H, W = _map_dims(src, cl, renorm)
    _require_cuda(dst, "dst")
    if dst.dtype != torch.float32 or dst.shape != src.shape or not dst.is_contiguous() or dst.device != src.device:
        raise ValueError(f"dst must be a contiguous float32 tensor of shape {tuple(src.shape)} on {src.device}; got "
                         f"{dst.dtype} {tuple(dst.shape)} on {dst.device}")
    st = L.lib().rti_map_unsharp(_vp(src), k, cl, H, W, float(sigma), int(radius), float(amount), int(bool(renorm)),
                                 _vp(dst), _stream_of(src))
    L.check(st, "rti_map_unsharp")
    return dst


def unsharp(map, sigma, amount=1.0, *, radius=None, layout="pixel", renorm=False):
    """Unsharp masking of a k-channel map on the GPU (``rti_map_unsharp``): map + amount·(map − blur).

    map: CUDA fp32 [H, W], [H, W, k] (layout="pixel") or [k, H, W] ("planar"), k <= 16; returns the same
    shape.  On coefficient maps this is unsharp masking of the relit image at every light direction at once
    (relighting is linear in the coefficients): ``relight(unsharp(coef, s, a), lu, lv)``.  amount=-1 is the
    plain Gaussian blur.  NaN / inf pixels (``fit_robust``, ``normals`` kind 4) are left out of their
    neighbours' blur and copied.  radius None = max(1, ceil(3·sigma)); at most 32.  Not built: maps split
    over GPUs (``rti.parallel`` row tiles would need a halo exchange), fp64 and strided maps."""
    if not torch.is_tensor(map):
        raise ValueError("map must be a CUDA (HIP) tensor")
    src = map.contiguous()
    return map_unsharp_into(src, torch.empty_like(src), sigma=sigma, amount=amount, radius=0 if radius is None else radius,
                            layout=layout, renorm=renorm)


def normals_unsharp(n, sigma, amount=1.0, **kw):
    """Enhanced normals: ``unsharp`` of a normal map ([H, W, 3] / [3, H, W]) renormalised to unit length."""
    return unsharp(n, sigma, amount, renorm=True, **kw)


def shade_normals_into(n, lu, lv, out, *, albedo=None, kd=1.0, ks=0.0, exp=1, normal_layout="pixel"):
    """Launch ``rti_shade_normals`` on preallocated tensors (no allocation, graph-capturable).

    n: contiguous CUDA fp32 normals, [P, 3] (normal_layout="pixel") or [3, P], any spatial shape in place of P;
    albedo: None or fp32 [P]; out: fp32, int32 or uint8 with one element per pixel."""
    if not torch.is_tensor(n) or n.dtype != torch.float32 or not n.is_contiguous() or n.numel() == 0 or n.numel() % 3:
        raise ValueError("n must be a contiguous float32 normal map of 3 values per pixel; got "
                         f"{getattr(n, 'dtype', type(n))} {tuple(getattr(n, 'shape', ()))}")
    _require_cuda(n, "n")
    P = n.numel() // 3
    odt = _ENHANCED_DTYPES.get(out.dtype) if torch.is_tensor(out) else None
    if odt is None:
        raise ValueError("out must be a float32, int32 or uint8 tensor")
    st = L.lib().rti_shade_normals(_vp(n), _normal_layout_id(normal_layout),
                                   None if albedo is None else _map_out(albedo, "albedo", torch.float32, P, n), P,
                                   float(kd), float(ks), int(exp), float(lu), float(lv),
                                   _map_out(out, "out", out.dtype, P, n), odt, _stream_of(n))
    L.check(st, "rti_shade_normals")
    return out


def shade_normals(n, lu, lv, *, albedo=None, kd=1.0, ks=0.0, exp=1, normal_layout="pixel", out_dtype=torch.float32):
    """One image shaded from a normal map at the light direction (lu, lv) on the GPU (``rti_shade_normals``):
    kd·albedo·max(0, n·l) + ks·max(0, n·H)^exp with l = (lu, lv, sqrt(max(0, 1 − lu² − lv²))) and H the half
    vector between l and the viewer.  The renderer of ``normals_unsharp``: ``relight_enhanced`` recomputes its
    normals from the coefficients and cannot take a map.

    n: CUDA fp32 [H, W, 3] / [P, 3] (normal_layout="pixel") or [3, H, W] / [3, P] ("planar"); albedo: None (1)
    or fp32 with one value per pixel (e.g. the peak of ``normals``).  Returns the spatial shape in out_dtype
    (float32, or int32 / uint8 converted as ``relight`` does); NaN normals or albedo give NaN."""
    if not torch.is_tensor(n) or n.dtype != torch.float32:
        raise ValueError(f"n must be a float32 normal map; got {getattr(n, 'dtype', type(n))}")
    nl = _normal_layout_id(normal_layout)
    spatial = _coef_spatial(n, 3, nl)
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    _require_cuda(n, "n")
    P = int(np.prod(spatial))
    if albedo is not None:
        _require_cuda(albedo, "albedo")
        if tuple(albedo.shape) != spatial:
            raise ValueError(f"albedo {tuple(albedo.shape)} does not match the normal map's pixels {spatial}")
        albedo = albedo.contiguous().reshape(P)
    out = torch.empty((1, P), dtype=out_dtype, device=n.device)
    shade_normals_into(n.contiguous(), lu, lv, out, albedo=albedo, kd=kd, ks=ks, exp=exp, normal_layout=nl)
    return _unflatten(out, spatial, False)


# ---- LRGB PTMs: colour fit and one-pass RGB relight (rti_lrgb.hip) ------------

def gram(lu, lv):
    """Host fp64 Gram matrix AᵀA [6, 6] of the shared PTM-6 design (``design_matrix``): with it the
    least-squares colour of a pixel follows from its three coefficient vectors (``lrgb_from_rgb``)."""
    A = design_matrix(lu, lv, "ptm")
    return A.T @ A


def _gram_host(gram):
    g = np.ascontiguousarray(np.asarray(gram.detach().cpu() if torch.is_tensor(gram) else gram, dtype=np.float64))
    if g.shape != (6, 6):
        raise ValueError(f"gram must be [6, 6] (rti.gram(lu, lv)); got {g.shape}")
    return g


def _weights_host(weights):
    if weights is None:
        return None
    w = np.ascontiguousarray(np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights,
                                        dtype=np.float64).ravel())
    if w.size != 3:
        raise ValueError(f"weights must be 3 channel weights; got {w.size}")
    return w


def _lrgb_map(lrgb):
    """A contiguous CUDA fp32 LRGB map of 9 values per pixel -> P."""
    _require_cuda(lrgb, "lrgb")
    if lrgb.dtype != torch.float32 or not lrgb.is_contiguous() or lrgb.numel() == 0 or lrgb.numel() % 9:
        raise ValueError(f"lrgb must be a contiguous float32 map of 9 values per pixel; got {lrgb.dtype} "
                         f"{tuple(lrgb.shape)}")
    return lrgb.numel() // 9


def lrgb_from_rgb_into(coef, gram, lrgb, *, weights=None, layout="pixel", lrgb_layout="pixel"):
    """Launch ``rti_lrgb_from_rgb`` on preallocated tensors (no allocation, graph-capturable).

    coef: contiguous CUDA fp32, three PTM-6 maps [3, P, 6] (layout="pixel") or [3, 6, P] ("planar"), any
    spatial shape in place of P; gram: host fp64 [6, 6] (``gram``); weights: None (1/3 each) or 3 host
    values; lrgb: fp32 with 9 values per pixel, [P, 9] (lrgb_layout="pixel") or [9, P]."""
    _require_cuda(coef, "coef")
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.dim() < 2 or coef.shape[0] != 3 \
            or coef.numel() == 0 or coef.numel() % 18:
        raise ValueError(f"coef must be three contiguous float32 PTM-6 maps [3, ...]; got {coef.dtype} "
                         f"{tuple(coef.shape)}")
    P = coef.numel() // 18
    g, w = _gram_host(gram), _weights_host(weights)
    st = L.lib().rti_lrgb_from_rgb(_vp(coef), _layout_id(layout), 6 * P, P, _dptr(g), None if w is None else _dptr(w),
                                   _map_out(lrgb, "lrgb", torch.float32, 9 * P, coef), _layout_id(lrgb_layout),
                                   _stream_of(coef))
    L.check(st, "rti_lrgb_from_rgb")
    return lrgb


def lrgb_from_rgb(coef, gram, *, weights=None, layout="pixel", lrgb_layout="pixel"):
    """Three per-channel PTM-6 maps -> one LRGB map on the GPU (``rti_lrgb_from_rgb``): the luminance
    coefficients a = Σ_c w_c·coef_c and, per pixel, the RGB colour that best explains the three channels as
    colour · luminance over the lights of the fit (least squares, from the coefficients and the Gram matrix
    alone: no second pass over the stack).

    coef: CUDA fp32 [3, H, W, 6] (layout="pixel") or [3, 6, H, W] ("planar"), as ``fit`` returns it for a
    [3, N, H, W] stack; gram: ``gram(lu, lv)`` of the fit's directions; weights: None (1/3 each) or 3
    non-negative values (not normalised).  Returns fp32 [H, W, 9] (lrgb_layout="pixel") or [9, H, W]:
    (a0..a5, cR, cG, cB), Σ_c w_c·chroma_c = 1; a black pixel has chroma 1, a non-finite one nine NaNs."""
    _require_cuda(coef, "coef")
    cl, ol = _layout_id(layout), _layout_id(lrgb_layout)
    if coef.dim() < 2 or coef.shape[0] != 3:
        raise ValueError(f"coef must be three PTM-6 maps [3, ...]; got {tuple(coef.shape)}")
    spatial = _coef_spatial(coef[0], 6, cl)
    out = _coef_empty(1, int(np.prod(spatial)), 9, ol, torch.float32, coef.device)
    lrgb_from_rgb_into(coef.contiguous(), gram, out, weights=weights, layout=cl, lrgb_layout=ol)
    return _unflatten(out, spatial, False, ol)


def fit_lrgb(I, lu, lv, *, weights=None, rcond=None, lrgb_layout="pixel", **fit_kw):
    """Fit an LRGB PTM to a colour stack on the GPU: ``fit`` of the three channels (one pass over the stack),
    then ``lrgb_from_rgb``.

    I: CUDA [3, N, H, W] light-major, any dtype ``fit`` takes; lu, lv: the N directions.  fit_kw: ``fit``'s
    keywords (kernel, layout of the intermediate maps, ...); PTM-6, shared mode.  Returns fp32 [H, W, 9] or
    [9, H, W] (lrgb_layout)."""
    _require_cuda(I, "I")
    if I.dim() != 4 or I.shape[0] != 3:
        raise ValueError(f"I must be a colour stack [3, N, H, W]; got {tuple(I.shape)}")
    if basis_id(fit_kw.pop("basis", "ptm")) != L.RTI_BASIS_PTM6:
        raise NotImplementedError("rti_lrgb_from_rgb: LRGB maps are PTM-6 only")
    if fit_kw.pop("mode", "shared") != "shared":
        raise NotImplementedError("fit_lrgb: the Gram matrix is that of a shared light set (mode='shared')")
    layout = fit_kw.pop("layout", "pixel")
    coef = fit(I, lu, lv, "ptm", "shared", rcond, layout=layout, **fit_kw)
    return lrgb_from_rgb(coef, gram(lu, lv), weights=weights, layout=layout, lrgb_layout=lrgb_layout)


def relight_lrgb_into(lrgb, luv_dev, out, *, layout="pixel"):
    """Launch ``rti_relight_lrgb`` on preallocated tensors (no allocation, graph-capturable).

    lrgb: contiguous CUDA fp32 [P, 9] (layout="pixel") or [9, P], any spatial shape in place of P; luv_dev:
    CUDA fp64 [E, 2]; out: float32, int32 or uint8 with E·P·3 elements ([E, P, 3], RGB interleaved)."""
    P = _lrgb_map(lrgb)
    _require_cuda(luv_dev, "luv")
    if luv_dev.dtype != torch.float64 or luv_dev.dim() != 2 or luv_dev.shape[1] != 2 or luv_dev.shape[0] < 1 \
            or not luv_dev.is_contiguous() or luv_dev.device != lrgb.device:
        raise ValueError(f"luv must be a contiguous float64 [E, 2] tensor on {lrgb.device}; got {luv_dev.dtype} "
                         f"{tuple(luv_dev.shape)} on {luv_dev.device}")
    E = luv_dev.shape[0]
    odt = _ENHANCED_DTYPES.get(out.dtype) if torch.is_tensor(out) else None
    if odt is None:
        raise ValueError("out must be a float32, int32 or uint8 tensor")
    st = L.lib().rti_relight_lrgb(_vp(lrgb), _layout_id(layout), P, _vp(luv_dev), E,
                                  _map_out(out, "out", out.dtype, E * P * 3, lrgb), odt, _stream_of(lrgb))
    L.check(st, "rti_relight_lrgb")
    return out


def relight_lrgb(lrgb, lu, lv, *, layout="pixel", out_dtype=torch.float32):
    """Relight an LRGB map to RGB images on the GPU in one launch (``rti_relight_lrgb``): per pixel
    chroma_c · L(lu, lv), the map read once for every direction.

    lrgb: CUDA fp32 [H, W, 9] / [P, 9] (layout="pixel") or [9, H, W] / [9, P] ("planar").  lu, lv: scalars or
    E directions.  Returns [E, H, W, 3], squeezed to [H, W, 3] for scalar directions, in out_dtype: float32,
    or int32 / uint8 converted as ``relight`` does."""
    _require_cuda(lrgb, "lrgb")
    cl = _layout_id(layout)
    spatial = _coef_spatial(lrgb, 9, cl)
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    scalar = np.ndim(lu) == 0 and np.ndim(lv) == 0
    luv = np.stack([np.asarray(lu, np.float64).ravel(), np.asarray(lv, np.float64).ravel()], -1)
    luv_d = torch.as_tensor(np.ascontiguousarray(luv), device=lrgb.device)
    E = luv.shape[0]
    out = torch.empty((E,) + spatial + (3,), dtype=out_dtype, device=lrgb.device)
    relight_lrgb_into(lrgb.contiguous(), luv_d, out, layout=cl)
    return out[0] if scalar else out


def lrgb_luminance(lrgb, layout="planar"):
    """The luminance planes [6, H, W] of a planar LRGB map [9, H, W]: a view of the same storage, no copy.  It
    is a dense planar PTM-6 map: ``normals``, ``relight_enhanced`` and ``unsharp`` take it with
    layout="planar" (and ``relight`` gives the grey image).  Pixel-major maps raise ValueError: their
    luminance is a strided map, which those entries do not support (fit with lrgb_layout="planar")."""
    if _layout_id(layout) != L.RTI_COEF_PLANAR:
        raise ValueError("lrgb_luminance needs a planar LRGB map [9, ...]: the luminance of a pixel-major map is "
                         "strided, which normals / relight_enhanced / unsharp do not take")
    if not torch.is_tensor(lrgb) or lrgb.dim() < 2 or lrgb.shape[0] != 9 or not lrgb.is_contiguous():
        raise ValueError(f"lrgb must be a contiguous planar LRGB map [9, ...]; got {tuple(getattr(lrgb, 'shape', ()))}")
    return lrgb[:6]


# ---- 8-bit maps: what the three quantised objects and their entry points share ----------------

class _Quantised:
    """The base of ``QuantisedLRGB``, ``QuantisedHSH`` and ``QuantisedRGB``: a contiguous uint8 ``coef`` and a
    ``qparams`` vector on one device, immutable.  A subclass lists its slots in its constructor's order, says in
    TAKES what the constructor takes and in MADE_BY where such an object comes from, sets QDTYPE, and gives
    ``_set`` its shape rule and the length of its qparams."""
    __slots__ = ()
    QDTYPE = torch.float64

    def _set(self, tensors, coef_form, coef_ok, nq, then=None):
        """Check and store the tensors (name -> tensor, coef first, qparams last); ``then`` checks what a subclass
        holds besides, once coef is known to be sound."""
        coef, qparams = tensors["coef"], tensors["qparams"]
        if not all(torch.is_tensor(t) for t in tensors.values()):
            raise ValueError(f"{type(self).__name__} takes {self.TAKES}")
        if coef.dtype != torch.uint8 or coef.numel() == 0 or not coef.is_contiguous() or not coef_ok(coef):
            raise ValueError(f"coef must be a contiguous uint8 {coef_form} tensor; got {coef.dtype} "
                             f"{tuple(coef.shape)}")
        if then is not None:
            then()
        if qparams.dtype != self.QDTYPE or tuple(qparams.shape) != (nq,) or not qparams.is_contiguous():
            raise ValueError(f"qparams must be a contiguous {_dtype_name(self.QDTYPE)} [{nq}] tensor; got "
                             f"{qparams.dtype} {tuple(qparams.shape)}")
        if len({t.device for t in tensors.values()}) != 1:
            names = list(tensors)
            raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} must be on one device; got "
                             f"{', '.join(str(t.device) for t in tensors.values())}")
        for name, t in tensors.items():
            object.__setattr__(self, "_" + name, t)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    coef = property(lambda self: self._coef)
    qparams = property(lambda self: self._qparams)
    device = property(lambda self: self._coef.device)

    def _host(self):
        return self._qparams.detach().cpu().numpy()

    def _args(self):
        return tuple(getattr(self, slot) for slot in self.__slots__)

    def to(self, device):
        return type(self)(*(a.to(device) if torch.is_tensor(a) else a for a in self._args()))

    def _file_qparams(self):
        """qparams on the host with the six scales rounded to the nine significant digits of a .ptm header."""
        qp = self._host().copy()
        qp[:6] = [float("%.9g" % x) for x in qp[:6]]
        return qp

    def _with_qparams(self, qp):
        """The same bytes with the host array qp for qparams."""
        return type(self)(*(torch.as_tensor(qp).to(self.device) if a is self._qparams else a for a in self._args()))


def _dtype_name(dtype):
    return str(dtype).replace("torch.", "")


def _quantised(q, cls, name="q"):
    """q must be a cls on the GPU."""
    if not isinstance(q, cls):
        raise ValueError(f"{name} must be a {cls.__name__} ({cls.MADE_BY}); got {type(q).__name__}")
    _require_cuda(q.coef, f"{name}.coef")


def _bytes_map(coef8, nbytes, what):
    """A contiguous CUDA uint8 map of nbytes per pixel (``what`` in words) -> P."""
    _require_cuda(coef8, "coef8")
    if coef8.dtype != torch.uint8 or not coef8.is_contiguous() or coef8.numel() == 0 or coef8.numel() % nbytes:
        raise ValueError(f"coef8 must be a contiguous uint8 map of {what} per pixel; got {coef8.dtype} "
                         f"{tuple(coef8.shape)}")
    return coef8.numel() // nbytes


def _qparams_arg(qparams, dtype, n, like):
    _require_cuda(qparams, "qparams")
    if qparams.dtype != dtype or qparams.numel() != n or not qparams.is_contiguous() or qparams.device != like.device:
        raise ValueError(f"qparams must be a contiguous {_dtype_name(dtype)} [{n}] tensor on {like.device}; got "
                         f"{qparams.dtype} {tuple(qparams.shape)} on {qparams.device}")
    return _vp(qparams)


def _workspace_bytes(n, P):
    """What a ``rti_*_qparams_workspace`` query returned -> the bytes, or P was not positive."""
    if n <= 0:
        raise ValueError(f"P must be positive; got {P}")
    return int(n)


def _workspace_arg(workspace, need, like):
    _require_cuda(workspace, "workspace")
    if not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need \
            or workspace.device != like.device:
        raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on {like.device}; got "
                         f"{workspace.numel() * workspace.element_size()} bytes on {workspace.device}")
    return _vp(workspace)


def _luv_arg(luv_dev, like):
    """CUDA fp64 [E, 2] on like's device -> (pointer, E)."""
    _require_cuda(luv_dev, "luv")
    if luv_dev.dtype != torch.float64 or luv_dev.dim() != 2 or luv_dev.shape[1] != 2 or luv_dev.shape[0] < 1 \
            or not luv_dev.is_contiguous() or luv_dev.device != like.device:
        raise ValueError(f"luv must be a contiguous float64 [E, 2] tensor on {like.device}; got {luv_dev.dtype} "
                         f"{tuple(luv_dev.shape)} on {luv_dev.device}")
    return _vp(luv_dev), luv_dev.shape[0]


def _out8_dtype(out):
    odt = _ENHANCED_DTYPES.get(out.dtype) if torch.is_tensor(out) else None
    if odt is None:
        raise ValueError("out must be a float32, int32 or uint8 tensor")
    return odt


def _relight8(q, lu, lv, out_dtype, launch):
    """What ``relight_lrgb8``, ``relight_hsh8`` and ``relight_rgb8`` do around their launch(luv_dev, out)."""
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    scalar = np.ndim(lu) == 0 and np.ndim(lv) == 0
    luv = np.stack([np.asarray(lu, np.float64).ravel(), np.asarray(lv, np.float64).ravel()], -1)
    luv_d = torch.as_tensor(np.ascontiguousarray(luv), device=q.device)
    out = torch.empty((luv.shape[0],) + q.shape + (3,), dtype=out_dtype, device=q.device)
    launch(luv_d, out)
    return out[0] if scalar else out


# ---- 8-bit LRGB PTMs: the .ptm payload on the device (rti_lrgb8.hip) ---------

class QuantisedLRGB(_Quantised):
    """An 8-bit LRGB PTM: the two blocks of a ``PTM_FORMAT_LRGB`` payload and its header values.

    coef: uint8 [H, W, 6] or [P, 6], the bytes a0..a5 per pixel; rgb: uint8 [..., 3]; qparams: fp64 [13] =
    scale[0..5], bias[0..5] (integral), s (the chroma scale the quantiser used; 1 for a map read from a file,
    which does not carry it).  Rows top first.  All three tensors on one device (the GPU, or the host for
    ``read_ptm(path, quantised=True)``); immutable.  ``scale`` / ``bias`` / ``s`` copy qparams to the host: they
    are the one accessor that synchronises."""
    __slots__ = ("_coef", "_rgb", "_qparams")
    TAKES = "three tensors (coef, rgb, qparams)"
    MADE_BY = "quantise_lrgb, or read_ptm(path, quantised=True)"

    def __init__(self, coef, rgb, qparams):
        def rgb_block():
            want = tuple(coef.shape[:-1]) + (3,)
            if rgb.dtype != torch.uint8 or tuple(rgb.shape) != want or not rgb.is_contiguous():
                raise ValueError(f"rgb must be a contiguous uint8 {want} tensor; got {rgb.dtype} {tuple(rgb.shape)}")
        self._set({"coef": coef, "rgb": rgb, "qparams": qparams}, "[..., 6]",
                  lambda c: c.dim() >= 2 and c.shape[-1] == 6, 13, rgb_block)

    rgb = property(lambda self: self._rgb)
    shape = property(lambda self: tuple(self._coef.shape[:-1]), doc="the spatial shape: (H, W) or (P,)")
    scale = property(lambda self: self._host()[:6].copy(), doc="host fp64 [6] (synchronises)")
    bias = property(lambda self: self._host()[6:12].copy(), doc="host fp64 [6], integral values (synchronises)")
    s = property(lambda self: float(self._host()[12]), doc="the chroma scale, a host float (synchronises)")

    def with_file_scales(self):
        """The map as a .ptm round trip yields it: the same bytes, the scales rounded to the nine significant
        digits ``write_ptm`` puts in the header, s = 1.  ``quantise_lrgb`` keeps the full fp64 scales the bytes
        were made with; a file does not, so ``dequantise_lrgb`` / ``relight_lrgb8`` of this map, not of the fresh
        one, equal ``read_ptm`` of the written file to the bit.  Synchronises."""
        qp = self._file_qparams()
        qp[12] = 1.0
        return self._with_qparams(qp)

    def __repr__(self):
        return f"QuantisedLRGB(shape={self.shape}, device={self.device})"


def lrgb_qparams_workspace(P):
    """Bytes of device scratch ``lrgb_qparams_into`` needs for P pixels (``rti_lrgb_qparams_workspace``)."""
    return _workspace_bytes(L.lib().rti_lrgb_qparams_workspace(int(P)), P)


def lrgb_qparams_into(lrgb, workspace, qparams, *, layout="pixel"):
    """Launch ``rti_lrgb_qparams`` on preallocated tensors (no allocation, graph-capturable): the six scales, six
    biases and the chroma scale ``write_ptm`` would give the map.

    lrgb: contiguous CUDA fp32 [P, 9] (layout="pixel") or [9, P], any spatial shape in place of P; workspace: a
    contiguous CUDA tensor of at least ``lrgb_qparams_workspace(P)`` bytes (it need not be initialised);
    qparams: CUDA fp64 [13]."""
    P = _lrgb_map(lrgb)
    ws = _workspace_arg(workspace, lrgb_qparams_workspace(P), lrgb)
    st = L.lib().rti_lrgb_qparams(_vp(lrgb), _layout_id(layout), P, ws, _qparams_arg(qparams, torch.float64, 13, lrgb),
                                  _stream_of(lrgb))
    L.check(st, "rti_lrgb_qparams")
    return qparams


def lrgb_quantise_into(lrgb, qparams, coef8, rgb8, *, layout="pixel"):
    """Launch ``rti_lrgb_quantise`` on preallocated tensors (no allocation, graph-capturable).

    lrgb: as ``lrgb_qparams_into``; qparams: CUDA fp64 [13] (``lrgb_qparams_into``); coef8: uint8 with 6·P
    elements ([P, 6]); rgb8: uint8 with 3·P elements ([P, 3]).  Returns (coef8, rgb8)."""
    P = _lrgb_map(lrgb)
    st = L.lib().rti_lrgb_quantise(_vp(lrgb), _layout_id(layout), P, _qparams_arg(qparams, torch.float64, 13, lrgb),
                                   _map_out(coef8, "coef8", torch.uint8, 6 * P, lrgb),
                                   _map_out(rgb8, "rgb8", torch.uint8, 3 * P, lrgb), _stream_of(lrgb))
    L.check(st, "rti_lrgb_quantise")
    return coef8, rgb8


def quantise_lrgb(lrgb, *, layout="pixel"):
    """Quantise an LRGB map to the 9 bytes per pixel of a .ptm file on the GPU (``rti_lrgb_qparams`` then
    ``rti_lrgb_quantise``): the bytes, scales and biases ``write_ptm`` computes on the host, without the copy.

    lrgb: CUDA fp32 [H, W, 9] / [P, 9] (layout="pixel") or [9, H, W] / [9, P] ("planar").  Returns a
    ``QuantisedLRGB`` on lrgb's device; ``write_ptm(path, q)`` writes it, ``relight_lrgb8`` renders it."""
    _require_cuda(lrgb, "lrgb")
    cl = _layout_id(layout)
    spatial = _coef_spatial(lrgb, 9, cl)
    m = lrgb.contiguous()
    P = _lrgb_map(m)
    ws = torch.empty(lrgb_qparams_workspace(P), dtype=torch.uint8, device=m.device)
    qparams = torch.empty(13, dtype=torch.float64, device=m.device)
    coef8 = torch.empty(spatial + (6,), dtype=torch.uint8, device=m.device)
    rgb8 = torch.empty(spatial + (3,), dtype=torch.uint8, device=m.device)
    lrgb_qparams_into(m, ws, qparams, layout=cl)
    lrgb_quantise_into(m, qparams, coef8, rgb8, layout=cl)
    return QuantisedLRGB(coef8, rgb8, qparams)


def dequantise_lrgb(q):
    """The fp32 LRGB map [..., 9] of a quantised one, with ``read_ptm``'s arithmetic: (byte − bias)·scale and
    byte/255 in fp64, rounded once to fp32.  Plain torch operations on q's device (not a hot path): what
    ``normals``, ``relight_enhanced`` and ``unsharp`` need to take a loaded file's luminance."""
    if not isinstance(q, QuantisedLRGB):
        raise ValueError(f"q must be a QuantisedLRGB; got {type(q).__name__}")
    qp = q.qparams
    coef = (q.coef.double() - qp[6:12]) * qp[:6]
    # a tensor divisor: division by a Python scalar may be evaluated as a product with its reciprocal
    rgb = q.rgb.double() / torch.full((1,), 255.0, dtype=torch.float64, device=q.device)
    return torch.cat([coef, rgb], -1).float()


def relight_lrgb8_into(coef8, rgb8, qparams, luv_dev, out):
    """Launch ``rti_relight_lrgb8`` on preallocated tensors (no allocation, graph-capturable).

    coef8: contiguous CUDA uint8 [P, 6], any spatial shape in place of P; rgb8: uint8 [P, 3]; qparams: CUDA fp64
    [13]; luv_dev: CUDA fp64 [E, 2]; out: float32, int32 or uint8 with E·P·3 elements ([E, P, 3])."""
    P = _bytes_map(coef8, 6, "6 bytes")
    _require_cuda(rgb8, "rgb8")
    if rgb8.dtype != torch.uint8 or not rgb8.is_contiguous() or rgb8.numel() != 3 * P or rgb8.device != coef8.device:
        raise ValueError(f"rgb8 must be a contiguous uint8 tensor of {3 * P} elements on {coef8.device}; got "
                         f"{rgb8.dtype} {tuple(rgb8.shape)} on {rgb8.device}")
    luv, E = _luv_arg(luv_dev, coef8)
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_lrgb8(_vp(coef8), _vp(rgb8), P, _qparams_arg(qparams, torch.float64, 13, coef8), luv, E,
                                   _map_out(out, "out", out.dtype, E * P * 3, coef8), odt, _stream_of(coef8))
    L.check(st, "rti_relight_lrgb8")
    return out


def relight_lrgb8(q, lu, lv, *, out_dtype=torch.float32):
    """Relight a quantised LRGB map to RGB images on the GPU in one launch (``rti_relight_lrgb8``), reading 9
    bytes per pixel once for every direction.  The images equal ``relight_lrgb(dequantise_lrgb(q), lu, lv)``
    bit for bit.

    q: a ``QuantisedLRGB`` on the GPU.  lu, lv: scalars or E directions.  Returns [E, H, W, 3], squeezed to
    [H, W, 3] for scalar directions, in out_dtype: float32, or int32 / uint8 converted as ``relight`` does."""
    _quantised(q, QuantisedLRGB)
    return _relight8(q, lu, lv, out_dtype,
                     lambda luv_d, out: relight_lrgb8_into(q.coef, q.rgb, q.qparams, luv_d, out))


# ---- 8-bit RGB HSH maps: the .rti payload on the device (rti_hsh8.hip) -------

_HSH8_NAMES = {L.RTI_BASIS_HSH9: "hsh9", L.RTI_BASIS_HSH16: "hsh16"}
_HSH8_TERMS = {L.RTI_BASIS_HSH9: 9, L.RTI_BASIS_HSH16: 16}


def _hsh8_basis(basis):
    """A basis name or id -> the id of HSH-9 or HSH-16; anything else is not built."""
    b = basis_id(basis)
    if b not in _HSH8_NAMES:
        raise NotImplementedError(f"8-bit HSH maps are HSH-9 and HSH-16 only; got basis {basis!r}")
    return b


class QuantisedHSH(_Quantised):
    """An 8-bit RGB HSH map: the payload of an HSH ``.rti`` file and its header values.

    coef: uint8 [H, W, 3, k] or [P, 3, k], per pixel the k bytes of R, then G, then B; qparams: fp32 [2k] =
    scale[0..k-1], bias[0..k-1], shared by the three channels; basis: "hsh9" (k = 9) or "hsh16" (k = 16).  A
    coefficient is ``byte·(scale/255) + bias`` in fp32 (``dequantise_hsh``).  Rows top first.  Both tensors on one
    device (the GPU, or the host for ``read_rti(path, quantised=True)``); immutable.  ``scale`` / ``bias`` copy
    qparams to the host: they are the one accessor that synchronises."""
    __slots__ = ("_coef", "_qparams", "_basis")
    TAKES = "two tensors (coef, qparams) and a basis"
    MADE_BY = "quantise_hsh, or read_rti(path, quantised=True)"
    QDTYPE = torch.float32

    def __init__(self, coef, qparams, basis):
        b = _hsh8_basis(basis)
        k = _HSH8_TERMS[b]
        self._set({"coef": coef, "qparams": qparams}, f"[..., 3, {k}]",
                  lambda c: c.dim() >= 3 and tuple(c.shape[-2:]) == (3, k), 2 * k)
        object.__setattr__(self, "_basis", b)

    basis = property(lambda self: _HSH8_NAMES[self._basis], doc='"hsh9" or "hsh16"')
    k = property(lambda self: _HSH8_TERMS[self._basis], doc="terms per channel: 9 or 16")
    shape = property(lambda self: tuple(self._coef.shape[:-2]), doc="the spatial shape: (H, W) or (P,)")
    scale = property(lambda self: self._host()[:self.k].copy(), doc="host fp32 [k] (synchronises)")
    bias = property(lambda self: self._host()[self.k:].copy(), doc="host fp32 [k] (synchronises)")

    def __repr__(self):
        return f"QuantisedHSH(shape={self.shape}, basis={self.basis!r}, device={self.device})"


def _hsh_maps(coef, k):
    """Three contiguous CUDA fp32 HSH maps of k terms per pixel, [3, ...] -> P."""
    _require_cuda(coef, "coef")
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.dim() < 2 or coef.shape[0] != 3 \
            or coef.numel() == 0 or coef.numel() % (3 * k):
        raise ValueError(f"coef must be three contiguous float32 maps of {k} terms per pixel, [3, ...]; got "
                         f"{coef.dtype} {tuple(coef.shape)}")
    return coef.numel() // (3 * k)


def hsh_qparams_workspace(P, basis="hsh16"):
    """Bytes of device scratch ``hsh_qparams_into`` needs for P pixels (``rti_hsh_qparams_workspace``)."""
    return _workspace_bytes(L.lib().rti_hsh_qparams_workspace(_HSH8_TERMS[_hsh8_basis(basis)], int(P)), P)


def hsh_qparams_into(coef, workspace, qparams, *, basis="hsh16", layout="pixel"):
    """Launch ``rti_hsh_qparams`` on preallocated tensors (no allocation, graph-capturable): the k scales and k
    biases ``write_rti`` would give the maps.

    coef: contiguous CUDA fp32 [3, P, k] (layout="pixel") or [3, k, P] ("planar"), any spatial shape in place of
    P; workspace: a contiguous CUDA tensor of at least ``hsh_qparams_workspace(P, basis)`` bytes (it need not be
    initialised); qparams: CUDA fp32 [2k]."""
    b = _hsh8_basis(basis)
    k = _HSH8_TERMS[b]
    P = _hsh_maps(coef, k)
    ws = _workspace_arg(workspace, hsh_qparams_workspace(P, b), coef)
    st = L.lib().rti_hsh_qparams(_vp(coef), b, _layout_id(layout), 0, P, ws,
                                 _qparams_arg(qparams, torch.float32, 2 * k, coef), _stream_of(coef))
    L.check(st, "rti_hsh_qparams")
    return qparams


def hsh_quantise_into(coef, qparams, coef8, *, basis="hsh16", layout="pixel"):
    """Launch ``rti_hsh_quantise`` on preallocated tensors (no allocation, graph-capturable).

    coef: as ``hsh_qparams_into``; qparams: CUDA fp32 [2k] (``hsh_qparams_into``); coef8: uint8 with 3·k·P
    elements ([P, 3, k]).  Returns coef8."""
    b = _hsh8_basis(basis)
    k = _HSH8_TERMS[b]
    P = _hsh_maps(coef, k)
    st = L.lib().rti_hsh_quantise(_vp(coef), b, _layout_id(layout), 0, P,
                                  _qparams_arg(qparams, torch.float32, 2 * k, coef),
                                  _map_out(coef8, "coef8", torch.uint8, 3 * k * P, coef), _stream_of(coef))
    L.check(st, "rti_hsh_quantise")
    return coef8


def quantise_hsh(coef, basis="hsh16", *, layout="pixel"):
    """Quantise three HSH maps to the 3k bytes per pixel of an .rti file on the GPU (``rti_hsh_qparams`` then
    ``rti_hsh_quantise``): the bytes, scales and biases ``write_rti`` computes on the host, without the copy.

    coef: CUDA fp32 [3, H, W, k] / [3, P, k] (layout="pixel") or [3, k, H, W] / [3, k, P] ("planar"), as ``fit``
    returns it for a [3, N, H, W] stack.  Returns a ``QuantisedHSH`` on coef's device; ``write_rti(path, q)``
    writes it, ``relight_hsh8`` renders it."""
    b = _hsh8_basis(basis)
    _require_cuda(coef, "coef")
    k = _HSH8_TERMS[b]
    cl = _layout_id(layout)
    if coef.dim() < 3 or coef.shape[0] != 3:
        raise ValueError(f"coef must be three HSH maps [3, ...]; got {tuple(coef.shape)}")
    spatial = _coef_spatial(coef[0], k, cl)
    m = coef.contiguous()
    P = _hsh_maps(m, k)
    ws = torch.empty(hsh_qparams_workspace(P, b), dtype=torch.uint8, device=m.device)
    qparams = torch.empty(2 * k, dtype=torch.float32, device=m.device)
    coef8 = torch.empty(spatial + (3, k), dtype=torch.uint8, device=m.device)
    hsh_qparams_into(m, ws, qparams, basis=b, layout=cl)
    hsh_quantise_into(m, qparams, coef8, basis=b, layout=cl)
    return QuantisedHSH(coef8, qparams, b)


def dequantise_hsh(q):
    """The three fp32 HSH maps [3, ..., k] of a quantised one, with ``read_rti``'s arithmetic: step = scale/255
    (one fp32 division per term), byte·step, + bias, each rounded to fp32.  Plain torch operations on q's device
    (not a hot path); ``relight(dequantise_hsh(q)[c], ...)`` is channel c of ``relight_hsh8(q, ...)`` bit for
    bit."""
    if not isinstance(q, QuantisedHSH):
        raise ValueError(f"q must be a QuantisedHSH; got {type(q).__name__}")
    k = q.k
    # A tensor divisor: division by a Python scalar may be evaluated as a product with its reciprocal.  The
    # quotient of two fp32 values formed in fp64 and rounded to fp32 is the correctly rounded fp32 quotient
    # (53 >= 2·24 + 2 bits), whatever a backend's fp32 division does.
    step = (q.qparams[:k].double() / torch.full((1,), 255.0, dtype=torch.float64, device=q.device)).float()
    c = q.coef.to(torch.float32) * step  # a separate multiply and add: no FMA
    c = c + q.qparams[k:]
    return c.movedim(-2, 0).contiguous()


def relight_hsh8_into(coef8, qparams, luv_dev, out, *, basis="hsh16"):
    """Launch ``rti_relight_hsh8`` on preallocated tensors (no allocation, graph-capturable).

    coef8: contiguous CUDA uint8 [P, 3, k], any spatial shape in place of P; qparams: CUDA fp32 [2k]; luv_dev:
    CUDA fp64 [E, 2]; out: float32, int32 or uint8 with E·P·3 elements ([E, P, 3])."""
    b = _hsh8_basis(basis)
    k = _HSH8_TERMS[b]
    P = _bytes_map(coef8, 3 * k, f"{3 * k} bytes")
    luv, E = _luv_arg(luv_dev, coef8)
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_hsh8(_vp(coef8), b, P, _qparams_arg(qparams, torch.float32, 2 * k, coef8), luv, E,
                                  _map_out(out, "out", out.dtype, E * P * 3, coef8), odt, _stream_of(coef8))
    L.check(st, "rti_relight_hsh8")
    return out


def relight_hsh8(q, lu, lv, *, out_dtype=torch.float32):
    """Relight a quantised RGB HSH map to RGB images on the GPU in one launch (``rti_relight_hsh8``), reading 3k
    bytes per pixel once for every direction.  Channel c of the images equals
    ``relight(dequantise_hsh(q)[c], lu, lv, basis=q.basis)`` bit for bit.

    q: a ``QuantisedHSH`` on the GPU.  lu, lv: scalars or E directions.  Returns [E, H, W, 3], squeezed to
    [H, W, 3] for scalar directions, in out_dtype: float32, or int32 / uint8 converted as ``relight`` does."""
    _quantised(q, QuantisedHSH)
    return _relight8(q, lu, lv, out_dtype,
                     lambda luv_d, out: relight_hsh8_into(q.coef, q.qparams, luv_d, out, basis=q._basis))


# ---- HSH surface normals: a peak-direction search (rti_hsh_normals.hip) ------

_PEAK_TABLES = {}


def peak_grid_points(grid):
    """E, the number of grid directions of ``grid`` in [4, 16] (``rti_peak_grid_points``)."""
    E = int(L.lib().rti_peak_grid_points(int(grid)))
    if E < 0:
        raise ValueError(f"grid must lie in [4, 16]; got {grid}")
    return E


def peak_table(basis, grid, device):
    """The basis values of the grid directions of (basis, grid) on ``device`` (``rti_peak_table``): an opaque
    uint8 tensor, built once per (basis, grid, device) and kept.  The first call launches one small kernel and
    waits for it, so make it before a graph capture; later calls return the kept tensor."""
    b = _hsh8_basis(basis)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("device must be a CUDA (HIP) device: librti runs only on the GPU, there is no CPU path")
    peak_grid_points(grid)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (b, int(grid), dev.index)
    t = _PEAK_TABLES.get(key)
    if t is None:
        t = torch.empty(int(L.lib().rti_peak_table_bytes(b, int(grid))), dtype=torch.uint8, device=dev)
        L.check(L.lib().rti_peak_table(b, int(grid), _vp(t), _stream_of(t)), "rti_peak_table")
        torch.cuda.current_stream(dev).synchronize()  # any stream may read it from now on
        _PEAK_TABLES[key] = t
    return t


def _luma_weights(weights):
    """None (the library's 0.299, 0.587, 0.114) or three floats -> what the C entries take."""
    if weights is None:
        return None
    w = np.asarray(weights, np.float32).ravel()
    if w.size != 3:
        raise ValueError(f"weights must be three values (R, G, B); got {weights!r}")
    return (ctypes.c_float * 3)(*w.tolist())


def _peak_table_arg(table, b, grid, like):
    _require_cuda(table, "table")
    need = int(L.lib().rti_peak_table_bytes(b, int(grid)))
    if need <= 0:
        raise ValueError(f"grid must lie in [4, 16]; got {grid}")
    if table.dtype != torch.uint8 or table.numel() != need or not table.is_contiguous() or table.device != like.device:
        raise ValueError(f"table must be peak_table(basis, grid, device): {need} uint8 on {like.device}; got "
                         f"{table.dtype} {tuple(table.shape)} on {table.device}")
    return _vp(table)


def hsh_normals_into(coef, table, normals, kind=None, peak=None, *, basis="hsh16", layout="pixel",
                     normal_layout="pixel", grid=10, weights=None):
    """Launch ``rti_hsh_normals`` on preallocated tensors (no allocation, graph-capturable).

    coef: CUDA fp32, one map [P, k] (layout="pixel") or [k, P] ("planar"), or three [3, P, k] / [3, k, P], any
    spatial shape in place of P; contiguous, or three contiguous maps a constant stride apart (a [3, ...] view).
    table: ``peak_table(basis, grid, device)``.  normals: fp32 with 3 values per pixel, [P, 3] or [3, P]; kind:
    uint8 [P] or None; peak: fp32 [P] or None.  P is normals' pixel count."""
    b = _hsh8_basis(basis)
    k = _HSH8_TERMS[b]
    _require_cuda(coef, "coef")
    _require_cuda(normals, "normals")
    P = normals.numel() // 3
    if coef.dtype != torch.float32 or P < 1 or coef.numel() not in (P * k, 3 * P * k):
        raise ValueError(f"coef must be float32 with {k} or 3·{k} terms for each of normals' {P} pixels; got "
                         f"{coef.dtype} {tuple(coef.shape)}")
    C = coef.numel() // (P * k)
    if coef.is_contiguous():
        stride = 0
    elif C == 3 and coef.shape[0] == 3 and coef[0].is_contiguous() and coef.stride(0) >= P * k:
        stride = coef.stride(0)
    else:
        raise ValueError("coef must be contiguous, or three contiguous maps [3, ...] a constant stride apart")
    st = L.lib().rti_hsh_normals(_vp(coef), b, _layout_id(layout), C, stride, P, _luma_weights(weights), int(grid),
                                 _peak_table_arg(table, b, grid, coef),
                                 _map_out(normals, "normals", torch.float32, 3 * P, coef),
                                 _normal_layout_id(normal_layout),
                                 None if kind is None else _map_out(kind, "kind", torch.uint8, P, coef),
                                 None if peak is None else _map_out(peak, "peak", torch.float32, P, coef),
                                 _stream_of(coef))
    L.check(st, "rti_hsh_normals")
    return normals


def hsh8_normals_into(coef8, qparams, table, normals, kind=None, peak=None, *, basis="hsh16", normal_layout="pixel",
                      grid=10, weights=None):
    """Launch ``rti_hsh8_normals`` on preallocated tensors (no allocation, graph-capturable).

    coef8: contiguous CUDA uint8 [P, 3, k], any spatial shape in place of P; qparams: CUDA fp32 [2k]; the rest as
    ``hsh_normals_into``."""
    b = _hsh8_basis(basis)
    k = _HSH8_TERMS[b]
    P = _bytes_map(coef8, 3 * k, f"{3 * k} bytes")
    st = L.lib().rti_hsh8_normals(_vp(coef8), b, P, _qparams_arg(qparams, torch.float32, 2 * k, coef8),
                                  _luma_weights(weights),
                                  int(grid), _peak_table_arg(table, b, grid, coef8),
                                  _map_out(normals, "normals", torch.float32, 3 * P, coef8),
                                  _normal_layout_id(normal_layout),
                                  None if kind is None else _map_out(kind, "kind", torch.uint8, P, coef8),
                                  None if peak is None else _map_out(peak, "peak", torch.float32, P, coef8),
                                  _stream_of(coef8))
    L.check(st, "rti_hsh8_normals")
    return normals


def _normal_outputs(spatial, nl, return_kind, return_peak, device):
    P = int(np.prod(spatial))
    n = _coef_empty(1, P, 3, nl, torch.float32, device)
    kind = torch.empty((1, P), dtype=torch.uint8, device=device) if return_kind else None
    peak = torch.empty((1, P), dtype=torch.float32, device=device) if return_peak else None
    return n, kind, peak


def _normal_results(n, kind, peak, spatial, nl):
    out = (_unflatten(n, spatial, False, nl),) + tuple(_unflatten(t, spatial, False) for t in (kind, peak)
                                                       if t is not None)
    return out if len(out) > 1 else out[0]


def hsh_normals(coef, basis="hsh16", *, layout="pixel", normal_layout="pixel", grid=10, weights=None,
                return_kind=False, return_peak=False):
    """Per-pixel surface normals of HSH maps on the GPU (``rti_hsh_normals``): the light direction at which each
    pixel's fitted function peaks, searched on a grid of directions (i/grid, j/grid) inside the unit disc and
    refined by one parabolic step.  Each grid value is ``relight``'s float32 value there bit for bit.

    coef: CUDA fp32; one map [H, W, k] / [P, k], or an RGB fit [3, H, W, k] / [3, P, k], whose luminance map
    (weights, default 0.299, 0.587, 0.114) is searched; with layout="planar" [k, H, W] / [k, P] and
    [3, k, H, W] / [3, k, P].  A pixel-major 3-D tensor whose first dimension is 3 is read as [3, P, k]: pass a
    single map of three rows as [P, k].  grid in [4, 16].  Returns what ``normals`` returns: fp32 unit normals
    [H, W, 3] (or [3, H, W]); with return_kind also uint8 [H, W] (0 peak inside the unit disc, 1 outside it and
    scaled onto its edge, 2 a flat function: (0, 0, 1), 4 non-finite: NaN); with return_peak also fp32 [H, W], the
    grid maximum (an albedo proxy)."""
    _require_cuda(coef, "coef")
    b = _hsh8_basis(basis)
    k = _HSH8_TERMS[b]
    cl, nl = _layout_id(layout), _normal_layout_id(normal_layout)
    if coef.dtype != torch.float32:
        raise ValueError("coef must be float32")
    if cl == L.RTI_COEF_PIXEL_MAJOR:
        rgb = coef.dim() == 4 or (coef.dim() == 3 and coef.shape[0] == 3)
    else:
        rgb = coef.dim() == 4 or (coef.dim() == 3 and coef.shape[0] == 3 and coef.shape[1] == k)
    if coef.dim() < 2 or coef.dim() > 4 or (rgb and coef.shape[0] != 3):
        raise ValueError(f"coef must be one HSH map or three, [3, ...]; got {tuple(coef.shape)}")
    spatial = _coef_spatial(coef[0] if rgb else coef, k, cl)
    n, kind, peak = _normal_outputs(spatial, nl, return_kind, return_peak, coef.device)
    hsh_normals_into(coef.contiguous(), peak_table(b, grid, coef.device), n, kind, peak, basis=b, layout=cl,
                     normal_layout=nl, grid=grid, weights=weights)
    return _normal_results(n, kind, peak, spatial, nl)


def hsh8_normals(q, *, normal_layout="pixel", grid=10, weights=None, return_kind=False, return_peak=False):
    """Per-pixel surface normals of a quantised RGB HSH map on the GPU (``rti_hsh8_normals``), from the bytes:
    ``hsh_normals(dequantise_hsh(q), q.basis, ...)`` bit for bit, without the fp32 maps.

    q: a ``QuantisedHSH`` on the GPU.  Returns what ``hsh_normals`` returns."""
    _quantised(q, QuantisedHSH)
    nl = _normal_layout_id(normal_layout)
    n, kind, peak = _normal_outputs(q.shape, nl, return_kind, return_peak, q.device)
    hsh8_normals_into(q.coef, q.qparams, peak_table(q._basis, grid, q.device), n, kind, peak, basis=q._basis,
                      normal_layout=nl, grid=grid, weights=weights)
    return _normal_results(n, kind, peak, q.shape, nl)


# ---- 8-bit RGB PTMs: the PTM_FORMAT_RGB payload on the device (rti_rgb8.hip) --

class QuantisedRGB(_Quantised):
    """An 8-bit RGB PTM: the three coefficient blocks of a ``PTM_FORMAT_RGB`` payload and its header values.

    coef: uint8 [3, H, W, 6] or [3, P, 6]: block R, then G, then B, each the bytes a0..a5 per pixel; qparams: fp64
    [12] = scale[0..5], bias[0..5] (integral), shared by the three channels as the file header shares them.  A
    coefficient is ``(byte − bias)·scale`` (``dequantise_rgb``).  Rows top first.  Both tensors on one device (the
    GPU, or the host for ``read_ptm8``); immutable.  ``scale`` / ``bias`` copy qparams to the host: they are the
    one accessor that synchronises."""
    __slots__ = ("_coef", "_qparams")
    TAKES = "two tensors (coef, qparams)"
    MADE_BY = "quantise_rgb, or read_ptm8(path)"

    def __init__(self, coef, qparams):
        self._set({"coef": coef, "qparams": qparams}, "[3, ..., 6]",
                  lambda c: c.dim() >= 3 and c.shape[0] == 3 and c.shape[-1] == 6, 12)

    shape = property(lambda self: tuple(self._coef.shape[1:-1]), doc="the spatial shape: (H, W) or (P,)")
    scale = property(lambda self: self._host()[:6].copy(), doc="host fp64 [6] (synchronises)")
    bias = property(lambda self: self._host()[6:].copy(), doc="host fp64 [6], integral values (synchronises)")

    def with_file_scales(self):
        """The map as a .ptm round trip yields it: the same bytes, the scales rounded to the nine significant
        digits ``write_ptm`` puts in the header.  ``quantise_rgb`` keeps the full fp64 scales the bytes were made
        with; a file does not, so ``dequantise_rgb`` / ``relight_rgb8`` / ``rgb8_normals`` of this map, not of the
        fresh one, equal those of the written file to the bit.  Synchronises."""
        return self._with_qparams(self._file_qparams())

    def __repr__(self):
        return f"QuantisedRGB(shape={self.shape}, device={self.device})"


def _rgb_maps(coef):
    """Three contiguous CUDA fp32 PTM-6 maps, [3, ...] -> P."""
    _require_cuda(coef, "coef")
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.dim() < 2 or coef.shape[0] != 3 \
            or coef.numel() == 0 or coef.numel() % 18:
        raise ValueError(f"coef must be three contiguous float32 maps of 6 terms per pixel, [3, ...]; got "
                         f"{coef.dtype} {tuple(coef.shape)}")
    return coef.numel() // 18


def rgb8_qparams_workspace(P):
    """Bytes of device scratch ``rgb8_qparams_into`` needs for P pixels (``rti_rgb8_qparams_workspace``)."""
    return _workspace_bytes(L.lib().rti_rgb8_qparams_workspace(int(P)), P)


def rgb8_qparams_into(coef, workspace, qparams, *, layout="pixel"):
    """Launch ``rti_rgb8_qparams`` on preallocated tensors (no allocation, graph-capturable): the six scales and
    six biases ``write_ptm(..., format="rgb")`` would give the maps.

    coef: contiguous CUDA fp32 [3, P, 6] (layout="pixel") or [3, 6, P] ("planar"), any spatial shape in place of
    P; workspace: a contiguous CUDA tensor of at least ``rgb8_qparams_workspace(P)`` bytes (it need not be
    initialised); qparams: CUDA fp64 [12]."""
    P = _rgb_maps(coef)
    ws = _workspace_arg(workspace, rgb8_qparams_workspace(P), coef)
    st = L.lib().rti_rgb8_qparams(_vp(coef), _layout_id(layout), 0, P, ws,
                                  _qparams_arg(qparams, torch.float64, 12, coef), _stream_of(coef))
    L.check(st, "rti_rgb8_qparams")
    return qparams


def rgb8_quantise_into(coef, qparams, coef8, *, layout="pixel"):
    """Launch ``rti_rgb8_quantise`` on preallocated tensors (no allocation, graph-capturable).

    coef: as ``rgb8_qparams_into``; qparams: CUDA fp64 [12] (``rgb8_qparams_into``); coef8: uint8 with 18·P
    elements ([3, P, 6]).  Returns coef8."""
    P = _rgb_maps(coef)
    st = L.lib().rti_rgb8_quantise(_vp(coef), _layout_id(layout), 0, P, _qparams_arg(qparams, torch.float64, 12, coef),
                                   _map_out(coef8, "coef8", torch.uint8, 18 * P, coef), _stream_of(coef))
    L.check(st, "rti_rgb8_quantise")
    return coef8


def quantise_rgb(coef, *, layout="pixel"):
    """Quantise three PTM-6 maps to the 18 bytes per pixel of a ``PTM_FORMAT_RGB`` file on the GPU
    (``rti_rgb8_qparams`` then ``rti_rgb8_quantise``): the bytes, scales and biases ``write_ptm(...,
    format="rgb")`` computes on the host, without the copy.

    coef: CUDA fp32 [3, H, W, 6] / [3, P, 6] (layout="pixel") or [3, 6, H, W] / [3, 6, P] ("planar"), as ``fit``
    returns it for a [3, N, H, W] stack.  Returns a ``QuantisedRGB`` on coef's device; ``write_ptm(path, q)``
    writes it, ``relight_rgb8`` renders it, ``rgb8_normals`` reads its surface normals."""
    _require_cuda(coef, "coef")
    cl = _layout_id(layout)
    if coef.dim() < 3 or coef.shape[0] != 3:
        raise ValueError(f"coef must be three PTM-6 maps [3, ...]; got {tuple(coef.shape)}")
    spatial = _coef_spatial(coef[0], 6, cl)
    m = coef.contiguous()
    P = _rgb_maps(m)
    ws = torch.empty(rgb8_qparams_workspace(P), dtype=torch.uint8, device=m.device)
    qparams = torch.empty(12, dtype=torch.float64, device=m.device)
    coef8 = torch.empty((3,) + spatial + (6,), dtype=torch.uint8, device=m.device)
    rgb8_qparams_into(m, ws, qparams, layout=cl)
    rgb8_quantise_into(m, qparams, coef8, layout=cl)
    return QuantisedRGB(coef8, qparams)


def dequantise_rgb(q):
    """The three fp32 PTM-6 maps [3, ..., 6] of a quantised one, with ``read_ptm``'s arithmetic: (byte − bias)·scale
    in fp64, rounded once to fp32.  Plain torch operations on q's device, the host included (not a hot path);
    ``relight(dequantise_rgb(q)[c], ...)`` is channel c of ``relight_rgb8(q, ...)`` bit for bit."""
    if not isinstance(q, QuantisedRGB):
        raise ValueError(f"q must be a QuantisedRGB; got {type(q).__name__}")
    qp = q.qparams
    return ((q.coef.double() - qp[6:]) * qp[:6]).float()


def relight_rgb8_into(coef8, qparams, luv_dev, out):
    """Launch ``rti_relight_rgb8`` on preallocated tensors (no allocation, graph-capturable).

    coef8: contiguous CUDA uint8 [3, P, 6], any spatial shape in place of P; qparams: CUDA fp64 [12]; luv_dev:
    CUDA fp64 [E, 2]; out: float32, int32 or uint8 with E·P·3 elements ([E, P, 3])."""
    P = _bytes_map(coef8, 18, "three blocks of 6 bytes")
    luv, E = _luv_arg(luv_dev, coef8)
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_rgb8(_vp(coef8), P, _qparams_arg(qparams, torch.float64, 12, coef8), luv, E,
                                  _map_out(out, "out", out.dtype, E * P * 3, coef8), odt, _stream_of(coef8))
    L.check(st, "rti_relight_rgb8")
    return out


def relight_rgb8(q, lu, lv, *, out_dtype=torch.float32):
    """Relight a quantised RGB PTM to RGB images on the GPU in one launch (``rti_relight_rgb8``), reading 18 bytes
    per pixel once for every direction.  Channel c of the images equals ``relight(dequantise_rgb(q)[c], lu, lv)``
    bit for bit.

    q: a ``QuantisedRGB`` on the GPU.  lu, lv: scalars or E directions.  Returns [E, H, W, 3], squeezed to
    [H, W, 3] for scalar directions, in out_dtype: float32, or int32 / uint8 converted as ``relight`` does."""
    _quantised(q, QuantisedRGB)
    return _relight8(q, lu, lv, out_dtype, lambda luv_d, out: relight_rgb8_into(q.coef, q.qparams, luv_d, out))


def rgb8_normals_into(coef8, qparams, normals, kind=None, peak=None, *, normal_layout="pixel", weights=None):
    """Launch ``rti_rgb8_normals`` on preallocated tensors (no allocation, graph-capturable).

    coef8 / qparams as ``relight_rgb8_into``; normals: fp32 with 3 values per pixel, [P, 3] (normal_layout="pixel")
    or [3, P]; kind: uint8 [P] or None; peak: fp32 [P] or None; weights: None (0.299, 0.587, 0.114) or three
    values (R, G, B)."""
    P = _bytes_map(coef8, 18, "three blocks of 6 bytes")
    st = L.lib().rti_rgb8_normals(_vp(coef8), P, _qparams_arg(qparams, torch.float64, 12, coef8),
                                  _luma_weights(weights),
                                  _map_out(normals, "normals", torch.float32, 3 * P, coef8),
                                  _normal_layout_id(normal_layout),
                                  None if kind is None else _map_out(kind, "kind", torch.uint8, P, coef8),
                                  None if peak is None else _map_out(peak, "peak", torch.float32, P, coef8),
                                  _stream_of(coef8))
    L.check(st, "rti_rgb8_normals")
    return normals


def rgb8_normals(q, *, normal_layout="pixel", weights=None, return_kind=False, return_peak=False):
    """Per-pixel surface normals of a quantised RGB PTM on the GPU (``rti_rgb8_normals``), from the bytes: with
    r, g, b = ``dequantise_rgb(q)`` and l = (w0·r + w1·g) + w2·b formed in float32, ``normals(l, ...)`` bit for
    bit, without the fp32 maps.

    q: a ``QuantisedRGB`` on the GPU; weights: None (0.299, 0.587, 0.114) or three values.  Returns what
    ``normals`` returns."""
    _quantised(q, QuantisedRGB)
    nl = _normal_layout_id(normal_layout)
    n, kind, peak = _normal_outputs(q.shape, nl, return_kind, return_peak, q.device)
    rgb8_normals_into(q.coef, q.qparams, n, kind, peak, normal_layout=nl, weights=weights)
    return _normal_results(n, kind, peak, q.shape, nl)


# ---- diffuse gain and specular rendering of the colour forms ----------------

def _enhance_scalars(mode, gain, kd, ks, exp, lu, lv):
    """What the three ``rti_relight_*_enhanced`` entries take between their map and their output."""
    return (_enhance_mode_id(mode), float(gain), float(kd), float(ks), int(exp), float(lu), float(lv))


def relight_lrgb_enhanced_into(lrgb, lu, lv, mode, out, *, gain=1.0, kd=1.0, ks=0.0, exp=1, layout="pixel"):
    """Launch ``rti_relight_lrgb_enhanced`` on preallocated tensors (no allocation, graph-capturable).

    lrgb as ``relight_lrgb_into``; mode, gain, kd, ks, exp as ``relight_enhanced_into``; out: float32, int32 or
    uint8 with P·3 elements ([P, 3], RGB interleaved)."""
    P = _lrgb_map(lrgb)
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_lrgb_enhanced(_vp(lrgb), _layout_id(layout), P,
                                           *_enhance_scalars(mode, gain, kd, ks, exp, lu, lv),
                                           _map_out(out, "out", out.dtype, P * 3, lrgb), odt, _stream_of(lrgb))
    L.check(st, "rti_relight_lrgb_enhanced")
    return out


def relight_lrgb8_enhanced_into(coef8, rgb8, qparams, lu, lv, mode, out, *, gain=1.0, kd=1.0, ks=0.0, exp=1):
    """Launch ``rti_relight_lrgb8_enhanced`` on preallocated tensors (no allocation, graph-capturable).

    coef8 / rgb8 / qparams as ``relight_lrgb8_into``; the rest as ``relight_lrgb_enhanced_into``."""
    P = _bytes_map(coef8, 6, "6 bytes")
    _require_cuda(rgb8, "rgb8")
    if rgb8.dtype != torch.uint8 or not rgb8.is_contiguous() or rgb8.numel() != 3 * P or rgb8.device != coef8.device:
        raise ValueError(f"rgb8 must be a contiguous uint8 tensor of {3 * P} elements on {coef8.device}; got "
                         f"{rgb8.dtype} {tuple(rgb8.shape)} on {rgb8.device}")
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_lrgb8_enhanced(_vp(coef8), _vp(rgb8), P, _qparams_arg(qparams, torch.float64, 13, coef8),
                                            *_enhance_scalars(mode, gain, kd, ks, exp, lu, lv),
                                            _map_out(out, "out", out.dtype, P * 3, coef8), odt, _stream_of(coef8))
    L.check(st, "rti_relight_lrgb8_enhanced")
    return out


def relight_rgb8_enhanced_into(coef8, qparams, lu, lv, mode, out, *, gain=1.0, kd=1.0, ks=0.0, exp=1, weights=None):
    """Launch ``rti_relight_rgb8_enhanced`` on preallocated tensors (no allocation, graph-capturable).

    coef8 / qparams as ``relight_rgb8_into``; weights as ``rgb8_normals_into``; the rest as
    ``relight_lrgb_enhanced_into``."""
    P = _bytes_map(coef8, 18, "three blocks of 6 bytes")
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_rgb8_enhanced(_vp(coef8), P, _qparams_arg(qparams, torch.float64, 12, coef8),
                                           _luma_weights(weights),
                                           *_enhance_scalars(mode, gain, kd, ks, exp, lu, lv),
                                           _map_out(out, "out", out.dtype, P * 3, coef8), odt, _stream_of(coef8))
    L.check(st, "rti_relight_rgb8_enhanced")
    return out


def _enhanced_rgb_out(spatial, out_dtype, device):
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    return torch.empty(tuple(spatial) + (3,), dtype=out_dtype, device=device)


def relight_lrgb_enhanced(lrgb, lu, lv, mode, *, gain=1.0, kd=1.0, ks=0.0, exp=1, layout="pixel",
                          out_dtype=torch.float32):
    """One enhanced RGB rendering of an LRGB map at the light direction (lu, lv) on the GPU in one launch
    (``rti_relight_lrgb_enhanced``): ``relight_enhanced`` of the luminance under the pixel's chroma.

    mode="diffuse_gain": chroma_c · L'(lu, lv), the luminance's curvature scaled by ``gain`` about its peak.
    mode="specular": kd·chroma_c·L(lu, lv) + ks·max(0, n·H)^exp, a white highlight at the luminance's normal.
    lrgb as ``relight_lrgb``.  Returns [H, W, 3] in out_dtype: float32, or int32 / uint8 converted as ``relight``
    does.  With chroma 1 every channel is ``relight_enhanced`` of the luminance planes bit for bit."""
    _require_cuda(lrgb, "lrgb")
    cl = _layout_id(layout)
    out = _enhanced_rgb_out(_coef_spatial(lrgb, 9, cl), out_dtype, lrgb.device)
    return relight_lrgb_enhanced_into(lrgb.contiguous(), lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp, layout=cl)


def relight_lrgb8_enhanced(q, lu, lv, mode, *, gain=1.0, kd=1.0, ks=0.0, exp=1, out_dtype=torch.float32):
    """``relight_lrgb_enhanced`` of a quantised LRGB map, from its 9 bytes per pixel in one launch
    (``rti_relight_lrgb8_enhanced``): ``relight_lrgb_enhanced(dequantise_lrgb(q), ...)`` bit for bit.

    q: a ``QuantisedLRGB`` on the GPU.  Returns [H, W, 3] in out_dtype."""
    _quantised(q, QuantisedLRGB)
    out = _enhanced_rgb_out(q.shape, out_dtype, q.device)
    return relight_lrgb8_enhanced_into(q.coef, q.rgb, q.qparams, lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp)


def relight_rgb8_enhanced(q, lu, lv, mode, *, gain=1.0, kd=1.0, ks=0.0, exp=1, out_dtype=torch.float32, weights=None):
    """One enhanced RGB rendering of a quantised RGB PTM at (lu, lv), from its 18 bytes per pixel in one launch
    (``rti_relight_rgb8_enhanced``).  The peak and the normal are those of the luminance ``rgb8_normals`` reads
    (weights: None = 0.299, 0.587, 0.114, or three values); every channel keeps its own coefficients.

    mode="diffuse_gain": each channel's curvature scaled by ``gain`` about the luminance's peak, so the colour at
    the peak stays and the channels do not part.  mode="specular": kd·L_c(lu, lv) + ks·max(0, n·H)^exp.
    q: a ``QuantisedRGB`` on the GPU.  Returns [H, W, 3] in out_dtype.  With a unit weight on channel c, that
    channel is ``relight_enhanced(dequantise_rgb(q)[c], ...)`` bit for bit."""
    _quantised(q, QuantisedRGB)
    out = _enhanced_rgb_out(q.shape, out_dtype, q.device)
    return relight_rgb8_enhanced_into(q.coef, q.qparams, lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp,
                                      weights=weights)


# ---- three fp32 RGB maps rendered in one pass (rti_rgb.hip) -------------------

def _ptm_only(basis, what):
    """The basis of an entry that reads PTM-6 maps alone; anything else is not built."""
    if basis_id(basis) != L.RTI_BASIS_PTM6:
        raise NotImplementedError(f"{what} reads PTM-6 maps only; got basis {basis!r}")


class _RGBMaps:
    """What ``_relight8`` asks of its map, for three fp32 maps: the device and the spatial shape."""
    __slots__ = ("device", "shape")

    def __init__(self, device, shape):
        self.device, self.shape = device, tuple(shape)


def _rgb_spatial(coef, k, cl, name="coef"):
    """Three maps [3, ..., k] (pixel-major) or [3, k, ...] (planar) -> their spatial shape."""
    _require_cuda(coef, name)
    if coef.dtype != torch.float32:
        raise ValueError(f"{name} must be float32; got {coef.dtype}")
    if coef.dim() < 3 or coef.shape[0] != 3:
        raise ValueError(f"{name} must be three maps of {k} terms per pixel, [3, ...]; got {tuple(coef.shape)}")
    return _coef_spatial(coef[0], k, cl)


def relight_rgb_into(coef, luv_dev, out, *, basis="ptm", layout="pixel"):
    """Launch ``rti_relight_rgb`` on preallocated tensors (no allocation, graph-capturable).

    coef: contiguous CUDA fp32 [3, P, k] (layout="pixel") or [3, k, P] ("planar"), any spatial shape in place of P,
    as ``fit`` returns it for a [3, N, H, W] stack; basis "ptm", "hsh9" or "hsh16"; luv_dev: CUDA fp64 [E, 2]; out:
    float32, int32 or uint8 with E·P·3 elements ([E, P, 3], RGB interleaved)."""
    b = basis_id(basis)
    P = _hsh_maps(coef, basis_terms(b))
    luv, E = _luv_arg(luv_dev, coef)
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_rgb(_vp(coef), b, _layout_id(layout), 0, P, luv, E,
                                 _map_out(out, "out", out.dtype, E * P * 3, coef), odt, _stream_of(coef))
    L.check(st, "rti_relight_rgb")
    return out


def relight_rgb_enhanced_into(coef, lu, lv, mode, out, *, gain=1.0, kd=1.0, ks=0.0, exp=1, layout="pixel",
                              weights=None, basis="ptm"):
    """Launch ``rti_relight_rgb_enhanced`` on preallocated tensors (no allocation, graph-capturable).

    coef: contiguous CUDA fp32 PTM-6 maps [3, P, 6] / [3, 6, P] as ``relight_rgb_into``; weights as
    ``rgb8_normals_into``; the rest as ``relight_lrgb_enhanced_into``: out float32, int32 or uint8 with P·3
    elements ([P, 3])."""
    _ptm_only(basis, "rti_relight_rgb_enhanced")
    P = _rgb_maps(coef)
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_rgb_enhanced(_vp(coef), _layout_id(layout), 0, P, _luma_weights(weights),
                                          *_enhance_scalars(mode, gain, kd, ks, exp, lu, lv),
                                          _map_out(out, "out", out.dtype, P * 3, coef), odt, _stream_of(coef))
    L.check(st, "rti_relight_rgb_enhanced")
    return out


def rgb_normals_into(coef, normals, kind=None, peak=None, *, layout="pixel", normal_layout="pixel", weights=None,
                     basis="ptm"):
    """Launch ``rti_rgb_normals`` on preallocated tensors (no allocation, graph-capturable).

    coef as ``relight_rgb_enhanced_into``; normals: fp32 with 3 values per pixel, [P, 3] (normal_layout="pixel")
    or [3, P]; kind: uint8 [P] or None; peak: fp32 [P] or None; weights: None (0.299, 0.587, 0.114) or three
    values (R, G, B)."""
    _ptm_only(basis, "rti_rgb_normals")
    P = _rgb_maps(coef)
    st = L.lib().rti_rgb_normals(_vp(coef), _layout_id(layout), 0, P, _luma_weights(weights),
                                 _map_out(normals, "normals", torch.float32, 3 * P, coef),
                                 _normal_layout_id(normal_layout),
                                 None if kind is None else _map_out(kind, "kind", torch.uint8, P, coef),
                                 None if peak is None else _map_out(peak, "peak", torch.float32, P, coef),
                                 _stream_of(coef))
    L.check(st, "rti_rgb_normals")
    return normals


def relight_rgb(coef, lu, lv, basis="ptm", *, layout="pixel", out_dtype=torch.float32):
    """Relight the three fp32 maps of a colour fit to RGB images on the GPU in one launch (``rti_relight_rgb``),
    reading the maps once for every direction.  Channel c of the images equals ``relight(coef[c], lu, lv, basis)``
    bit for bit.

    coef: CUDA fp32 [3, H, W, k] / [3, P, k] (layout="pixel") or [3, k, H, W] / [3, k, P] ("planar"), as ``fit``
    returns it for a [3, N, H, W] stack; basis "ptm", "hsh9" or "hsh16".  lu, lv: scalars or E directions.
    Returns [E, H, W, 3], squeezed to [H, W, 3] for scalar directions, in out_dtype: float32, or int32 / uint8
    converted as ``relight`` does."""
    b = basis_id(basis)
    cl = _layout_id(layout)
    spatial = _rgb_spatial(coef, basis_terms(b), cl)
    m = coef.contiguous()
    return _relight8(_RGBMaps(m.device, spatial), lu, lv, out_dtype,
                     lambda luv_d, out: relight_rgb_into(m, luv_d, out, basis=b, layout=cl))


def relight_rgb_enhanced(coef, lu, lv, mode, *, gain=1.0, kd=1.0, ks=0.0, exp=1, layout="pixel",
                         out_dtype=torch.float32, weights=None, basis="ptm"):
    """One enhanced RGB rendering of the three fp32 PTM-6 maps of a colour fit at (lu, lv) on the GPU in one launch
    (``rti_relight_rgb_enhanced``), without quantising them or compressing them to LRGB.  The peak and the normal
    are those of the luminance ``rgb_normals`` reads (weights: None = 0.299, 0.587, 0.114, or three values); every
    channel keeps its own coefficients.

    mode="diffuse_gain": each channel's curvature scaled by ``gain`` about the luminance's peak.  mode="specular":
    kd·L_c(lu, lv) + ks·max(0, n·H)^exp.  coef as ``relight_rgb`` with 6 terms; any other basis raises
    NotImplementedError.  Returns [H, W, 3] in out_dtype.  With a unit weight on channel c, that channel is
    ``relight_enhanced(coef[c], ...)`` bit for bit."""
    _ptm_only(basis, "rti_relight_rgb_enhanced")
    cl = _layout_id(layout)
    spatial = _rgb_spatial(coef, 6, cl)
    out = _enhanced_rgb_out(spatial, out_dtype, coef.device)
    return relight_rgb_enhanced_into(coef.contiguous(), lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp,
                                     layout=cl, weights=weights)


def rgb_normals(coef, *, layout="pixel", normal_layout="pixel", weights=None, return_kind=False, return_peak=False,
                basis="ptm"):
    """Per-pixel surface normals of the three fp32 PTM-6 maps of a colour fit on the GPU (``rti_rgb_normals``): with
    l = (w0·r + w1·g) + w2·b formed in float32, ``normals(l, ...)`` bit for bit, without building l.

    coef as ``relight_rgb`` with 6 terms (any other basis raises NotImplementedError); weights: None (0.299,
    0.587, 0.114) or three values.  Returns what ``normals`` returns."""
    _ptm_only(basis, "rti_rgb_normals")
    cl, nl = _layout_id(layout), _normal_layout_id(normal_layout)
    spatial = _rgb_spatial(coef, 6, cl)
    n, kind, peak = _normal_outputs(spatial, nl, return_kind, return_peak, coef.device)
    rgb_normals_into(coef.contiguous(), n, kind, peak, layout=cl, normal_layout=nl, weights=weights)
    return _normal_results(n, kind, peak, spatial, nl)


# ---- specular enhancement of HSH maps under a normal map (rti_hsh_specular.hip) -

def _specular_basis(basis, what="relight_hsh_specular"):
    """A basis name or id -> the id of HSH-9 or HSH-16; PTM-6 has entries of its own."""
    b = basis_id(basis)
    if b not in _HSH8_NAMES:
        raise NotImplementedError(f"{what} reads HSH-9 and HSH-16 maps only; got basis {basis!r} "
                                  "(PTM-6 maps: relight_rgb_enhanced, relight_enhanced)")
    return b


def _specular_dirs(lu, lv):
    """Scalars or up to RTI_SPECULAR_MAX_DIRS directions -> (host fp64 [E, 2], whether they were scalars)."""
    scalar = np.ndim(lu) == 0 and np.ndim(lv) == 0
    u, v = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64).ravel() for x in (lu, lv))
    if u.size != v.size or u.size == 0:
        raise ValueError(f"lu and lv must hold the same number of directions, at least one; got {u.size} and {v.size}")
    if u.size > L.RTI_SPECULAR_MAX_DIRS:
        raise ValueError(f"at most {L.RTI_SPECULAR_MAX_DIRS} directions per launch; got {u.size} (call once per "
                         f"{L.RTI_SPECULAR_MAX_DIRS})")
    return np.ascontiguousarray(np.stack([u, v], -1)), scalar


def _specular_normals(n, like):
    """A contiguous CUDA fp32 normal map on like's device -> P."""
    if not torch.is_tensor(n) or n.dtype != torch.float32 or not n.is_contiguous() or n.numel() == 0 or n.numel() % 3:
        raise ValueError("n must be a contiguous float32 normal map of 3 values per pixel; got "
                         f"{getattr(n, 'dtype', type(n))} {tuple(getattr(n, 'shape', ()))}")
    _require_cuda(n, "n")
    if n.device != like.device:
        raise ValueError(f"n is on {n.device}, the coefficients on {like.device}")
    return n.numel() // 3


def relight_hsh_specular_into(coef, n, lu, lv, out, *, basis="hsh16", kd=1.0, ks=0.0, exp=1, layout="pixel",
                              normal_layout="pixel"):
    """Launch ``rti_relight_hsh_specular`` on preallocated tensors (no allocation, no copy, graph-capturable: the
    directions travel as kernel arguments and become part of a capture).

    coef: contiguous CUDA fp32, one map [P, k] (layout="pixel") or [k, P] ("planar"), or three [3, P, k] /
    [3, k, P], any spatial shape in place of P; n: contiguous fp32 normals [P, 3] or [3, P]; lu, lv: scalars or up
    to 16 directions on the host; out: float32, int32 or uint8 with E·P elements ([E, P]) for one map, E·P·3
    ([E, P, 3], RGB interleaved) for three.  P is n's pixel count."""
    b = _specular_basis(basis)
    k = _HSH8_TERMS[b]
    _require_cuda(coef, "coef")
    P = _specular_normals(n, coef)
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() not in (P * k, 3 * P * k):
        raise ValueError(f"coef must be contiguous float32 with {k} or 3·{k} terms for each of n's {P} pixels; got "
                         f"{coef.dtype} {tuple(coef.shape)}")
    C = coef.numel() // (P * k)
    luv, _ = _specular_dirs(lu, lv)
    E = luv.shape[0]
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_hsh_specular(_vp(coef), b, _layout_id(layout), C, 0, P, _vp(n),
                                          _normal_layout_id(normal_layout), float(kd), float(ks), int(exp),
                                          _dptr(luv), E, _map_out(out, "out", out.dtype, E * P * C, coef), odt,
                                          _stream_of(coef))
    L.check(st, "rti_relight_hsh_specular")
    return out


def relight_hsh8_specular_into(coef8, qparams, n, lu, lv, out, *, basis="hsh16", kd=1.0, ks=0.0, exp=1,
                               normal_layout="pixel"):
    """Launch ``rti_relight_hsh8_specular`` on preallocated tensors (no allocation, no copy, graph-capturable).

    coef8: contiguous CUDA uint8 [P, 3, k], any spatial shape in place of P; qparams: CUDA fp32 [2k]; n, lu, lv
    as ``relight_hsh_specular_into``; out: float32, int32 or uint8 with E·P·3 elements ([E, P, 3])."""
    b = _specular_basis(basis)
    k = _HSH8_TERMS[b]
    P = _bytes_map(coef8, 3 * k, f"{3 * k} bytes")
    if _specular_normals(n, coef8) != P:
        raise ValueError(f"n has {n.numel() // 3} pixels, coef8 {P}")
    luv, _ = _specular_dirs(lu, lv)
    E = luv.shape[0]
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_hsh8_specular(_vp(coef8), b, P, _qparams_arg(qparams, torch.float32, 2 * k, coef8),
                                           _vp(n), _normal_layout_id(normal_layout), float(kd), float(ks), int(exp),
                                           _dptr(luv), E, _map_out(out, "out", out.dtype, E * P * 3, coef8), odt,
                                           _stream_of(coef8))
    L.check(st, "rti_relight_hsh8_specular")
    return out


def _specular_maps(coef, k, cl):
    """One CUDA fp32 HSH map or three of k terms in layout cl -> (spatial shape, whether there are three)."""
    _require_cuda(coef, "coef")
    if coef.dtype != torch.float32:
        raise ValueError(f"coef must be float32; got {coef.dtype}")
    if cl == L.RTI_COEF_PIXEL_MAJOR:
        rgb = coef.dim() == 4 or (coef.dim() == 3 and coef.shape[0] == 3)
    else:
        rgb = coef.dim() == 4 or (coef.dim() == 3 and coef.shape[0] == 3 and coef.shape[1] == k)
    if coef.dim() < 2 or coef.dim() > 4:
        raise ValueError(f"coef must be one HSH map or three, [3, ...]; got {tuple(coef.shape)}")
    return (_rgb_spatial(coef, k, cl) if rgb else _coef_spatial(coef, k, cl)), rgb


def _specular_frame(n, nl, spatial, E, rgb, out_dtype, device):
    """What the two specular renderers do before their launch: n's pixels against the map's, and the output ->
    (n contiguous, out [E, *spatial(, 3)])."""
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    if not torch.is_tensor(n) or n.dtype != torch.float32:
        raise ValueError(f"n must be a float32 normal map; got {getattr(n, 'dtype', type(n))}")
    _require_cuda(n, "n")
    if _coef_spatial(n, 3, nl) != tuple(spatial):
        raise ValueError(f"n's pixels {_coef_spatial(n, 3, nl)} do not match the map's {tuple(spatial)}")
    out = torch.empty((E,) + tuple(spatial) + ((3,) if rgb else ()), dtype=out_dtype, device=device)
    return n.contiguous(), out


def relight_hsh_specular(coef, n, lu, lv, basis="hsh16", *, kd=1.0, ks=0.0, exp=1, layout="pixel",
                         normal_layout="pixel", out_dtype=torch.float32):
    """Specular enhancement of fp32 HSH maps under a normal map on the GPU in one launch
    (``rti_relight_hsh_specular``): per channel kd·L(lu, lv) + ks·max(0, n·H)^exp with L ``relight``'s float32
    value and H the half vector between the light and the viewer; the highlight is white.  The maps and the normal
    are read once for every direction.

    coef: CUDA fp32; one map [H, W, k] / [P, k] or an RGB fit [3, H, W, k] / [3, P, k]; with layout="planar"
    [k, H, W] / [k, P] and [3, k, H, W] / [3, k, P] (read as ``hsh_normals`` reads them).  n: fp32 normals of the
    same pixels, [H, W, 3] (normal_layout="pixel") or [3, H, W]: ``hsh_normals(coef)``, optionally through
    ``normals_unsharp``.  lu, lv: scalars or up to 16 directions (more raise ValueError).  Returns [E, H, W] or
    [E, H, W, 3], without the leading E for scalar directions, in out_dtype: float32, or int32 / uint8 converted as
    ``relight`` does.  NaN normals give NaN pixels.  PTM maps raise NotImplementedError: ``relight_rgb_enhanced``
    renders those."""
    b = _specular_basis(basis)
    cl, nl = _layout_id(layout), _normal_layout_id(normal_layout)
    luv, scalar = _specular_dirs(lu, lv)
    spatial, rgb = _specular_maps(coef, _HSH8_TERMS[b], cl)
    nc, out = _specular_frame(n, nl, spatial, luv.shape[0], rgb, out_dtype, coef.device)
    relight_hsh_specular_into(coef.contiguous(), nc, lu, lv, out, basis=b, kd=kd, ks=ks, exp=exp, layout=cl,
                              normal_layout=nl)
    return out[0] if scalar else out


def relight_hsh8_specular(q, n, lu, lv, *, kd=1.0, ks=0.0, exp=1, normal_layout="pixel", out_dtype=torch.float32):
    """Specular enhancement of a quantised RGB HSH map under a normal map on the GPU in one launch, from the bytes
    (``rti_relight_hsh8_specular``): ``relight_hsh_specular(dequantise_hsh(q), n, ...)`` bit for bit, without the
    fp32 maps.  The loaded-file workflow: ``q = read_rti(path, quantised=True)[1].to("cuda")``,
    ``n = normals_unsharp(hsh8_normals(q), ...)`` once, then one launch per frame.

    q: a ``QuantisedHSH`` on the GPU; the rest as ``relight_hsh_specular``.  Returns [E, H, W, 3], without the
    leading E for scalar directions."""
    nl = _normal_layout_id(normal_layout)
    luv, scalar = _specular_dirs(lu, lv)
    _quantised(q, QuantisedHSH)
    nc, out = _specular_frame(n, nl, q.shape, luv.shape[0], True, out_dtype, q.device)
    relight_hsh8_specular_into(q.coef, q.qparams, nc, lu, lv, out, basis=q._basis, kd=kd, ks=ks, exp=exp,
                               normal_layout=nl)
    return out[0] if scalar else out


# ---- diffuse gain for HSH maps under a normal map (rti_hsh_gain.hip) ------------

def _gain_value(gain):
    g = float(gain)
    if not np.isfinite(g):
        raise ValueError(f"gain must be finite; got {gain!r}")
    return g


def relight_hsh_gain_into(coef, n, lu, lv, out, *, basis="hsh16", gain=1.0, layout="pixel", normal_layout="pixel"):
    """Launch ``rti_relight_hsh_gain`` on preallocated tensors (no allocation, no copy, graph-capturable: the
    directions and the gain travel as kernel arguments and become part of a capture).

    coef, n, lu, lv and out exactly as ``relight_hsh_specular_into`` takes them; gain: any finite value."""
    b = _specular_basis(basis, "relight_hsh_gain")
    k = _HSH8_TERMS[b]
    _require_cuda(coef, "coef")
    P = _specular_normals(n, coef)
    if coef.dtype != torch.float32 or not coef.is_contiguous() or coef.numel() not in (P * k, 3 * P * k):
        raise ValueError(f"coef must be contiguous float32 with {k} or 3·{k} terms for each of n's {P} pixels; got "
                         f"{coef.dtype} {tuple(coef.shape)}")
    C = coef.numel() // (P * k)
    luv, _ = _specular_dirs(lu, lv)
    E = luv.shape[0]
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_hsh_gain(_vp(coef), b, _layout_id(layout), C, 0, P, _vp(n),
                                      _normal_layout_id(normal_layout), _gain_value(gain), _dptr(luv), E,
                                      _map_out(out, "out", out.dtype, E * P * C, coef), odt, _stream_of(coef))
    L.check(st, "rti_relight_hsh_gain")
    return out


def relight_hsh8_gain_into(coef8, qparams, n, lu, lv, out, *, basis="hsh16", gain=1.0, normal_layout="pixel"):
    """Launch ``rti_relight_hsh8_gain`` on preallocated tensors (no allocation, no copy, graph-capturable).

    coef8, qparams, n, lu, lv and out exactly as ``relight_hsh8_specular_into`` takes them; gain: any finite value."""
    b = _specular_basis(basis, "relight_hsh8_gain")
    k = _HSH8_TERMS[b]
    P = _bytes_map(coef8, 3 * k, f"{3 * k} bytes")
    if _specular_normals(n, coef8) != P:
        raise ValueError(f"n has {n.numel() // 3} pixels, coef8 {P}")
    luv, _ = _specular_dirs(lu, lv)
    E = luv.shape[0]
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_hsh8_gain(_vp(coef8), b, P, _qparams_arg(qparams, torch.float32, 2 * k, coef8), _vp(n),
                                       _normal_layout_id(normal_layout), _gain_value(gain), _dptr(luv), E,
                                       _map_out(out, "out", out.dtype, E * P * 3, coef8), odt, _stream_of(coef8))
    L.check(st, "rti_relight_hsh8_gain")
    return out


def relight_hsh_gain(coef, n, lu, lv, basis="hsh16", *, gain=1.0, layout="pixel", normal_layout="pixel",
                     out_dtype=torch.float32):
    """Diffuse gain for fp32 HSH maps under a normal map on the GPU in one launch (``rti_relight_hsh_gain``): per
    channel L(lu, lv) + (gain − 1)·(L(lu, lv) − L(n_x, n_y)) with L ``relight``'s float32 value.  The value at the
    pixel's own normal and its direction stay, the fall-off away from it is multiplied by gain; gain = 1 is the plain
    relight.  The maps and the normal are read once for every direction.

    coef, n, lu, lv, layout, normal_layout and out_dtype as ``relight_hsh_specular`` takes them (n:
    ``hsh_normals(coef)``, optionally through ``normals_unsharp``; up to 16 directions, more raise ValueError);
    gain: any finite value.  Returns [E, H, W] or [E, H, W, 3], without the leading E for scalar directions.  NaN
    normals give NaN pixels.  PTM maps raise NotImplementedError: ``relight_rgb_enhanced`` renders those."""
    b = _specular_basis(basis, "relight_hsh_gain")
    cl, nl = _layout_id(layout), _normal_layout_id(normal_layout)
    luv, scalar = _specular_dirs(lu, lv)
    spatial, rgb = _specular_maps(coef, _HSH8_TERMS[b], cl)
    nc, out = _specular_frame(n, nl, spatial, luv.shape[0], rgb, out_dtype, coef.device)
    relight_hsh_gain_into(coef.contiguous(), nc, lu, lv, out, basis=b, gain=gain, layout=cl, normal_layout=nl)
    return out[0] if scalar else out


def relight_hsh8_gain(q, n, lu, lv, *, gain=1.0, normal_layout="pixel", out_dtype=torch.float32):
    """Diffuse gain for a quantised RGB HSH map under a normal map on the GPU in one launch, from the bytes
    (``rti_relight_hsh8_gain``): ``relight_hsh_gain(dequantise_hsh(q), n, ...)`` bit for bit, without the fp32
    maps.  The loaded-file workflow of ``relight_hsh8_specular``: the normals once per object, one launch per frame.

    q: a ``QuantisedHSH`` on the GPU; the rest as ``relight_hsh_gain``.  Returns [E, H, W, 3], without the leading
    E for scalar directions."""
    nl = _normal_layout_id(normal_layout)
    luv, scalar = _specular_dirs(lu, lv)
    _quantised(q, QuantisedHSH)
    nc, out = _specular_frame(n, nl, q.shape, luv.shape[0], True, out_dtype, q.device)
    relight_hsh8_gain_into(q.coef, q.qparams, nc, lu, lv, out, basis=q._basis, gain=gain, normal_layout=nl)
    return out[0] if scalar else out


# ---- surface height from a normal map: masked Poisson integration (rti_height.hip) ------------

HEIGHT_PRECONDS = {"multigrid": L.RTI_HEIGHT_MULTIGRID, "jacobi": L.RTI_HEIGHT_JACOBI}


def _height_precond_id(precond):
    if isinstance(precond, int) and not isinstance(precond, bool):
        return precond
    try:
        return HEIGHT_PRECONDS[precond]
    except (KeyError, TypeError):
        raise ValueError(f"unknown preconditioner {precond!r} (expected one of {sorted(HEIGHT_PRECONDS)})") from None


def _height_dims(n, nl):
    """A dense fp32 normal map [H, W, 3] (pixel-major) or [3, H, W] (planar) on the GPU -> (H, W)."""
    if torch.is_tensor(n) and n.dtype == torch.float32 and (n.dim() != 3 or n.shape[2 if nl == 0 else 0] != 3):
        raise ValueError(f"n must be a normal map [H, W, 3] (pixel) or [3, H, W] (planar); got {tuple(n.shape)}")
    _, H, W = _map_dims(n, nl)  # the dtype and the shape are judged before the device
    return H, W


def height_levels(H, W):
    """Grids of the aggregation hierarchy of an H×W map (``rti_height_levels``, host)."""
    n = L.lib().rti_height_levels(int(H), int(W))
    if n < 1:
        raise ValueError(f"H and W must be positive with H·W below 2^31; got {H}×{W}")
    return n


def height_workspace(H, W, precond="multigrid", device="cuda"):
    """The device scratch of ``height_from_normals_into`` for an H×W map: an uninitialised uint8 tensor of
    ``rti_height_workspace_bytes`` bytes on ``device`` (the one allocation of a solve; reusable across solves)."""
    nbytes = L.lib().rti_height_workspace_bytes(int(H), int(W), _height_precond_id(precond))
    if nbytes <= 0:
        raise ValueError(f"H and W must be positive with H·W below 2^31 and precond known; got {H}×{W}, {precond!r}")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def height_from_normals_into(n, workspace, height, *, valid=None, z0=None, nz_min=0.1, flip_y=False, rtol=1e-6,
                             max_iters=2000, check_every=8, precond="multigrid", layout="pixel", stats=None):
    """Launch ``rti_height_from_normals`` on preallocated tensors (no allocation; it synchronises the stream every
    ``check_every`` iterations, so it is not graph-capturable).

    n: contiguous CUDA fp32 [H, W, 3] (layout="pixel") or [3, H, W] ("planar"); workspace: ``height_workspace``;
    height: fp32 [H, W]; valid: uint8 [H, W] or None; z0: fp32 [H, W] or None (it may be ``height``); stats: a
    float64 NumPy array of 6 or None.  Returns height."""
    nl = _normal_layout_id(layout)
    H, W = _height_dims(n, nl)
    pc = _height_precond_id(precond)
    need = L.lib().rti_height_workspace_bytes(H, W, pc)
    if need <= 0:
        raise ValueError(f"H·W must be below 2^31 and precond known; got {H}×{W}, {precond!r}")
    ws = _workspace_arg(workspace, need, n)
    if stats is not None and (not isinstance(stats, np.ndarray) or stats.dtype != np.float64 or stats.size != 6
                              or not stats.flags.c_contiguous):
        raise ValueError("stats must be a contiguous float64 NumPy array of 6 values")
    st = L.lib().rti_height_from_normals(
        _vp(n), nl, H, W, float(nz_min), int(bool(flip_y)),
        None if z0 is None else _map_out(z0, "z0", torch.float32, H * W, n), float(rtol), int(max_iters),
        int(check_every), pc, ws, _map_out(height, "height", torch.float32, H * W, n),
        None if valid is None else _map_out(valid, "valid", torch.uint8, H * W, n),
        None if stats is None else _dptr(stats), _stream_of(n))
    L.check(st, "rti_height_from_normals")
    return height


def height_from_normals(n, nz_min=0.1, flip_y=False, rtol=1e-6, max_iters=2000, precond="multigrid", z0=None,
                        layout="pixel", return_valid=False, stats=None, check_every=8):
    """The height (depth) map of a normal map on the GPU (``rti_height_from_normals``): the least-squares surface
    with ∂z/∂x = −n_x/n_z, ∂z/∂y = −n_y/n_z (x the column, y the row; ``flip_y`` negates the y-gradient) over the
    valid pixels -- finite normals with n_z >= nz_min and a valid 4-neighbour -- in pixel units, zero mean over
    the valid pixels, NaN elsewhere.  Holes and irregular outlines are natural boundaries; separate components
    float independently.  Preconditioned conjugate gradients in fp64 until ‖r‖ <= rtol·‖b‖ or max_iters;
    precond "multigrid" (aggregation V-cycle) or "jacobi".  Not converging is not an error: see stats.

    n: CUDA fp32 [H, W, 3] (layout="pixel") or [3, H, W] ("planar"), e.g. of ``photometric_stereo``, ``normals``,
    ``hsh_normals``; z0: None or a start [H, W] fp32; stats: None or a float64 NumPy array of 6 that receives
    iterations run, the iteration the criterion was met (−1: not), the final recursive and the true relative
    residual, the count of valid pixels and ‖b‖.  Returns [H, W] fp32, with return_valid (height, valid uint8
    [H, W]).  Allocates the workspace (``height_workspace``).  Not built: confidence weights, robust (L1)
    integration, perspective cameras, a per-component gauge, ``rti.parallel``."""
    nl = _normal_layout_id(layout)
    if not torch.is_tensor(n):
        raise ValueError("n must be a CUDA (HIP) tensor")
    src = n.contiguous()
    H, W = _height_dims(src, nl)
    if z0 is not None:
        _require_cuda(z0, "z0")
        if tuple(z0.shape) != (H, W) or z0.dtype != torch.float32:
            raise ValueError(f"z0 must be a float32 [{H}, {W}] tensor; got {z0.dtype} {tuple(z0.shape)}")
        z0 = z0.contiguous()
    ws = height_workspace(H, W, precond, src.device)
    height = torch.empty((H, W), dtype=torch.float32, device=src.device)
    valid = torch.empty((H, W), dtype=torch.uint8, device=src.device) if return_valid else None
    height_from_normals_into(src, ws, height, valid=valid, z0=z0, nz_min=nz_min, flip_y=flip_y, rtol=rtol,
                             max_iters=max_iters, check_every=check_every, precond=precond, layout=nl, stats=stats)
    return (height, valid) if return_valid else height


# ---- multi-light detail enhancement (rti_multilight.hip) ----------------------

LIGHT_TILES = (8, 16, 32)


def light_candidates(lu, lv, radius=0.3, rings=2, per_ring=8):
    """The candidate lights of the multi-light search around the main light (lu, lv), on the host: fp64 [E, 2] with
    E = 1 + rings·per_ring.  The main light comes first, then ring r = 1..rings at radius·r/rings with the angles
    2πj/per_ring, j = 0..per_ring − 1.  A point outside the unit disc is scaled onto it."""
    lu, lv, radius = float(lu), float(lv), float(radius)
    rings, per_ring = int(rings), int(per_ring)
    if not (np.isfinite(lu) and np.isfinite(lv) and np.isfinite(radius)) or radius < 0.0:
        raise ValueError(f"lu, lv must be finite and radius finite and not negative; got {lu}, {lv}, {radius}")
    if rings < 0 or per_ring < 1:
        raise ValueError(f"rings must be >= 0 and per_ring >= 1; got {rings}, {per_ring}")
    E = 1 + rings * per_ring
    if E > L.RTI_LIGHT_MAX_CANDIDATES:
        raise ValueError(f"at most {L.RTI_LIGHT_MAX_CANDIDATES} candidates; 1 + {rings}·{per_ring} = {E}")
    pts = [(lu, lv)]
    for r in range(1, rings + 1):
        rad = radius * r / rings
        for j in range(per_ring):
            a = 2.0 * np.pi * j / per_ring
            pts.append((lu + rad * np.cos(a), lv + rad * np.sin(a)))
    out = np.array(pts, np.float64)
    for i in range(E):
        n = np.hypot(out[i, 0], out[i, 1])
        if n > 1.0:
            out[i] /= n
        while out[i, 0] * out[i, 0] + out[i, 1] * out[i, 1] > 1.0:  # the division's rounding
            out[i] *= 1.0 - 2.0 ** -52
    return out


def _tile_edge(tile):
    if isinstance(tile, bool) or tile not in LIGHT_TILES:
        raise ValueError(f"tile must be one of {LIGHT_TILES}; got {tile!r}")
    return int(tile)


def _tile_grid(H, W, T):
    return (H + T - 1) // T, (W + T - 1) // T


def _candidates_arg(luv):
    """Candidate lights as light_candidates returns them -> host fp64 [E, 2], 1 <= E <= RTI_LIGHT_MAX_CANDIDATES."""
    a = np.ascontiguousarray(np.asarray(luv.detach().cpu() if torch.is_tensor(luv) else luv, np.float64))
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"luv must be [E, 2] with at least one candidate; got {a.shape}")
    if a.shape[0] > L.RTI_LIGHT_MAX_CANDIDATES:
        raise ValueError(f"at most {L.RTI_LIGHT_MAX_CANDIDATES} candidates per call; got {a.shape[0]}")
    if not np.isfinite(a).all():
        raise ValueError("luv must be finite")
    return a


def _image_maps(coef, b, cl):
    """One CUDA fp32 map of an H x W image or three, contiguous or three contiguous maps a constant stride apart ->
    (C, H, W, channel stride in elements or 0)."""
    k = basis_terms(b)
    if k < 0:
        raise ValueError(f"unknown basis {b!r}")
    _require_cuda(coef, "coef")
    if coef.dtype != torch.float32:
        raise ValueError(f"coef must be float32; got {coef.dtype}")
    if coef.dim() == 4 and coef.shape[0] == 3:
        one, C = coef[0], 3
    elif coef.dim() == 3:
        one, C = coef, 1
    else:
        raise ValueError("coef must be one map of an image, [H, W, k] (or [k, H, W] planar), or three, [3, ...]; got "
                         f"{tuple(coef.shape)}")
    H, W = _coef_spatial(one, k, cl)
    if H < 1 or W < 1:
        raise ValueError(f"the image must have at least one pixel; got {H}x{W}")
    if coef.is_contiguous():
        stride = 0
    elif C == 3 and one.is_contiguous() and coef.stride(0) >= H * W * k:
        stride = coef.stride(0)
    else:
        raise ValueError("coef must be contiguous, or three contiguous maps [3, ...] a constant stride apart")
    return C, int(H), int(W), int(stride)


def light_scores_into(coef, luv, scores, count=None, *, basis="ptm", tile=16, layout="pixel", weights=None):
    """Launch ``rti_light_scores`` on preallocated tensors (no allocation, graph-capturable: the candidates travel as
    kernel arguments and become part of a capture).

    coef: CUDA fp32 [H, W, k] or [3, H, W, k] (layout="pixel"), [k, H, W] or [3, k, H, W] ("planar"); contiguous, or
    three contiguous maps a constant stride apart.  luv: host [E, 2], E <= 64.  scores: float64 with Ty·Tx·E·2
    elements ([Ty, Tx, E, 2]: sharpness, brightness); count: int32 [Ty, Tx] or None."""
    b, cl, T = basis_id(basis), _layout_id(layout), _tile_edge(tile)
    cand = _candidates_arg(luv)
    E = cand.shape[0]
    C, H, W, stride = _image_maps(coef, b, cl)
    Ty, Tx = _tile_grid(H, W, T)
    st = L.lib().rti_light_scores(_vp(coef), b, cl, C, stride, H, W, T, _luma_weights(weights), _dptr(cand), E,
                                  _map_out(scores, "scores", torch.float64, Ty * Tx * E * 2, coef),
                                  None if count is None else _map_out(count, "count", torch.int32, Ty * Tx, coef),
                                  _stream_of(coef))
    L.check(st, "rti_light_scores")
    return scores


def light_scores(coef, luv, basis="ptm", *, tile=16, layout="pixel", weights=None):
    """The multi-light search on the GPU in one launch (``rti_light_scores``): for every tile x tile block of the
    image and every candidate light, the local sharpness (the mean squared difference of neighbouring pixels inside
    the tile) and the brightness (the mean) of ``relight``'s float32 value of the luminance map, with no candidate
    frame written to memory.  Pixels with a non-finite coefficient are left out.

    coef: as ``light_scores_into``; luv: ``light_candidates(...)`` or any host [E, 2], E <= 64; tile 8, 16 or 32.
    Returns (scores float64 [Ty, Tx, E, 2], count int32 [Ty, Tx], the usable pixels of each tile)."""
    b, cl, T = basis_id(basis), _layout_id(layout), _tile_edge(tile)
    E = _candidates_arg(luv).shape[0]
    _, H, W, _ = _image_maps(coef, b, cl)
    Ty, Tx = _tile_grid(H, W, T)
    scores = torch.empty((Ty, Tx, E, 2), dtype=torch.float64, device=coef.device)
    count = torch.empty((Ty, Tx), dtype=torch.int32, device=coef.device)
    light_scores_into(coef, luv, scores, count, basis=b, tile=T, layout=cl, weights=weights)
    return scores, count


def light_field_workspace(Ty, Tx, device="cuda"):
    """The device scratch of ``light_field_into`` for a Ty x Tx tile grid (``rti_light_field_workspace_bytes``)."""
    nbytes = L.lib().rti_light_field_workspace_bytes(int(Ty), int(Tx))
    if nbytes <= 0:
        raise ValueError(f"Ty and Tx must be positive; got {Ty}x{Tx}")
    return torch.empty(int(nbytes) // 8, dtype=torch.float64, device=device)


def _field_scalars(lu, lv, ws, wb, smooth):
    lu, lv, ws, wb = float(lu), float(lv), float(ws), float(wb)
    if not (np.isfinite(lu) and np.isfinite(lv)):
        raise ValueError(f"the main light must be finite; got ({lu}, {lv})")
    if not (np.isfinite(ws) and np.isfinite(wb)) or ws < 0.0 or wb < 0.0:
        raise ValueError(f"ws and wb must be finite and not negative; got {ws}, {wb}")
    if isinstance(smooth, bool) or int(smooth) != smooth or not 0 <= smooth <= 8:
        raise ValueError(f"smooth must be an integer in [0, 8]; got {smooth!r}")
    return lu, lv, ws, wb, int(smooth)


def light_field_into(scores, count, luv, workspace, field, choice=None, *, lu, lv, ws=1.0, wb=0.5, smooth=2):
    """Launch ``rti_light_field`` on preallocated tensors (no allocation, graph-capturable; 1 + smooth launches).

    scores: CUDA float64 [Ty, Tx, E, 2] and count: int32 [Ty, Tx] of ``light_scores``; luv: the same candidates;
    workspace: ``light_field_workspace(Ty, Tx)``; field: float32 [Ty, Tx, 2]; choice: int32 [Ty, Tx] or None;
    (lu, lv): the main light, taken by tiles without a usable pixel."""
    _require_cuda(scores, "scores")
    cand = _candidates_arg(luv)
    E = cand.shape[0]
    if scores.dtype != torch.float64 or scores.dim() != 4 or tuple(scores.shape[2:]) != (E, 2) \
            or not scores.is_contiguous() or scores.numel() == 0:
        raise ValueError(f"scores must be a contiguous float64 [Ty, Tx, {E}, 2] tensor; got {scores.dtype} "
                         f"{tuple(scores.shape)}")
    Ty, Tx = int(scores.shape[0]), int(scores.shape[1])
    lu, lv, ws, wb, smooth = _field_scalars(lu, lv, ws, wb, smooth)
    need = int(L.lib().rti_light_field_workspace_bytes(Ty, Tx))
    wsp = _workspace_arg(workspace, need, scores)
    st = L.lib().rti_light_field(_vp(scores), _map_out(count, "count", torch.int32, Ty * Tx, scores), Ty, Tx,
                                 _dptr(cand), E, ws, wb, lu, lv, smooth, wsp,
                                 workspace.numel() * workspace.element_size(),
                                 _map_out(field, "field", torch.float32, Ty * Tx * 2, scores),
                                 None if choice is None else _map_out(choice, "choice", torch.int32, Ty * Tx, scores),
                                 _stream_of(scores))
    L.check(st, "rti_light_field")
    return field


def light_field(scores, count, luv, lu, lv, *, ws=1.0, wb=0.5, smooth=2, return_choice=False):
    """The light field of the multi-light mode on the GPU (``rti_light_field``): per tile the candidate with the
    largest ws·sharpness + wb·brightness (each normalised by its largest value over the tile's candidates), a tile
    without a usable pixel taking the main light (lu, lv), then ``smooth`` passes of the 3x3 binomial over the tile
    grid.  Returns float32 [Ty, Tx, 2]; with return_choice also int32 [Ty, Tx] (−1: the main light)."""
    _field_scalars(lu, lv, ws, wb, smooth)
    _candidates_arg(luv)
    _require_cuda(scores, "scores")
    if scores.dim() != 4 or scores.numel() == 0:
        raise ValueError(f"scores must be [Ty, Tx, E, 2]; got {tuple(scores.shape)}")
    Ty, Tx = int(scores.shape[0]), int(scores.shape[1])
    field = torch.empty((Ty, Tx, 2), dtype=torch.float32, device=scores.device)
    choice = torch.empty((Ty, Tx), dtype=torch.int32, device=scores.device) if return_choice else None
    light_field_into(scores.contiguous(), count.contiguous() if torch.is_tensor(count) else count, luv,
                     light_field_workspace(Ty, Tx, scores.device), field, choice, lu=lu, lv=lv, ws=ws, wb=wb,
                     smooth=smooth)
    return (field, choice) if return_choice else field


def relight_field_into(coef, light, out, *, basis="ptm", tile=None, layout="pixel"):
    """Launch ``rti_relight_field`` on preallocated tensors (no allocation, graph-capturable).

    coef: as ``light_scores_into``.  light: contiguous CUDA float32; with tile = 8, 16 or 32 a tile field
    [Ty, Tx, 2], sampled bilinearly between the tile centres; with tile=None a light per pixel [H, W, 2].  out:
    float32, int32 or uint8 with H·W elements for one map, H·W·3 ([H, W, 3]) for three."""
    b, cl = basis_id(basis), _layout_id(layout)
    T = 0 if tile is None else _tile_edge(tile)
    C, H, W, stride = _image_maps(coef, b, cl)
    n = H * W * 2 if tile is None else 2 * int(np.prod(_tile_grid(H, W, T)))
    odt = _out8_dtype(out)
    st = L.lib().rti_relight_field(_vp(coef), b, cl, C, stride, H, W, _map_out(light, "light", torch.float32, n, coef),
                                   L.RTI_LIGHT_PIXELS if tile is None else L.RTI_LIGHT_TILES, T,
                                   _map_out(out, "out", out.dtype, H * W * C, coef), odt, _stream_of(coef))
    L.check(st, "rti_relight_field")
    return out


def relight_field(coef, light, basis="ptm", *, tile=None, layout="pixel", out_dtype=torch.float32):
    """Relight under a light direction per pixel on the GPU in one launch (``rti_relight_field``): per channel
    ``relight``'s float32 value at that pixel's own light, the basis evaluated per pixel on the device.

    coef: CUDA fp32 [H, W, k] or [3, H, W, k] (planar: [k, H, W], [3, k, H, W]).  light: CUDA float32 [H, W, 2], a
    direction per pixel (e.g. a near-light correction), or with tile = 8, 16 or 32 the tile field [Ty, Tx, 2] of
    ``light_field``.  Returns [H, W] or [H, W, 3] in out_dtype: float32, or int32 / uint8 converted as ``relight``
    does.  A pixel whose light is not finite is NaN (INT32_MIN, 0)."""
    b, cl = basis_id(basis), _layout_id(layout)
    T = 0 if tile is None else _tile_edge(tile)
    if out_dtype not in _ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    C, H, W, _ = _image_maps(coef, b, cl)
    _require_cuda(light, "light")
    want = (H, W, 2) if tile is None else _tile_grid(H, W, T) + (2,)
    if light.dtype != torch.float32 or tuple(light.shape) != want:
        raise ValueError(f"light must be float32 {list(want)}; got {light.dtype} {tuple(light.shape)}")
    out = torch.empty((H, W) + ((3,) if C == 3 else ()), dtype=out_dtype, device=coef.device)
    return relight_field_into(coef, light.contiguous(), out, basis=b, tile=tile, layout=cl)


def relight_multilight(coef, lu, lv, basis="ptm", *, tile=16, radius=0.3, rings=2, per_ring=8, ws=1.0, wb=0.5,
                       smooth=2, layout="pixel", out_dtype=torch.float32, return_field=False):
    """Multi-light detail enhancement on the GPU (Palma et al. 2010; RTIViewer's multi-light mode): every tile of the
    image is lit by the candidate around (lu, lv) that shows its relief best, the choices are smoothed into a light
    field and the image is relit with a light per pixel.  ``light_candidates``, ``light_scores``, ``light_field`` and
    ``relight_field(..., tile=tile)`` composed: 3 + smooth launches, no candidate frame in memory.

    coef: CUDA fp32 [H, W, k] or [3, H, W, k] (planar: [k, H, W], [3, k, H, W]); the search runs on the luminance of
    three maps, the relight on each channel.  Returns [H, W] or [H, W, 3] in out_dtype; with return_field also the
    float32 field [Ty, Tx, 2] it used."""
    luv = light_candidates(lu, lv, radius, rings, per_ring)
    scores, count = light_scores(coef, luv, basis, tile=tile, layout=layout)
    field = light_field(scores, count, luv, lu, lv, ws=ws, wb=wb, smooth=smooth)
    out = relight_field(coef, field, basis, tile=tile, layout=layout, out_dtype=out_dtype)
    return (out, field) if return_field else out


# ---- light operators (RBF, fused PTM/HSH fit + evaluation) ----------------------------------

def _query(qu, qv):
    qu = np.ascontiguousarray(np.asarray(qu, np.float64).ravel())
    qv = np.ascontiguousarray(np.asarray(qv, np.float64).ravel())
    if qu.size != qv.size or qu.size == 0:
        raise ValueError("query directions: qu and qv must be non-empty and of equal length")
    return qu, qv


def rbf_operator(lu, lv, qu, qv):
    """Host fp64 linear-RBF operator opT[N, E] (SciPy Rbf 'linear', analysis.py:249-260).

    Raises numpy.linalg.LinAlgError for a singular system, as SciPy does."""
    lu, lv = _dirs(lu, lv)
    qu, qv = _query(qu, qv)
    out = np.empty((lu.size, qu.size), np.float64)
    L.check(L.lib().rti_rbf_operator(_fptr(lu), _fptr(lv), lu.size, _dptr(qu), _dptr(qv), qu.size, _dptr(out)),
            "rti_rbf_operator")
    return out


def basis_operator(lu, lv, qu, qv, basis="ptm", rcond=None):
    """Host fp64 operator opT[N, E] = (B(q) · pinv)ᵀ: fit and evaluation fused (analysis.py:293-315)."""
    lu, lv = _dirs(lu, lv)
    qu, qv = _query(qu, qv)
    out = np.empty((lu.size, qu.size), np.float64)
    rc = _rcond(rcond)
    L.check(L.lib().rti_basis_operator(basis_id(basis), _fptr(lu), _fptr(lv), lu.size, _dptr(qu), _dptr(qv),
                                       qu.size, rc, _dptr(out)), "rti_basis_operator")
    return out


def split_operator_f16(opT, device):
    """Host split of an fp64 operator opT[N, E] for rti_apply_operator_f16: fp16 halves
    hi, lo [E, Kp] on ``device`` (M·s = hi + lo, Kp = N rounded up to 16) and 1/s."""
    op = np.ascontiguousarray(opT.detach().cpu().numpy() if torch.is_tensor(opT) else opT, np.float64)
    if op.ndim != 2:
        raise ValueError("operator must be [N, E]")
    N, E = op.shape
    Kp = max(16, (N + 15) // 16 * 16)
    hi = np.empty((E, Kp), np.uint16)
    lo = np.empty((E, Kp), np.uint16)
    inv = ctypes.c_float()
    L.check(L.lib().rti_operator_split_f16(_dptr(op), N, E, E, Kp, hi.ctypes.data_as(ctypes.c_void_p),
                                           lo.ctypes.data_as(ctypes.c_void_p), ctypes.byref(inv)),
            "rti_operator_split_f16")
    return (torch.from_numpy(hi).to(device), torch.from_numpy(lo).to(device), Kp, float(inv.value))


def apply_operator(opT, I, out_dtype=torch.float32, precision="auto"):
    """out[.., E, H, W] = Σ_n opT[n, e] · I[.., n, H, W] on the GPU (MFMA).

    opT: [N, E] operator (host array or tensor).  I: CUDA [N, H, W], [N, P] or
    [C, N, H, W], fp32/u8/int32, light-major.
    precision: "split16" (AUTO for N <= 256) = the fp64 operator split into two fp16
    halves on v_mfma_f32_32x32x16_f16 (22-bit operator, fp32 accumulation);
    "fp32" = the operator rounded to fp32 on v_mfma_f32_16x16x4_f32."""
    _require_cuda(I, "I")
    odt = _OUT_DTYPES.get(out_dtype)
    if odt is None:
        raise ValueError("out_dtype must be float32, float64, int32 or uint8")
    if precision not in ("auto", "split16", "fp32"):
        raise ValueError("precision must be 'auto', 'split16' or 'fp32'")
    N, E = tuple(opT.shape)
    C, n_img, P, spatial = _stack_shape(I)
    if n_img != N:
        raise ValueError(f"operator has {N} lights, I has {n_img}")
    Ic = I.contiguous()
    out = torch.empty((C, E) + spatial, dtype=out_dtype, device=I.device)
    if precision == "split16" or (precision == "auto" and N <= 256):
        hi, lo, Kp, inv = split_operator_f16(opT, I.device)
        st = L.lib().rti_apply_operator_f16(_vp(hi), _vp(lo), Kp, inv, E, N, _vp(Ic), _IN_DTYPES[Ic.dtype], P, C, P,
                                            N * P, _vp(out), odt, P, E * P, _stream_of(I))
        L.check(st, "rti_apply_operator_f16")
    else:
        op = torch.as_tensor(opT, device=I.device).to(torch.float32).contiguous()
        st = L.lib().rti_apply_operator(_vp(op), E, N, E, _vp(Ic), _IN_DTYPES[Ic.dtype], P, C, P, N * P, _vp(out),
                                        odt, P, E * P, _stream_of(I))
        L.check(st, "rti_apply_operator")
    return out if I.dim() == 4 else out[0]


def interpolate_rbf(I, lu, lv, qu, qv, out_dtype=torch.float32):
    """Linear-RBF interpolation of every pixel at (qu, qv) for a SHARED light set -> [.., E, H, W]."""
    return apply_operator(rbf_operator(lu, lv, qu, qv), I, out_dtype=out_dtype)


def interpolate_rbf_perpixel(I, lu, lv, qu, qv, out_dtype=torch.float64, out_layout="pixel", stats=None):
    """Per-pixel linear RBF (the reference's default with per-pixel light lists) on the GPU.

    I, lu, lv: pixel-major [.., N] (compute_intensities' layout), on any device.
    Returns [.., E] (out_layout="pixel") or [E, ..] ("eval").  Raises
    numpy.linalg.LinAlgError if any pixel's system is singular, as SciPy does.
    stats: a dict receives "fallback_px", the pixels (81 <= N <= 256) re-solved by the fp64 fallback."""
    _require_cuda(I, "I")
    dev = I.device
    odt = _OUT_DTYPES.get(out_dtype)
    if odt is None:
        raise ValueError("out_dtype must be float32, float64, int32 or uint8")
    lu_d = torch.as_tensor(lu, device=dev).to(torch.float32).contiguous()
    lv_d = torch.as_tensor(lv, device=dev).to(torch.float32).contiguous()
    if lu_d.shape != I.shape or lv_d.shape != I.shape:
        raise ValueError("per-pixel lu, lv and I must share the pixel-major shape [.., N]")
    N = I.shape[-1]
    spatial = tuple(I.shape[:-1])
    P = int(np.prod(spatial)) if spatial else 1
    qu, qv = _query(qu, qv)
    luv = torch.as_tensor(np.ascontiguousarray(np.stack([qu, qv], -1)), device=dev)
    E = qu.size
    ol = L.RTI_OUT_PIXEL_MAJOR if out_layout == "pixel" else L.RTI_OUT_EVAL_MAJOR
    out = torch.empty(spatial + (E,) if ol == L.RTI_OUT_PIXEL_MAJOR else (E,) + spatial, dtype=out_dtype, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    Ic = I.contiguous()
    fb = torch.zeros(1, dtype=torch.int32, device=dev)
    st = L.lib().rti_rbf_perpixel_ex(_vp(lu_d), _vp(lv_d), _vp(Ic), _IN_DTYPES[Ic.dtype], N, P, _vp(luv), E,
                                     _vp(out), odt, ol, _vp(status), _vp(fb), _stream_of(I))
    L.check(st, "rti_rbf_perpixel")
    if stats is not None:
        stats["fallback_px"] = int(fb.item())
    if int(status.item()) == L.RTI_ERR_SINGULAR:
        raise np.linalg.LinAlgError("Matrix is singular.")
    return out
