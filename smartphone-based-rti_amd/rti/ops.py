"""PyTorch custom ops over the C ABI: ``torch.ops.rti.fit_shared`` / ``fit_shared_residual`` /
``fit_robust`` / ``photometric_stereo`` / ``photometric_stereo_near`` / ``fit_accumulate`` / ``fit_accum_solve`` / ``fit_residual`` / ``relight`` /
``ptm_normals`` / ``relight_enhanced`` / ``map_unsharp`` / ``shade_normals`` / ``lrgb_from_rgb`` / ``relight_lrgb`` /
``lrgb_quantise`` / ``relight_lrgb8`` / ``hsh_quantise`` / ``relight_hsh8`` / ``hsh_normals`` / ``hsh8_normals`` /
``rgb8_quantise`` / ``relight_rgb8`` / ``rgb8_normals`` / ``relight_lrgb_enhanced`` / ``relight_lrgb8_enhanced`` /
``relight_rgb8_enhanced`` / ``relight_rgb`` / ``relight_rgb_enhanced`` / ``rgb_normals`` / ``relight_hsh_specular`` /
``relight_hsh8_specular`` / ``relight_hsh_gain`` / ``relight_hsh8_gain`` / ``height_from_normals`` / ``light_scores`` /
``light_field`` / ``relight_field``.

They let the fit and relight kernels sit inside torch programs (and
``torch.library`` fake-tensor tracing) while the compute stays in librti's
HIP kernels on the current stream.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib as L
from . import api


def _same_device(**tensors):
    """Every tensor on one device: a pointer from another GPU must not reach a kernel launched
    on this GPU's stream."""
    devs = {name: t.device for name, t in tensors.items()}
    if len(set(devs.values())) > 1:
        raise ValueError("tensors on different devices: " + ", ".join(f"{n}={d}" for n, d in devs.items()))


def _in_dtype(I):
    if I.dtype not in api._IN_DTYPES:
        raise ValueError(f"I dtype {I.dtype} unsupported (float32, uint8 or int32)")


def _batched(I):
    """[N, P] or [C, N, P] -> the contiguous [C, N, P] the launchers take."""
    return I.contiguous() if I.dim() == 3 else I.contiguous().unsqueeze(0)


def _lead(t):
    """The caller's channel axis: (C,) of a 3-D stack or state, () of a 2-D one."""
    return (t.shape[0],) if t.dim() == 3 else ()


def _outputs(like, lead, P, k, planar, maps=()):
    """An op's outputs on ``like``'s device: fp32 coefficients lead + [P, k] (or [k, P] if planar), then one
    per-pixel map lead + [P] for each dtype of ``maps``.  The real ops pass lead = (C,) and un-batch after the
    launch, their fakes the caller's own lead, so both shapes come from this expression."""
    coef = like.new_empty(lead + ((k, P) if planar else (P, k)), dtype=torch.float32)
    return (coef,) + tuple(like.new_empty(lead + (P,), dtype=dt) for dt in maps)


def _unbatched(t, *outs):
    """The outputs as the caller's 2-D or 3-D ``t`` asked for them: without the leading C for 2-D."""
    return outs if t.dim() == 3 else tuple(o[0] for o in outs)


@torch.library.custom_op("rti::fit_shared", mutates_args=())
def fit_shared(pinv: torch.Tensor, I: torch.Tensor, planar: bool = False, kernel: int = 0) -> torch.Tensor:
    """coef = pinv (fp32 [k, N]) applied to I (CUDA [N, P] or [C, N, P]) -> [C?, P, k] or [C?, k, P]."""
    api._require_cuda(I, "I")
    api._require_cuda(pinv, "pinv")
    if pinv.dtype != torch.float32:
        raise ValueError("pinv must be float32")
    _same_device(pinv=pinv, I=I)
    _in_dtype(I)
    k = pinv.shape[0]
    I3 = _batched(I)
    C, N, P = I3.shape
    if pinv.shape[1] != N:
        raise ValueError(f"pinv is [{k}, {pinv.shape[1]}] but I has {N} lights")
    coef, = _outputs(I, (C,), P, k, planar)
    api.fit_shared_into(pinv.contiguous(), I3, coef, k=k, layout="planar" if planar else "pixel", kernel=kernel)
    return _unbatched(I, coef)[0]


@fit_shared.register_fake
def _(pinv, I, planar=False, kernel=0):
    return _outputs(I, _lead(I), I.shape[-1], pinv.shape[0], planar)[0]


@torch.library.custom_op("rti::fit_shared_residual", mutates_args=())
def fit_shared_residual(U: torch.Tensor, W: torch.Tensor, I: torch.Tensor, planar: bool = False,
                        chunks: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The north_star fit with per-pixel residuals in ONE pass over the stack
    (``rti_fit_shared_residual_svd``; the reference's solve, analysis.py:293-298, as y = Uᵀ I,
    coef = W y with the thin SVD A = U Σ Vᵀ, W = V Σ⁻¹).

    U fp64 [N, k], W fp64 [k, k] (``rti.lsq_factors``), I CUDA [N, P] or [C, N, P] (fp32/u8/int32) ->
    ``(coef, res, partial)``: coef fp32 [C?, P, k] (or [C?, k, P] if planar), res fp32 [C?, P] =
    sqrt(Σ_n (I_n − A_n·coef)² / N), partial fp64 [C?, rti_fit_shared_residual_blocks(P)] = each
    workgroup's residual energy from wavefront reductions (sum / (P·N) = mean squared residual)."""
    api._require_cuda(I, "I")
    api._require_cuda(U, "U")
    api._require_cuda(W, "W")
    if U.dtype != torch.float64 or W.dtype != torch.float64:
        raise ValueError("U and W must be float64 (rti.lsq_factors)")
    _same_device(U=U, W=W, I=I)
    _in_dtype(I)
    I3 = _batched(I)
    C, N, P = I3.shape
    k = U.shape[1]
    if U.shape[0] != N or W.shape != (k, k):
        raise ValueError(f"U must be [{N}, k] and W [k, k]; got {tuple(U.shape)} and {tuple(W.shape)}")
    if N < k:
        raise ValueError(f"shapes not aligned: {N} lights < {k} basis terms (analysis.py:298)")
    coef, res = _outputs(I, (C,), P, k, planar, (torch.float32,))
    partial = torch.zeros((C, int(L.lib().rti_fit_shared_residual_blocks(P))), dtype=torch.float64, device=I.device)
    api.fit_shared_residual_into(U.contiguous(), W.contiguous(), I3, coef, res, partial, k=k,
                                 layout="planar" if planar else "pixel", chunks=chunks)
    return _unbatched(I, coef, res, partial)


@fit_shared_residual.register_fake
def _(U, W, I, planar=False, chunks=0):
    P = I.shape[-1]
    nb = (P + 255) // 256  # rti_fit_shared_residual_blocks(P): one slot per 256-pixel workgroup span
    return _outputs(I, _lead(I), P, U.shape[1], planar, (torch.float32,)) + (
        I.new_empty(_lead(I) + (nb,), dtype=torch.float64),)


@torch.library.custom_op("rti::fit_robust", mutates_args=())
def fit_robust(A: torch.Tensor, I: torch.Tensor, lo: float, hi: float, min_lights: int, iters: int = 0,
               delta: float = 0.0, planar: bool = False,
               kernel: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The robust shared fit (``rti_fit_shared_robust``: intensity window [lo, hi], ±inf = no bound, and
    ``iters`` Huber IRLS steps of width delta).  A fp64 CUDA [N, k] (``rti.design_matrix``), I CUDA [N, P] or
    [C, N, P] (fp32/u8/int32) -> ``(coef, res, kept, fallback_px)``: coef fp32 [C?, P, k] (or [C?, k, P] if
    planar), res fp32 [C?, P], kept int32 [C?, P], fallback_px int32 [1]."""
    api._require_cuda(I, "I")
    api._require_cuda(A, "A")
    if A.dtype != torch.float64:
        raise ValueError("A must be float64 (rti.design_matrix)")
    _same_device(A=A, I=I)
    _in_dtype(I)
    I3 = _batched(I)
    C, N, P = I3.shape
    k = A.shape[1]
    if A.shape[0] != N:
        raise ValueError(f"A must be [{N}, k]; got {tuple(A.shape)}")
    coef, res, kept = _outputs(I, (C,), P, k, planar, (torch.float32, torch.int32))
    fallback = torch.zeros(1, dtype=torch.int32, device=I.device)
    api.fit_robust_into(A.contiguous(), I3, coef, res, kept, fallback, k=k, lo=lo, hi=hi, min_lights=min_lights,
                        iters=iters, delta=delta, layout="planar" if planar else "pixel", kernel=kernel)
    return _unbatched(I, coef, res, kept) + (fallback,)


@fit_robust.register_fake
def _(A, I, lo, hi, min_lights, iters=0, delta=0.0, planar=False, kernel=0):
    return _outputs(I, _lead(I), I.shape[-1], A.shape[1], planar, (torch.float32, torch.int32)) + (
        I.new_empty((1,), dtype=torch.int32),)


def _ps_outputs(I, lead, P, planar):
    """photometric_stereo's outputs on I's device: normals [P, 3] (or [3, P] if planar), albedo lead + [P], kind
    [P], res and kept lead + [P], fallback_px [1]; lead = (C,) or the caller's own."""
    return (I.new_empty((3, P) if planar else (P, 3), dtype=torch.float32),
            I.new_empty(lead + (P,), dtype=torch.float32), I.new_empty((P,), dtype=torch.uint8),
            I.new_empty(lead + (P,), dtype=torch.float32), I.new_empty(lead + (P,), dtype=torch.int32),
            I.new_zeros((1,), dtype=torch.int32))


@torch.library.custom_op("rti::photometric_stereo", mutates_args=())
def photometric_stereo(A: torch.Tensor, I: torch.Tensor, lo: float, hi: float, min_lights: int, iters: int = 0,
                       delta: float = 0.0, weights: Optional[Sequence[float]] = None, planar: bool = False,
                       kernel: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                 torch.Tensor]:
    """Photometric stereo (``rti_photometric_stereo``: the robust Lambertian fit with the intensity window
    [lo, hi], ±inf = no bound, and ``iters`` Huber IRLS steps of width delta).  A fp64 CUDA [N, 3]
    (``rti.ps_design``), I CUDA [N, P] or [3, N, P] (fp32/u8/int32) -> ``(normals, albedo, kind, res, kept,
    fallback_px)``: normals fp32 [P, 3] (or [3, P] if planar), albedo fp32 [C?, P], kind uint8 [P], res fp32
    [C?, P], kept int32 [C?, P], fallback_px int32 [1]."""
    api._require_cuda(I, "I")
    api._require_cuda(A, "A")
    if A.dtype != torch.float64:
        raise ValueError("A must be float64 (rti.ps_design)")
    _same_device(A=A, I=I)
    _in_dtype(I)
    I3 = _batched(I)
    C, N, P = I3.shape
    normals, albedo, kind, res, kept, fallback = _ps_outputs(I, (C,), P, planar)
    api.photometric_stereo_into(A.contiguous(), I3, normals, albedo, kind, res, kept, fallback, lo=lo, hi=hi,
                                min_lights=min_lights, iters=iters, delta=delta, weights=weights,
                                normal_layout="planar" if planar else "pixel", kernel=kernel)
    return (normals,) + _unbatched(I, albedo) + (kind,) + _unbatched(I, res, kept) + (fallback,)


@photometric_stereo.register_fake
def _(A, I, lo, hi, min_lights, iters=0, delta=0.0, weights=None, planar=False, kernel=0):
    return _ps_outputs(I, _lead(I), I.shape[-1], planar)


@torch.library.custom_op("rti::photometric_stereo_near", mutates_args=())
def photometric_stereo_near(lights: torch.Tensor, I: torch.Tensor, H: int, W: int, lo: float, hi: float,
                            min_lights: int, iters: int = 0, delta: float = 0.0,
                            weights: Optional[Sequence[float]] = None, planar: bool = False, kernel: int = 0,
                            x0: float = 0.0, y0: float = 0.0, height: Optional[torch.Tensor] = None,
                            z_offset: float = 0.0, falloff: bool = True,
                            r0: float = 1.0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                      torch.Tensor, torch.Tensor]:
    """Near-light photometric stereo (``rti_photometric_stereo_near``): ``photometric_stereo`` with a row per pixel
    from the light positions.  lights fp64 CUDA [N, 4] (``rti.ps_near_lights``), I CUDA [N, H·W] or [3, N, H·W];
    pixel y·W + x sits at (x0 + x, y0 + y, z_offset + height), height fp32 [H·W] or None.  The outputs are
    ``photometric_stereo``'s."""
    api._require_cuda(I, "I")
    api._require_cuda(lights, "lights")
    if lights.dtype != torch.float64:
        raise ValueError("lights must be float64 (rti.ps_near_lights)")
    _same_device(lights=lights, I=I, **({} if height is None else {"height": height}))
    _in_dtype(I)
    I3 = _batched(I)
    C, N, P = I3.shape
    normals, albedo, kind, res, kept, fallback = _ps_outputs(I, (C,), P, planar)
    api.photometric_stereo_near_into(lights.contiguous(), I3, H, W, normals, albedo, kind, res, kept, fallback, lo=lo,
                                     hi=hi, min_lights=min_lights, origin=(x0, y0),
                                     height=None if height is None else height.contiguous(), z_offset=z_offset,
                                     falloff=falloff, r0=r0, iters=iters, delta=delta, weights=weights,
                                     normal_layout="planar" if planar else "pixel", kernel=kernel)
    return (normals,) + _unbatched(I, albedo) + (kind,) + _unbatched(I, res, kept) + (fallback,)


@photometric_stereo_near.register_fake
def _(lights, I, H, W, lo, hi, min_lights, iters=0, delta=0.0, weights=None, planar=False, kernel=0, x0=0.0, y0=0.0,
      height=None, z_offset=0.0, falloff=True, r0=1.0):
    return _ps_outputs(I, _lead(I), I.shape[-1], planar)


def _accum_state(state, k):
    if state.dtype != torch.float64 or state.dim() not in (2, 3) or state.shape[-2] != k + 1:
        raise ValueError(f"state must be float64 [{k + 1}, P] or [C, {k + 1}, P]; got {state.dtype} {tuple(state.shape)}")
    if not state.is_contiguous():
        raise ValueError("state must be contiguous")
    return state if state.dim() == 3 else state.unsqueeze(0)


@torch.library.custom_op("rti::fit_accumulate", mutates_args=("state",))
def fit_accumulate(R: torch.Tensor, I: torch.Tensor, state: torch.Tensor, init: bool) -> None:
    """Add a chunk of light planes to a fit state in place (``rti_fit_accumulate``).  R fp64 CUDA [B, k]: the
    chunk's rows of the design matrix (or of U); I CUDA [B, P] or [C, B, P] (fp32/u8/int32); state fp64
    [k+1, P] or [C, k+1, P]; init: overwrite the state instead of adding to it."""
    api._require_cuda(I, "I")
    api._require_cuda(R, "R")
    api._require_cuda(state, "state")
    _same_device(R=R, I=I, state=state)
    _in_dtype(I)
    if I.dim() != state.dim() or I.dim() not in (2, 3):
        raise ValueError(f"I {tuple(I.shape)} and state {tuple(state.shape)} must both be 2-D or both 3-D")
    k = R.shape[1]
    s3 = _accum_state(state, k)
    I3 = _batched(I)
    if I3.shape[0] != s3.shape[0] or I3.shape[2] != s3.shape[2]:
        raise ValueError(f"I {tuple(I.shape)} does not match state {tuple(state.shape)}")
    api.fit_accumulate_into(R.contiguous(), I3, s3, k=k, init=init)


@fit_accumulate.register_fake
def _(R, I, state, init):
    return None


@torch.library.custom_op("rti::fit_accum_solve", mutates_args=())
def fit_accum_solve(M: torch.Tensor, state: torch.Tensor, n_lights: int, orth: bool = False,
                    planar: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """Coefficients and residuals from a fit state (``rti_fit_accum_solve``).  M fp64 CUDA [k, k]
    (``rti.gram_inverse`` over every direction accumulated, or W of ``rti.lsq_factors`` with orth); state fp64
    [k+1, P] or [C, k+1, P] -> ``(coef, res)``: coef fp32 [C?, P, k] (or [C?, k, P] if planar), res fp32 [C?, P]."""
    api._require_cuda(M, "M")
    api._require_cuda(state, "state")
    _same_device(M=M, state=state)
    k = M.shape[0]
    s3 = _accum_state(state, k)
    C, _, P = s3.shape
    coef, res = _outputs(state, (C,), P, k, planar, (torch.float32,))
    api.fit_accum_solve_into(M.contiguous(), s3, coef, res, k=k, n_lights=n_lights, orth=orth,
                             layout="planar" if planar else "pixel")
    return _unbatched(state, coef, res)


@fit_accum_solve.register_fake
def _(M, state, n_lights, orth=False, planar=False):
    return _outputs(state, _lead(state), state.shape[-1], M.shape[0], planar, (torch.float32,))


@torch.library.custom_op("rti::fit_residual", mutates_args=())
def fit_residual(A: torch.Tensor, I: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """Per-pixel RMS residual of coef (fp32 [P, k], fit_shared's pixel-major output) against
    I (CUDA [N, P]) under the fp32 design matrix A [N, k] -> fp32 [P]."""
    api._require_cuda(I, "I")
    api._require_cuda(A, "A")
    api._require_cuda(coef, "coef")
    if A.dtype != torch.float32 or coef.dtype != torch.float32:
        raise ValueError("A and coef must be float32")
    _same_device(A=A, I=I, coef=coef)
    _in_dtype(I)
    if I.dim() != 2:
        raise ValueError("I must be [N, P]")
    N, P = I.shape
    k = A.shape[1]
    if A.shape[0] != N or coef.shape != (P, k):
        raise ValueError(f"A must be [{N}, k] and coef [{P}, k]")
    Ic, Ac, cc = I.contiguous(), A.contiguous(), coef.contiguous()
    res = torch.empty(P, dtype=torch.float32, device=I.device)
    api.fit_residual_into(Ac, Ic.unsqueeze(0), cc, res, None, k=k, layout="pixel")
    return res


@fit_residual.register_fake
def _(A, I, coef):
    return I.new_empty((I.shape[-1],), dtype=torch.float32)


@torch.library.custom_op("rti::relight", mutates_args=())
def relight(coef: torch.Tensor, luv: torch.Tensor, basis: int = L.RTI_BASIS_PTM6) -> torch.Tensor:
    """coef CUDA [P, k] (fp32/fp64), luv [E, 2] -> [E, P] in coef's dtype."""
    lu = luv[:, 0].detach().cpu().double().numpy()
    lv = luv[:, 1].detach().cpu().double().numpy()
    return api.relight(coef, lu, lv, basis=basis, out_dtype=coef.dtype)


@relight.register_fake
def _(coef, luv, basis=L.RTI_BASIS_PTM6):
    return coef.new_empty((luv.shape[0], coef.shape[0]))


def _ptm_pixels(coef, planar):
    """P of PTM-6 maps [P, 6] (or [6, P] if planar)."""
    if coef.dim() != 2 or coef.shape[0 if planar else 1] != 6:
        raise ValueError(f"coef must be {'[6, P]' if planar else '[P, 6]'}; got {tuple(coef.shape)}")
    return coef.shape[1 if planar else 0]


@torch.library.custom_op("rti::ptm_normals", mutates_args=())
def ptm_normals(coef: torch.Tensor, planar: bool = False,
                normals_planar: bool = False) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Surface normals of PTM-6 maps (``rti_ptm_normals``).  coef CUDA fp32/fp64 [P, 6] (or [6, P] if planar) ->
    ``(normals, kind, peak)``: normals fp32 [P, 3] (or [3, P] if normals_planar), kind uint8 [P], peak fp32 [P]."""
    api._require_cuda(coef, "coef")
    P = _ptm_pixels(coef, planar)
    normals = coef.new_empty((3, P) if normals_planar else (P, 3), dtype=torch.float32)
    kind = coef.new_empty((P,), dtype=torch.uint8)
    peak = coef.new_empty((P,), dtype=torch.float32)
    api.ptm_normals_into(coef.contiguous(), normals, kind, peak, layout="planar" if planar else "pixel",
                         normal_layout="planar" if normals_planar else "pixel")
    return normals, kind, peak


@ptm_normals.register_fake
def _(coef, planar=False, normals_planar=False):
    P = coef.shape[1 if planar else 0]
    return (coef.new_empty((3, P) if normals_planar else (P, 3), dtype=torch.float32),
            coef.new_empty((P,), dtype=torch.uint8), coef.new_empty((P,), dtype=torch.float32))


@torch.library.custom_op("rti::relight_enhanced", mutates_args=())
def relight_enhanced(coef: torch.Tensor, lu: float, lv: float, mode: int, gain: float = 1.0, kd: float = 1.0,
                     ks: float = 0.0, exp: int = 1, planar: bool = False,
                     out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One enhanced rendering of PTM-6 maps at (lu, lv) (``rti_relight_enhanced``).  coef CUDA fp32/fp64 [P, 6]
    (or [6, P] if planar), mode RTI_ENHANCE_DIFFUSE_GAIN (1) or RTI_ENHANCE_SPECULAR (2) -> [P] in out_dtype
    (float32, int32 or uint8)."""
    api._require_cuda(coef, "coef")
    P = _ptm_pixels(coef, planar)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    out = coef.new_empty((P,), dtype=out_dtype)
    return api.relight_enhanced_into(coef.contiguous(), lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp,
                                     layout="planar" if planar else "pixel")


@relight_enhanced.register_fake
def _(coef, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1, planar=False, out_dtype=torch.float32):
    return coef.new_empty((coef.shape[1 if planar else 0],), dtype=out_dtype)


@torch.library.custom_op("rti::map_unsharp", mutates_args=())
def map_unsharp(src: torch.Tensor, sigma: float, amount: float = 1.0, radius: int = 0, planar: bool = False,
                renorm: bool = False) -> torch.Tensor:
    """Unsharp masking of a map (``rti_map_unsharp``).  src CUDA fp32 [H, W], [H, W, k] (or [k, H, W] if planar)
    -> the same shape; radius 0 = max(1, ceil(3·sigma)); renorm (k = 3): unit-length result."""
    s = src.contiguous()
    return api.map_unsharp_into(s, torch.empty_like(s), sigma=sigma, amount=amount, radius=radius,
                                layout="planar" if planar else "pixel", renorm=renorm)


@map_unsharp.register_fake
def _(src, sigma, amount=1.0, radius=0, planar=False, renorm=False):
    return src.new_empty(src.shape)


@torch.library.custom_op("rti::shade_normals", mutates_args=())
def shade_normals(n: torch.Tensor, lu: float, lv: float, albedo: torch.Tensor | None = None, kd: float = 1.0,
                  ks: float = 0.0, exp: int = 1, planar: bool = False,
                  out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One image shaded from a normal map at (lu, lv) (``rti_shade_normals``).  n CUDA fp32 [P, 3] (or [3, P] if
    planar), albedo None or fp32 [P] -> [P] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(n, "n")
    if n.dim() != 2 or n.shape[0 if planar else 1] != 3:
        raise ValueError(f"n must be {'[3, P]' if planar else '[P, 3]'}; got {tuple(n.shape)}")
    if albedo is not None:
        api._require_cuda(albedo, "albedo")
        _same_device(n=n, albedo=albedo)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    out = n.new_empty((n.shape[1 if planar else 0],), dtype=out_dtype)
    return api.shade_normals_into(n.contiguous(), lu, lv, out, albedo=None if albedo is None else albedo.contiguous(),
                                  kd=kd, ks=ks, exp=exp, normal_layout="planar" if planar else "pixel")


@shade_normals.register_fake
def _(n, lu, lv, albedo=None, kd=1.0, ks=0.0, exp=1, planar=False, out_dtype=torch.float32):
    return n.new_empty((n.shape[1 if planar else 0],), dtype=out_dtype)


@torch.library.custom_op("rti::lrgb_from_rgb", mutates_args=())
def lrgb_from_rgb(coef: torch.Tensor, gram: torch.Tensor, weights: Optional[Sequence[float]] = None,
                  planar: bool = False, lrgb_planar: bool = False) -> torch.Tensor:
    """Three PTM-6 maps -> one LRGB map (``rti_lrgb_from_rgb``).  coef CUDA fp32 [3, P, 6] (or [3, 6, P] if
    planar), gram [6, 6] (``rti.gram``; read on the host), weights None (1/3 each) or 3 values -> fp32 [P, 9]
    (or [9, P] if lrgb_planar)."""
    api._require_cuda(coef, "coef")
    if coef.dim() != 3 or coef.shape[0] != 3 or coef.shape[1 if planar else 2] != 6:
        raise ValueError(f"coef must be {'[3, 6, P]' if planar else '[3, P, 6]'}; got {tuple(coef.shape)}")
    P = coef.shape[2 if planar else 1]
    out = coef.new_empty((9, P) if lrgb_planar else (P, 9), dtype=torch.float32)
    return api.lrgb_from_rgb_into(coef.contiguous(), gram, out, weights=weights,
                                  layout="planar" if planar else "pixel",
                                  lrgb_layout="planar" if lrgb_planar else "pixel")


@lrgb_from_rgb.register_fake
def _(coef, gram, weights=None, planar=False, lrgb_planar=False):
    P = coef.shape[2 if planar else 1]
    return coef.new_empty((9, P) if lrgb_planar else (P, 9), dtype=torch.float32)


@torch.library.custom_op("rti::relight_lrgb", mutates_args=())
def relight_lrgb(lrgb: torch.Tensor, luv: torch.Tensor, planar: bool = False,
                 out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """RGB images of an LRGB map (``rti_relight_lrgb``).  lrgb CUDA fp32 [P, 9] (or [9, P] if planar), luv
    [E, 2] -> [E, P, 3] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(lrgb, "lrgb")
    if lrgb.dim() != 2 or lrgb.shape[0 if planar else 1] != 9:
        raise ValueError(f"lrgb must be {'[9, P]' if planar else '[P, 9]'}; got {tuple(lrgb.shape)}")
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    luv_d = luv.detach().to(device=lrgb.device, dtype=torch.float64).contiguous()
    out = lrgb.new_empty((luv.shape[0], lrgb.shape[1 if planar else 0], 3), dtype=out_dtype)
    return api.relight_lrgb_into(lrgb.contiguous(), luv_d, out, layout="planar" if planar else "pixel")


@relight_lrgb.register_fake
def _(lrgb, luv, planar=False, out_dtype=torch.float32):
    return lrgb.new_empty((luv.shape[0], lrgb.shape[1 if planar else 0], 3), dtype=out_dtype)


@torch.library.custom_op("rti::lrgb_quantise", mutates_args=())
def lrgb_quantise(lrgb: torch.Tensor, planar: bool = False) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """An LRGB map -> its .ptm bytes and header values (``rti_lrgb_qparams`` then ``rti_lrgb_quantise``).  lrgb
    CUDA fp32 [P, 9] (or [9, P] if planar) -> (coef8 uint8 [P, 6], rgb8 uint8 [P, 3], qparams fp64 [13])."""
    api._require_cuda(lrgb, "lrgb")
    if lrgb.dim() != 2 or lrgb.shape[0 if planar else 1] != 9:
        raise ValueError(f"lrgb must be {'[9, P]' if planar else '[P, 9]'}; got {tuple(lrgb.shape)}")
    P = lrgb.shape[1 if planar else 0]
    layout = "planar" if planar else "pixel"
    m = lrgb.contiguous()
    ws = lrgb.new_empty((api.lrgb_qparams_workspace(P),), dtype=torch.uint8)
    qparams = lrgb.new_empty((13,), dtype=torch.float64)
    coef8, rgb8 = lrgb.new_empty((P, 6), dtype=torch.uint8), lrgb.new_empty((P, 3), dtype=torch.uint8)
    api.lrgb_qparams_into(m, ws, qparams, layout=layout)
    api.lrgb_quantise_into(m, qparams, coef8, rgb8, layout=layout)
    return coef8, rgb8, qparams


@lrgb_quantise.register_fake
def _(lrgb, planar=False):
    P = lrgb.shape[1 if planar else 0]
    return (lrgb.new_empty((P, 6), dtype=torch.uint8), lrgb.new_empty((P, 3), dtype=torch.uint8),
            lrgb.new_empty((13,), dtype=torch.float64))


@torch.library.custom_op("rti::relight_lrgb8", mutates_args=())
def relight_lrgb8(coef8: torch.Tensor, rgb8: torch.Tensor, qparams: torch.Tensor, luv: torch.Tensor,
                  out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """RGB images of a quantised LRGB map (``rti_relight_lrgb8``).  coef8 CUDA uint8 [P, 6], rgb8 uint8 [P, 3],
    qparams fp64 [13], luv [E, 2] -> [E, P, 3] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef8, "coef8")
    if coef8.dim() != 2 or coef8.shape[1] != 6 or rgb8.dim() != 2 or tuple(rgb8.shape) != (coef8.shape[0], 3):
        raise ValueError(f"coef8 must be [P, 6] and rgb8 [P, 3]; got {tuple(coef8.shape)} and {tuple(rgb8.shape)}")
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    luv_d = luv.detach().to(device=coef8.device, dtype=torch.float64).contiguous()
    out = coef8.new_empty((luv.shape[0], coef8.shape[0], 3), dtype=out_dtype)
    return api.relight_lrgb8_into(coef8.contiguous(), rgb8.contiguous(), qparams.contiguous(), luv_d, out)


@relight_lrgb8.register_fake
def _(coef8, rgb8, qparams, luv, out_dtype=torch.float32):
    return coef8.new_empty((luv.shape[0], coef8.shape[0], 3), dtype=out_dtype)


@torch.library.custom_op("rti::hsh_quantise", mutates_args=())
def hsh_quantise(coef: torch.Tensor, k: int = 16, planar: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """Three HSH maps -> their .rti bytes and header values (``rti_hsh_qparams`` then ``rti_hsh_quantise``).  coef
    CUDA fp32 [3, P, k] (or [3, k, P] if planar), k = 9 or 16 -> (coef8 uint8 [P, 3, k], qparams fp32 [2k])."""
    api._require_cuda(coef, "coef")
    if k not in (9, 16):
        raise NotImplementedError(f"8-bit HSH maps are HSH-9 and HSH-16 only; got k = {k}")
    if coef.dim() != 3 or coef.shape[0] != 3 or coef.shape[1 if planar else 2] != k:
        raise ValueError(f"coef must be {f'[3, {k}, P]' if planar else f'[3, P, {k}]'}; got {tuple(coef.shape)}")
    P = coef.shape[2 if planar else 1]
    basis, layout = f"hsh{k}", "planar" if planar else "pixel"
    m = coef.contiguous()
    ws = coef.new_empty((api.hsh_qparams_workspace(P, basis),), dtype=torch.uint8)
    qparams = coef.new_empty((2 * k,), dtype=torch.float32)
    coef8 = coef.new_empty((P, 3, k), dtype=torch.uint8)
    api.hsh_qparams_into(m, ws, qparams, basis=basis, layout=layout)
    api.hsh_quantise_into(m, qparams, coef8, basis=basis, layout=layout)
    return coef8, qparams


@hsh_quantise.register_fake
def _(coef, k=16, planar=False):
    P = coef.shape[2 if planar else 1]
    return coef.new_empty((P, 3, k), dtype=torch.uint8), coef.new_empty((2 * k,), dtype=torch.float32)


@torch.library.custom_op("rti::relight_hsh8", mutates_args=())
def relight_hsh8(coef8: torch.Tensor, qparams: torch.Tensor, luv: torch.Tensor,
                 out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """RGB images of a quantised RGB HSH map (``rti_relight_hsh8``).  coef8 CUDA uint8 [P, 3, k] with k = 9 or
    16, qparams fp32 [2k], luv [E, 2] -> [E, P, 3] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef8, "coef8")
    if coef8.dim() != 3 or coef8.shape[1] != 3 or coef8.shape[2] not in (9, 16):
        raise ValueError(f"coef8 must be [P, 3, 9] or [P, 3, 16]; got {tuple(coef8.shape)}")
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    luv_d = luv.detach().to(device=coef8.device, dtype=torch.float64).contiguous()
    out = coef8.new_empty((luv.shape[0], coef8.shape[0], 3), dtype=out_dtype)
    return api.relight_hsh8_into(coef8.contiguous(), qparams.contiguous(), luv_d, out, basis=f"hsh{coef8.shape[2]}")


@relight_hsh8.register_fake
def _(coef8, qparams, luv, out_dtype=torch.float32):
    return coef8.new_empty((luv.shape[0], coef8.shape[0], 3), dtype=out_dtype)


def _normal_triple(like, P, normals_planar):
    """(normals, kind, peak) for P pixels on ``like``'s device."""
    return (like.new_empty((3, P) if normals_planar else (P, 3), dtype=torch.float32),
            like.new_empty((P,), dtype=torch.uint8), like.new_empty((P,), dtype=torch.float32))


def _hsh_map_pixels(coef, k, planar):
    """P of one HSH map [P, k] / [k, P] or of three [3, P, k] / [3, k, P]."""
    if k not in (9, 16):
        raise NotImplementedError(f"HSH normals are HSH-9 and HSH-16 only; got k = {k}")
    if coef.dim() not in (2, 3) or (coef.dim() == 3 and coef.shape[0] != 3) or coef.shape[-2 if planar else -1] != k:
        want = f"[{k}, P] or [3, {k}, P]" if planar else f"[P, {k}] or [3, P, {k}]"
        raise ValueError(f"coef must be {want}; got {tuple(coef.shape)}")
    return coef.shape[-1 if planar else -2]


@torch.library.custom_op("rti::hsh_normals", mutates_args=())
def hsh_normals(coef: torch.Tensor, k: int = 16, planar: bool = False, normals_planar: bool = False, grid: int = 10,
                weights: Optional[Sequence[float]] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Surface normals of HSH maps by peak search (``rti_hsh_normals``).  coef CUDA fp32 [P, k] or [3, P, k] (or
    [k, P] / [3, k, P] if planar), k = 9 or 16, grid in [4, 16], weights None (0.299, 0.587, 0.114) or 3 values ->
    ``(normals, kind, peak)``: normals fp32 [P, 3] (or [3, P] if normals_planar), kind uint8 [P], peak fp32 [P]."""
    api._require_cuda(coef, "coef")
    P = _hsh_map_pixels(coef, k, planar)
    normals, kind, peak = _normal_triple(coef, P, normals_planar)
    api.hsh_normals_into(coef.contiguous(), api.peak_table(f"hsh{k}", grid, coef.device), normals, kind, peak,
                         basis=f"hsh{k}", layout="planar" if planar else "pixel",
                         normal_layout="planar" if normals_planar else "pixel", grid=grid, weights=weights)
    return normals, kind, peak


@hsh_normals.register_fake
def _(coef, k=16, planar=False, normals_planar=False, grid=10, weights=None):
    return _normal_triple(coef, coef.shape[-1 if planar else -2], normals_planar)


@torch.library.custom_op("rti::hsh8_normals", mutates_args=())
def hsh8_normals(coef8: torch.Tensor, qparams: torch.Tensor, normals_planar: bool = False, grid: int = 10,
                 weights: Optional[Sequence[float]] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Surface normals of a quantised RGB HSH map by peak search (``rti_hsh8_normals``).  coef8 CUDA uint8
    [P, 3, k] with k = 9 or 16, qparams fp32 [2k] -> ``(normals, kind, peak)`` as ``hsh_normals``."""
    api._require_cuda(coef8, "coef8")
    if coef8.dim() != 3 or coef8.shape[1] != 3 or coef8.shape[2] not in (9, 16):
        raise ValueError(f"coef8 must be [P, 3, 9] or [P, 3, 16]; got {tuple(coef8.shape)}")
    P, basis = coef8.shape[0], f"hsh{coef8.shape[2]}"
    normals, kind, peak = _normal_triple(coef8, P, normals_planar)
    api.hsh8_normals_into(coef8.contiguous(), qparams.contiguous(), api.peak_table(basis, grid, coef8.device), normals,
                          kind, peak, basis=basis, normal_layout="planar" if normals_planar else "pixel", grid=grid,
                          weights=weights)
    return normals, kind, peak


@hsh8_normals.register_fake
def _(coef8, qparams, normals_planar=False, grid=10, weights=None):
    return _normal_triple(coef8, coef8.shape[0], normals_planar)


@torch.library.custom_op("rti::rgb8_quantise", mutates_args=())
def rgb8_quantise(coef: torch.Tensor, planar: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """Three PTM-6 maps -> their PTM_FORMAT_RGB bytes and header values (``rti_rgb8_qparams`` then
    ``rti_rgb8_quantise``).  coef CUDA fp32 [3, P, 6] (or [3, 6, P] if planar) -> (coef8 uint8 [3, P, 6], qparams
    fp64 [12])."""
    api._require_cuda(coef, "coef")
    if coef.dim() != 3 or coef.shape[0] != 3 or coef.shape[1 if planar else 2] != 6:
        raise ValueError(f"coef must be {'[3, 6, P]' if planar else '[3, P, 6]'}; got {tuple(coef.shape)}")
    P = coef.shape[2 if planar else 1]
    layout = "planar" if planar else "pixel"
    m = coef.contiguous()
    ws = coef.new_empty((api.rgb8_qparams_workspace(P),), dtype=torch.uint8)
    qparams = coef.new_empty((12,), dtype=torch.float64)
    coef8 = coef.new_empty((3, P, 6), dtype=torch.uint8)
    api.rgb8_qparams_into(m, ws, qparams, layout=layout)
    api.rgb8_quantise_into(m, qparams, coef8, layout=layout)
    return coef8, qparams


@rgb8_quantise.register_fake
def _(coef, planar=False):
    P = coef.shape[2 if planar else 1]
    return coef.new_empty((3, P, 6), dtype=torch.uint8), coef.new_empty((12,), dtype=torch.float64)


def _rgb8_pixels(coef8):
    if coef8.dim() != 3 or coef8.shape[0] != 3 or coef8.shape[2] != 6:
        raise ValueError(f"coef8 must be [3, P, 6]; got {tuple(coef8.shape)}")
    return coef8.shape[1]


@torch.library.custom_op("rti::relight_rgb8", mutates_args=())
def relight_rgb8(coef8: torch.Tensor, qparams: torch.Tensor, luv: torch.Tensor,
                 out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """RGB images of a quantised RGB PTM (``rti_relight_rgb8``).  coef8 CUDA uint8 [3, P, 6], qparams fp64 [12],
    luv [E, 2] -> [E, P, 3] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef8, "coef8")
    P = _rgb8_pixels(coef8)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    luv_d = luv.detach().to(device=coef8.device, dtype=torch.float64).contiguous()
    out = coef8.new_empty((luv.shape[0], P, 3), dtype=out_dtype)
    return api.relight_rgb8_into(coef8.contiguous(), qparams.contiguous(), luv_d, out)


@relight_rgb8.register_fake
def _(coef8, qparams, luv, out_dtype=torch.float32):
    return coef8.new_empty((luv.shape[0], coef8.shape[1], 3), dtype=out_dtype)


@torch.library.custom_op("rti::rgb8_normals", mutates_args=())
def rgb8_normals(coef8: torch.Tensor, qparams: torch.Tensor, normals_planar: bool = False,
                 weights: Optional[Sequence[float]] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Surface normals of a quantised RGB PTM (``rti_rgb8_normals``).  coef8 CUDA uint8 [3, P, 6], qparams fp64
    [12], weights None (0.299, 0.587, 0.114) or 3 values -> ``(normals, kind, peak)``: normals fp32 [P, 3] (or
    [3, P] if normals_planar), kind uint8 [P], peak fp32 [P]."""
    api._require_cuda(coef8, "coef8")
    P = _rgb8_pixels(coef8)
    normals, kind, peak = _normal_triple(coef8, P, normals_planar)
    api.rgb8_normals_into(coef8.contiguous(), qparams.contiguous(), normals, kind, peak,
                          normal_layout="planar" if normals_planar else "pixel", weights=weights)
    return normals, kind, peak


@rgb8_normals.register_fake
def _(coef8, qparams, normals_planar=False, weights=None):
    return _normal_triple(coef8, coef8.shape[1], normals_planar)


# ---- diffuse gain and specular rendering of the colour forms ----------------

def _enhanced_rgb_out(like, P, out_dtype):
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    return like.new_empty((P, 3), dtype=out_dtype)


@torch.library.custom_op("rti::relight_lrgb_enhanced", mutates_args=())
def relight_lrgb_enhanced(lrgb: torch.Tensor, lu: float, lv: float, mode: int, gain: float = 1.0, kd: float = 1.0,
                          ks: float = 0.0, exp: int = 1, planar: bool = False,
                          out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One enhanced RGB rendering of an LRGB map at (lu, lv) (``rti_relight_lrgb_enhanced``).  lrgb CUDA fp32
    [P, 9] (or [9, P] if planar), mode RTI_ENHANCE_DIFFUSE_GAIN (1) or RTI_ENHANCE_SPECULAR (2) -> [P, 3] in
    out_dtype (float32, int32 or uint8)."""
    api._require_cuda(lrgb, "lrgb")
    if lrgb.dim() != 2 or lrgb.shape[0 if planar else 1] != 9:
        raise ValueError(f"lrgb must be {'[9, P]' if planar else '[P, 9]'}; got {tuple(lrgb.shape)}")
    out = _enhanced_rgb_out(lrgb, lrgb.shape[1 if planar else 0], out_dtype)
    return api.relight_lrgb_enhanced_into(lrgb.contiguous(), lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp,
                                          layout="planar" if planar else "pixel")


@relight_lrgb_enhanced.register_fake
def _(lrgb, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1, planar=False, out_dtype=torch.float32):
    return lrgb.new_empty((lrgb.shape[1 if planar else 0], 3), dtype=out_dtype)


@torch.library.custom_op("rti::relight_lrgb8_enhanced", mutates_args=())
def relight_lrgb8_enhanced(coef8: torch.Tensor, rgb8: torch.Tensor, qparams: torch.Tensor, lu: float, lv: float,
                           mode: int, gain: float = 1.0, kd: float = 1.0, ks: float = 0.0, exp: int = 1,
                           out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One enhanced RGB rendering of a quantised LRGB map (``rti_relight_lrgb8_enhanced``).  coef8 CUDA uint8
    [P, 6], rgb8 uint8 [P, 3], qparams fp64 [13] -> [P, 3] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef8, "coef8")
    if coef8.dim() != 2 or coef8.shape[1] != 6 or rgb8.dim() != 2 or tuple(rgb8.shape) != (coef8.shape[0], 3):
        raise ValueError(f"coef8 must be [P, 6] and rgb8 [P, 3]; got {tuple(coef8.shape)} and {tuple(rgb8.shape)}")
    out = _enhanced_rgb_out(coef8, coef8.shape[0], out_dtype)
    return api.relight_lrgb8_enhanced_into(coef8.contiguous(), rgb8.contiguous(), qparams.contiguous(), lu, lv, mode,
                                           out, gain=gain, kd=kd, ks=ks, exp=exp)


@relight_lrgb8_enhanced.register_fake
def _(coef8, rgb8, qparams, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1, out_dtype=torch.float32):
    return coef8.new_empty((coef8.shape[0], 3), dtype=out_dtype)


@torch.library.custom_op("rti::relight_rgb8_enhanced", mutates_args=())
def relight_rgb8_enhanced(coef8: torch.Tensor, qparams: torch.Tensor, lu: float, lv: float, mode: int,
                          gain: float = 1.0, kd: float = 1.0, ks: float = 0.0, exp: int = 1,
                          weights: Optional[Sequence[float]] = None,
                          out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One enhanced RGB rendering of a quantised RGB PTM (``rti_relight_rgb8_enhanced``).  coef8 CUDA uint8
    [3, P, 6], qparams fp64 [12], weights None (0.299, 0.587, 0.114) or 3 values -> [P, 3] in out_dtype (float32,
    int32 or uint8)."""
    api._require_cuda(coef8, "coef8")
    out = _enhanced_rgb_out(coef8, _rgb8_pixels(coef8), out_dtype)
    return api.relight_rgb8_enhanced_into(coef8.contiguous(), qparams.contiguous(), lu, lv, mode, out, gain=gain,
                                          kd=kd, ks=ks, exp=exp, weights=weights)


@relight_rgb8_enhanced.register_fake
def _(coef8, qparams, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1, weights=None, out_dtype=torch.float32):
    return coef8.new_empty((coef8.shape[1], 3), dtype=out_dtype)


# ---- three fp32 RGB maps rendered in one pass -------------------------------

def _rgb_pixels(coef, k, planar):
    api._require_cuda(coef, "coef")
    if coef.dim() != 3 or coef.shape[0] != 3 or coef.shape[1 if planar else 2] != k:
        raise ValueError(f"coef must be {f'[3, {k}, P]' if planar else f'[3, P, {k}]'}; got {tuple(coef.shape)}")
    return coef.shape[2 if planar else 1]


@torch.library.custom_op("rti::relight_rgb", mutates_args=())
def relight_rgb(coef: torch.Tensor, luv: torch.Tensor, basis: int = L.RTI_BASIS_PTM6, planar: bool = False,
                out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """RGB images of three fp32 maps (``rti_relight_rgb``).  coef CUDA fp32 [3, P, k] (or [3, k, P] if planar),
    basis PTM-6, HSH-9 or HSH-16, luv [E, 2] -> [E, P, 3] in out_dtype (float32, int32 or uint8)."""
    P = _rgb_pixels(coef, api.basis_terms(basis), planar)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    luv_d = luv.detach().to(device=coef.device, dtype=torch.float64).contiguous()
    out = coef.new_empty((luv.shape[0], P, 3), dtype=out_dtype)
    return api.relight_rgb_into(coef.contiguous(), luv_d, out, basis=basis, layout="planar" if planar else "pixel")


@relight_rgb.register_fake
def _(coef, luv, basis=L.RTI_BASIS_PTM6, planar=False, out_dtype=torch.float32):
    return coef.new_empty((luv.shape[0], coef.shape[2 if planar else 1], 3), dtype=out_dtype)


@torch.library.custom_op("rti::relight_rgb_enhanced", mutates_args=())
def relight_rgb_enhanced(coef: torch.Tensor, lu: float, lv: float, mode: int, gain: float = 1.0, kd: float = 1.0,
                         ks: float = 0.0, exp: int = 1, planar: bool = False,
                         weights: Optional[Sequence[float]] = None,
                         out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One enhanced RGB rendering of three fp32 PTM-6 maps (``rti_relight_rgb_enhanced``).  coef CUDA fp32
    [3, P, 6] (or [3, 6, P] if planar), weights None (0.299, 0.587, 0.114) or 3 values -> [P, 3] in out_dtype
    (float32, int32 or uint8)."""
    out = _enhanced_rgb_out(coef, _rgb_pixels(coef, 6, planar), out_dtype)
    return api.relight_rgb_enhanced_into(coef.contiguous(), lu, lv, mode, out, gain=gain, kd=kd, ks=ks, exp=exp,
                                         layout="planar" if planar else "pixel", weights=weights)


@relight_rgb_enhanced.register_fake
def _(coef, lu, lv, mode, gain=1.0, kd=1.0, ks=0.0, exp=1, planar=False, weights=None, out_dtype=torch.float32):
    return coef.new_empty((coef.shape[2 if planar else 1], 3), dtype=out_dtype)


@torch.library.custom_op("rti::rgb_normals", mutates_args=())
def rgb_normals(coef: torch.Tensor, planar: bool = False, normals_planar: bool = False,
                weights: Optional[Sequence[float]] = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Surface normals of three fp32 PTM-6 maps (``rti_rgb_normals``).  coef CUDA fp32 [3, P, 6] (or [3, 6, P] if
    planar), weights None (0.299, 0.587, 0.114) or 3 values -> ``(normals, kind, peak)``: normals fp32 [P, 3] (or
    [3, P] if normals_planar), kind uint8 [P], peak fp32 [P]."""
    P = _rgb_pixels(coef, 6, planar)
    normals, kind, peak = _normal_triple(coef, P, normals_planar)
    api.rgb_normals_into(coef.contiguous(), normals, kind, peak, layout="planar" if planar else "pixel",
                         normal_layout="planar" if normals_planar else "pixel", weights=weights)
    return normals, kind, peak


@rgb_normals.register_fake
def _(coef, planar=False, normals_planar=False, weights=None):
    return _normal_triple(coef, coef.shape[2 if planar else 1], normals_planar)


# ---- specular enhancement of HSH maps under a normal map --------------------

def _specular_luv(luv):
    """luv [E, 2] on any device -> (lu, lv) on the host: the directions travel as kernel arguments."""
    if luv.dim() != 2 or luv.shape[1] != 2:
        raise ValueError(f"luv must be [E, 2]; got {tuple(luv.shape)}")
    h = luv.detach().cpu().double().numpy()
    return h[:, 0], h[:, 1]


def _specular_n(n, P, normals_planar):
    api._require_cuda(n, "n")
    if tuple(n.shape) != ((3, P) if normals_planar else (P, 3)):
        raise ValueError(f"n must be {f'[3, {P}]' if normals_planar else f'[{P}, 3]'}; got {tuple(n.shape)}")
    return n.contiguous()


@torch.library.custom_op("rti::relight_hsh_specular", mutates_args=())
def relight_hsh_specular(coef: torch.Tensor, n: torch.Tensor, luv: torch.Tensor, k: int = 16, kd: float = 1.0,
                         ks: float = 0.0, exp: int = 1, planar: bool = False, normals_planar: bool = False,
                         out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Specular enhancement of fp32 HSH maps under a normal map (``rti_relight_hsh_specular``).  coef CUDA fp32
    [P, k] or [3, P, k] (or [k, P] / [3, k, P] if planar), k = 9 or 16, n fp32 [P, 3] (or [3, P] if normals_planar),
    luv [E, 2] with E <= 16 (read on the host) -> [E, P] or [E, P, 3] in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef, "coef")
    P = _hsh_map_pixels(coef, k, planar)
    _same_device(coef=coef, n=n)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    lu, lv = _specular_luv(luv)
    out = coef.new_empty((luv.shape[0], P) + ((3,) if coef.dim() == 3 else ()), dtype=out_dtype)
    return api.relight_hsh_specular_into(coef.contiguous(), _specular_n(n, P, normals_planar), lu, lv, out,
                                         basis=f"hsh{k}", kd=kd, ks=ks, exp=exp,
                                         layout="planar" if planar else "pixel",
                                         normal_layout="planar" if normals_planar else "pixel")


@relight_hsh_specular.register_fake
def _(coef, n, luv, k=16, kd=1.0, ks=0.0, exp=1, planar=False, normals_planar=False, out_dtype=torch.float32):
    P = coef.shape[-1 if planar else -2]
    return coef.new_empty((luv.shape[0], P) + ((3,) if coef.dim() == 3 else ()), dtype=out_dtype)


@torch.library.custom_op("rti::relight_hsh8_specular", mutates_args=())
def relight_hsh8_specular(coef8: torch.Tensor, qparams: torch.Tensor, n: torch.Tensor, luv: torch.Tensor,
                          kd: float = 1.0, ks: float = 0.0, exp: int = 1, normals_planar: bool = False,
                          out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Specular enhancement of a quantised RGB HSH map under a normal map (``rti_relight_hsh8_specular``).  coef8
    CUDA uint8 [P, 3, k] with k = 9 or 16, qparams fp32 [2k], n and luv as ``relight_hsh_specular`` -> [E, P, 3]
    in out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef8, "coef8")
    if coef8.dim() != 3 or coef8.shape[1] != 3 or coef8.shape[2] not in (9, 16):
        raise ValueError(f"coef8 must be [P, 3, 9] or [P, 3, 16]; got {tuple(coef8.shape)}")
    _same_device(coef8=coef8, n=n)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    P = coef8.shape[0]
    lu, lv = _specular_luv(luv)
    out = coef8.new_empty((luv.shape[0], P, 3), dtype=out_dtype)
    return api.relight_hsh8_specular_into(coef8.contiguous(), qparams.contiguous(), _specular_n(n, P, normals_planar),
                                          lu, lv, out, basis=f"hsh{coef8.shape[2]}", kd=kd, ks=ks, exp=exp,
                                          normal_layout="planar" if normals_planar else "pixel")


@relight_hsh8_specular.register_fake
def _(coef8, qparams, n, luv, kd=1.0, ks=0.0, exp=1, normals_planar=False, out_dtype=torch.float32):
    return coef8.new_empty((luv.shape[0], coef8.shape[0], 3), dtype=out_dtype)


# ---- diffuse gain for HSH maps under a normal map ----------------------------

@torch.library.custom_op("rti::relight_hsh_gain", mutates_args=())
def relight_hsh_gain(coef: torch.Tensor, n: torch.Tensor, luv: torch.Tensor, k: int = 16, gain: float = 1.0,
                     planar: bool = False, normals_planar: bool = False,
                     out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Diffuse gain for fp32 HSH maps under a normal map (``rti_relight_hsh_gain``).  coef, n, luv, k, planar,
    normals_planar and out_dtype as ``relight_hsh_specular`` -> [E, P] or [E, P, 3]."""
    api._require_cuda(coef, "coef")
    P = _hsh_map_pixels(coef, k, planar)
    _same_device(coef=coef, n=n)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    lu, lv = _specular_luv(luv)
    out = coef.new_empty((luv.shape[0], P) + ((3,) if coef.dim() == 3 else ()), dtype=out_dtype)
    return api.relight_hsh_gain_into(coef.contiguous(), _specular_n(n, P, normals_planar), lu, lv, out,
                                     basis=f"hsh{k}", gain=gain, layout="planar" if planar else "pixel",
                                     normal_layout="planar" if normals_planar else "pixel")


@relight_hsh_gain.register_fake
def _(coef, n, luv, k=16, gain=1.0, planar=False, normals_planar=False, out_dtype=torch.float32):
    P = coef.shape[-1 if planar else -2]
    return coef.new_empty((luv.shape[0], P) + ((3,) if coef.dim() == 3 else ()), dtype=out_dtype)


@torch.library.custom_op("rti::relight_hsh8_gain", mutates_args=())
def relight_hsh8_gain(coef8: torch.Tensor, qparams: torch.Tensor, n: torch.Tensor, luv: torch.Tensor,
                      gain: float = 1.0, normals_planar: bool = False,
                      out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Diffuse gain for a quantised RGB HSH map under a normal map (``rti_relight_hsh8_gain``).  coef8, qparams, n,
    luv, normals_planar and out_dtype as ``relight_hsh8_specular`` -> [E, P, 3]."""
    api._require_cuda(coef8, "coef8")
    if coef8.dim() != 3 or coef8.shape[1] != 3 or coef8.shape[2] not in (9, 16):
        raise ValueError(f"coef8 must be [P, 3, 9] or [P, 3, 16]; got {tuple(coef8.shape)}")
    _same_device(coef8=coef8, n=n)
    if out_dtype not in api._ENHANCED_DTYPES:
        raise ValueError("out_dtype must be float32, int32 or uint8")
    P = coef8.shape[0]
    lu, lv = _specular_luv(luv)
    out = coef8.new_empty((luv.shape[0], P, 3), dtype=out_dtype)
    return api.relight_hsh8_gain_into(coef8.contiguous(), qparams.contiguous(), _specular_n(n, P, normals_planar),
                                      lu, lv, out, basis=f"hsh{coef8.shape[2]}", gain=gain,
                                      normal_layout="planar" if normals_planar else "pixel")


@relight_hsh8_gain.register_fake
def _(coef8, qparams, n, luv, gain=1.0, normals_planar=False, out_dtype=torch.float32):
    return coef8.new_empty((luv.shape[0], coef8.shape[0], 3), dtype=out_dtype)


@torch.library.custom_op("rti::height_from_normals", mutates_args=())
def height_from_normals(n: torch.Tensor, nz_min: float = 0.1, flip_y: bool = False, rtol: float = 1e-6,
                        max_iters: int = 2000, jacobi: bool = False, z0: torch.Tensor | None = None,
                        planar: bool = False, check_every: int = 8) -> torch.Tensor:
    """The height map of a normal map (``rti_height_from_normals``).  n CUDA fp32 [H, W, 3] (or [3, H, W] if
    planar), z0 None or a start fp32 [H, W] -> fp32 [H, W], zero mean over the valid pixels, NaN elsewhere;
    jacobi selects the diagonal preconditioner instead of the multigrid V-cycle."""
    api._require_cuda(n, "n")
    if z0 is not None:
        api._require_cuda(z0, "z0")
        _same_device(n=n, z0=z0)
    return api.height_from_normals(n, nz_min, flip_y, rtol, max_iters, "jacobi" if jacobi else "multigrid", z0,
                                   "planar" if planar else "pixel", check_every=check_every)


@height_from_normals.register_fake
def _(n, nz_min=0.1, flip_y=False, rtol=1e-6, max_iters=2000, jacobi=False, z0=None, planar=False, check_every=8):
    return n.new_empty(tuple(n.shape[1:]) if planar else tuple(n.shape[:2]))


# ---- multi-light detail enhancement ------------------------------------------

def _candidates(luv):
    """luv [E, 2] on any device -> host fp64 [E, 2]: the candidates travel as kernel arguments."""
    if luv.dim() != 2 or luv.shape[1] != 2:
        raise ValueError(f"luv must be [E, 2]; got {tuple(luv.shape)}")
    return luv.detach().cpu().double().numpy()


def _image_dims(coef, planar):
    """Maps [H, W, k] / [3, H, W, k] (or [k, H, W] / [3, k, H, W] if planar) -> (H, W)."""
    return tuple(coef.shape[-2:]) if planar else tuple(coef.shape[-3:-1])


@torch.library.custom_op("rti::light_scores", mutates_args=())
def light_scores(coef: torch.Tensor, luv: torch.Tensor, basis: int = L.RTI_BASIS_PTM6, tile: int = 16,
                 planar: bool = False, weights: Optional[Sequence[float]] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The multi-light search (``rti_light_scores``).  coef CUDA fp32 [H, W, k] or [3, H, W, k] (or [k, H, W] /
    [3, k, H, W] if planar), luv [E, 2] with E <= 64 (read on the host), tile 8, 16 or 32 -> (scores fp64
    [Ty, Tx, E, 2], count int32 [Ty, Tx])."""
    api._require_cuda(coef, "coef")
    return api.light_scores(coef.contiguous(), _candidates(luv), basis, tile=tile,
                            layout="planar" if planar else "pixel", weights=weights)


@light_scores.register_fake
def _(coef, luv, basis=L.RTI_BASIS_PTM6, tile=16, planar=False, weights=None):
    H, W = _image_dims(coef, planar)
    Ty, Tx = (H + tile - 1) // tile, (W + tile - 1) // tile
    return (coef.new_empty((Ty, Tx, luv.shape[0], 2), dtype=torch.float64),
            coef.new_empty((Ty, Tx), dtype=torch.int32))


@torch.library.custom_op("rti::light_field", mutates_args=())
def light_field(scores: torch.Tensor, count: torch.Tensor, luv: torch.Tensor, lu: float, lv: float, ws: float = 1.0,
                wb: float = 0.5, smooth: int = 2) -> torch.Tensor:
    """The light field of the multi-light mode (``rti_light_field``).  scores fp64 [Ty, Tx, E, 2] and count int32
    [Ty, Tx] of ``light_scores``, luv the same candidates, (lu, lv) the main light -> fp32 [Ty, Tx, 2]."""
    api._require_cuda(scores, "scores")
    api._require_cuda(count, "count")
    _same_device(scores=scores, count=count)
    return api.light_field(scores, count, _candidates(luv), lu, lv, ws=ws, wb=wb, smooth=smooth)


@light_field.register_fake
def _(scores, count, luv, lu, lv, ws=1.0, wb=0.5, smooth=2):
    return scores.new_empty(tuple(scores.shape[:2]) + (2,), dtype=torch.float32)


@torch.library.custom_op("rti::relight_field", mutates_args=())
def relight_field(coef: torch.Tensor, light: torch.Tensor, basis: int = L.RTI_BASIS_PTM6, tile: int = 0,
                  planar: bool = False, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Relight under a light per pixel (``rti_relight_field``).  coef as ``light_scores``; light fp32 [H, W, 2]
    (tile = 0) or the tile field [Ty, Tx, 2] of ``light_field`` (tile 8, 16 or 32) -> [H, W] or [H, W, 3] in
    out_dtype (float32, int32 or uint8)."""
    api._require_cuda(coef, "coef")
    api._require_cuda(light, "light")
    _same_device(coef=coef, light=light)
    return api.relight_field(coef.contiguous(), light, basis, tile=tile if tile else None,
                             layout="planar" if planar else "pixel", out_dtype=out_dtype)


@relight_field.register_fake
def _(coef, light, basis=L.RTI_BASIS_PTM6, tile=0, planar=False, out_dtype=torch.float32):
    return coef.new_empty(_image_dims(coef, planar) + ((3,) if coef.dim() == 4 else ()), dtype=out_dtype)
