"""rti -- MI355X-native PTM/HSH reflectance fitter (drop-in for the hot path of
bara96/Smartphone-based-RTI: analysis.py:196-411, interactive_relighting.py:11-39).

    import rti
    coef = rti.fit(I, lu, lv, basis="ptm")          # I: CUDA [N, H, W]
    img = rti.relight(coef, 0.3, -0.2)               # [H, W]
    coef, res, kept = rti.fit_robust(I, lu, lv, lo=1, hi=254, iters=3, delta=5.0)  # clipped samples left out
    n, albedo = rti.photometric_stereo(I, lu, lv, lo=1, hi=254)   # Lambertian normals [H, W, 3] from the stack itself
    n, albedo = rti.photometric_stereo_near(I, cams, refine=2)    # the same for a light near the object: a row per pixel

    acc = rti.FitAccumulator((H, W))                 # planes fed as they arrive, or a stack larger than HBM
    for frame, u, v in frames: acc.add(frame, u, v)
    coef, res = acc.solve()                          # any time: a preview, add() may go on

    n = rti.normals(coef)                            # [H, W, 3]: where each pixel's PTM peaks
    img = rti.relight_enhanced(coef, 0.3, -0.2, "specular", kd=0.4, ks=150, exp=75)

    sharp = rti.relight(rti.unsharp(coef, 2.0, 1.5), 0.3, -0.2)   # unsharp masking, for every light at once
    img = rti.shade_normals(rti.normals_unsharp(n, 2.0, 1.5), 0.3, -0.2)          # enhanced normals, shaded

    m = rti.fit_lrgb(Irgb, lu, lv)                   # Irgb: CUDA [3, N, H, W] -> LRGB PTM [H, W, 9]
    rgb = rti.relight_lrgb(m, 0.3, -0.2, out_dtype=torch.uint8)   # [H, W, 3] in one launch
    rti.write_ptm("object.ptm", m)                   # opens in a PTM viewer

    q = rti.quantise_lrgb(m)                         # the file's 9 bytes per pixel, made on the GPU
    rgb = rti.relight_lrgb8(q, 0.3, -0.2, out_dtype=torch.uint8)  # rendered from the bytes
    rti.write_ptm("object.ptm", q)                   # the same file, without the fp32 copy to the host
    q = rti.read_ptm("object.ptm", quantised=True)[1].to("cuda")  # a loaded file stays 9 bytes per pixel

    h = rti.quantise_hsh(rti.fit(Irgb, lu, lv, basis="hsh16"))    # RGB HSH-16 as 48 bytes per pixel
    rgb = rti.relight_hsh8(h, 0.3, -0.2, out_dtype=torch.uint8)   # one launch, from the bytes
    rti.write_rti("object.rti", h)                   # and back: rti.read_rti("object.rti", quantised=True)
    n, albedo = rti.hsh8_normals(h, return_peak=True)             # where each pixel's HSH function peaks
    img = rti.shade_normals(rti.normals_unsharp(n, 2.0, 1.5), 0.3, -0.2, albedo=albedo, ks=150, exp=75)

    p = rti.quantise_rgb(rti.fit(Irgb, lu, lv))      # RGB PTM as the 18 bytes per pixel of PTM_FORMAT_RGB
    rgb = rti.relight_rgb8(p, 0.3, -0.2, out_dtype=torch.uint8)   # one launch, from the bytes
    n = rti.rgb8_normals(p)                          # normals of the luminance, from the bytes
    rti.write_ptm("object.ptm", p)                   # and back: rti.read_ptm8("object.ptm")[1].to("cuda")

    rgb = rti.relight_rgb8_enhanced(p, 0.3, -0.2, "specular", kd=0.4, ks=150, exp=75, out_dtype=torch.uint8)
    rgb = rti.relight_lrgb8_enhanced(q, 0.3, -0.2, "diffuse_gain", gain=3.5)      # and relight_lrgb_enhanced(m, ...)

    c3 = rti.fit(Irgb, lu, lv)                       # the three fp32 maps themselves, [3, H, W, 6], in one launch each:
    rgb = rti.relight_rgb(c3, 0.3, -0.2, out_dtype=torch.uint8)   # [H, W, 3]; also basis="hsh9" / "hsh16"
    rgb = rti.relight_rgb_enhanced(c3, 0.3, -0.2, "diffuse_gain", gain=3.5)       # nothing quantised or compressed
    n = rti.rgb_normals(c3)                          # normals of the fp32 luminance

    h = rti.read_rti("object.rti", quantised=True)[1].to("cuda")  # a loaded HSH object: highlights under its normals
    n = rti.normals_unsharp(rti.hsh8_normals(h), 2.0, 1.5)        # searched and sharpened once per object
    rgb = rti.relight_hsh8_specular(h, n, 0.3, -0.2, kd=0.4, ks=150, exp=75, out_dtype=torch.uint8)  # one launch a frame
    rgb = rti.relight_hsh8_gain(h, n, 0.3, -0.2, gain=3.5, out_dtype=torch.uint8)  # diffuse gain about the same normals

    n, albedo = rti.photometric_stereo(I, lu, lv)    # normals to geometry: the least-squares height map, on the GPU
    z = rti.height_from_normals(n)                   # [H, W] in pixel units, zero mean, NaN where the normal is unusable

    img = rti.relight_multilight(coef, 0.3, -0.2)    # multi-light detail enhancement: each tile under its best light

Compute runs in HIP kernels of librti.so (include/rti.h); importing this
package does not touch the GPU.
"""
from . import _lib
from ._lib import RTIError, RTILibraryMissing
from .api import (BASES, FitAccumulator, apply_operator, basis_eval, basis_id, basis_operator, basis_terms,
                  design_matrix, fit, fit_accum_solve_into, fit_accumulate_into, fit_chunked, fit_residual, fit_robust, fit_robust_into, photometric_stereo, photometric_stereo_into, ps_design, photometric_stereo_near, photometric_stereo_near_into, ps_near_lights, fit_shared_into, fit_shared_residual_into, fit_with_residual,
                  gram_inverse,
                  interpolate_rbf, interpolate_rbf_perpixel, light_dirs, lsq_factors, pinv, q8_operator, h16_operator, rbf_operator,
                  normals, ptm_normals_into, relight, relight_enhanced, relight_enhanced_into, relight_frame,
                  gauss_taps, map_unsharp_into, normals_unsharp, shade_normals, shade_normals_into, unsharp,
                  fit_lrgb, gram, lrgb_from_rgb, lrgb_from_rgb_into, lrgb_luminance, relight_lrgb, relight_lrgb_into,
                  QuantisedLRGB, dequantise_lrgb, lrgb_qparams_into, lrgb_qparams_workspace, lrgb_quantise_into,
                  quantise_lrgb, relight_lrgb8, relight_lrgb8_into,
                  QuantisedHSH, dequantise_hsh, hsh_qparams_into, hsh_qparams_workspace, hsh_quantise_into,
                  quantise_hsh, relight_hsh8, relight_hsh8_into,
                  hsh8_normals, hsh8_normals_into, hsh_normals, hsh_normals_into, peak_grid_points, peak_table,
                  QuantisedRGB, dequantise_rgb, quantise_rgb, relight_rgb8, relight_rgb8_into, rgb8_normals,
                  rgb8_normals_into, rgb8_qparams_into, rgb8_qparams_workspace, rgb8_quantise_into,
                  relight_lrgb_enhanced, relight_lrgb_enhanced_into, relight_lrgb8_enhanced,
                  relight_lrgb8_enhanced_into, relight_rgb8_enhanced, relight_rgb8_enhanced_into,
                  relight_rgb, relight_rgb_into, relight_rgb_enhanced, relight_rgb_enhanced_into, rgb_normals,
                  rgb_normals_into,
                  relight_hsh_specular, relight_hsh_specular_into, relight_hsh8_specular, relight_hsh8_specular_into,
                  relight_hsh_gain, relight_hsh_gain_into, relight_hsh8_gain, relight_hsh8_gain_into,
                  height_from_normals, height_from_normals_into, height_levels, height_workspace,
                  light_candidates, light_scores, light_scores_into, light_field, light_field_into,
                  light_field_workspace, relight_field, relight_field_into, relight_multilight)
from .io import read_ptm, read_ptm8, read_rti, write_ptm, write_rti

__all__ = ["BASES", "FitAccumulator", "fit_accum_solve_into", "fit_accumulate_into", "fit_chunked",
           "RTIError", "RTILibraryMissing", "apply_operator", "basis_eval", "basis_id", "basis_operator",
           "basis_terms", "design_matrix", "fit", "fit_residual", "fit_robust", "fit_robust_into", "photometric_stereo",
           "photometric_stereo_into", "ps_design", "photometric_stereo_near", "photometric_stereo_near_into",
           "ps_near_lights", "fit_shared_into",
           "fit_shared_residual_into",
           "fit_with_residual", "gram_inverse", "interpolate_rbf", "interpolate_rbf_perpixel", "light_dirs",
           "lsq_factors", "pinv", "q8_operator", "h16_operator",
           "rbf_operator", "relight", "relight_frame", "normals", "ptm_normals_into", "relight_enhanced",
           "relight_enhanced_into", "gauss_taps", "map_unsharp_into", "normals_unsharp", "shade_normals",
           "shade_normals_into", "unsharp", "fit_lrgb", "gram", "lrgb_from_rgb", "lrgb_from_rgb_into",
           "lrgb_luminance", "relight_lrgb", "relight_lrgb_into", "QuantisedLRGB", "dequantise_lrgb",
           "lrgb_qparams_into", "lrgb_qparams_workspace", "lrgb_quantise_into", "quantise_lrgb", "relight_lrgb8",
           "relight_lrgb8_into", "QuantisedHSH", "dequantise_hsh", "hsh_qparams_into", "hsh_qparams_workspace",
           "hsh_quantise_into", "quantise_hsh", "relight_hsh8", "relight_hsh8_into", "hsh8_normals",
           "hsh8_normals_into", "hsh_normals", "hsh_normals_into", "peak_grid_points", "peak_table", "QuantisedRGB",
           "dequantise_rgb", "quantise_rgb", "relight_rgb8", "relight_rgb8_into", "rgb8_normals", "rgb8_normals_into",
           "rgb8_qparams_into", "rgb8_qparams_workspace", "rgb8_quantise_into", "relight_lrgb_enhanced",
           "relight_lrgb_enhanced_into", "relight_lrgb8_enhanced", "relight_lrgb8_enhanced_into",
           "relight_rgb8_enhanced", "relight_rgb8_enhanced_into", "relight_rgb", "relight_rgb_into",
           "relight_rgb_enhanced", "relight_rgb_enhanced_into", "rgb_normals", "rgb_normals_into",
           "relight_hsh_specular", "relight_hsh_specular_into", "relight_hsh8_specular",
           "relight_hsh8_specular_into", "relight_hsh_gain", "relight_hsh_gain_into", "relight_hsh8_gain",
           "relight_hsh8_gain_into", "height_from_normals", "height_from_normals_into", "height_levels",
           "height_workspace", "light_candidates", "light_scores", "light_scores_into", "light_field",
           "light_field_into", "light_field_workspace", "relight_field", "relight_field_into", "relight_multilight",
           "read_ptm", "read_ptm8", "write_ptm",
           "read_rti", "write_rti", "library_path", "load"]

__version__ = "0.1.0"


def library_path():
    return _lib.LIB_PATH


def load():
    """Load librti.so now (raises RTILibraryMissing if it was not built)."""
    return _lib.lib()
