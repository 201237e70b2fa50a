"""Reference for rti_relight_rgb / rti_relight_rgb_enhanced / rti_rgb_normals (include/rti.h),
assembled from the references the project already has and adding no arithmetic of its own:

    normals           normals_ref.normals_ref of rgb8_ref.luminance (fp32) of the three maps
    enhanced modes    enhance_rgb_ref.rgb_enhanced_ref of the three maps, then enhance_rgb_ref.convert
    plain relight     the fp32 FMA chain of the oracle as tests/test_gpu_rgb8.py obtains it: rti.relight of each
                      map, stacked (the one function here that needs the GPU)

Also the seeded maps and the far-stride plans tests/test_gpu_rgb.py uses, so that tests/test_rgb_abi.py can check
the plans on the CPU as tests/test_far_ref.py checks far_ref.PLANS."""
import functools

import numpy as np

import far_ref as fr
from enhance_rgb_ref import convert, peaked_rgb, rgb_enhanced_ref
from hsh8_ref import finite_hsh
from normals_ref import normals_ref
from rgb8_ref import LUMA, luminance

F32 = np.float32
TERMS = {"ptm": 6, "hsh9": 9, "hsh16": 16}


def rgb_normals_ref(m, weights=None):
    """m fp32 [3, P, 6] -> (n fp32 [P, 3], kind uint8 [P], peak fp32 [P]) as rti_rgb_normals stores them."""
    r = normals_ref(luminance(m, LUMA if weights is None else weights))
    with np.errstate(all="ignore"):
        return r["n"].astype(F32), r["kind"], r["peak"].astype(F32)


def rgb_enhanced(m, lu, lv, mode, dtype_name, **kw):
    """m fp32 [3, P, 6] -> the stored image [P, 3] of rti_relight_rgb_enhanced in "float32", "int32" or "uint8"."""
    return convert(rgb_enhanced_ref(m, lu, lv, mode, **kw), dtype_name)


def relight_rgb_ref(rti, coef, lu, lv, basis, out_dtype, layout="pixel"):
    """coef: device fp32 [3, P, k] / [3, k, P] -> rti.relight of each map, interleaved: [E, P, 3] (or [P, 3])."""
    import torch

    return torch.stack([rti.relight(coef[c], lu, lv, basis=basis, layout=layout, out_dtype=out_dtype)
                        for c in range(3)], -1)


# ---- seeded maps ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nonfinite_rgb(P):
    """enhance_rgb_ref.peaked_rgb (interior maxima, maxima outside the disc, minima) with a handful of pixels that
    carry NaN, +inf or -inf in ONE channel: kinds 0, 1, 2 and 4 all occur for P >= 255 -> fp32 [3, P, 6], never
    written."""
    m = peaked_rgb(P).copy()
    rng = np.random.default_rng(4100 + P)
    bad = rng.choice(P, min(P, max(1, min(9, P // 8))), replace=False) if P > 1 else np.array([], int)
    for i, p in enumerate(bad):
        m[i % 3, p, rng.integers(0, 6)] = (np.nan, np.inf, -np.inf)[i % 3]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def nonfinite_hsh(P, k):
    """hsh8_ref.finite_hsh with the same handful of non-finite pixels -> fp32 [3, P, k], never written."""
    m = finite_hsh(P, k, 8100 + P)
    rng = np.random.default_rng(4200 + P)
    bad = rng.choice(P, min(P, max(1, min(9, P // 8))), replace=False) if P > 1 else np.array([], int)
    for i, p in enumerate(bad):
        m[i % 3, p, rng.integers(0, k)] = (np.nan, np.inf, -np.inf)[i % 3]
    m.setflags(write=False)
    return m


def bad_pixels(m):
    """the pixels of m [3, P, 6] with a non-finite value in some channel"""
    return ~np.isfinite(m).all(axis=(0, 2))


# ---- far strides ----------------------------------------------------------------------------------------------------

def far_maps_plan(k, variant):
    """far_ref's channel plan for three fp32 maps of k terms at far_ref.P16: channel 1 starts past 2^32 bytes and
    channel 2 past 2^31 elements (three channels each past 2^31 elements would be 24 GiB and more once the base
    absorbs the signed truncation: over far_ref.CAP_BYTES)."""
    return fr.channel_plan(f"rgbmaps-farchan-k{k}-P{fr.P16}-{variant}", 4, 3, 1, fr.P16 * k, variant)
