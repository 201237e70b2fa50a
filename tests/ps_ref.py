"""fp64 restatement of rti_photometric_stereo's semantics (include/rti.h): robust_ref.fit_robust_ref per channel on
the 3-column design, then the normal / albedo / kind tail, in plain NumPy.  Imports nothing from the package.  Also
the synthetic Lambertian scene the tests share, and the conditions under which a rounding difference cannot flip a
decision of the fit or a kind."""
import numpy as np

from robust_ref import check_inputs, fit_robust_ref

LUMA = (0.299, 0.587, 0.114)
GOLDEN_ANGLE = 2.399963229728653


def ps_design(lu, lv):
    """fp64 [N, 3] = (lu, lv, sqrt(max(0, 1 − lu² − lv²))) from the fp32 values of lu, lv."""
    u, v = np.asarray(lu, np.float32).astype(np.float64), np.asarray(lv, np.float32).astype(np.float64)
    return np.stack([u, v, np.sqrt(np.maximum(0.0, 1.0 - u * u - v * v))], axis=1)


def ps_ref(A, I, lo=-np.inf, hi=np.inf, min_lights=3, iters=0, delta=0.0, weights=None):
    """A fp64 [N, 3], I [N, P] or [3, N, P] -> dict(normals [P, 3], albedo [C, P], kind [P], g [C, P, 3], res [C, P],
    kept [C, P], fallback_px, fits: the per-channel dicts of fit_robust_ref)."""
    I = np.asarray(I)
    I3 = I[None] if I.ndim == 2 else I
    C, N, P = I3.shape
    fits = [fit_robust_ref(A, I3[c], lo, hi, min_lights, iters, delta) for c in range(C)]
    gc = np.stack([f["coef"] for f in fits])  # [C, P, 3]
    if C == 1:
        g = gc[0].copy()
    else:
        w = np.asarray(LUMA if weights is None else weights, np.float32).astype(np.float64)
        g = w[2] * gc[2] + (w[1] * gc[1] + w[0] * gc[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2 + g[:, 2] ** 2)
        n = g / s[:, None]
    bad = ~np.isfinite(gc).all(axis=(0, 2))
    flat = ~bad & (s == 0)
    n[flat] = (0.0, 0.0, 1.0)
    kind = np.where(bad, 4, np.where(flat, 2, np.where(g[:, 2] < 0, 1, 0))).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        albedo = np.einsum("cpj,pj->cp", gc, n)
    n[bad], albedo[:, bad] = np.nan, np.nan
    return dict(normals=n, albedo=albedo, kind=kind, g=gc, s=s, res=np.stack([f["res"] for f in fits]),
                kept=np.stack([f["kept"] for f in fits]), fallback_px=sum(f["fallback_px"] for f in fits), fits=fits)


def check_ps_inputs(ref, I, lo=-np.inf, hi=np.inf, rank_fallback=(), margin=1e-3):
    """robust_ref.check_inputs per channel, and more: every successful solve's smallest pivot >= 1e-3·max diag G, no
    sample within `margin` of a bound, and for the pixels of kind 0 or 1 |g_z| >= 1e-3·s, so rounding cannot flip a
    kind.  NaN samples are on neither side of a bound.

    margin: 1e-3 wherever the scene allows it.  The window is compared on the input value: the kernel and the
    restatement compare the same fp32 sample, converted exactly to fp64, with the same fp32 bounds, so no rounding
    enters the comparison and any sample that is not the bound itself is on one side of it for both.  FP32_MARGIN,
    two ulps of an fp32 value below 256 (the number format's own resolution there), is the margin a case states
    when samples of its scene fall within 1e-3 of a bound."""
    I = np.asarray(I, np.float64)
    I3 = I[None] if I.ndim == 2 else I
    for f, Ic in zip(ref["fits"], I3):
        check_inputs(f, Ic, rank_fallback=rank_fallback)
        ok = np.isfinite(f["coef"]).all(-1)
        assert (f["min_pivot"][ok] >= 1e-3).all(), f["min_pivot"][ok].min()
        y = Ic[np.isfinite(Ic)]
        for bound in (lo, hi):
            if np.isfinite(bound):
                assert np.abs(y - bound).min() > margin, (bound, np.abs(y - bound).min())
    g = ref["kind"] <= 1
    gz = (ref["normals"] * ref["s"][:, None])[g, 2]
    assert (np.abs(gz) >= 1e-3 * ref["s"][g]).all()


FP32_MARGIN = 2.0 ** -15


# ---- the scene ---------------------------------------------------------------------------------------------------

def spiral_dirs(N=24):
    """N lights on the golden-angle spiral: r_i = 0.9·sqrt((i + ½)/N), θ_i = i·GOLDEN_ANGLE, as fp32."""
    i = np.arange(N)
    r, th = 0.9 * np.sqrt((i + 0.5) / N), i * GOLDEN_ANGLE
    return (r * np.cos(th)).astype(np.float32), (r * np.sin(th)).astype(np.float32)


def scene(P, N=24, rgb=False):
    """-> (lu, lv, A [N, 3], n_true [P, 3], albedo_true [C, P], I fp32 [N, P] or [3, N, P]).  P pixels with tilt
    0..60° and azimuth 0..6π linearly, albedo 150..400 (×1.0, 0.8, 0.6 per channel for RGB),
    I = clip(albedo·(n·l), 0, 255)."""
    lu, lv = spiral_dirs(N)
    A = ps_design(lu, lv)
    t = np.linspace(0.0, 1.0, P) if P > 1 else np.array([0.5])
    tilt, az = np.radians(60.0) * t, 6.0 * np.pi * t
    n = np.stack([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], axis=1)
    alb = (150.0 + 250.0 * t)[None] * (np.array([1.0, 0.8, 0.6])[:, None] if rgb else np.ones((1, 1)))
    I = np.clip(alb[:, None, :] * (A @ n.T)[None], 0.0, 255.0).astype(np.float32)
    return lu, lv, A, n, alb, (I if rgb else I[0])


def angle_deg(a, b):
    """The angle between unit vectors [..., 3], from the chord (accurate near 0)."""
    return np.degrees(2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.linalg.norm(a - b, axis=-1))))
