"""fp64 restatement of rti_photometric_stereo_near's semantics (include/rti.h) in plain NumPy: the design row of every
pixel and light as the header states it, then, one pixel at a time, ps_ref.ps_ref on that pixel's [N, 3] design
(robust_ref.fit_robust_ref per channel and the normal / albedo / kind tail, reused as they stand).  Imports nothing
from the package.  Also the near-light scene the tests share, the conditions under which a rounding difference cannot
flip a decision of the fit or a kind, and the CPU alternation normals -> height -> normals.

The scene (scene()): lights at centre + R·l with l on ps_ref.spiral_dirs(N) and R = 2·W, a Gaussian bump of amplitude
6 px and sigma 12 px at 64×64, both scaled by min(H, W)/64, mean removed, normals from the bump's analytic gradient,
albedo 150..400 over the pixel index (× 1.0, 0.8, 0.6 for RGB), I = clip(albedo·(n·d)·r0²/r³, 0, 255) with r0 = R.
No shape of the tests needed R or the amplitude adjusted to meet check_ps_near_inputs at the margins they state."""
import functools

import numpy as np

from ps_ref import check_ps_inputs, ps_design, ps_ref, spiral_dirs


def near_rows(lights, H, W, origin=(0.0, 0.0), height=None, z_offset=0.0, falloff=1, r0=1.0):
    """lights fp64 [N, 4] (x, y, z, scale) -> the rows a[p][n][3] of pixel p = y·W + x, fp64 [H·W, N, 3]:
    pos = (x0 + x, y0 + y, z_offset + h), h = height[p] where given and finite, else 0; d = L_n − pos; r² = d·d;
    a = s_n·d/r, times r0²/r² with fall-off.  r² = 0 or a non-finite light gives a NaN row."""
    lights = np.asarray(lights, np.float64)
    y, x = np.mgrid[0:H, 0:W]
    h = np.zeros(H * W) if height is None else np.asarray(height, np.float32).astype(np.float64).reshape(H * W)
    h = np.where(np.isfinite(h), h, 0.0)
    pos = np.stack([origin[0] + x.reshape(-1).astype(np.float64), origin[1] + y.reshape(-1).astype(np.float64),
                    z_offset + h], axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = lights[None, :, :3] - pos[:, None, :]
        r2 = (d * d).sum(-1)
        r = np.sqrt(r2)
        f = lights[None, :, 3] / r
        if falloff:
            f = f * (r0 * r0 / r2)
        a = f[..., None] * d
    a[~(np.isfinite(r2) & (r2 > 0.0) & np.isfinite(lights).all(-1)[None, :])] = np.nan
    return a


def ps_near_ref(lights, I, H, W, origin=(0.0, 0.0), height=None, z_offset=0.0, falloff=1, r0=1.0, lo=-np.inf,
                hi=np.inf, min_lights=3, iters=0, delta=0.0, weights=None):
    """I [N, P] or [3, N, P], P = H·W -> ps_ref's dict over all pixels (fits: per channel, the fields of
    fit_robust_ref concatenated over the pixels), and rows: near_rows."""
    I = np.asarray(I)
    I3 = I[None] if I.ndim == 2 else I
    C, N, P = I3.shape
    assert P == H * W
    rows = near_rows(lights, H, W, origin, height, z_offset, falloff, r0)
    with np.errstate(invalid="ignore"):
        px = [ps_ref(rows[p], I3[:, :, p:p + 1], lo, hi, min_lights, iters, delta, weights) for p in range(P)]
    out = {k: np.concatenate([r[k] for r in px], axis=0 if k in ("normals", "kind", "s") else 1)
           for k in ("normals", "albedo", "kind", "g", "s", "res", "kept")}
    out["fallback_px"] = sum(r["fallback_px"] for r in px)
    out["fits"] = [{k: np.concatenate([r["fits"][c][k] for r in px]) for k in ("coef", "res", "kept", "min_pivot",
                                                                               "fail_pivot")} for c in range(C)]
    out["rows"] = rows
    return out


def check_ps_near_inputs(ref, I, lo=-np.inf, hi=np.inf, rank_fallback=(), margin=1e-3):
    """ps_ref.check_ps_inputs' conditions with every pixel judged on its own design: the pivots reported per pixel
    are those of that pixel's G, so the same assertions hold them -- every successful solve's smallest pivot >=
    1e-3·max diag G, no sample within `margin` of a bound, |g_z| >= 1e-3·s for kinds 0 and 1.  A pixel whose rows are
    NaN (a light on it) has no successful solve and no failing pivot, and is judged by neither."""
    check_ps_inputs(ref, I, lo, hi, rank_fallback=rank_fallback, margin=margin)


# ---- the scene ---------------------------------------------------------------------------------------------------

def bump(H, W):
    """-> (h [H, W] zero-mean, n [H·W, 3]): the Gaussian bump at the image centre and its analytic unit normals
    (−h_x, −h_y, 1)/‖·‖ (x the column, y the row, as rti_height_from_normals reads them)."""
    f = min(H, W) / 64.0
    amp, sigma = 6.0 * f, 12.0 * f
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = x - 0.5 * (W - 1), y - 0.5 * (H - 1)
    h = amp * np.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma))
    hx, hy = -dx / (sigma * sigma) * h, -dy / (sigma * sigma) * h
    n = np.stack([-hx, -hy, np.ones_like(h)], -1).reshape(-1, 3)
    return h - h.mean(), n / np.linalg.norm(n, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def scene(H, W, N=24, rgb=False, origin=(0.0, 0.0), z_offset=0.0, falloff=1):
    """-> dict(lights [N, 4], lu, lv, r0, h [H, W], n [P, 3], albedo [C, P], I fp32 [N, P] or [3, N, P]): the scene of
    the module docstring; the surface sits at z_offset + h and is lit with fall-off (falloff=0: without)."""
    lu, lv = spiral_dirs(N)
    l = ps_design(lu, lv)
    R = 2.0 * W
    centre = np.array([origin[0] + 0.5 * (W - 1), origin[1] + 0.5 * (H - 1), z_offset])
    lights = np.concatenate([centre + R * l, np.ones((N, 1))], axis=1)
    h, n = bump(H, W)
    P = H * W
    t = np.linspace(0.0, 1.0, P) if P > 1 else np.array([0.5])
    alb = (150.0 + 250.0 * t)[None] * (np.array([1.0, 0.8, 0.6])[:, None] if rgb else np.ones((1, 1)))
    rows = near_rows(lights, H, W, origin, h, z_offset, falloff, R)  # [P, N, 3]
    shade = np.einsum("pnj,pj->np", rows, n)
    I = np.clip(alb[:, None, :] * shade[None], 0.0, 255.0).astype(np.float32)
    for a in (lights, h, n, alb, I):
        a.setflags(write=False)
    return dict(lights=lights, lu=lu, lv=lv, r0=R, h=h, n=n, albedo=alb, I=I if rgb else I[0])


# ---- the alternation ---------------------------------------------------------------------------------------------

def integrate(n_map):
    """The exact least-squares height of a normal map [H, W, 3] whose pixels are all valid: height_ref's Laplacian
    and right-hand side, solved directly (A + 11ᵀ/n is non-singular on a connected grid and its solution has zero
    mean)."""
    from height_ref import Problem

    prob = Problem(n_map)
    assert prob.valid.all()
    n = prob.A.shape[0]
    return np.linalg.solve(prob.A + 1.0 / n, prob.b.ravel()).reshape(prob.H, prob.W)


def refine_ref(sc, H, W, rounds, lo, hi, **kw):
    """Rounds 0..rounds of normals -> height -> normals on the scene `sc` from the plane -> [ps_near_ref dict per
    round], each with the height it used under "height"."""
    out, h = [], None
    for k in range(rounds + 1):
        ref = ps_near_ref(sc["lights"], sc["I"], H, W, height=h, r0=sc["r0"], lo=lo, hi=hi, **kw)
        ref["height"] = h
        out.append(ref)
        if k < rounds:
            h = integrate(ref["normals"].reshape(H, W, 3).astype(np.float32)).astype(np.float32)
    return out
