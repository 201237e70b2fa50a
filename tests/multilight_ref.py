"""NumPy restatement of the multi-light entries of include/rti.h (rti_multilight.hip), importing nothing
from the package.  It builds on relight_ref (the exact fp32 chain and basis) and hsh_normals_ref.luminance.

    scores_ref         rti_light_scores: per tile and candidate the exactly rounded quotients.  A candidate's values are
                       relight_ref's (the kernel must reproduce them bit for bit), a difference of two of them is exact
                       in fp64 and its square is one rounded fp64 product, as in the kernel; the sums over a tile are
                       math.fsum's, the correctly rounded sum, and the quotient is one division.
    field_ref          rti_light_field, operation by operation in Python floats (IEEE doubles, no contraction): there
                       is no sum whose order could differ, so a kernel must match it exactly.
    bilinear_ref       the tile field at every pixel, in fp64.
    relight_field_ref  rti_relight_field from per-pixel lights: basis32 per pixel, the fma32 chain, convert.

Also the seeded maps, candidates and shapes the CPU and the GPU tests share."""
import functools
import math

import numpy as np

from hsh_normals_ref import luminance
from relight_ref import TERMS, basis32, const_column, convert, dirs, fma32, maps, relight_ref

F32, F64 = np.float32, np.float64
BASES = ("ptm", "hsh9", "hsh16")
TILES = (8, 16, 32)
MAX_CANDIDATES = 64
# (H, W, T): one pixel; exactly one tile; partial tiles in both axes at two tile edges; H < T; a last tile one pixel wide
# and one pixel high (no pairs); T = 32 with a partial row and column of tiles
SHAPES = ((1, 1, 8), (8, 8, 8), (19, 37, 8), (19, 37, 16), (5, 64, 16), (17, 33, 16), (33, 70, 32))
CANDIDATE_COUNTS = (1, 17, 64)


def tile_grid(H, W, T):
    return -(-H // T), -(-W // T)


def candidates(E):
    """E candidate lights as host fp64 [E, 2]: relight_ref.dirs' (a seeded point, the pole, the axes, the rim, a point
    outside the disc, then seeded points)."""
    lu, lv = dirs(E)
    return np.ascontiguousarray(np.stack([lu, lv], -1))


@functools.lru_cache(maxsize=None)
def image_maps(H, W, k, C):
    """fp32 [C, H·W, k], never written: relight_ref.maps with its planted rows (NaN, ±inf, the int32 edges), a seed per
    channel.  The planted pixels are the same in every channel."""
    m = np.stack([maps(H * W, k, 900 + 7 * c) for c in range(C)])
    m.setflags(write=False)
    return m


def luminance_map(m, weights=None):
    """[C, P, k] -> the fp32 map the search runs on."""
    m = np.asarray(m, F32)
    return m[0] if m.shape[0] == 1 else luminance(m, weights)


# ---- rti_light_scores ------------------------------------------------------------------------------------------------

def scores_ref(m, H, W, T, luv, basis, weights=None):
    """m fp32 [C, H·W, k] -> dict: scores fp64 [Ty, Tx, E, 2], count int32 [Ty, Tx], pairs int [Ty, Tx] (n_S) and
    mean_abs fp64 [Ty, Tx, E] (the mean |V| of the usable pixels, what the brightness bound scales by)."""
    lum = luminance_map(m, weights)
    luv = np.asarray(luv, F64)
    E = luv.shape[0]
    V = relight_ref(lum, luv[:, 0], luv[:, 1], basis).astype(F64).reshape(E, H, W)
    usable = np.isfinite(lum).all(-1).reshape(H, W)
    Ty, Tx = tile_grid(H, W, T)
    scores = np.zeros((Ty, Tx, E, 2), F64)
    mean_abs = np.zeros((Ty, Tx, E), F64)
    count = np.zeros((Ty, Tx), np.int32)
    pairs = np.zeros((Ty, Tx), np.int64)
    for ty in range(Ty):
        for tx in range(Tx):
            ys, xs = slice(ty * T, min((ty + 1) * T, H)), slice(tx * T, min((tx + 1) * T, W))
            u = usable[ys, xs]
            horizontal, vertical = u[:, :-1] & u[:, 1:], u[:-1] & u[1:]
            nS, nP = int(horizontal.sum() + vertical.sum()), int(u.sum())
            count[ty, tx], pairs[ty, tx] = nP, nS
            for e in range(E):
                v = V[e, ys, xs]
                with np.errstate(all="ignore"):
                    dh = (v[:, 1:] - v[:, :-1])[horizontal]  # exact
                    dv = (v[1:] - v[:-1])[vertical]
                    squares = np.concatenate([dh * dh, dv * dv])  # one rounding each
                if nS:
                    scores[ty, tx, e, 0] = math.fsum(squares.tolist()) / nS
                if nP:
                    scores[ty, tx, e, 1] = math.fsum(v[u].tolist()) / nP
                    mean_abs[ty, tx, e] = math.fsum(np.abs(v[u]).tolist()) / nP
    return dict(scores=scores, count=count, pairs=pairs, mean_abs=mean_abs)


def scores_within_bound(got, ref):
    """The header's bound: |sharp − ref| <= (n_S + 2)·2^-53·ref and |bright − ref| <= (n_P + 1)·2^-53·mean|V|.
    -> (ok, the worst error in units of its bound)."""
    u = 2.0 ** -53
    got = np.asarray(got, F64)
    bound_s = (ref["pairs"][..., None] + 2) * u * ref["scores"][..., 0]
    bound_b = (ref["count"][..., None].astype(F64) + 1) * u * ref["mean_abs"]
    err_s = np.abs(got[..., 0] - ref["scores"][..., 0])
    err_b = np.abs(got[..., 1] - ref["scores"][..., 1])
    ok = bool((err_s <= bound_s).all() and (err_b <= bound_b).all())
    with np.errstate(all="ignore"):
        worst = max(float(np.nanmax(np.where(bound_s > 0, err_s / bound_s, err_s))),
                    float(np.nanmax(np.where(bound_b > 0, err_b / bound_b, err_b))))
    return ok, worst


# ---- rti_light_field -------------------------------------------------------------------------------------------------

def field_ref(scores, count, luv, ws, wb, lu0, lv0, smooth):
    """scores fp64 [Ty, Tx, E, 2], count [Ty, Tx] -> (field fp32 [Ty, Tx, 2], choice int32 [Ty, Tx])."""
    scores, luv = np.asarray(scores, F64), np.asarray(luv, F64)
    Ty, Tx, E, _ = scores.shape
    ws, wb = float(ws), float(wb)
    choice = np.full((Ty, Tx), -1, np.int32)
    f = [[None] * Tx for _ in range(Ty)]
    for ty in range(Ty):
        for tx in range(Tx):
            sharp, bright = scores[ty, tx, :, 0].tolist(), scores[ty, tx, :, 1].tolist()
            smax = bmax = 0.0
            for e in range(E):  # raised from 0 with >: a NaN never raises it
                smax = sharp[e] if sharp[e] > smax else smax
                bmax = bright[e] if bright[e] > bmax else bmax
            best, top = -1, 0.0
            if int(count[ty, tx]) != 0:
                for e in range(E):
                    sn = sharp[e] / smax if smax > 0.0 else 0.0
                    bn = bright[e] / bmax if bmax > 0.0 else 0.0
                    a, b = ws * sn, wb * bn
                    score = a + b
                    if score == score and (best < 0 or score > top):
                        best, top = e, score
            choice[ty, tx] = best
            f[ty][tx] = (float(lu0), float(lv0)) if best < 0 else (float(luv[best, 0]), float(luv[best, 1]))
    for _ in range(int(smooth)):
        g = [[None] * Tx for _ in range(Ty)]
        for ty in range(Ty):
            for tx in range(Tx):
                au = av = wsum = 0.0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        y, x = ty + dy, tx + dx
                        if not (0 <= y < Ty and 0 <= x < Tx):
                            continue
                        wt = float((2 - abs(dy)) * (2 - abs(dx)))
                        au = au + wt * f[y][x][0]
                        av = av + wt * f[y][x][1]
                        wsum = wsum + wt
                g[ty][tx] = (au / wsum, av / wsum)
        f = g
    return np.array(f, F64).reshape(Ty, Tx, 2).astype(F32), choice


# ---- rti_relight_field -----------------------------------------------------------------------------------------------

def bilinear_ref(field, H, W, T):
    """field fp32 [Ty, Tx, 2] -> (lu, lv) fp64 [H·W] each: bilinear between the tile centres."""
    field = np.asarray(field, F32).astype(F64)
    Ty, Tx, _ = field.shape
    assert (Ty, Tx) == tile_grid(H, W, T)

    def axis(n, tiles):
        t = (np.arange(n).astype(F64) - F64(T - 1) / F64(2.0)) / F64(T)
        t = np.minimum(np.maximum(t, F64(0.0)), F64(tiles - 1))
        i0 = np.floor(t).astype(np.int64)
        return i0, np.minimum(i0 + 1, tiles - 1), t - i0.astype(F64)

    i0, i1, a = axis(W, Tx)
    j0, j1, b = axis(H, Ty)
    a, b = a[None, :], b[:, None]
    out = []
    with np.errstate(all="ignore"):
        for c in range(2):
            g = field[..., c]
            f00, f10 = g[j0][:, i0], g[j0][:, i1]
            f01, f11 = g[j1][:, i0], g[j1][:, i1]
            top = f00 + a * (f10 - f00)
            bottom = f01 + a * (f11 - f01)
            out.append((top + b * (bottom - top)).reshape(-1))
    return out[0], out[1]


def relight_field_ref(m, lu, lv, basis, dtype_name="float32"):
    """m fp32 [C, P, k], a light per pixel (lu, lv [P], fp64 or fp32; cast to fp32 as the kernel casts them) ->
    [P] (C = 1) or [P, C] in dtype_name: per channel relight_ref's chain at the pixel's own basis row; a light with a
    non-finite component gives NaN, converted like any other value."""
    m = np.asarray(m, F32)
    C, P, k = m.shape
    assert k == TERMS[basis]
    lu32, lv32 = np.asarray(lu).astype(F32), np.asarray(lv).astype(F32)
    bad = ~(np.isfinite(lu32) & np.isfinite(lv32))
    B = basis32(lu32.astype(F64), lv32.astype(F64), basis)  # [P, k]; the fp64 round trip of an fp32 value is exact
    out = np.empty((P, C), F32)
    with np.errstate(all="ignore"):
        for c in range(C):
            acc = m[c, :, 0] * B[:, 0]
            for j in range(1, k):
                acc = fma32(m[c, :, j], B[:, j], acc)
            out[:, c] = np.where(bad, F32(np.nan), acc)
    out = convert(out, dtype_name)
    return out[:, 0] if C == 1 else out


def same_bits(a, b):
    """Equal arrays of one dtype, a NaN equal to any NaN (a NaN's payload is not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(np.ascontiguousarray(a)[~nan].view(view), np.ascontiguousarray(b)[~nan].view(view)))


def constant_term_maps(H, W, k, value=3.25):
    """fp32 [1, H·W, k]: only the constant column is non-zero, so every candidate gives the same image."""
    basis = {6: "ptm", 9: "hsh9", 16: "hsh16"}[k]
    rng = np.random.default_rng(5)
    m = np.zeros((1, H * W, k), F32)
    m[0, :, const_column(basis)] = (value + rng.uniform(0.0, 50.0, H * W)).astype(F32)
    return m
