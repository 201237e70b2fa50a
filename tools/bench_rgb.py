#!/usr/bin/env python3
"""Time the one-pass kernels over three fp32 RGB maps (rti_rgb.hip) at 3840x2160 against the
routes they replace and the entries next to them, all in one process:

  relight                          rti.relight, one direction, PTM-6 fp32 in, fp32 out (the time-per-byte yardstick)
  rgb_<b>_u8 / rgb_<b>_f32         rti_relight_rgb, one direction, uint8 / fp32 RGB out; <b> = ptm, hsh9, hsh16
  rgb_<b>_u8_e8 / rgb_<b>_f32_e8   the same, eight directions in one launch
  three_<b>_u8 / three_<b>_f32     three rti_relight launches over the same maps and torch.stack(..., -1) into a
                                   preallocated [P, 3] tensor: the same image without the entry
  rgb_dg / rgb_spec                rti_relight_rgb_enhanced, diffuse gain / specular, fp32 out
  rgb8_dg / rgb8_spec              rti_relight_rgb8_enhanced of the quantised maps, fp32 out
  grey_dg / grey_spec              rti_relight_enhanced of one map, fp32 out
  rgb_normals                      rti_rgb_normals, normals only
  rgb8_normals                     rti_rgb8_normals of the quantised maps, normals only
  ptm_normals                      rti_ptm_normals of a resident fp32 luminance map [p][6], normals only

Method as tools/bench_rgb8.py.  Cold reads: the launches rotate over --map-sets sets of maps and as many outputs.
Every timed window is a run of back-to-back launches between two HIP events sized to last >= 1 ms; the variants
alternate window by window and the time is the median over the windows.  Byte models per pixel, k terms: one pass
12k + 3·s per direction (s = 4 or 1), three launches 3·(4k + s) + 2·3·s for the interleave (3·s read, 3·s written);
enhanced and normals 72 + 12 from fp32 maps, 18 + 12 from bytes, 24 + 4 (grey) and 24 + 12 (ptm_normals) from one
map -> fraction of the 8 TB/s HBM peak.  x_relight = time over relight's time, x_bytes = the same per byte of the
model (1.0 = relight's time per byte), x_three = the one-pass time over the three-launch route's, next to the byte
model's ratio.  Prints one JSON line per variant; --out also writes them to a file."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smartphone-based-rti_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rti  # noqa: E402
from bench_lrgb import synth_rgb_maps, window_ms  # noqa: E402
from rti import _lib as L  # noqa: E402
from rti import api  # noqa: E402

HBM_BPS = 8.0e12
BASES = {"ptm": (L.RTI_BASIS_PTM6, 6), "hsh9": (L.RTI_BASIS_HSH9, 9), "hsh16": (L.RTI_BASIS_HSH16, 16)}
KW = dict(gain=3.5, kd=0.4, ks=150.0, exp=75)
LU, LV = 0.3, -0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--map-sets", type=int, default=3)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rgb: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    P, sets = a.height * a.width, max(1, a.map_sets)
    empty = lambda dt, *shape: [torch.empty(shape, dtype=dt, device=dev) for _ in range(sets)]  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(7)
    maps = {"ptm": [synth_rgb_maps(P, 10 + i, dev) for i in range(sets)]}
    for b in ("hsh9", "hsh16"):  # HSH maps of a lit surface: a large constant term, smaller higher ones
        k = BASES[b][1]
        fall = torch.tensor([120.0] + [30.0 / (1 + j) for j in range(1, k)], device=dev)
        maps[b] = [(torch.randn((3, P, k), device=dev, generator=g) * 0.2 + 1.0) * fall for _ in range(sets)]
    qs = [rti.quantise_rgb(m) for m in maps["ptm"]]
    w = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float32, device=dev)
    lum = []
    for m in maps["ptm"]:
        lum.append(((w[0] * m[0] + w[1] * m[1]) + w[2] * m[2]).contiguous())
    img, plane32, plane8 = empty(torch.float32, P), empty(torch.float32, 3, P), empty(torch.uint8, 3, P)
    out32, out8 = empty(torch.float32, 8, P, 3), empty(torch.uint8, 8, P, 3)
    nrm = empty(torch.float32, P, 3)
    luv8 = torch.as_tensor(np.stack([np.linspace(-0.6, 0.6, 8), np.linspace(0.5, -0.5, 8)], -1), device=dev)
    luv1 = luv8[:1].contiguous()
    stream = torch.cuda.current_stream(dev)
    sp = api._stream_of(luv1)
    lib = rti.load()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def relight_map(coef, b, out, odt):  # the launch rti.relight makes, on preallocated tensors
        L.check(lib.rti_relight(api._vp(coef), L.RTI_F32, BASES[b][0], P, L.RTI_COEF_PIXEL_MAJOR, api._vp(luv1), 1,
                                api._vp(out), odt, L.RTI_OUT_EVAL_MAJOR, sp), "rti_relight")

    def three(b, i, planes, out):
        odt = L.RTI_F32 if planes[i].dtype == torch.float32 else L.RTI_U8
        for c in range(3):
            relight_map(maps[b][i][c], b, planes[i][c], odt)
        torch.stack((planes[i][0], planes[i][1], planes[i][2]), -1, out=out[i][0])

    def one_pass(b, i, luv, out):
        api.relight_rgb_into(maps[b][i], luv, out[i][:luv.shape[0]], basis=b)

    variants = {"relight": rotating(lambda i: relight_map(maps["ptm"][i][0], "ptm", img[i], L.RTI_F32))}
    model = {"relight": 28.0}
    three_of = {}
    for b, (_, k) in BASES.items():
        for tag, out, planes, s in (("u8", out8, plane8, 1), ("f32", out32, plane32, 4)):
            variants[f"rgb_{b}_{tag}"] = rotating(lambda i, b=b, out=out: one_pass(b, i, luv1, out))
            model[f"rgb_{b}_{tag}"] = 12.0 * k + 3 * s
            variants[f"rgb_{b}_{tag}_e8"] = rotating(lambda i, b=b, out=out: one_pass(b, i, luv8, out))
            model[f"rgb_{b}_{tag}_e8"] = 12.0 * k + 8 * 3 * s
            variants[f"three_{b}_{tag}"] = rotating(lambda i, b=b, out=out, planes=planes: three(b, i, planes, out))
            model[f"three_{b}_{tag}"] = 3.0 * (4 * k + s) + 6 * s
            three_of[f"rgb_{b}_{tag}"] = f"three_{b}_{tag}"
    for tag, mode in (("dg", "diffuse_gain"), ("spec", "specular")):
        variants[f"rgb_{tag}"] = rotating(
            lambda i, mode=mode: api.relight_rgb_enhanced_into(maps["ptm"][i], LU, LV, mode, out32[i][0], **KW))
        variants[f"rgb8_{tag}"] = rotating(
            lambda i, mode=mode: api.relight_rgb8_enhanced_into(qs[i].coef, qs[i].qparams, LU, LV, mode, out32[i][0],
                                                                **KW))
        variants[f"grey_{tag}"] = rotating(
            lambda i, mode=mode: api.relight_enhanced_into(maps["ptm"][i][0], LU, LV, mode, img[i], **KW))
        model.update({f"rgb_{tag}": 84.0, f"rgb8_{tag}": 30.0, f"grey_{tag}": 28.0})
    variants["rgb_normals"] = rotating(lambda i: api.rgb_normals_into(maps["ptm"][i], nrm[i]))
    variants["rgb8_normals"] = rotating(lambda i: api.rgb8_normals_into(qs[i].coef, qs[i].qparams, nrm[i]))
    variants["ptm_normals"] = rotating(lambda i: api.ptm_normals_into(lum[i], nrm[i]))
    model.update({"rgb_normals": 84.0, "rgb8_normals": 30.0, "ptm_normals": 36.0})

    reps = {}
    for v, fn in variants.items():  # warm-up, and the launches per window
        for _ in range(6):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 10, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    # the timed launches computed the real thing: on set 0 the one-pass image is the three-launch image, bit for
    # bit, and the normals are those of the luminance map
    for b in BASES:
        for out, planes in ((out8, plane8), (out32, plane32)):
            three(b, 0, planes, out)
            want = out[0][0].clone()
            one_pass(b, 0, luv8, out)
            assert torch.equal(out[0][0].view(torch.uint8), want.view(torch.uint8)) and bool(want.any()), b
    api.rgb_normals_into(maps["ptm"][0], nrm[0])
    assert torch.equal(nrm[0].view(torch.int32), rti.normals(lum[0]).view(torch.int32))
    lines = []
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height} RGB fp32 maps, {sets} map sets",
              "launches_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
              "model_bytes_per_px": model[v], "achieved_GBs": round(P * model[v] / (med[v] * 1e-3) / 1e9, 1),
              "frac_of_8TBs": round(P * model[v] / (med[v] * 1e-3) / HBM_BPS, 4),
              "x_relight": round(med[v] / med["relight"], 3),
              "x_bytes": round((med[v] / model[v]) / (med["relight"] / model["relight"]), 3)}
        if v in three_of:
            ln["x_three"] = round(med[v] / med[three_of[v]], 3)
            ln["x_three_byte_model"] = round(model[v] / model[three_of[v]], 3)
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
