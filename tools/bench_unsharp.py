#!/usr/bin/env python3
"""Time the unsharp-masking kernel (rti_map_unsharp) at 3840x2160 against rti_relight for one
direction, all in one process:

  relight                       rti.relight of a PTM-6 fp32 map, one direction, fp32 out (the yardstick)
  unsharp_{pixel,planar}_s2     6-channel fp32 map, sigma = 2 (R = 6), both layouts
  unsharp_{pixel,planar}_s8     the same at sigma = 8 (R = 24)
  normals_unsharp_s2            3-channel map with renorm, sigma = 2, pixel-major

Cold reads as bench.py's relight config: the launches rotate over --map-sets map sets (3 x 199 MB is past the
256 MiB Infinity Cache) and as many outputs.  Every timed window is a run of back-to-back launches between two HIP
events sized to last >= 1 ms; the variants alternate window by window and the time is the median over the windows.
Byte models per pixel: 8·channels for the unsharp variants (the map read once and written once: the algorithmic
minimum, halo re-reads not counted), 24 in + 4 out = 28 for relight.  x_relight = time over relight's time, x_bytes =
the same with each side divided by its byte model (1.0 = relight's time per byte).  Prints one JSON line per variant;
--out also writes them to a file."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smartphone-based-rti_amd"))
import rti  # noqa: E402
from rti import _lib as L  # noqa: E402
from rti import api  # noqa: E402

HBM_BPS = 8.0e12


def window_ms(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--map-sets", type=int, default=3)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_unsharp: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    H, W, sets = a.height, a.width, max(1, a.map_sets)
    P = H * W
    g = torch.Generator(device=dev).manual_seed(7)
    rand = lambda *shape: torch.randn(shape, device=dev, generator=g) * 100.0  # noqa: E731
    pix = [rand(H, W, 6) for _ in range(sets)]
    pla = [m.permute(2, 0, 1).contiguous() for m in pix]
    nrm = [torch.nn.functional.normalize(rand(H, W, 3), dim=-1).contiguous() for _ in range(sets)]
    out6 = [torch.empty(H * W * 6, dtype=torch.float32, device=dev) for _ in range(sets)]
    img = [torch.empty(P, dtype=torch.float32, device=dev) for _ in range(sets)]
    luv = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = api._stream_of(pix[0])
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def relight(i):  # the launch rti.relight makes, on preallocated tensors
        L.check(rti.load().rti_relight(api._vp(pix[i]), L.RTI_F32, L.RTI_BASIS_PTM6, P, L.RTI_COEF_PIXEL_MAJOR,
                                       api._vp(luv), 1, api._vp(img[i]), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR, sp),
                "rti_relight")

    def unsharp(maps, layout, sigma, ch, renorm=False):
        return rotating(lambda i: api.map_unsharp_into(maps[i], out6[i][:P * ch].view(maps[i].shape), sigma=sigma,
                                                       amount=1.5, layout=layout, renorm=renorm))

    variants = {
        "relight": (rotating(relight), 28.0, None),
        "unsharp_pixel_s2": (unsharp(pix, "pixel", 2.0, 6), 48.0, 6),
        "unsharp_planar_s2": (unsharp(pla, "planar", 2.0, 6), 48.0, 6),
        "unsharp_pixel_s8": (unsharp(pix, "pixel", 8.0, 6), 48.0, 24),
        "unsharp_planar_s8": (unsharp(pla, "planar", 8.0, 6), 48.0, 24),
        "normals_unsharp_s2": (unsharp(nrm, "pixel", 2.0, 3, True), 24.0, 6),
    }
    reps = {}
    for v, (fn, _, _) in variants.items():  # warm-up, and the launches per window
        for _ in range(3):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 3, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, (fn, _, _) in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    lines = []
    for v, (_, bpp, R) in variants.items():
        model = P * bpp
        lines.append({"variant": v, "config": f"{W}x{H} fp32, {sets} map sets", "radius": R,
                      "launches_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
                      "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
                      "model_bytes_per_px": bpp, "achieved_GBs": round(model / (med[v] * 1e-3) / 1e9, 1),
                      "frac_of_8TBs": round(model / (med[v] * 1e-3) / HBM_BPS, 4),
                      "x_relight": round(med[v] / med["relight"], 3),
                      "x_bytes": round((med[v] / model) / (med["relight"] / (P * 28.0)), 3)})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
