#!/usr/bin/env python3
"""Time the PTM normals and enhanced-relight kernels (rti_ptm_normals / rti_relight_enhanced) at
3840x2160 on PTM-6 fp32 maps against rti_relight for one direction, all in one process:

  relight                 rti.relight, one direction, fp32 out (the yardstick)
  diffuse_gain, specular  rti.relight_enhanced, fp32 out
  normals_pixel / planar  rti.normals with kind and peak, both normal layouts

Cold reads as bench.py's relight config: the launches rotate over --map-sets coefficient-map sets (3 x 199 MB is
past the 256 MiB Infinity Cache) and as many outputs.  Every timed window is a run of back-to-back launches between
two HIP events sized to last >= 1 ms; the variants alternate window by window and the time is the median over the
windows.  Byte models per pixel: 24 in + 4 out = 28 for relight and the enhanced modes, 24 + 12 + 1 (kind) + 4
(peak) = 41 for normals -> fraction of the 8 TB/s HBM peak; x_relight = time over relight's time, x_bytes = the
same with each side divided by its byte model (1.0 = relight's bytes per second).  Prints one JSON line per
variant; --out also writes them to a file."""
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


def synth_maps(P, seed, dev):
    """PTM-6 maps with a maximum in 85 % of the pixels (a third of those outside the disc) and none in the rest."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda lo, hi: torch.rand(P, device=dev, generator=g) * (hi - lo) + lo  # noqa: E731
    s1, s2, t = u(50, 200), u(50, 200), u(0, math.pi)
    sign = torch.where(u(0, 1) < 0.85, -1.0, 1.0)
    c, s = torch.cos(t), torch.sin(t)
    a0, a1, a2 = 0.5 * sign * (c * c * s1 + s * s * s2), 0.5 * sign * (s * s * s1 + c * c * s2), sign * c * s * (s1 - s2)
    r, phi = u(0, 1.5), u(0, 2 * math.pi)
    u0, v0 = r * torch.cos(phi), r * torch.sin(phi)
    a3, a4 = -(2 * a0 * u0 + a2 * v0), -(a2 * u0 + 2 * a1 * v0)
    a5 = u(20, 250) - (a0 * u0 * u0 + a1 * v0 * v0 + a2 * u0 * v0 + a3 * u0 + a4 * v0)
    return torch.stack([a0, a1, a2, a3, a4, a5], -1).contiguous()


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
        sys.exit("bench_enhance: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    P, sets = a.height * a.width, max(1, a.map_sets)
    maps = [synth_maps(P, 10 + i, dev) for i in range(sets)]
    f32 = lambda *shape: [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(sets)]  # noqa: E731
    img, npix, npla, peak = f32(P), f32(P, 3), f32(3, P), f32(P)
    kind = [torch.empty(P, dtype=torch.uint8, device=dev) for _ in range(sets)]
    luv = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = api._stream_of(maps[0])
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def relight(i):  # the launch rti.relight makes, on preallocated tensors
        L.check(rti.load().rti_relight(api._vp(maps[i]), L.RTI_F32, L.RTI_BASIS_PTM6, P, L.RTI_COEF_PIXEL_MAJOR,
                                       api._vp(luv), 1, api._vp(img[i]), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR, sp),
                "rti_relight")

    variants = {
        "relight": rotating(relight),
        "diffuse_gain": rotating(lambda i: api.relight_enhanced_into(maps[i], 0.3, -0.45, "diffuse_gain", img[i], gain=3.0)),
        "specular": rotating(lambda i: api.relight_enhanced_into(maps[i], 0.3, -0.45, "specular", img[i], kd=0.4,
                                                                  ks=150.0, exp=75)),
        "normals_pixel": rotating(lambda i: api.ptm_normals_into(maps[i], npix[i], kind[i], peak[i])),
        "normals_planar": rotating(lambda i: api.ptm_normals_into(maps[i], npla[i], kind[i], peak[i],
                                                                   normal_layout="planar")),
    }
    model = {v: P * (41.0 if v.startswith("normals") else 28.0) for v in variants}
    reps = {}
    for v, fn in variants.items():  # warm-up, and the launches per window
        for _ in range(10):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 20, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    lines = []
    for v in variants:
        lines.append({"variant": v, "config": f"{a.width}x{a.height} PTM-6 fp32, {sets} map sets",
                      "launches_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
                      "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
                      "model_bytes_per_px": model[v] / P, "achieved_GBs": round(model[v] / (med[v] * 1e-3) / 1e9, 1),
                      "frac_of_8TBs": round(model[v] / (med[v] * 1e-3) / HBM_BPS, 4),
                      "x_relight": round(med[v] / med["relight"], 3),
                      "x_bytes": round((med[v] / model[v]) / (med["relight"] / model["relight"]), 3)})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
