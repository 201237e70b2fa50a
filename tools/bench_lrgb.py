#!/usr/bin/env python3
"""Time the LRGB kernels (rti_lrgb_from_rgb / rti_relight_lrgb) at 3840x2160 against rti_relight,
all in one process:

  relight                    rti.relight, one direction, PTM-6 fp32 in, fp32 out (the yardstick)
  relight_x3                 three rti.relight launches over an 18-coefficient fit: a colour image without LRGB
  lrgb_f32_pixel / _planar   rti.relight_lrgb, one direction, fp32 RGB out, both map layouts
  lrgb_u8_pixel / _planar    the same with uint8 RGB out
  from_rgb_pixel / _planar   rti.lrgb_from_rgb, coefficient and LRGB maps in the same layout

Method as tools/bench_enhance.py.  Cold reads: the launches rotate over --map-sets sets of maps (each far past the
256 MiB Infinity Cache) and as many outputs.  Every timed window is a run of back-to-back launches between two HIP
events sized to last >= 1 ms; the variants alternate window by window and the time is the median over the windows.
Byte models per pixel: relight 24 + 4 = 28, relight_x3 3·28 = 84, lrgb_f32 36 + 12 = 48, lrgb_u8 36 + 3 = 39,
from_rgb 72 + 36 = 108 -> fraction of the 8 TB/s HBM peak; x_relight = time over relight's time, x_bytes = the same
with each side divided by its byte model (1.0 = relight's time per byte; the expectation is <= 1.10).  Prints one
JSON line per variant; --out also writes them to a file."""
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
MODEL = {"relight": 28.0, "relight_x3": 84.0, "lrgb_f32": 48.0, "lrgb_u8": 39.0, "from_rgb": 108.0}


def window_ms(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def synth_rgb_maps(P, seed, dev):
    """Three PTM-6 maps [3, P, 6]: one biquadratic with a maximum per pixel, scaled per channel by a colour in
    [0.5, 1.5]³ and perturbed by 2 %, so that the channels are nearly but not exactly proportional."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*(s or (P,)), device=dev, generator=g) * (hi - lo) + lo  # noqa: E731
    s1, s2, t = u(50, 200), u(50, 200), u(0, math.pi)
    c, s = torch.cos(t), torch.sin(t)
    a0, a1, a2 = -0.5 * (c * c * s1 + s * s * s2), -0.5 * (s * s * s1 + c * c * s2), -c * s * (s1 - s2)
    r, phi = u(0, 0.9), u(0, 2 * math.pi)
    u0, v0 = r * torch.cos(phi), r * torch.sin(phi)
    a3, a4 = -(2 * a0 * u0 + a2 * v0), -(a2 * u0 + 2 * a1 * v0)
    a5 = u(20, 250) - (a0 * u0 * u0 + a1 * v0 * v0 + a2 * u0 * v0 + a3 * u0 + a4 * v0)
    base = torch.stack([a0, a1, a2, a3, a4, a5], -1)
    return (u(0.5, 1.5, 3, P, 1) * base[None] * u(0.98, 1.02, 3, P, 6)).contiguous()


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
        sys.exit("bench_lrgb: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    P, sets = a.height * a.width, max(1, a.map_sets)
    rng = np.random.default_rng(0)
    rad, phi = np.sqrt(rng.uniform(0, 0.81, 24)), rng.uniform(0, 2 * np.pi, 24)
    gram = rti.gram((rad * np.cos(phi)).astype(np.float32), (rad * np.sin(phi)).astype(np.float32))
    rgb_pix = [synth_rgb_maps(P, 10 + i, dev) for i in range(sets)]            # [3, P, 6]
    rgb_pla = [m.transpose(1, 2).contiguous() for m in rgb_pix]                 # [3, 6, P]
    empty = lambda dt, *shape: [torch.empty(shape, dtype=dt, device=dev) for _ in range(sets)]  # noqa: E731
    lrgb_pix, lrgb_pla = empty(torch.float32, P, 9), empty(torch.float32, 9, P)
    for i in range(sets):  # the maps the relight variants read
        api.lrgb_from_rgb_into(rgb_pix[i], gram, lrgb_pix[i])
        api.lrgb_from_rgb_into(rgb_pla[i], gram, lrgb_pla[i], layout="planar", lrgb_layout="planar")
    out_pix, out_pla = empty(torch.float32, P, 9), empty(torch.float32, 9, P)
    img, img3 = empty(torch.float32, P), empty(torch.float32, 3, P)
    rgb32, rgb8 = empty(torch.float32, 1, P, 3), empty(torch.uint8, 1, P, 3)
    luv = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = api._stream_of(luv)
    lib = rti.load()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def relight_one(src, dst):  # the launch rti.relight makes, on preallocated tensors
        L.check(lib.rti_relight(api._vp(src), L.RTI_F32, L.RTI_BASIS_PTM6, P, L.RTI_COEF_PIXEL_MAJOR, api._vp(luv), 1,
                                api._vp(dst), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR, sp), "rti_relight")

    def relight_x3(i):
        for c in range(3):
            relight_one(rgb_pix[i][c], img3[i][c])

    variants = {
        "relight": rotating(lambda i: relight_one(rgb_pix[i][0], img[i])),
        "relight_x3": rotating(relight_x3),
        "lrgb_f32_pixel": rotating(lambda i: api.relight_lrgb_into(lrgb_pix[i], luv, rgb32[i])),
        "lrgb_f32_planar": rotating(lambda i: api.relight_lrgb_into(lrgb_pla[i], luv, rgb32[i], layout="planar")),
        "lrgb_u8_pixel": rotating(lambda i: api.relight_lrgb_into(lrgb_pix[i], luv, rgb8[i])),
        "lrgb_u8_planar": rotating(lambda i: api.relight_lrgb_into(lrgb_pla[i], luv, rgb8[i], layout="planar")),
        "from_rgb_pixel": rotating(lambda i: api.lrgb_from_rgb_into(rgb_pix[i], gram, out_pix[i])),
        "from_rgb_planar": rotating(lambda i: api.lrgb_from_rgb_into(rgb_pla[i], gram, out_pla[i], layout="planar",
                                                                     lrgb_layout="planar")),
    }
    model = {v: P * MODEL[v.rsplit("_", 1)[0] if v.endswith(("_pixel", "_planar")) else v] for v in variants}
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
