#!/usr/bin/env python3
"""Time the 8-bit HSH kernels (rti_hsh8.hip) at 3840x2160 against the path the project had before
them, three rti.relight launches over the fp32 maps, all in one process, for k = 16 and k = 9:

  relight3_u8 / relight3_f32   rti_relight on each of the three fp32 [p][k] maps, one direction, uint8 / fp32 out
                               (three launches, three planar images: the comparison)
  hsh8_u8 / hsh8_f32           rti_relight_hsh8 from the 3k bytes per pixel, one direction, interleaved RGB out
  quantise_pair                rti_hsh_qparams followed by rti_hsh_quantise on the [3][p][k] fp32 maps

Method as tools/bench_lrgb8.py.  Cold reads: the launches rotate over --map-sets sets of maps and as many outputs.
Every timed window is a run of back-to-back launches between two HIP events sized to last >= 1 ms; the variants
alternate window by window and the time is the median over the windows.  Byte models per pixel: relight3_u8
3·(4k + 1), relight3_f32 3·(4k + 4), hsh8_u8 3k + 3, hsh8_f32 3k + 12, quantise_pair 12k + 12k + 3k -> fraction of
the 8 TB/s HBM peak.  Three sets of HSH-16 bytes (398 MB each) do not fit the 256 MiB Infinity Cache.
x_three_launch = hsh8 time over the three-launch time with the same output type (the byte model's ratio beside it),
x_bytes = time per model byte over relight3_f32's time per model byte from the same run (1.0 = rti_relight's time
per byte).  Prints one JSON line per variant; --out also writes them to a file."""
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
from bench_lrgb import window_ms  # noqa: E402
from rti import _lib as L  # noqa: E402
from rti import api  # noqa: E402

HBM_BPS = 8.0e12
THREE = {"hsh8_u8": "relight3_u8", "hsh8_f32": "relight3_f32"}


def model_bytes(k):
    return {"relight3_u8": 3.0 * (4 * k + 1), "relight3_f32": 3.0 * (4 * k + 4), "hsh8_u8": 3.0 * k + 3,
            "hsh8_f32": 3.0 * k + 12, "quantise_pair": 27.0 * k}


def synth_hsh_maps(P, k, seed, dev):
    """Three HSH maps [3, P, k]: a constant term that alone renders 40..240 grey levels, higher terms falling off
    with the order, each channel scaled by a colour in [0.5, 1.5]."""
    g = torch.Generator(device=dev).manual_seed(seed)
    m = torch.randn((3, P, k), device=dev, generator=g)
    order = torch.as_tensor([int(math.isqrt(j)) for j in range(k)], device=dev)
    m *= 40.0 / (1.0 + order) ** 2
    m[..., 0] = torch.rand((3, P), device=dev, generator=g) * 500.0 + 100.0
    return (m * (torch.rand((3, 1, 1), device=dev, generator=g) + 0.5)).contiguous()


def bench_k(k, a, dev, lines):
    basis, bid = f"hsh{k}", api.basis_id(f"hsh{k}")
    P, sets = a.height * a.width, max(1, a.map_sets)
    empty = lambda dt, *shape: [torch.empty(shape, dtype=dt, device=dev) for _ in range(sets)]  # noqa: E731
    maps = [synth_hsh_maps(P, k, 10 + i, dev) for i in range(sets)]
    qs = [rti.quantise_hsh(m, basis) for m in maps]  # the bytes the hsh8 variants read
    ws = empty(torch.uint8, api.hsh_qparams_workspace(P, basis))
    qp, c8 = empty(torch.float32, 2 * k), empty(torch.uint8, P, 3, k)
    out32, out8 = empty(torch.float32, 1, P, 3), empty(torch.uint8, 1, P, 3)
    pl32, pl8 = empty(torch.float32, 3, P), empty(torch.uint8, 3, P)
    luv1 = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = api._stream_of(luv1)
    lib = rti.load()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def relight3(i, planes, odt):  # the launches rti.relight makes per channel, on preallocated tensors
        for c in range(3):
            L.check(lib.rti_relight(api._vp(maps[i][c]), L.RTI_F32, bid, P, L.RTI_COEF_PIXEL_MAJOR, api._vp(luv1), 1,
                                    api._vp(planes[i][c]), odt, L.RTI_OUT_EVAL_MAJOR, sp), "rti_relight")

    def pair(i):
        api.hsh_qparams_into(maps[i], ws[i], qp[i], basis=basis)
        api.hsh_quantise_into(maps[i], qp[i], c8[i], basis=basis)

    variants = {
        "relight3_u8": rotating(lambda i: relight3(i, pl8, L.RTI_U8)),
        "relight3_f32": rotating(lambda i: relight3(i, pl32, L.RTI_F32)),
        "hsh8_u8": rotating(lambda i: api.relight_hsh8_into(qs[i].coef, qs[i].qparams, luv1, out8[i], basis=basis)),
        "hsh8_f32": rotating(lambda i: api.relight_hsh8_into(qs[i].coef, qs[i].qparams, luv1, out32[i], basis=basis)),
        "quantise_pair": rotating(pair),
    }
    model = {v: P * b for v, b in model_bytes(k).items()}
    reps = {}
    for v, fn in variants.items():  # warm-up, and the launches per window
        for _ in range(6):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 9, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    # the timed launches computed the real thing: the pair left quantise_hsh's bytes, and the image from the bytes
    # is the three-launch image to within the quantisation (a few grey levels at most)
    assert torch.equal(c8[0], qs[0].coef.reshape(P, 3, k)) and torch.equal(qp[0], qs[0].qparams)
    assert float((out32[0][0].T - pl32[0]).abs().max()) < 8.0 and float(pl32[0].max()) > 100.0
    per_byte = med["relight3_f32"] / model["relight3_f32"]
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height} RGB HSH-{k}, {sets} map sets",
              "launches_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
              "model_bytes_per_px": model[v] / P, "achieved_GBs": round(model[v] / (med[v] * 1e-3) / 1e9, 1),
              "frac_of_8TBs": round(model[v] / (med[v] * 1e-3) / HBM_BPS, 4),
              "x_bytes": round((med[v] / model[v]) / per_byte, 3)}
        if v in THREE:
            ln["x_three_launch"] = round(med[v] / med[THREE[v]], 3)
            ln["x_three_launch_byte_model"] = round(model[v] / model[THREE[v]], 3)
        lines.append(ln)
        print(json.dumps(ln), flush=True)


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
        sys.exit("bench_hsh8: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    lines = []
    for k in (16, 9):
        bench_k(k, a, dev, lines)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
