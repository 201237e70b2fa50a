#!/usr/bin/env python3
"""Time the 8-bit LRGB kernels (rti_lrgb8.hip) at 3840x2160 against rti_relight and the fp32-map
rti_relight_lrgb, all in one process:

  relight              rti.relight, one direction, PTM-6 fp32 in, fp32 out (the yardstick)
  lrgb_u8 / lrgb_f32   rti.relight_lrgb from the [p][9] fp32 map, one direction, uint8 / fp32 RGB out
  lrgb8_u8 / lrgb8_f32 rti.relight_lrgb8 from the 9 bytes per pixel, one direction
  lrgb8_u8_e8 / lrgb8_f32_e8   the same, eight directions in one launch
  quantise_pair        rti_lrgb_qparams followed by rti_lrgb_quantise on the [p][9] fp32 map

Method as tools/bench_lrgb.py.  Cold reads: the launches rotate over --map-sets sets of maps and as many outputs.
Every timed window is a run of back-to-back launches between two HIP events sized to last >= 1 ms; the variants
alternate window by window and the time is the median over the windows.  Byte models per pixel: relight 24 + 4 = 28,
lrgb_u8 36 + 3 = 39, lrgb_f32 36 + 12 = 48, lrgb8_u8 9 + 3 = 12, lrgb8_f32 9 + 12 = 21, with eight directions
9 + 8·3 = 33 and 9 + 8·12 = 105, quantise_pair 36 + 36 + 9 = 81 -> fraction of the 8 TB/s HBM peak.  Three sets of
9-byte maps (75 MB each) fit the 256 MiB Infinity Cache together, so the lrgb8 reads are cold to L2 but may be served
by that cache; --map-sets raises the rotation past it.  x_relight = time over relight's time, x_bytes = the same
per byte of the model (1.0 = relight's time per byte), x_fp32_map = lrgb8 time over the fp32-map kernel's time with
the same output (the byte model says 12/39 and 21/48).  host_quantise_ms: today's path on one map, the .cpu() copy
plus rti.io._ptm_quantise and the colour bytes, timed with the host clock (median of --host-reps).  Prints one JSON
line per variant; --out also writes them to a file."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smartphone-based-rti_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rti  # noqa: E402
from bench_lrgb import synth_rgb_maps, window_ms  # noqa: E402
from rti import _lib as L  # noqa: E402
from rti import api  # noqa: E402
from rti.io import _ptm_quantise  # noqa: E402

HBM_BPS = 8.0e12
MODEL = {"relight": 28.0, "lrgb_u8": 39.0, "lrgb_f32": 48.0, "lrgb8_u8": 12.0, "lrgb8_f32": 21.0,
         "lrgb8_u8_e8": 33.0, "lrgb8_f32_e8": 105.0, "quantise_pair": 81.0}
FP32_MAP = {"lrgb8_u8": "lrgb_u8", "lrgb8_f32": "lrgb_f32"}
BYTE_RATIO = {"lrgb8_u8": 12.0 / 39.0, "lrgb8_f32": 21.0 / 48.0}


def host_quantise_ms(lrgb, reps):
    """Today's write_ptm up to the payload: the map to the host, then the colour bytes and _ptm_quantise."""
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = lrgb.cpu().numpy().astype(np.float64)
        chroma = m[..., 6:]
        fin = chroma[np.isfinite(chroma)]
        s = float(fin.max()) if fin.size and fin.max() > 0 else 1.0
        rgb = np.where(np.isnan(chroma), 0, np.clip(np.rint(255.0 * chroma / s), 0, 255)).astype(np.uint8)
        raw, _, _ = _ptm_quantise(m[..., :6] * s)
        times.append((time.perf_counter() - t0) * 1e3)
        del m, rgb, raw
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--map-sets", type=int, default=3)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lrgb8: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    P, sets = a.height * a.width, max(1, a.map_sets)
    rng = np.random.default_rng(0)
    rad, phi = np.sqrt(rng.uniform(0, 0.81, 24)), rng.uniform(0, 2 * np.pi, 24)
    gram = rti.gram((rad * np.cos(phi)).astype(np.float32), (rad * np.sin(phi)).astype(np.float32))
    empty = lambda dt, *shape: [torch.empty(shape, dtype=dt, device=dev) for _ in range(sets)]  # noqa: E731
    coef6, lrgb = empty(torch.float32, P, 6), empty(torch.float32, P, 9)
    for i in range(sets):
        rgb_maps = synth_rgb_maps(P, 10 + i, dev)
        api.lrgb_from_rgb_into(rgb_maps, gram, lrgb[i])
        coef6[i].copy_(rgb_maps[0])
        del rgb_maps
    qs = [rti.quantise_lrgb(m) for m in lrgb]  # the maps the lrgb8 variants read
    ws = empty(torch.uint8, api.lrgb_qparams_workspace(P))
    qp, c8, r8 = empty(torch.float64, 13), empty(torch.uint8, P, 6), empty(torch.uint8, P, 3)
    img = empty(torch.float32, P)
    out32, out8 = empty(torch.float32, 8, P, 3), empty(torch.uint8, 8, P, 3)
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

    def relight_one(i):  # the launch rti.relight makes, on preallocated tensors
        L.check(lib.rti_relight(api._vp(coef6[i]), L.RTI_F32, L.RTI_BASIS_PTM6, P, L.RTI_COEF_PIXEL_MAJOR,
                                api._vp(luv1), 1, api._vp(img[i]), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR, sp), "rti_relight")

    def lrgb8(i, luv, out):
        api.relight_lrgb8_into(qs[i].coef, qs[i].rgb, qs[i].qparams, luv, out[i][:luv.shape[0]])

    def pair(i):
        api.lrgb_qparams_into(lrgb[i], ws[i], qp[i])
        api.lrgb_quantise_into(lrgb[i], qp[i], c8[i], r8[i])

    variants = {
        "relight": rotating(relight_one),
        "lrgb_u8": rotating(lambda i: api.relight_lrgb_into(lrgb[i], luv1, out8[i][:1])),
        "lrgb_f32": rotating(lambda i: api.relight_lrgb_into(lrgb[i], luv1, out32[i][:1])),
        "lrgb8_u8": rotating(lambda i: lrgb8(i, luv1, out8)),
        "lrgb8_f32": rotating(lambda i: lrgb8(i, luv1, out32)),
        "lrgb8_u8_e8": rotating(lambda i: lrgb8(i, luv8, out8)),
        "lrgb8_f32_e8": rotating(lambda i: lrgb8(i, luv8, out32)),
        "quantise_pair": rotating(pair),
    }
    model = {v: P * MODEL[v] for v in variants}
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
    # the device pair left the same bytes as quantise_lrgb did: the timed launches computed the real thing
    assert torch.equal(c8[0], qs[0].coef) and torch.equal(r8[0], qs[0].rgb) and torch.equal(qp[0], qs[0].qparams)
    host_ms = host_quantise_ms(lrgb[0], a.host_reps) if a.host_reps > 0 else None
    lines = []
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height} PTM-6, {sets} map sets",
              "launches_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
              "model_bytes_per_px": model[v] / P, "achieved_GBs": round(model[v] / (med[v] * 1e-3) / 1e9, 1),
              "frac_of_8TBs": round(model[v] / (med[v] * 1e-3) / HBM_BPS, 4),
              "x_relight": round(med[v] / med["relight"], 3),
              "x_bytes": round((med[v] / model[v]) / (med["relight"] / model["relight"]), 3)}
        if v in FP32_MAP:
            ln["x_fp32_map"] = round(med[v] / med[FP32_MAP[v]], 3)
            ln["x_fp32_map_byte_model"] = round(BYTE_RATIO[v], 3)
        if v == "quantise_pair" and host_ms is not None:
            ln["host_quantise_ms"] = round(host_ms, 1)
            ln["x_host"] = round(host_ms / med[v], 1)
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
