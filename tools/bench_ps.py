#!/usr/bin/env python3
"""Time rti_photometric_stereo at 3840x2160, N=100 on fp32 and uint8, grey and RGB stacks, all in
one process:

  ps_iters0 / ps_iters3          the one launch: normals, albedo, kind, res and kept (iters3: the resident form)
  ps_iters3_streaming            the same with RTI_KERNEL_ONE_LAUNCH: five reads of the stack instead of the LDS tile
  robust_normals_iters0 / _3     what the library offered before: rti_fit_shared_robust (PTM-6, coefficients, res and
                                 kept) followed by rti_ptm_normals (grey) or rti_rgb_normals (RGB) on the same stack
  relight                        the plain PTM-6 relight of one map, one direction: the yardstick of bytes per second

Every timed region is a run of back-to-back launches between two HIP events sized to last >= --region-ms; the
variants alternate region by region and the time is the median over the regions.  The byte model of the one launch
per pixel: C·N·sizeof(element) in + 12 (normal) + 12·C (albedo, res, kept) + 1 (kind) out; model_ms is that at the
bytes per second the plain relight (28 bytes per pixel) achieved in this run, x_model the time over it, x_robust the
time over robust_normals with the same iters (required <= 1 for iters = 0).  Prints one JSON line per variant; --out
also writes them to a file."""
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


def region_ms(fn, reps, stream):
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
    ap.add_argument("--lights", type=int, default=100)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ps: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    N, P = a.lights, a.height * a.width
    rng = np.random.default_rng(2)
    r, t = np.sqrt(rng.uniform(0.02, 0.8, N)), rng.uniform(0, 2 * np.pi, N)
    lu, lv = (r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32)
    A3 = torch.as_tensor(rti.ps_design(lu, lv), device=dev)
    A6 = torch.as_tensor(rti.design_matrix(lu, lv), device=dev)
    stream = torch.cuda.current_stream(dev)
    normals = torch.empty((P, 3), dtype=torch.float32, device=dev)
    kind = torch.empty(P, dtype=torch.uint8, device=dev)
    img = torch.empty(P, dtype=torch.float32, device=dev)
    luv = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)
    fallback = torch.zeros(1, dtype=torch.int32, device=dev)
    lines = []
    for C in (1, 3):
        coef = torch.empty((C, P, 6), dtype=torch.float32, device=dev)
        albedo = torch.empty((C, P), dtype=torch.float32, device=dev)
        res = torch.empty((C, P), dtype=torch.float32, device=dev)
        kept = torch.empty((C, P), dtype=torch.int32, device=dev)
        for name, dt in (("fp32", torch.float32), ("u8", torch.uint8)):
            I = torch.randint(0, 256, (C, N, P), device=dev, dtype=torch.uint8).to(dt)
            es = I.element_size()

            def ps(iters, kernel=0):
                return lambda: api.photometric_stereo_into(A3, I, normals, albedo, kind, res, kept, fallback, lo=1.0,
                                                           hi=254.0, min_lights=3, iters=iters, delta=5.0,
                                                           kernel=kernel)

            def robust_normals(iters):
                def call():
                    api.fit_robust_into(A6, I, coef, res, kept, fallback, k=6, lo=1.0, hi=254.0, min_lights=6,
                                        iters=iters, delta=5.0)
                    if C == 1:
                        api.ptm_normals_into(coef[0], normals, kind)
                    else:
                        api.rgb_normals_into(coef, normals, kind)
                return call

            def relight():
                L.check(rti.load().rti_relight(api._vp(coef), L.RTI_F32, L.RTI_BASIS_PTM6, P, L.RTI_COEF_PIXEL_MAJOR,
                                               api._vp(luv), 1, api._vp(img), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR,
                                               api._stream_of(coef)), "rti_relight")

            variants = {"relight": relight, "robust_normals_iters0": robust_normals(0), "ps_iters0": ps(0),
                        "robust_normals_iters3": robust_normals(3), "ps_iters3": ps(3),
                        "ps_iters3_streaming": ps(3, L.RTI_KERNEL_ONE_LAUNCH)}
            plan = int(L.lib().rti_photometric_stereo_plan(N, api._IN_DTYPES[dt], C, 3, 0))
            reps = {}
            for v, fn in variants.items():  # warm-up, and the launches per region
                fn()
                reps[v] = max(1, math.ceil(a.region_ms / max(region_ms(fn, 2, stream), 1e-3)))
            ms = {v: [] for v in variants}
            for _ in range(a.regions):
                for v, fn in variants.items():
                    ms[v].append(region_ms(fn, reps[v], stream))
            med = {v: float(np.median(ms[v])) for v in variants}
            relight_bps = 28.0 * P / (med["relight"] * 1e-3)
            ps_bytes = float(P) * (C * N * es + 12 + 12 * C + 1)
            for v in variants:
                ln = {"variant": v, "dtype": name, "channels": C, "config": f"{a.width}x{a.height} N={N}",
                      "launches_per_region": reps[v], "regions": a.regions, "median_ms": round(med[v], 4),
                      "min_ms": round(min(ms[v]), 4), "max_ms": round(max(ms[v]), 4)}
                if v == "relight":
                    ln["achieved_GBs"] = round(relight_bps / 1e9, 1)
                if v.startswith("ps_"):
                    iters = v[8]
                    ln.update({"resident_tile_px": plan if v == "ps_iters3" else 0, "model_bytes_per_px": ps_bytes / P,
                               "achieved_GBs": round(ps_bytes / (med[v] * 1e-3) / 1e9, 1),
                               "frac_of_8TBs": round(ps_bytes / (med[v] * 1e-3) / HBM_BPS, 4),
                               "model_ms": round(ps_bytes / relight_bps * 1e3, 4),
                               "x_model": round(med[v] / (ps_bytes / relight_bps * 1e3), 3),
                               "x_robust": round(med[v] / med["robust_normals_iters" + iters], 3)})
                lines.append(ln)
                print(json.dumps(ln), flush=True)
            del I
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
