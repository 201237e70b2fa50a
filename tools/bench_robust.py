#!/usr/bin/env python3
"""Time rti_fit_shared_robust at 3840x2160, N=100, PTM-6 on fp32 and uint8 stacks:

  (a) iters=0 (window only, streaming) against rti.fit_with_residual's kernel on the same stack, same process;
  (b) iters=3 resident (AUTO) against iters=3 streaming (RTI_KERNEL_ONE_LAUNCH), same process.

Every timed region is a run of back-to-back launches between two HIP events sized to last >= 50 ms; the
variants alternate region by region and the per-launch time is the median over the regions.  Algorithmic
bytes per launch = es·P·N (one stack read) + 4·P·k (coef) + 4·P (res) [+ 4·P (kept)] -> fraction of the
8 TB/s HBM peak; fp64 FMA-class operations per launch are counted from the shapes (k(k+1)/2 + 2k + 2 per sample
and Gram pass) against the 78.6 TFLOP/s vector fp64 peak.  Prints one JSON line per variant; --out also writes
them to a file."""
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
FP64_FLOPS = 78.6e12


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
        sys.exit("bench_robust: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    N, P, k = a.lights, a.height * a.width, 6
    rng = np.random.default_rng(2)
    r, t = np.sqrt(rng.uniform(0.02, 0.8, N)), rng.uniform(0, 2 * np.pi, N)
    lu, lv = (r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32)
    A = torch.as_tensor(rti.design_matrix(lu, lv), device=dev)
    U, W = (torch.as_tensor(x, device=dev) for x in rti.lsq_factors(lu, lv))
    coef = torch.empty((1, P, k), dtype=torch.float32, device=dev)
    res = torch.empty((1, P), dtype=torch.float32, device=dev)
    kept = torch.empty((1, P), dtype=torch.int32, device=dev)
    fallback = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    gram = k * (k + 1) // 2 + 2 * k + 2  # fp64 FMA-class ops per sample of a Gram pass (wa, G, b, wy, q)
    lines = []
    for name, dt in (("fp32", torch.float32), ("u8", torch.uint8)):
        I = torch.randint(0, 256, (1, N, P), device=dev, dtype=torch.uint8).to(dt)
        es = I.element_size()

        def robust(iters, kernel):
            return lambda: api.fit_robust_into(A, I, coef, res, kept, fallback, k=k, lo=1.0, hi=254.0, min_lights=k,
                                               iters=iters, delta=5.0, kernel=kernel)

        variants = {
            "fit_with_residual": lambda: api.fit_shared_residual_into(U, W, I, coef, res, None, k=k),
            "robust_iters0": robust(0, 0),
            "robust_iters3_resident": robust(3, 0),
            "robust_iters3_streaming": robust(3, L.RTI_KERNEL_ONE_LAUNCH),
        }
        plan = int(L.lib().rti_fit_shared_robust_plan(k, N, api._IN_DTYPES[dt], 3, 0))
        reps = {}
        for v, fn in variants.items():  # warm-up, and the launches per region
            fn()
            reps[v] = max(1, math.ceil(a.region_ms / max(region_ms(fn, 2, stream), 1e-3)))
        ms = {v: [] for v in variants}
        for _ in range(a.regions):
            for v, fn in variants.items():
                ms[v].append(region_ms(fn, reps[v], stream))
        fallback_px = int(fallback.item())
        for v in variants:
            med = float(np.median(ms[v]))
            out_bytes = 4.0 * P * k + 4.0 * P + (0.0 if v == "fit_with_residual" else 4.0 * P)
            reads = 5 if v == "robust_iters3_streaming" else 1  # window + 3 IRLS + residual passes
            alg = float(es) * P * N * reads + out_bytes
            if v == "fit_with_residual":
                per = k + 1  # Uᵀ I and ‖I‖²
            elif v == "robust_iters0":
                per = gram
            else:  # window pass, 3 IRLS passes (residual + weight + Gram), the last residual pass
                per = (gram - 1) + 3 * (gram - 1 + k + 1) + (k + 1)
            fma = float(P) * N * per
            lines.append({"variant": v, "dtype": name, "config": f"{a.width}x{a.height} N={N} PTM-6",
                          "resident_tile_px": plan if v == "robust_iters3_resident" else 0,
                          "launches_per_region": reps[v], "regions": a.regions, "median_ms": round(med, 4),
                          "min_ms": round(min(ms[v]), 4), "max_ms": round(max(ms[v]), 4), "hbm_bytes": alg,
                          "achieved_GBs": round(alg / (med * 1e-3) / 1e9, 1),
                          "frac_of_8TBs": round(alg / (med * 1e-3) / HBM_BPS, 4), "fp64_fma_ops": fma,
                          "frac_of_fp64_peak": round(2.0 * fma / (med * 1e-3) / FP64_FLOPS, 4),
                          "fallback_px_total": fallback_px})
            print(json.dumps(lines[-1]), flush=True)
        del I
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
