#!/usr/bin/env python3
"""Time the chunked shared fit (rti_fit_accumulate / rti_fit_accum_solve) at 3840x2160, N=100, PTM-6 on fp32 and
uint8 stacks, all in one process:

  (a) accumulate alone at B = 1, 8, 25, 100 planes per call, with and without init;
  (b) solve alone;
  (c) the whole fit as chunks of 25 (the first with init) plus solve;
  (d) rti.fit_with_residual's kernel on the same stack.

Every timed region is a run of back-to-back launches between two HIP events sized to last >= 50 ms; the variants
alternate region by region and the time is the median over the regions.  The byte model per pixel: accumulate
B·es in + 8(k+1) state in (not with init) + 8(k+1) state out; solve 8(k+1) in + 4k + 4 out; the one-pass fit
N·es in + 4k + 4 out -> fraction of the 8 TB/s HBM peak.  x_model = the time over what the line's own byte model
takes at the fraction of peak (d) reaches in this run.  Prints one JSON line per variant; --out also writes them
to a file."""
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
    ap.add_argument("--chunk", type=int, default=25, help="planes per call of the whole fit (c)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_accum: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    N, P, k = a.lights, a.height * a.width, 6
    rng = np.random.default_rng(2)
    r, t = np.sqrt(rng.uniform(0.02, 0.8, N)), rng.uniform(0, 2 * np.pi, N)
    lu, lv = (r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32)
    A = torch.as_tensor(rti.design_matrix(lu, lv), device=dev)
    ginv = torch.as_tensor(rti.gram_inverse(lu, lv), device=dev)
    U, W = (torch.as_tensor(x, device=dev) for x in rti.lsq_factors(lu, lv))
    coef = torch.empty((1, P, k), dtype=torch.float32, device=dev)
    res = torch.empty((1, P), dtype=torch.float32, device=dev)
    partial = torch.zeros((1, int(rti.load().rti_fit_shared_residual_blocks(P))), dtype=torch.float64, device=dev)
    state = torch.zeros((1, k + 1, P), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    sbytes = 8.0 * (k + 1)
    edges = list(range(0, N, a.chunk)) + [N]
    lines = []
    for name, dt in (("fp32", torch.float32), ("u8", torch.uint8)):
        I = torch.randint(0, 256, (1, N, P), device=dev, dtype=torch.uint8).to(dt)
        es = float(I.element_size())

        def acc(lo, hi, init):
            R, chunk = A[lo:hi].contiguous(), I[:, lo:hi]  # a leading run of planes: contiguous
            return lambda: api.fit_accumulate_into(R, chunk, state, k=k, init=init)

        def solve():
            api.fit_accum_solve_into(ginv, state, coef, res, k=k, n_lights=N)

        parts = [acc(lo, hi, lo == 0) for lo, hi in zip(edges[:-1], edges[1:])]

        def whole():
            for fn in parts:
                fn()
            solve()

        variants, model = {}, {}
        for B in (1, 8, 25, 100):
            if B > N:
                continue
            for init in (True, False):
                v = f"accumulate_B{B}_{'init' if init else 'add'}"
                variants[v] = acc(0, B, init)
                model[v] = P * (B * es + (0.0 if init else sbytes) + sbytes)
        variants["solve"] = solve
        model["solve"] = P * (sbytes + 4.0 * k + 4.0)
        variants["chunked_fit"] = whole
        model["chunked_fit"] = P * (N * es + (2 * len(parts) - 1) * sbytes) + model["solve"]
        variants["fit_with_residual"] = lambda: api.fit_shared_residual_into(U, W, I, coef, res, partial, k=k)
        model["fit_with_residual"] = P * (N * es + 4.0 * k + 4.0)

        reps = {}
        for v, fn in variants.items():  # warm-up, and the launches per region
            fn()
            reps[v] = max(1, math.ceil(a.region_ms / max(region_ms(fn, 2, stream), 1e-3)))
        ms = {v: [] for v in variants}
        for _ in range(a.regions):
            for v, fn in variants.items():
                ms[v].append(region_ms(fn, reps[v], stream))
        med = {v: float(np.median(ms[v])) for v in variants}
        frac = {v: model[v] / (med[v] * 1e-3) / HBM_BPS for v in variants}
        for v in variants:
            lines.append({"variant": v, "dtype": name, "config": f"{a.width}x{a.height} N={N} PTM-6",
                          "calls_per_region": reps[v], "regions": a.regions, "median_ms": round(med[v], 4),
                          "min_ms": round(min(ms[v]), 4), "max_ms": round(max(ms[v]), 4), "model_bytes": model[v],
                          "achieved_GBs": round(model[v] / (med[v] * 1e-3) / 1e9, 1),
                          "frac_of_8TBs": round(frac[v], 4),
                          "x_model": round(frac["fit_with_residual"] / frac[v], 3)})
            print(json.dumps(lines[-1]), flush=True)
        lines.append({"variant": "chunked_fit / fit_with_residual", "dtype": name, "chunks": len(parts),
                      "measured": round(med["chunked_fit"] / med["fit_with_residual"], 3),
                      "byte_model": round(model["chunked_fit"] / model["fit_with_residual"], 3)})
        print(json.dumps(lines[-1]), flush=True)
        del I, parts, variants
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
