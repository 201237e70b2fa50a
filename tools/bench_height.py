#!/usr/bin/env python3
"""Time rti_height_from_normals at 3840x2160 on a synthetic relief under three masks (full rectangle, inscribed disc,
3 % scattered invalid pixels) with both preconditioners, rtol = 1e-6, all in one process:

  solve        the whole call: set-up, hierarchy, iterations until the criterion (or max_iters), gauge, output
  per_iter     (time of 40 iterations − time of 8) / 32, with rtol = 0 so that neither run stops early
  setup        the call with max_iters = 0: mask, gradients, b, weights, first residual, gauge, output; for the
               multigrid it includes the hierarchy, so hierarchy_build_ms = setup(multigrid) − setup(jacobi)
  relight      the plain PTM-6 relight of one map, one direction: the yardstick of bytes per second

The entry synchronises the stream, so a region is a run of back-to-back calls between two HIP events sized to last
>= --region-ms; the variants alternate region by region and the time is the median over the regions.  The byte model
of one iteration counts the fp64 vectors read and written over the dense grid (H·W cells: the kernels run over it,
invalid cells carry zeros): A·p 2, the z / r update 6, the direction 3, r·s 2 -- 13 with either preconditioner; the
V-cycle adds 12 on the pixel grid (pre-smoothing 2, restriction 2, prolongation 2, two sweeps 3 each) and a third of
that again for the coarse grids.  The int32 weights and degrees are counted beside them (weights_bytes_per_px).
model_ms is the model at the bytes per second the plain relight (28 bytes per pixel) achieved in this run.  Prints one
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

VECTORS = {"jacobi": 13.0, "multigrid": 13.0 + 12.0 * 4.0 / 3.0}
WEIGHT_BYTES = {"jacobi": 12.0 + 4.0, "multigrid": 12.0 + (12.0 + 12.0 + 4.0 + 24.0) * 4.0 / 3.0}
PROTOTYPE_ITERS = {"full": 9, "disc": 9, "scattered": 12}  # the NumPy prototype at 512², rtol 1e-8 (full: also 1024²)


def region_ms(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def relief_normals(H, W, dev):
    """Unit normals of a sum of low-frequency waves with a fine texture, slopes below 1; fp32 [H, W, 3]."""
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                          torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    zx, zy = torch.zeros_like(x), torch.zeros_like(x)
    for fx, fy, amp, ph in ((0.003, 0.002, 0.5, 0.3), (0.011, -0.017, 0.25, 1.1), (0.09, 0.05, 0.12, 2.0),
                            (0.31, -0.23, 0.05, 0.7)):
        c = amp * torch.cos(fx * x + fy * y + ph)
        zx += c * fx / max(abs(fx), abs(fy))
        zy += c * fy / max(abs(fx), abs(fy))
    n = torch.stack([-zx, -zy, torch.ones_like(zx)], -1)
    return (n / n.norm(dim=-1, keepdim=True)).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--region-ms", type=float, default=60.0)
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--jacobi-max-iters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_height: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    H, W = a.height, a.width
    P = H * W
    stream = torch.cuda.current_stream(dev)
    base = relief_normals(H, W, dev)
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    gen = torch.Generator(device=dev).manual_seed(5)
    masks = {"full": torch.ones((H, W), dtype=torch.bool, device=dev),
             "disc": (y - (H - 1) / 2) ** 2 + (x - (W - 1) / 2) ** 2 <= (min(H, W) / 2) ** 2,
             "scattered": torch.rand((H, W), device=dev, generator=gen) >= 0.03}
    coef = torch.rand((P, 6), device=dev)
    img = torch.empty(P, device=dev)
    luv = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)

    def relight():
        L.check(rti.load().rti_relight(api._vp(coef), L.RTI_F32, L.RTI_BASIS_PTM6, P, L.RTI_COEF_PIXEL_MAJOR,
                                       api._vp(luv), 1, api._vp(img), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR,
                                       api._stream_of(coef)), "rti_relight")

    ws = {pc: api.height_workspace(H, W, pc, dev) for pc in VECTORS}
    height = torch.empty((H, W), device=dev)
    lines = []
    for mname, m in masks.items():
        n = torch.where(m[..., None], base, torch.full_like(base, float("nan"))).contiguous()
        stats, limit = {}, {"multigrid": a.max_iters, "jacobi": a.jacobi_max_iters}

        def call(pc, rtol, iters):
            st = np.zeros(6)
            return lambda: (api.height_from_normals_into(n, ws[pc], height, rtol=rtol, max_iters=iters, precond=pc,
                                                         stats=st), stats.__setitem__((pc, rtol, iters), st.copy()))

        variants = {"relight": relight}
        for pc in VECTORS:
            variants.update({f"{pc}_solve": call(pc, 1e-6, limit[pc]), f"{pc}_setup": call(pc, 1e-6, 0),
                             f"{pc}_iters8": call(pc, 0.0, 8), f"{pc}_iters40": call(pc, 0.0, 40)})
        reps = {}
        for v, fn in variants.items():  # warm-up, and the calls per region
            fn()
            reps[v] = max(1, math.ceil(a.region_ms / max(region_ms(fn, 1, stream), 1e-3)))
        ms = {v: [] for v in variants}
        for _ in range(a.regions):
            for v, fn in variants.items():
                ms[v].append(region_ms(fn, reps[v], stream))
        med = {v: float(np.median(ms[v])) for v in variants}
        relight_bps = 28.0 * P / (med["relight"] * 1e-3)
        lines.append({"variant": "relight", "mask": mname, "config": f"{W}x{H}", "median_ms": round(med["relight"], 4),
                      "achieved_GBs": round(relight_bps / 1e9, 1), "calls_per_region": reps["relight"]})
        for pc in VECTORS:
            st = stats[(pc, 1e-6, limit[pc])]
            per_iter = (med[f"{pc}_iters40"] - med[f"{pc}_iters8"]) / 32.0
            model_bytes = (VECTORS[pc] * 8.0 + WEIGHT_BYTES[pc]) * P
            ln = {"variant": pc, "mask": mname, "config": f"{W}x{H}", "rtol": 1e-6, "max_iters": limit[pc],
                  "levels": api.height_levels(H, W) if pc == "multigrid" else 1,
                  "valid_pixels": int(st[4]), "iterations_run": int(st[0]), "iteration_met": int(st[1]),
                  "converged": bool(st[1] >= 0), "final_rel_residual": float(st[2]), "true_rel_residual": float(st[3]),
                  "solve_ms": round(med[f"{pc}_solve"], 3), "solve_min_ms": round(min(ms[f"{pc}_solve"]), 3),
                  "solve_max_ms": round(max(ms[f"{pc}_solve"]), 3), "setup_ms": round(med[f"{pc}_setup"], 3),
                  "per_iter_ms": round(per_iter, 4), "regions": a.regions, "calls_per_region": reps[f"{pc}_solve"],
                  "vectors_per_iter": round(VECTORS[pc], 2), "weights_bytes_per_px": round(WEIGHT_BYTES[pc], 1),
                  "model_bytes_per_px": round(model_bytes / P, 1),
                  "achieved_GBs": round(model_bytes / (per_iter * 1e-3) / 1e9, 1),
                  "model_ms": round(model_bytes / relight_bps * 1e3, 4),
                  "x_model": round(per_iter / (model_bytes / relight_bps * 1e3), 3)}
            if pc == "multigrid":
                ln["hierarchy_build_ms"] = round(med["multigrid_setup"] - med["jacobi_setup"], 3)
                ln["prototype_iterations_512"] = PROTOTYPE_ITERS[mname]
            lines.append(ln)
        for ln in lines[-3:]:
            print(json.dumps(ln), flush=True)
        del n
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
