#!/usr/bin/env python3
"""Time rti_photometric_stereo_near at 3840x2160, N=100 on fp32 and uint8, grey and RGB stacks, iters 0 and 3, each
against rti_photometric_stereo on the same stack in the same process:

  far_iters0 / far_iters3        rti_photometric_stereo: the shared design (iters3: the resident form)
  near_iters0 / near_iters3      rti_photometric_stereo_near with fall-off and a height map: a row per pixel and light
  refine2 (grey fp32 only)       one refine=2 run split into its launches: near, height, near, height, near

Every timed region is a run of back-to-back launches between two HIP events sized to last >= --region-ms; the
variants alternate region by region and the time is the median over the regions.  x_far is the near time over the
far time with the same iters; samples_per_ns counts pixel·light·channel·pass samples (passes: 1 for iters 0, iters + 2
otherwise; fallback passes run on no pixel of this stack's window).  Prints one JSON line per variant; --out also
writes them to a file."""
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
        sys.exit("bench_ps_near: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    H, W, N = a.height, a.width, a.lights
    P = H * W
    rng = np.random.default_rng(2)
    r, t = np.sqrt(rng.uniform(0.02, 0.8, N)), rng.uniform(0, 2 * np.pi, N)
    lu, lv = (r * np.cos(t)).astype(np.float32), (r * np.sin(t)).astype(np.float32)
    A = rti.ps_design(lu, lv)
    R = 2.0 * W
    centre = np.array([0.5 * (W - 1), 0.5 * (H - 1), 0.0])
    A3 = torch.as_tensor(A, device=dev)
    Ld = torch.as_tensor(rti.ps_near_lights(centre + R * A), device=dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    hmap = (0.02 * W * torch.exp(-((xx - W / 2) ** 2 + (yy - H / 2) ** 2) / (2 * (0.2 * W) ** 2))).float().contiguous()
    stream = torch.cuda.current_stream(dev)
    normals = torch.empty((P, 3), dtype=torch.float32, device=dev)
    kind = torch.empty(P, dtype=torch.uint8, device=dev)
    fallback = torch.zeros(1, dtype=torch.int32, device=dev)
    lines = []

    def emit(ln):
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    for C in (1, 3):
        albedo = torch.empty((C, P), dtype=torch.float32, device=dev)
        res = torch.empty((C, P), dtype=torch.float32, device=dev)
        kept = torch.empty((C, P), dtype=torch.int32, device=dev)
        for name, dt in (("fp32", torch.float32), ("u8", torch.uint8)):
            I = torch.randint(0, 256, (C, N, P), device=dev, dtype=torch.uint8).to(dt)

            def far(iters):
                return lambda: api.photometric_stereo_into(A3, I, normals, albedo, kind, res, kept, fallback, lo=1.0,
                                                           hi=254.0, min_lights=3, iters=iters, delta=5.0)

            def near(iters, h=hmap):
                return lambda: api.photometric_stereo_near_into(Ld, I, H, W, normals, albedo, kind, res, kept, fallback,
                                                                lo=1.0, hi=254.0, min_lights=3, height=h, r0=R,
                                                                iters=iters, delta=5.0)

            variants = {"far_iters0": far(0), "near_iters0": near(0), "far_iters3": far(3), "near_iters3": near(3)}
            plan = int(L.lib().rti_photometric_stereo_near_plan(N, api._IN_DTYPES[dt], C, 3, 0))
            reps = {}
            for v, fn in variants.items():  # warm-up, and the launches per region
                fn()
                reps[v] = max(1, math.ceil(a.region_ms / max(region_ms(fn, 2, stream), 1e-3)))
            ms = {v: [] for v in variants}
            for _ in range(a.regions):
                for v, fn in variants.items():
                    ms[v].append(region_ms(fn, reps[v], stream))
            med = {v: float(np.median(ms[v])) for v in variants}
            for v in variants:
                iters = int(v[-1])
                passes = 1 if iters == 0 else iters + 2
                ln = {"variant": v, "dtype": name, "channels": C, "config": f"{W}x{H} N={N}",
                      "launches_per_region": reps[v], "regions": a.regions, "median_ms": round(med[v], 4),
                      "min_ms": round(min(ms[v]), 4), "max_ms": round(max(ms[v]), 4),
                      "resident_tile_px": plan if iters else 0,
                      "samples_per_ns": round(float(P) * N * C * passes / (med[v] * 1e6), 2)}
                if v.startswith("near"):
                    ln["x_far"] = round(med[v] / med["far" + v[4:]], 3)
                emit(ln)
            if C == 1 and dt == torch.float32:
                # refine=2 by hand on preallocated tensors, each launch between its own events, on a rendered
                # stack (the bump hmap under the same lights) so that the height solves see a surface, not noise
                gy, gx = torch.gradient(hmap.double())
                nrm = torch.stack([-gx, -gy, torch.ones_like(gx)], 0).reshape(3, P)
                nrm /= nrm.norm(dim=0, keepdim=True)
                pos = torch.stack([xx.reshape(P).double(), yy.reshape(P).double(), hmap.reshape(P).double()], 0)
                for n in range(N):
                    d = Ld[n, :3, None] - pos
                    r2 = (d * d).sum(0)
                    I[0, n] = (200.0 * (nrm * d).sum(0) * (R * R) / (r2 * r2.sqrt())).clamp(0.0, 255.0).float()
                del d, r2, pos, nrm, gx, gy
                n_map = normals.reshape(H, W, 3)
                ws = api.height_workspace(H, W, "multigrid", dev)
                hbuf = torch.empty((H, W), dtype=torch.float32, device=dev)
                steps = [("near_round0", near(0, None)), ("height_round1", None), ("near_round1", near(0, hbuf)),
                         ("height_round2", None), ("near_round2", near(0, hbuf))]
                near(0, None)()
                api.height_from_normals_into(n_map, ws, hbuf)  # warm-up
                split, total = {}, 0.0
                for label, fn in steps:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    if fn is None:
                        api.height_from_normals_into(n_map, ws, hbuf)
                    else:
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    split[label] = round(e0.elapsed_time(e1), 3)
                    total += split[label]
                emit({"variant": "refine2", "dtype": name, "channels": C, "config": f"{W}x{H} N={N}", "iters": 0,
                      "launch_ms": split, "total_ms": round(total, 3)})
            del I
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
