#!/usr/bin/env python3
"""Time the HSH peak search (rti_hsh_normals.hip) at 3840x2160 against the composition it replaces
and against rti_relight_hsh8, all in one process, for k = 16 and k = 9:

  normals_f32_g10 / _g16   rti_hsh_normals on three fp32 [p][k] maps, grid 10 (E = 317) / 16 (E = 797)
  normals_u8_g10 / _g16    rti_hsh8_normals from the 3k bytes per pixel
  relight_argmax_g10       rti_relight of the luminance map at the 317 grid directions (fp32 [E][P] out) followed by
                           torch.argmax over E: the composition, without its refinement (which would only add to it)
  relight_hsh8_g10         rti_relight_hsh8 at the 317 directions, uint8 RGB out: the other E-direction kernel

Method as tools/bench_hsh8.py.  Cold reads: the launches rotate over --map-sets sets of maps.  Every timed window is a
run of back-to-back launches between two HIP events sized to last >= --window-ms; the variants alternate window by
window and the time is the median over the windows.  ps_per_term = time / (P·E·k): one fused multiply-add of the
search (for relight_hsh8, of one channel out of its three: it does 3·P·E·k).  x_relight_argmax and x_relight_hsh8:
the time over the yardstick's at the same k (grid 10 variants only).  Prints one JSON line per variant; --out also
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rti  # noqa: E402
from bench_hsh8 import synth_hsh_maps  # noqa: E402
from bench_lrgb import window_ms  # noqa: E402
from rti import _lib as L  # noqa: E402
from rti import api  # noqa: E402

LUMA = (0.299, 0.587, 0.114)


def grid_luv(G, dev):
    pts = [(i, j) for j in range(-G, G + 1) for i in range(-G, G + 1) if i * i + j * j <= G * G]
    return torch.as_tensor(np.array(pts, np.float64) / np.float64(G), device=dev)


def bench_k(k, a, dev, lines):
    basis, bid = f"hsh{k}", api.basis_id(f"hsh{k}")
    P, sets = a.height * a.width, max(1, a.map_sets)
    maps = [synth_hsh_maps(P, k, 10 + i, dev) for i in range(sets)]
    qs = [rti.quantise_hsh(m, basis) for m in maps]
    lum = [((LUMA[0] * m[0] + LUMA[1] * m[1]) + LUMA[2] * m[2]).contiguous() for m in maps]
    n = [torch.empty((P, 3), device=dev) for _ in range(sets)]
    n8 = [torch.empty((P, 3), device=dev) for _ in range(sets)]
    tables = {G: rti.peak_table(basis, G, dev) for G in (10, 16)}
    luv = grid_luv(10, dev)
    E10 = luv.shape[0]
    assert E10 == rti.peak_grid_points(10)
    values = torch.empty((E10, P), device=dev)               # the composition's 4·E bytes per pixel
    best = torch.empty(P, dtype=torch.int64, device=dev)
    rgb = torch.empty((E10, P, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = api._stream_of(luv)
    lib = rti.load()
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    def relight_argmax(i):
        L.check(lib.rti_relight(api._vp(lum[i]), L.RTI_F32, bid, P, L.RTI_COEF_PIXEL_MAJOR, api._vp(luv), E10,
                                api._vp(values), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR, sp), "rti_relight")
        torch.argmax(values, dim=0, out=best)

    variants = {}
    for G in (10, 16):
        variants[f"normals_f32_g{G}"] = rotating(
            lambda i, G=G: api.hsh_normals_into(maps[i], tables[G], n[i], basis=basis, grid=G))
        variants[f"normals_u8_g{G}"] = rotating(
            lambda i, G=G: api.hsh8_normals_into(qs[i].coef, qs[i].qparams, tables[G], n8[i], basis=basis, grid=G))
    variants["relight_argmax_g10"] = rotating(relight_argmax)
    variants["relight_hsh8_g10"] = rotating(
        lambda i: api.relight_hsh8_into(qs[i].coef, qs[i].qparams, luv, rgb, basis=basis))
    points = {v: rti.peak_grid_points(16) if v.endswith("g16") else E10 for v in variants}
    reps = {}
    for v, fn in variants.items():  # warm-up, and the launches per window
        for _ in range(2):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 2, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    # the timed launches computed the real thing: the search's grid point is the composition's argmax wherever the
    # refined normal is well inside its cell, and the normals are unit vectors
    api.hsh_normals_into(maps[0], tables[10], n[0], basis=basis, grid=10)
    relight_argmax(0)
    cell = (n[0][:, :2] * 10.0 - luv[best].float() * 10.0).abs().amax(dim=1)
    assert float((cell <= 0.5 + 1e-4).float().mean()) > 0.999, float((cell <= 0.5 + 1e-4).float().mean())
    assert float(((n[0] * n[0]).sum(-1) - 1.0).abs().max()) < 1e-5
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height} RGB HSH-{k}, {sets} map sets", "grid_points": points[v],
              "launches_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
              "ps_per_term": round(med[v] * 1e9 / (P * points[v] * k), 4)}
        if v.startswith("normals") and v.endswith("g10"):
            ln["x_relight_argmax"] = round(med[v] / med["relight_argmax_g10"], 3)
            ln["x_relight_hsh8"] = round(med[v] / med["relight_hsh8_g10"], 3)
        lines.append(ln)
        print(json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--map-sets", type=int, default=3)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hsh_normals: no HIP device (there is no CPU path to time)")
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
