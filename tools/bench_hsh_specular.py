#!/usr/bin/env python3
"""Time the specular HSH kernels (rti_hsh_specular.hip) at 3840x2160 against the route the project had
before them and against a plain relight, all in one process, for HSH-16 and HSH-9, the bytes (hsh8) and the three fp32
maps (rgb), uint8 and fp32 output, E = 1 and E = 8 directions per launch:

  fused_*      rti_relight_hsh8_specular / rti_relight_hsh_specular: one launch
  composed_*   relight_hsh8 / relight_rgb to fp32, rti_shade_normals(kd = 0) per direction, then torch: scale, add the
               highlight, (uint8: clamp and) convert -- E + 1 launches of the library and three or four of torch
  plain_*      relight_hsh8 / relight_rgb alone with the same output type: what a frame without highlights costs
  relight_f32  rti_relight of one fp32 map, one direction, fp32 out: the time per byte everything is compared to

Method as tools/bench_hsh8.py.  Cold reads: the launches rotate over --map-sets sets of maps, normals and outputs.
Every timed window is a run of back-to-back calls between two HIP events sized to last >= --window-ms; the variants
alternate window by window and the time is the median over the windows.  Byte model per pixel of fused and composed
alike (what the frame needs, not what the composed route moves): 3k bytes or 12k of coefficients, 12 of normal, and
3·sizeof(out) per direction; plain_* the same without the normal; relight_f32 4k + 4.  x_composed = fused time over
composed time, x_plain = fused time over plain time, x_bytes = time per model byte over relight_f32's from the same
run (1.0 = rti_relight's time per byte).  Prints one JSON line per variant; --out also writes them to a file."""
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

HBM_BPS = 8.0e12
KD, KS, EXP = 0.4, 150.0, 75
OUTS = {"u8": torch.uint8, "f32": torch.float32}


def synth_normals(P, seed, dev):
    """Unit normals [P, 3] within about 35 degrees of the viewer."""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = torch.randn((P, 3), device=dev, generator=g) * 0.4
    n[:, 2] = 1.0
    return (n / n.norm(dim=1, keepdim=True)).contiguous()


def dirs(E):
    t = np.linspace(0.0, 2 * np.pi, E, endpoint=False)
    return (0.3 * np.cos(t) + 0.1).tolist(), (0.3 * np.sin(t) - 0.2).tolist()


def bench_k(k, a, dev, lines):
    basis = f"hsh{k}"
    P, sets = a.height * a.width, max(1, a.map_sets)
    maps = [synth_hsh_maps(P, k, 10 + i, dev) for i in range(sets)]
    qs = [rti.quantise_hsh(m, basis) for m in maps]
    ns = [synth_normals(P, 20 + i, dev) for i in range(sets)]
    stream = torch.cuda.current_stream(dev)
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(turn[0])
        return call

    variants, model = {}, {}
    one = torch.empty((sets, 1, P), dtype=torch.float32, device=dev)
    luv1 = torch.as_tensor(np.array([[0.3, -0.45]]), device=dev)
    variants["relight_f32"] = rotating(lambda i: L.check(rti.load().rti_relight(
        api._vp(maps[i][0]), L.RTI_F32, api.basis_id(basis), P, L.RTI_COEF_PIXEL_MAJOR, api._vp(luv1), 1,
        api._vp(one[i]), L.RTI_F32, L.RTI_OUT_EVAL_MAJOR, api._stream_of(luv1)), "rti_relight"))
    model["relight_f32"] = P * (4.0 * k + 4)
    keep = {}
    for E in (1, 8):
        lu, lv = dirs(E)
        luv = torch.as_tensor(np.stack([lu, lv], -1), device=dev)
        img = torch.empty((sets, E, P, 3), dtype=torch.float32, device=dev)   # the composed route's fp32 images
        spec = torch.empty((sets, E, P), dtype=torch.float32, device=dev)     # and its highlights
        for oname, dt in OUTS.items():
            plain = torch.empty((sets, E, P, 3), dtype=dt, device=dev)
            for src in ("hsh8", "rgb"):
                fused = torch.empty((sets, E, P, 3), dtype=dt, device=dev)  # kept for the check after the timing
                comp = torch.empty((sets, E, P, 3), dtype=dt, device=dev)
                cbytes = 3.0 * k if src == "hsh8" else 12.0 * k
                tag = f"{src}_{oname}_E{E}"

                def relight_into(i, out, src=src, luv=luv):
                    if src == "hsh8":
                        api.relight_hsh8_into(qs[i].coef, qs[i].qparams, luv, out, basis=basis)
                    else:
                        api.relight_rgb_into(maps[i], luv, out, basis=basis)

                def run_fused(i, src=src, lu=lu, lv=lv, out=fused):
                    if src == "hsh8":
                        api.relight_hsh8_specular_into(qs[i].coef, qs[i].qparams, ns[i], lu, lv, out[i], basis=basis,
                                                       kd=KD, ks=KS, exp=EXP)
                    else:
                        api.relight_hsh_specular_into(maps[i], ns[i], lu, lv, out[i], basis=basis, kd=KD, ks=KS,
                                                      exp=EXP)

                def run_composed(i, lu=lu, lv=lv, out=comp, img=img, spec=spec, dt=dt, relight_into=relight_into):
                    relight_into(i, img[i])
                    for e in range(len(lu)):
                        api.shade_normals_into(ns[i], lu[e], lv[e], spec[i][e], kd=0.0, ks=KS, exp=EXP)
                    img[i].mul_(KD).add_(spec[i].unsqueeze(-1))
                    if dt == torch.uint8:
                        img[i].clamp_(0.0, 255.0)
                    out[i].copy_(img[i])

                variants[f"fused_{tag}"] = rotating(run_fused)
                variants[f"composed_{tag}"] = rotating(run_composed)
                variants[f"plain_{tag}"] = rotating(lambda i, out=plain, relight_into=relight_into: relight_into(i, out[i]))
                model[f"fused_{tag}"] = model[f"composed_{tag}"] = P * (cbytes + 12 + 3.0 * fused.element_size() * E)
                model[f"plain_{tag}"] = P * (cbytes + 3.0 * fused.element_size() * E)
                keep[tag] = (fused, comp)

    reps = {}
    for v, fn in variants.items():  # warm-up, and the calls per window
        for _ in range(4):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 5, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    # the timed calls computed the real thing: the fused frame is the composed one to within a grey level (the
    # composed route rounds to fp32 three times), and it is an image
    for tag, (fused, comp) in keep.items():
        diff = (fused[0].double() - comp[0].double()).abs()
        assert float(diff.max()) <= (1.0 if fused.dtype == torch.uint8 else 1e-2), (tag, float(diff.max()))
        assert float(fused[0].double().std()) > 1.0, tag
    per_byte = med["relight_f32"] / model["relight_f32"]
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height} HSH-{k}, {sets} map sets, kd={KD} ks={KS} exp={EXP}",
              "calls_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
              "model_bytes_per_px": model[v] / P, "achieved_GBs": round(model[v] / (med[v] * 1e-3) / 1e9, 1),
              "frac_of_8TBs": round(model[v] / (med[v] * 1e-3) / HBM_BPS, 4),
              "x_bytes": round((med[v] / model[v]) / per_byte, 3)}
        if v.startswith("fused_"):
            tag = v[len("fused_"):]
            ln["x_composed"] = round(med[v] / med[f"composed_{tag}"], 3)
            ln["x_plain"] = round(med[v] / med[f"plain_{tag}"], 3)
        lines.append(ln)
        print(json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--map-sets", type=int, default=3)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hsh_specular: no HIP device (there is no CPU path to time)")
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
