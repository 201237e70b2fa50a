#!/usr/bin/env python3
"""Time the diffuse-gain HSH kernels (rti_hsh_gain.hip) at 3840x2160 against a plain relight, the
specular entry on the same inputs and a composed route in torch, all in one process, for HSH-16 and HSH-9, the bytes
(hsh8) and the three fp32 maps (rgb), uint8 and fp32 output, E = 1 and E = 8 directions per launch:

  gain_*       rti_relight_hsh8_gain / rti_relight_hsh_gain: one launch
  plain_*      relight_hsh8 / relight_rgb alone with the same output type: what a frame without enhancement costs
  specular_*   rti_relight_hsh8_specular / rti_relight_hsh_specular on the same maps, normals and directions
  composed_*   what the project offered before: (bytes: dequantise_hsh,) the HSH basis at every pixel's normal restated
               in torch, an einsum for the anchors, relight_hsh8 / relight_rgb to fp32, scale and add, (uint8: clamp
               and) convert
  relight_f32  rti_relight of one fp32 map, one direction, fp32 out: the time per byte everything is compared to

Method as tools/bench_hsh_specular.py.  Cold reads: the launches rotate over --map-sets sets of maps, normals and
outputs.  Every timed window is a run of back-to-back calls between two HIP events sized to last >= --window-ms; the
variants alternate window by window and the time is the median over the windows.  Byte model per pixel of gain,
specular and composed alike (what the frame needs, not what the composed route moves): 3k bytes or 12k of
coefficients, 12 of normal, and 3·sizeof(out) per direction; plain_* the same without the normal; relight_f32
4k + 4.  x_plain, x_specular and x_composed = the gain entry's time over that variant's, x_bytes = time per model byte
over relight_f32's from the same run.  Prints one JSON line per variant; --out also writes them to a file."""
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
from bench_hsh_specular import dirs, synth_normals  # noqa: E402
from bench_lrgb import window_ms  # noqa: E402
from rti import _lib as L  # noqa: E402
from rti import api  # noqa: E402

HBM_BPS = 8.0e12
GAIN = 3.5
KD, KS, EXP = 0.4, 150.0, 75  # the specular entry's parameters in tools/bench_hsh_specular.py
OUTS = {"u8": torch.uint8, "f32": torch.float32}
K = {(0, 0): 0.39894228040143267794, (1, 0): 0.69098829894267095853, (1, 1): 0.48860251190291992159,
     (2, 0): 0.89206205807638555727, (2, 1): 0.36418281019735969018, (2, 2): 0.18209140509867984509,
     (3, 0): 1.05550206141118803141, (3, 1): 0.30469719964297715744, (3, 2): 0.09635371475468513518,
     (3, 3): 0.03933623932844290069}


def torch_hsh(lu, lv, k):
    """csrc/rti_basis.h's hsh_eval in torch at per-pixel directions: fp32 [P] each -> [P, k]."""
    r2 = lu * lu + lv * lv
    lw = (1.0 - r2).clamp(min=0.0).sqrt()
    t = 2.0 * lw - 1.0
    st2 = ((1.0 - t) * (1.0 + t)).clamp(min=0.0)
    st = st2.sqrt()
    s = r2.sqrt()
    lit = s > 0
    safe = torch.where(lit, s, torch.ones_like(s))
    c1, s1 = torch.where(lit, lu / safe, torch.ones_like(s)), torch.where(lit, lv / safe, torch.zeros_like(s))
    c2, s2 = c1 * c1 - s1 * s1, 2.0 * s1 * c1
    c3, s3 = c1 * c2 - s1 * s2, s1 * c2 + c1 * s2
    r = math.sqrt(2.0)
    p21, p22 = 3.0 * t * st, 3.0 * st2
    cols = [torch.full_like(lu, K[0, 0]), r * K[1, 1] * s1 * st, K[1, 0] * t, r * K[1, 1] * c1 * st,
            r * K[2, 2] * s2 * p22, r * K[2, 1] * s1 * p21, K[2, 0] * (3.0 * t * t - 1.0) * 0.5, r * K[2, 1] * c1 * p21,
            r * K[2, 2] * c2 * p22]
    if k > 9:
        p31, p32, p33 = 1.5 * (5.0 * t * t - 1.0) * st, 15.0 * t * st2, 15.0 * st2 * st
        cols += [r * K[3, 3] * s3 * p33, r * K[3, 2] * s2 * p32, r * K[3, 1] * s1 * p31,
                 K[3, 0] * (5.0 * t * t * t - 3.0 * t) * 0.5, r * K[3, 1] * c1 * p31, r * K[3, 2] * c2 * p32,
                 r * K[3, 3] * c3 * p33]
    return torch.stack(cols, -1)


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
        img = torch.empty((sets, E, P, 3), dtype=torch.float32, device=dev)  # the composed route's fp32 images
        for oname, dt in OUTS.items():
            plain = torch.empty((sets, E, P, 3), dtype=dt, device=dev)
            spec = torch.empty((sets, E, P, 3), dtype=dt, device=dev)
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

                def run_gain(i, src=src, lu=lu, lv=lv, out=fused):
                    if src == "hsh8":
                        api.relight_hsh8_gain_into(qs[i].coef, qs[i].qparams, ns[i], lu, lv, out[i], basis=basis,
                                                   gain=GAIN)
                    else:
                        api.relight_hsh_gain_into(maps[i], ns[i], lu, lv, out[i], basis=basis, gain=GAIN)

                def run_specular(i, src=src, lu=lu, lv=lv, out=spec):
                    if src == "hsh8":
                        api.relight_hsh8_specular_into(qs[i].coef, qs[i].qparams, ns[i], lu, lv, out[i], basis=basis,
                                                       kd=KD, ks=KS, exp=EXP)
                    else:
                        api.relight_hsh_specular_into(maps[i], ns[i], lu, lv, out[i], basis=basis, kd=KD, ks=KS,
                                                      exp=EXP)

                def run_composed(i, src=src, out=comp, img=img, dt=dt, relight_into=relight_into):
                    m = rti.dequantise_hsh(qs[i]).reshape(3, P, k) if src == "hsh8" else maps[i]
                    anchor = torch.einsum("cpk,pk->pc", m, torch_hsh(ns[i][:, 0], ns[i][:, 1], k))
                    relight_into(i, img[i])
                    img[i].mul_(GAIN).sub_(anchor.mul_(GAIN - 1.0))  # V + (g − 1)(V − A)
                    if dt == torch.uint8:
                        img[i].clamp_(0.0, 255.0)
                    out[i].copy_(img[i])

                variants[f"gain_{tag}"] = rotating(run_gain)
                variants[f"plain_{tag}"] = rotating(lambda i, out=plain, relight_into=relight_into: relight_into(i, out[i]))
                variants[f"specular_{tag}"] = rotating(run_specular)
                variants[f"composed_{tag}"] = rotating(run_composed)
                for v in ("gain", "specular", "composed"):
                    model[f"{v}_{tag}"] = P * (cbytes + 12 + 3.0 * fused.element_size() * E)
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
    # composed route sums in another order and rounds to fp32 throughout), and it is an image
    for tag, (fused, comp) in keep.items():
        diff = (fused[0].double() - comp[0].double()).abs()
        assert float(diff.max()) <= (1.0 if fused.dtype == torch.uint8 else 2e-2), (tag, float(diff.max()))
        assert float(fused[0].double().std()) > 1.0, tag
    per_byte = med["relight_f32"] / model["relight_f32"]
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height} HSH-{k}, {sets} map sets, gain={GAIN}",
              "calls_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2),
              "model_bytes_per_px": model[v] / P, "achieved_GBs": round(model[v] / (med[v] * 1e-3) / 1e9, 1),
              "frac_of_8TBs": round(model[v] / (med[v] * 1e-3) / HBM_BPS, 4),
              "x_bytes": round((med[v] / model[v]) / per_byte, 3)}
        if v.startswith("gain_"):
            tag = v[len("gain_"):]
            for other in ("plain", "specular", "composed"):
                ln[f"x_{other}"] = round(med[v] / med[f"{other}_{tag}"], 3)
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
        sys.exit("bench_hsh_gain: no HIP device (there is no CPU path to time)")
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
