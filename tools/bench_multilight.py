#!/usr/bin/env python3
"""Time the multi-light mode (rti_multilight.hip) at 3840x2160 against the composition it replaces,
in one process, for PTM-6 and HSH-16, one map and three, T = 16, E = 17 and 64:

  light_scores     rti_light_scores: per tile and candidate sharpness and brightness, no frame in memory
  light_field      rti_light_field, smooth = 2 (three launches of a thread per tile)
  relight_field    rti_relight_field under the tile field, fp32 out
  relight          rti.relight (one map) / rti.relight_rgb (three) at one direction, fp32 out: the yardstick of
                   relight_field, which moves the same bytes
  fused            the three entries back to back: the whole mode
  composed         the same mode from what existed before: rti.relight of the luminance map at the E candidates
                   (E frames in memory), torch differences and avg_pool2d for the two tile scores, the normalised
                   score, argmax and gather, a nearest upsample of the choice, and a relight per distinct chosen light
                   gathered per pixel (for three maps the luminance is formed by torch first).  It does not smooth or
                   interpolate the field: it does less, and only its time is compared.

Method as tools/bench_hsh_normals.py: every timed window is a run of back-to-back calls between two HIP events sized to
last >= --window-ms; the variants alternate window by window and the time is the median over the windows.
ps_per_term = light_scores' time / (P·E·k), one fused multiply-add of the search, next to rti_hsh_normals' figure in
the same unit; ns_per_byte = time over the 4·C·k bytes in and 4·C out per pixel.  Prints one JSON line per variant;
--out also writes them to a file."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smartphone-based-rti_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rti  # noqa: E402
from bench_lrgb import window_ms  # noqa: E402

LUMA = (0.299, 0.587, 0.114)
MAIN = (0.3, -0.2)
T = 16


def synth_maps(C, H, W, k, const, dev):
    g = torch.Generator(device=dev).manual_seed(17 + k + C)
    m = torch.rand((C, H, W, k), device=dev, generator=g) * 120.0 - 60.0
    m[..., const] += 140.0
    return m if C == 3 else m[0].contiguous()


def bench_config(basis, k, C, E, a, dev, lines):
    H, W = a.height, a.width
    P = H * W
    coef = synth_maps(C, H, W, k, 5 if basis == "ptm" else 0, dev)
    luv = rti.light_candidates(*MAIN, rings=2 if E == 17 else 7, per_ring=8 if E == 17 else 9)
    assert luv.shape[0] == E
    luv_dev = torch.as_tensor(luv, device=dev)
    Ty, Tx = -(-H // T), -(-W // T)
    scores = torch.empty((Ty, Tx, E, 2), dtype=torch.float64, device=dev)
    count = torch.empty((Ty, Tx), dtype=torch.int32, device=dev)
    field = torch.empty((Ty, Tx, 2), device=dev)
    ws = rti.light_field_workspace(Ty, Tx, dev)
    out = torch.empty((H, W) + ((3,) if C == 3 else ()), device=dev)
    stream = torch.cuda.current_stream(dev)

    def light_scores():
        rti.light_scores_into(coef, luv, scores, count, basis=basis, tile=T)

    def light_field():
        rti.light_field_into(scores, count, luv, ws, field, lu=MAIN[0], lv=MAIN[1], smooth=2)

    def relight_field():
        rti.relight_field_into(coef, field, out, basis=basis, tile=T)

    def relight():
        if C == 3:
            rti.relight_rgb(coef, *MAIN, basis)
        else:
            rti.relight(coef, *MAIN, basis)

    def fused():
        light_scores()
        light_field()
        relight_field()

    def composed():
        lum = coef if C == 1 else ((LUMA[0] * coef[0] + LUMA[1] * coef[1]) + LUMA[2] * coef[2])
        V = rti.relight(lum, luv[:, 0], luv[:, 1], basis).unsqueeze(1)  # [E, 1, H, W]
        dx, dy = V[..., :, 1:] - V[..., :, :-1], V[..., 1:, :] - V[..., :-1, :]
        sharp = F.avg_pool2d(dx * dx, T, ceil_mode=True) + F.avg_pool2d(dy * dy, T, ceil_mode=True)
        bright = F.avg_pool2d(V, T, ceil_mode=True)
        score = sharp / sharp.amax(0, keepdim=True).clamp_min(1e-30) + 0.5 * bright / bright.amax(0, keepdim=True).clamp_min(1e-30)
        choice = score.argmax(0)  # [1, Ty, Tx]
        per_pixel = F.interpolate(choice[None].float(), size=(H, W), mode="nearest")[0, 0].long()
        distinct, inverse = torch.unique(per_pixel, return_inverse=True)  # the host learns how many lights were chosen
        d = luv_dev[distinct].cpu().numpy()
        chans = [coef] if C == 1 else [coef[c] for c in range(3)]
        frames = [rti.relight(ch, d[:, 0], d[:, 1], basis) for ch in chans]  # [D, H, W] each
        return torch.stack([f.gather(0, inverse[None])[0] for f in frames], -1)

    variants = {"light_scores": light_scores, "light_field": light_field, "relight_field": relight_field,
                "relight": relight, "fused": fused, "composed": composed}
    reps = {}
    for v, fn in variants.items():  # warm-up, and the calls per window
        for _ in range(2):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 2, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    nbytes = P * (4 * C * k + 4 * C)
    for v in variants:
        ln = {"variant": v, "config": f"{W}x{H} {basis} C={C} T={T} E={E}", "calls_per_window": reps[v],
              "windows": a.windows, "median_us": round(med[v] * 1e3, 2), "min_us": round(min(ms[v]) * 1e3, 2),
              "max_us": round(max(ms[v]) * 1e3, 2)}
        if v == "light_scores":
            ln["ps_per_term"] = round(med[v] * 1e9 / (P * E * k), 4)
        if v in ("relight_field", "relight"):
            ln["ns_per_byte"] = round(med[v] * 1e6 / nbytes, 6)
        if v == "relight_field":
            ln["x_relight"] = round(med[v] / med["relight"], 3)
        if v == "fused":
            ln["x_composed"] = round(med[v] / med["composed"], 3)
        lines.append(ln)
        print(json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_multilight: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    lines = []
    for basis, k in (("ptm", 6), ("hsh16", 16)):
        for C in (1, 3):
            for E in (17, 64):
                bench_config(basis, k, C, E, a, dev, lines)
                torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
