#!/usr/bin/env python3
"""Time the enhanced renderings of the colour forms at 3840x2160, for both modes and for uint8 and
fp32 output, against what the same object costs today, all in one process:

  lrgb_<mode>_<out> / lrgb8_<mode>_<out> / rgb8_<mode>_<out>
                             rti_relight_lrgb_enhanced (fp32 LRGB map, [p][9]), rti_relight_lrgb8_enhanced (9 bytes),
                             rti_relight_rgb8_enhanced (18 bytes): one launch, one RGB image
  plain_lrgb_<out> / plain_lrgb8_<out> / plain_rgb8_<out>
                             the plain relight of the same object, one direction
  grey_<mode>_<out>          rti_relight_enhanced of one fp32 PTM-6 map [p][6]: one grey image
  composed_<form>_<mode>_<out>
                             the path an entry replaces, from the same object with what the package had: dequantise
                             (8-bit forms) -> fp32 luminance map -> rti_relight_enhanced -> recombination with torch
                             operations -> the output type.  Diffuse gain, LRGB forms: chroma · relight_enhanced(lum).
                             Specular, LRGB forms: kd·chroma·relight_enhanced(lum; kd=1, ks=0) + relight_enhanced(lum;
                             kd=0, ks).  RGB8: the luminance by three torch products and two sums, then per channel
                             relight_enhanced (diffuse gain: about the channel's OWN peak, which is not what the entry
                             computes -- the package had no way to move a channel about another map's peak) or
                             kd·relight_enhanced(channel; kd=1, ks=0) + relight_enhanced(lum; kd=0, ks).

Method as tools/bench_rgb8.py.  Cold reads: the launches rotate over --map-sets sets of maps and as many outputs.
Every timed window is a run of back-to-back calls between two HIP events sized to last >= 1 ms; the variants
alternate window by window and the time is the median over the windows.  Byte models per pixel: lrgb 36 + 3·s, lrgb8
9 + 3·s, rgb8 18 + 3·s, grey 24 + s with s = 1 (uint8) or 4 (fp32) -> fraction of the 8 TB/s HBM peak.  x_plain =
time over the plain relight of the same object and output type, x_grey = over rti_relight_enhanced in the same mode
and output type, x_composed = over the composed path's.  Prints one JSON line per variant; --out also writes them to
a file."""
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
from bench_lrgb import synth_rgb_maps, window_ms  # noqa: E402
from rti import api  # noqa: E402

HBM_BPS = 8.0e12
IN_BYTES = {"lrgb": 36.0, "lrgb8": 9.0, "rgb8": 18.0, "grey": 24.0}
LU, LV = 0.3, -0.45
SETTINGS = {"gain": dict(mode="diffuse_gain", gain=3.5), "spec": dict(mode="specular", kd=0.4, ks=150.0, exp=75)}
OUTS = {"u8": torch.uint8, "f32": torch.float32}
LUMA = (0.299, 0.587, 0.114)


def to_out(x, dt):
    """An fp32 image -> the output type as a viewer would store it."""
    return x if dt == torch.float32 else x.clamp_(0.0, 255.0).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--map-sets", type=int, default=3)
    ap.add_argument("--windows", type=int, default=50)
    ap.add_argument("--window-ms", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_enhance_rgb: no HIP device (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    P, sets = a.height * a.width, max(1, a.map_sets)
    gram = rti.gram(*[np.asarray(v, np.float32) for v in
                      (np.cos(np.linspace(0, 6, 24)) * 0.7, np.sin(np.linspace(0, 6, 24)) * 0.7)])
    grey, lrgb, ql, qr = [], [], [], []
    for i in range(sets):
        maps = synth_rgb_maps(P, 10 + i, dev)
        grey.append(maps[1].contiguous())
        lrgb.append(rti.lrgb_from_rgb(maps, gram))
        ql.append(rti.quantise_lrgb(lrgb[-1]))
        qr.append(rti.quantise_rgb(maps))
        del maps
    luv = torch.tensor([[LU, LV]], dtype=torch.float64, device=dev)
    out3 = {o: [torch.empty((P, 3), dtype=dt, device=dev) for _ in range(sets)] for o, dt in OUTS.items()}
    out1 = {o: [torch.empty((P,), dtype=dt, device=dev) for _ in range(sets)] for o, dt in OUTS.items()}
    w = torch.tensor(LUMA, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    turn = [0]

    def rotating(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            return fn(turn[0])
        return call

    def enh(lum, **kw):  # rti_relight_enhanced of a [P, 6] fp32 map -> fp32 [P]
        kw = dict(kw)
        return rti.relight_enhanced(lum, LU, LV, kw.pop("mode"), **kw)

    def composed_lrgb(m, s, dt):
        lum, chroma = m[:, :6].contiguous(), m[:, 6:]
        if s["mode"] == "diffuse_gain":
            return to_out(chroma * enh(lum, **s)[:, None], dt)
        d, h = enh(lum, **dict(s, kd=1.0, ks=0.0)), enh(lum, **dict(s, kd=0.0))
        return to_out(s["kd"] * chroma * d[:, None] + h[:, None], dt)

    def composed_rgb8(q, s, dt):
        d = rti.dequantise_rgb(q)
        if s["mode"] == "diffuse_gain":
            return to_out(torch.stack([enh(d[c], **s) for c in range(3)], -1), dt)
        lum = (w[0] * d[0] + w[1] * d[1]) + w[2] * d[2]
        h = enh(lum, **dict(s, kd=0.0))
        return to_out(s["kd"] * torch.stack([enh(d[c], **dict(s, kd=1.0, ks=0.0)) for c in range(3)], -1) + h[:, None], dt)

    variants, model, rel = {}, {}, {}
    for o, dt in OUTS.items():
        so = 1.0 if dt == torch.uint8 else 4.0
        variants[f"plain_lrgb_{o}"] = rotating(lambda i, o=o: api.relight_lrgb_into(lrgb[i], luv, out3[o][i].view(1, P, 3)))
        variants[f"plain_lrgb8_{o}"] = rotating(lambda i, o=o: api.relight_lrgb8_into(ql[i].coef, ql[i].rgb, ql[i].qparams,
                                                                                    luv, out3[o][i].view(1, P, 3)))
        variants[f"plain_rgb8_{o}"] = rotating(lambda i, o=o: api.relight_rgb8_into(qr[i].coef, qr[i].qparams, luv,
                                                                                  out3[o][i].view(1, P, 3)))
        for form in ("lrgb", "lrgb8", "rgb8"):
            model[f"plain_{form}_{o}"] = IN_BYTES[form] + 3 * so
        for sname, s in SETTINGS.items():
            kw = {k: v for k, v in s.items() if k != "mode"}
            mode = s["mode"]
            variants[f"grey_{sname}_{o}"] = rotating(lambda i, o=o, mode=mode, kw=kw: api.relight_enhanced_into(
                grey[i], LU, LV, mode, out1[o][i], **kw))
            variants[f"lrgb_{sname}_{o}"] = rotating(lambda i, o=o, mode=mode, kw=kw: api.relight_lrgb_enhanced_into(
                lrgb[i], LU, LV, mode, out3[o][i], **kw))
            variants[f"lrgb8_{sname}_{o}"] = rotating(lambda i, o=o, mode=mode, kw=kw: api.relight_lrgb8_enhanced_into(
                ql[i].coef, ql[i].rgb, ql[i].qparams, LU, LV, mode, out3[o][i], **kw))
            variants[f"rgb8_{sname}_{o}"] = rotating(lambda i, o=o, mode=mode, kw=kw: api.relight_rgb8_enhanced_into(
                qr[i].coef, qr[i].qparams, LU, LV, mode, out3[o][i], **kw))
            variants[f"composed_lrgb_{sname}_{o}"] = rotating(lambda i, s=s, dt=dt: composed_lrgb(lrgb[i], s, dt))
            variants[f"composed_lrgb8_{sname}_{o}"] = rotating(
                lambda i, s=s, dt=dt: composed_lrgb(rti.dequantise_lrgb(ql[i]), s, dt))
            variants[f"composed_rgb8_{sname}_{o}"] = rotating(lambda i, s=s, dt=dt: composed_rgb8(qr[i], s, dt))
            model[f"grey_{sname}_{o}"] = IN_BYTES["grey"] + so
            for form in ("lrgb", "lrgb8", "rgb8"):
                v = f"{form}_{sname}_{o}"
                model[v] = IN_BYTES[form] + 3 * so
                rel[v] = (f"plain_{form}_{o}", f"grey_{sname}_{o}", f"composed_{form}_{sname}_{o}")
    reps = {}
    for v, fn in variants.items():  # warm-up, and the calls per window
        for _ in range(3):
            fn()
        reps[v] = max(1, math.ceil(a.window_ms / max(window_ms(fn, 5, stream), 1e-3)))
    ms = {v: [] for v in variants}
    for _ in range(a.windows):
        for v, fn in variants.items():
            ms[v].append(window_ms(fn, reps[v], stream))
    med = {v: float(np.median(ms[v])) for v in variants}
    # the timed launches computed the real thing, and the composed LRGB paths agree with the entries they stand for
    # (fp32: the composition rounds its intermediate images to fp32)
    checks = {}
    for sname, s in SETTINGS.items():
        kw = dict(s)
        mode = kw.pop("mode")
        api.relight_lrgb8_enhanced_into(ql[0].coef, ql[0].rgb, ql[0].qparams, LU, LV, mode, out3["f32"][0], **kw)
        assert torch.equal(out3["f32"][0].view(torch.int32),
                           rti.relight_lrgb_enhanced(rti.dequantise_lrgb(ql[0]), LU, LV, mode, **kw).view(torch.int32))
        comp = composed_lrgb(rti.dequantise_lrgb(ql[0]), s, torch.float32)
        err = float(((comp - out3["f32"][0]).abs() / out3["f32"][0].abs().clamp(min=255.0)).max())
        checks[f"composed_lrgb8_{sname}_f32"] = err
        assert err <= 1e-3 and bool(out3["f32"][0].any()), (sname, err)
        api.relight_rgb8_enhanced_into(qr[0].coef, qr[0].qparams, LU, LV, mode, out3["u8"][0], **kw)
        assert torch.equal(out3["u8"][0], rti.relight_rgb8_enhanced(qr[0], LU, LV, mode, out_dtype=torch.uint8, **kw))
        assert bool(out3["u8"][0].any())
    lines = []
    for v in variants:
        ln = {"variant": v, "config": f"{a.width}x{a.height}, {sets} map sets, light ({LU}, {LV})",
              "calls_per_window": reps[v], "windows": a.windows, "median_us": round(med[v] * 1e3, 2),
              "min_us": round(min(ms[v]) * 1e3, 2), "max_us": round(max(ms[v]) * 1e3, 2)}
        if v in model:
            ln["model_bytes_per_px"] = model[v]
            ln["achieved_GBs"] = round(P * model[v] / (med[v] * 1e-3) / 1e9, 1)
            ln["frac_of_8TBs"] = round(P * model[v] / (med[v] * 1e-3) / HBM_BPS, 4)
        if v in rel:
            plain, grey_v, comp_v = rel[v]
            ln["x_plain"] = round(med[v] / med[plain], 3)
            ln["x_grey"] = round(med[v] / med[grey_v], 3)
            ln["x_composed"] = round(med[v] / med[comp_v], 4)
        if v in checks:
            ln["max_rel_diff_to_entry"] = float(f"{checks[v]:.3g}")  # relative to max(|entry|, 255)
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
