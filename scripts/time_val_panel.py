#!/usr/bin/env python3
"""The numbers behind one plot_tensors_hist and one plot_index figure (utils/logging_helpers.py) of B = 5 tiles, at 256 x 256 (crop
240) and 532 x 532 (crop 500), on one MI355X, two ways in ONE process:

  torch   the reference's arithmetic with stock torch ops on the same device tensors: clamp, the x 1.5 stretch, per-image
          torch.quantile at 2 % / 98 % and the stretch, the centre-crop slices, torch.histc per image, the NDVI expression; the
          results gathered into one tensor per figure and copied to the host
  fused   TWO utils.logging_helpers.panel_device calls (nirgan_val_panel, csrc/valpanel.hip) and ONE host copy each

Both arms end with the numbers of the two figures on the host.  Warm-up, then interleaved rounds of `--steps` calls between HIP
events; median, min and max of the rounds per arm.  The fused call's effective GB/s is the algorithmic bytes (five input planes read
once, the outputs written once) over its time; no kernel trace is taken.  Prints one JSON line.

    python scripts/time_val_panel.py [--rounds 7] [--steps 20] [--batch 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "time_val_panel.py measures on an MI355X"
dev = "cuda:0"

from utils.logging_helpers import _host, figure_crop, panel_device

HIST = ("rgb_disp", "nir_disp", "pred_disp", "hist")
INDEX = ("rgb_disp", "ndvi_nir_disp", "ndvi_pred_disp")


def timed(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def stretch(c):
    """per image: clamp((c - lo) / (hi - lo), 0, 1) with the 2 % / 98 % torch.quantile of the image"""
    q = torch.quantile(c.flatten(1), torch.tensor([0.02, 0.98], device=c.device), dim=1)           # [2][B]
    lo, hi = q[0].view(-1, 1, 1, 1), q[1].view(-1, 1, 1, 1)
    return ((c - lo) / (hi - lo)).clamp(0, 1)


out = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "rounds": args.rounds, "steps_per_round": args.steps,
       "kernel_trace": "none taken"}
for S in (256, 532):
    B = args.batch
    g = torch.Generator().manual_seed(0)
    rgb = (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev)
    nir = (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)
    pred = (nir + 0.1 * torch.randn(B, 1, S, S, generator=g).to(dev)).clamp(0.01, 1.0)
    y0, x0, ch, cw = figure_crop(S, S)

    def stock():
        sl = (slice(None), slice(None), slice(y0, y0 + ch), slice(x0, x0 + cw))
        n, p = (nir * 1.5).clamp(0, 1)[sl], (pred * 1.5).clamp(0, 1)[sl]
        c = stretch(rgb.clamp(0, 1))[sl].permute(0, 2, 3, 1)
        hist = torch.stack([torch.histc(t[b], bins=100, min=0, max=1) for b in range(B) for t in (n, p)])
        fig1 = torch.cat([c.reshape(-1), n.reshape(-1), p.reshape(-1), hist.reshape(-1)]).cpu()
        red = rgb[:, :1]
        a, b = ((v - red) / (v + red + 1e-6) for v in (nir, pred))
        a, b = ((v.clamp(-1, 1) + 1) / 2 for v in (a, b))
        fig2 = torch.cat([stretch(rgb).permute(0, 2, 3, 1).reshape(-1), a.reshape(-1), b.reshape(-1)]).cpu()
        return fig1, fig2

    def fused():
        h1 = _host(panel_device(rgb, nir, pred, crop=(y0, x0, ch, cw), gain=1.5, perc=2.0, clamp_rgb=True, want=HIST), HIST, B)
        h2 = _host(panel_device(rgb, nir, pred, perc=2.0, clamp_rgb=False, want=INDEX), INDEX, B)
        return h1, h2

    def fused_device_only():
        panel_device(rgb, nir, pred, crop=(y0, x0, ch, cw), gain=1.5, perc=2.0, clamp_rgb=True, want=HIST)
        panel_device(rgb, nir, pred, perc=2.0, clamp_rgb=False, want=INDEX)

    (f1, f2), (h1, h2) = stock(), fused()
    nw = B * ch * cw
    diff = max((f1[:3 * nw] - torch.from_numpy(h1["rgb_disp"]).reshape(-1)).abs().max().item(),
               (f1[3 * nw:4 * nw] - torch.from_numpy(h1["nir_disp"]).reshape(-1)).abs().max().item(),
               (f2[3 * B * S * S:4 * B * S * S] - torch.from_numpy(h2["ndvi_nir_disp"]).reshape(-1)).abs().max().item())
    hist_diff = int((f1[5 * nw:].reshape(B, 2, 100) - torch.from_numpy(h1["hist"]).float()).abs().sum().item())
    fns = {"torch": stock, "fused": fused, "fused_device_only": fused_device_only}
    for f in fns.values():
        timed(f, 5)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            times[k].append(timed(f, args.steps))
    res = {k: stats(v) for k, v in times.items()}
    res["display_max_abs_difference"] = diff
    res["histogram_counts_differing_from_torch_histc"] = hist_diff
    res["torch_over_fused_median"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 2)
    res["spreads_overlap"] = not (res["fused"]["max_ms"] < res["torch"]["min_ms"] or res["torch"]["max_ms"] < res["fused"]["min_ms"])
    # algorithmic bytes of the two calls: 5 input planes read once each, outputs written once
    read = 2 * 5 * B * S * S * 4
    written = (5 * nw + B * 200) * 4 + 5 * B * S * S * 4
    res["algorithmic_bytes"] = read + written
    res["fused_device_only_effective_GBps"] = round((read + written) / (res["fused_device_only"]["median_ms"] * 1e-3) / 1e9, 1)
    res["launches_per_call"] = "4 kernels + 2 memsets"
    out[f"size_{S}"] = res
print(json.dumps(out), flush=True)
