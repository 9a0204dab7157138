#!/usr/bin/env python3
"""The NDVI time-series statistics (validation_utils/time_series_validation.py) of one stack of 24 dates of 256 x 256 tiles, on one
MI355X, two ways in ONE process, for mean_patch_size 4 and 32:

  torch   the reference's own arithmetic with stock torch ops on the same device tensors: the centre-crop slices, the NDVI of the
          64 x 64 crop, and per date a slice + .mean().item() for the two centroid means and a slice + .median().item() for the two
          NDVI medians (what plot_timeline / plot_ndvi_timeline compute, minus the copy to the CPU)
  fused   validation_utils.ndvi_timeline: TWO utils.calculate_metrics.window_stats_device calls (csrc/windowstats.hip) and ONE host copy

Both arms end with the numbers on the host.  Warm-up, then interleaved rounds of `--steps` calls between HIP events; median, min
and max of the rounds per arm.  The two arms' numbers are compared first.  Prints one JSON line.

    python scripts/time_window_stats.py [--rounds 7] [--steps 20] [--size 256] [--dates 24]
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
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--dates", type=int, default=24)
args = ap.parse_args()
assert torch.cuda.is_available(), "time_window_stats.py measures on an MI355X"
dev = "cuda:0"

from validation_utils.time_series_validation import ndvi_timeline

S, T = args.size, args.dates
g = torch.Generator().manual_seed(0)
rgb = (0.02 + 0.58 * torch.rand(T, 3, S, S, generator=g)).to(dev)
nir = (0.05 + 0.75 * torch.rand(T, 1, S, S, generator=g)).to(dev)
pred = (nir + 0.1 * torch.randn(T, 1, S, S, generator=g).to(dev)).clamp(0.01, 1.0)


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


def stock(patch):
    """time_series_validation.py:120-132 and :223-266 of the reference on the device tensors"""
    h, w = nir.shape[-2:]
    cx, cy, ps = w // 2, h // 2, patch // 2
    out = {"centroid_nir": [nir[i, 0, cy - ps:cy + ps, cx - ps:cx + ps].mean().item() for i in range(T)],
           "centroid_pred": [pred[i, 0, cy - ps:cy + ps, cx - ps:cx + ps].mean().item() for i in range(T)]}
    x1, y1, x2, y2 = max(cx - 32, 0), max(cy - 32, 0), min(cx + 32, w), min(cy + 32, h)
    c, n, p = (t[:, :, y1:y2, x1:x2] for t in (rgb, nir, pred))
    h, w = n.shape[-2:]
    cx, cy = w // 2, h // 2
    red = c[:, 0]
    nt, npd = (n[:, 0] - red) / (n[:, 0] + red + 1e-6), (p[:, 0] - red) / (p[:, 0] + red + 1e-6)
    x1, y1 = max(cx - ps - 3, 0), max(cy - ps - 10, 0)
    x2, y2 = min(cx + ps - 3, w), min(cy + ps - 10, h)
    out["ndvi_true"] = [nt[i, y1:y2, x1:x2].median().item() for i in range(T)]
    out["ndvi_pred"] = [npd[i, y1:y2, x1:x2].median().item() for i in range(T)]
    return out


out = {"device": torch.cuda.get_device_name(0), "size": S, "dates": T, "rounds": args.rounds, "steps_per_round": args.steps}
for patch in (4, 32):
    fns = {"torch": lambda: stock(patch), "fused": lambda: ndvi_timeline(rgb, nir, pred, mean_patch_size=patch)}
    a, b = fns["torch"](), fns["fused"]()
    diff = max(abs(x - y) for k in a for x, y in zip(a[k], b[k]))
    for f in fns.values():
        timed(f, 5)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            times[k].append(timed(f, args.steps))
    res = {k: stats(v) for k, v in times.items()}
    res["numbers_max_abs_difference"] = diff
    res["torch_over_fused_median"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 2)
    res["spreads_overlap"] = not (res["fused"]["max_ms"] < res["torch"]["min_ms"] or res["torch"]["max_ms"] < res["fused"]["min_ms"])
    out[f"mean_patch_size_{patch}"] = res
print(json.dumps(out), flush=True)
