#!/usr/bin/env python3
"""The land-cover-stratified metrics of one batch of 256 x 256 tiles on the centred 240 x 240 window against the unstratified per-tile
entry on the same tensors, on one MI355X, in ONE process:

  tile    utils.calculate_metrics.tile_metrics_device (csrc/tilemetrics.hip): one row per tile
  class   utils.calculate_metrics.class_metrics_device (csrc/classmetrics.hip) with a uint8 mask of 5 classes: one row per (tile, class)

for B = 16 and B = 64.  Warm-up, then interleaved rounds of `--steps` calls between HIP events; median, min and max of the rounds per
arm and the ratio of the medians.  Both are the CALL (two launches and two allocations), not a kernel alone.  The count-weighted class
rows are compared with the per-tile rows first.  Prints one JSON line (kept in profiles/class_metrics_vs_tile_metrics.json).

    python scripts/time_class_metrics.py [--rounds 7] [--steps 20] [--size 256] [--crop 240] [--classes 5]
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
ap.add_argument("--crop", type=int, default=240)
ap.add_argument("--classes", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "time_class_metrics.py measures on an MI355X"
dev = "cuda:0"

from utils.calculate_metrics import CLASS_METRIC_COLUMNS, TILE_METRIC_COLUMNS, class_metrics_device, tile_metrics_device

S, Cr, K = args.size, args.crop, args.classes


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


out = {"device": torch.cuda.get_device_name(0), "size": S, "crop": Cr, "classes": K, "rounds": args.rounds, "steps_per_round": args.steps,
       "columns_compared": ["l1", "l2", "ssim", "l1_ndvi", "l1_ndwi", "l1_evi"]}
for B in (16, 64):
    g = torch.Generator().manual_seed(0)
    rgb = (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev)
    nir = (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)
    pred = (nir + 0.1 * torch.randn(B, 1, S, S, generator=g).to(dev)).clamp(0.01, 1.0)
    mask = torch.randint(0, K, (B, S, S), generator=g, dtype=torch.uint8).to(dev)

    def tile():
        return tile_metrics_device(rgb, nir, pred, crop=Cr, window_size=11, patch=32)

    def klass():
        return class_metrics_device(rgb, nir, pred, mask, classes=K, crop=Cr, window_size=11)

    fns = {"tile": tile, "class": klass}
    rows, ref = klass().double(), tile().double()
    pooled = torch.stack([(rows[:, :, 0] * rows[:, :, CLASS_METRIC_COLUMNS.index(k)]).sum(1) / (Cr * Cr) for k in out["columns_compared"]], 1)
    ref = ref[:, [TILE_METRIC_COLUMNS.index(k) for k in out["columns_compared"]]]
    rel = ((pooled - ref).abs().max(0).values / ref.abs().max(0).values).max().item()
    for f in fns.values():
        timed(f, 5)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            times[k].append(timed(f, args.steps))
    res = {k: stats(v) for k, v in times.items()}
    res["pooled_rows_max_rel_difference"] = rel
    res["class_over_tile_median"] = round(res["class"]["median_ms"] / res["tile"]["median_ms"], 3)
    res["spreads_overlap"] = not (res["class"]["max_ms"] < res["tile"]["min_ms"] or res["tile"]["max_ms"] < res["class"]["min_ms"])
    res["class_tiles_per_s"] = round(B / (res["class"]["median_ms"] * 1e-3))
    nbytes = (5 * 4 + 1) * Cr * Cr * B
    res["algorithmic_bytes"] = nbytes
    res["class_gb_per_s"] = round(nbytes / (res["class"]["median_ms"] * 1e-3) / 1e9, 1)
    out[f"B{B}"] = res
print(json.dumps(out), flush=True)
