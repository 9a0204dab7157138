#!/usr/bin/env python3
"""The per-tile validation metrics table (validation_utils/) of one batch of 256 x 256 tiles on the centred 240 x 240 window, on one
MI355X, two ways in ONE process:

  per_tile  what a caller had before nirgan_tile_metrics, per tile: a crop copy of rgb / nir / pred, image_metrics_device(window 11)
            and functional.index_sums (2 B entry calls and 3 B copies per batch; the rows are stacked on the device, no sync per tile)
  fused     ONE utils.calculate_metrics.tile_metrics_device call (csrc/tilemetrics.hip), the crop by indexing

for B = 16 and B = 64.  Warm-up, then interleaved rounds of `--steps` calls between HIP events; median, min and max of the rounds
per arm.  `fused_gb_per_s` is the algorithmic traffic (5 planes x 240 x 240 x 4 B per tile, each read once) over the fused call's
median time -- the call, not the kernel alone: it includes both launches and the two allocations.  Both arms' rows are compared
first.  Prints one JSON line.

    python scripts/time_tile_metrics.py [--rounds 7] [--steps 20] [--size 256] [--crop 240]
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
args = ap.parse_args()
assert torch.cuda.is_available(), "time_tile_metrics.py measures on an MI355X"
dev = "cuda:0"

from nirgan_hip.functional import index_sums
from utils.calculate_metrics import TILE_METRIC_COLUMNS, image_metrics_device, tile_metrics_device

S, Cr = args.size, args.crop
o = (S - Cr) // 2


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


out = {"device": torch.cuda.get_device_name(0), "size": S, "crop": Cr, "rounds": args.rounds, "steps_per_round": args.steps,
       "columns_compared": ["l1", "l2", "ssim", "l1_ndvi", "l1_ndwi", "l1_evi"]}
for B in (16, 64):
    g = torch.Generator().manual_seed(0)
    rgb = (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev)
    nir = (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)
    pred = (nir + 0.1 * torch.randn(B, 1, S, S, generator=g).to(dev)).clamp(0.01, 1.0)

    def per_tile():
        rows = []
        for b in range(B):
            c, n, p = (t[b:b + 1, :, o:o + Cr, o:o + Cr].contiguous() for t in (rgb, nir, pred))
            rows.append(torch.cat([image_metrics_device(p, n, window_size=11), index_sums(c, n, p, 0)[[1, 2, 6]]]))
        return torch.stack(rows)

    def fused():
        return tile_metrics_device(rgb, nir, pred, crop=Cr, window_size=11, patch=32)

    fns = {"per_tile": per_tile, "fused": fused}
    cols = [TILE_METRIC_COLUMNS.index(k) for k in out["columns_compared"]]
    a, b_ = per_tile().double(), fused()[:, cols].double()
    rel = ((a - b_).abs().max(0).values / a.abs().max(0).values).max().item()
    for f in fns.values():
        timed(f, 5)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            times[k].append(timed(f, args.steps))
    res = {k: stats(v) for k, v in times.items()}
    res["rows_max_rel_difference"] = rel
    res["per_tile_over_fused_median"] = round(res["per_tile"]["median_ms"] / res["fused"]["median_ms"], 2)
    res["spreads_overlap"] = not (res["fused"]["max_ms"] < res["per_tile"]["min_ms"] or res["per_tile"]["max_ms"] < res["fused"]["min_ms"])
    res["fused_tiles_per_s"] = round(B / (res["fused"]["median_ms"] * 1e-3))
    nbytes = 5 * Cr * Cr * 4 * B
    res["algorithmic_bytes"] = nbytes
    res["fused_gb_per_s"] = round(nbytes / (res["fused"]["median_ms"] * 1e-3) / 1e9, 1)
    out[f"B{B}"] = res
print(json.dumps(out), flush=True)
