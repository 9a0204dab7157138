#!/usr/bin/env python3
"""Call time of the masked per-tile metrics entry beside the unmasked one, on one MI355X in ONE process:

  plain   nirgan_tile_metrics         (csrc/tilemetrics.hip)         5 planes read once, + the SSIM halo of nir and pred
  masked  nirgan_tile_metrics_masked  (csrc/tilemetrics_masked.hip)  6 planes read once, + the halo of nir, pred and the mask

on the same batch of 16 tiles of 256 x 256, centred 240 x 240 window, SSIM window 11, patch 32; the mask is 98 % valid (seeded).  The C
entries are called directly on buffers allocated once: a call is the two launches and nothing else.  After a warm-up, `--windows`
windows per arm, interleaved, of `--calls` calls back to back between two HIP events.  Median and [min, max] of the windows per
arm, the ratio of the medians beside the 6 : 5 ratio of the bytes read, and `masked_excess_over_plain_spread`: whether the masked arm
costs more than the byte ratio plus the plain arm's own max - min.  Both arms' rows are compared first (the masked means differ from
the unmasked ones by the 2 % of pixels dropped).  Prints one JSON line and writes it to `--out`.

    python scripts/bench_tile_metrics_masked.py [--windows 5] [--calls 200] [--out profiles/tile_metrics_masked_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--crop", type=int, default=240)
ap.add_argument("--valid", type=float, default=0.98)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_tile_metrics_masked.py measures on an MI355X"
dev = "cuda:0"

from nirgan_hip import lib as L

B, S, Cr = args.batch, args.size, args.crop
o = (S - Cr) // 2
g = torch.Generator().manual_seed(0)
rgb = (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev)
nir = (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)
pred = (nir + 0.1 * torch.randn(B, 1, S, S, generator=g).to(dev)).clamp(0.01, 1.0)
valid = (torch.rand(B, 1, S, S, generator=g) < args.valid).float().to(dev)
be = L.backend()
st = torch.cuda.current_stream().cuda_stream


def entry(masked):
    desc = (L.TileMetricsMaskedDesc if masked else L.TileMetricsDesc)()
    ws_elems = (be.nirgan_tile_metrics_masked_ws_elems if masked else be.nirgan_tile_metrics_ws_elems)(B, Cr, Cr)
    ws = torch.empty(int(ws_elems), device=dev)
    rows = torch.full((B, L.TILE_METRIC_MASKED_COLS if masked else L.TILE_METRIC_COLS), float("nan"), device=dev)
    desc.rgb, desc.nir, desc.pred, desc.B, desc.H, desc.W = rgb.data_ptr(), nir.data_ptr(), pred.data_ptr(), B, S, S
    desc.y0, desc.x0, desc.ch, desc.cw = o, o, Cr, Cr
    desc.window, desc.sigma, desc.max_val, desc.eps, desc.patch = 11, 1.5, 1.0, 1e-12, 32
    desc.ws, desc.ws_elems, desc.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    if masked:
        desc.valid = valid.data_ptr()
    fn = be.nirgan_tile_metrics_masked if masked else be.nirgan_tile_metrics
    ref = C.byref(desc)

    def call():
        rc = fn(ref, st)
        if rc:
            L.check(rc, "tile_metrics_masked" if masked else "tile_metrics")
    return call, rows, (desc, ws)


def timed(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls


def stats(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


arms = {"plain": entry(False), "masked": entry(True)}
for call, _, _ in arms.values():
    timed(call, 20)
plain_rows, masked_rows = arms["plain"][1].double().cpu(), arms["masked"][1].double().cpu()
window = valid[:, 0, o:o + Cr, o:o + Cr]
assert torch.equal(masked_rows[:, 9], window.sum((1, 2)).double().cpu()), "n_valid is not the count of the mask"
rel = ((plain_rows[:, :3] - masked_rows[:, :3]).abs().max(0).values / plain_rows[:, :3].abs().max(0).values).max().item()
times = {k: [] for k in arms}
for _ in range(args.windows):
    for k, (call, _, _) in arms.items():
        times[k].append(timed(call, args.calls))
out = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "crop": Cr, "ssim_window": 11, "windows": args.windows,
       "calls_per_window": args.calls, "valid_share": round(float(window.mean()), 4),
       "n_ssim_share": round(float(masked_rows[:, 10].sum()) / (B * Cr * Cr), 4),
       "l1_l2_ssim_max_rel_difference_masked_vs_plain": rel}
out.update({k: stats(v) for k, v in times.items()})
out["masked_over_plain_median"] = round(out["masked"]["median_ms"] / out["plain"]["median_ms"], 4)
out["bytes_ratio"] = 1.2
out["plain_spread_ms"] = round(out["plain"]["max_ms"] - out["plain"]["min_ms"], 5)
out["masked_excess_over_plain_spread"] = out["masked"]["median_ms"] > 1.2 * out["plain"]["median_ms"] + out["plain_spread_ms"]
out["plain_gb_per_s"] = round(5 * Cr * Cr * 4 * B / (out["plain"]["median_ms"] * 1e-3) / 1e9, 1)
out["masked_gb_per_s"] = round(6 * Cr * Cr * 4 * B / (out["masked"]["median_ms"] * 1e-3) / 1e9, 1)
line = json.dumps(out)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
