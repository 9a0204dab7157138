#!/usr/bin/env python3
"""The geo-context join's point-in-region query (validation_utils/geo_ablation.py) of N = 2 000 and N = 100 000 table rows against a
synthetic layer of 250 regions and about 500 000 vertices, on one MI355X, two ways in ONE process:

  host    the float64 numpy statement of include/nirgan_hip.h on the host, vectorised per region: the points inside the region's
          box on its three exact sides (y range, x <= xmax) against all of its edges, lowest region first.  It is what a caller
          had before nirgan_point_regions: the project had no implementation, and geopandas is not installed.
  device  ONE validation_utils.points_in_regions call on points that are already on the device (csrc/geocontext.hip): the
          workspace allocation and its memset, the crossing launch and the pick launch

Both arms' regions are compared first (they must be equal on every point).  Warm-up, then interleaved rounds between HIP events
(the host arm's events bracket host work on an idle stream: their distance is its wall time); `--steps` device calls and ONE host
call per round; median, min and max of the rounds per arm.  `device_edge_tests_per_s` counts N x V edge tests as if no box were
skipped -- the algorithmic size of the join, not the work done.  Prints one JSON line.

    python scripts/time_geo_context.py [--rounds 5] [--steps 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--regions", type=int, default=250)
ap.add_argument("--verts-per-region", type=int, default=2000)
args = ap.parse_args()
assert torch.cuda.is_available(), "time_geo_context.py measures on an MI355X"
dev = "cuda:0"

from validation_utils import PolygonLayer, points_in_regions

# 25 x 10 cells of 14.4 x 18 degrees, in each a star-shaped blob of `verts-per-region` vertices with seeded radial jitter
rng = np.random.default_rng(0)
G, K = args.regions, args.verts_per_region
cols = 25
rows_ = -(-G // cols)
cw, ch = 360.0 / cols, 180.0 / rows_
ang = 2 * np.pi * np.arange(K) / K
verts = np.empty((G, K, 2))
for g in range(G):
    cx, cy = -180.0 + (g % cols + 0.5) * cw, -90.0 + (g // cols + 0.5) * ch
    rad = 0.3 + 0.15 * rng.random(K) + 0.04 * np.sin(7 * ang)
    verts[g, :, 0], verts[g, :, 1] = cx + cw * rad * np.cos(ang), cy + ch * rad * np.sin(ang)
ring_start = np.arange(G + 1) * K
layer = PolygonLayer.from_arrays(verts.reshape(-1, 2), ring_start, np.arange(G), G, device=dev)
boxes = layer.region_box.cpu().numpy()


def host_regions(pts):
    out = np.full(pts.shape[0], -1, dtype=np.int64)
    for g in range(G - 1, -1, -1):                                   # descending: the lowest region is written last
        xmin, ymin, xmax, ymax = boxes[g]
        idx = np.flatnonzero((pts[:, 1] >= ymin) & (pts[:, 1] <= ymax) & (pts[:, 0] <= xmax))
        if idx.size == 0:
            continue
        px, py = pts[idx, 0][:, None], pts[idx, 1][:, None]
        x0, y0 = verts[g, :, 0][None, :], verts[g, :, 1][None, :]
        x1, y1 = np.roll(x0, -1, axis=1), np.roll(y0, -1, axis=1)
        straddles = (y0 > py) != (y1 > py)
        d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
        odd = ((straddles & np.where(y1 > y0, d > 0, d < 0)).sum(axis=1) & 1).astype(bool)
        out[idx[odd]] = g
    return out


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


out = {"device": torch.cuda.get_device_name(0), "regions": G, "vertices": G * K, "rounds": args.rounds, "device_steps_per_round": args.steps,
       "host_steps_per_round": 1}
for N in (2000, 100000):
    pts = np.stack([-180 + 360 * rng.random(N), -90 + 180 * rng.random(N)], axis=1)
    x, y = torch.from_numpy(pts[:, 0].copy()).to(dev), torch.from_numpy(pts[:, 1].copy()).to(dev)

    def device():
        return points_in_regions(x, y, layer)

    def host():
        return host_regions(pts)

    a, b = host(), device().cpu().numpy()
    res = {"points_inside": int((a >= 0).sum()), "points_that_differ": int((a != b).sum())}
    assert res["points_that_differ"] == 0, res
    timed(device, 5)
    times = {"host": [], "device": []}
    for _ in range(args.rounds):
        times["host"].append(timed(host, 1))
        times["device"].append(timed(device, args.steps))
    res.update({k: stats(v) for k, v in times.items()})
    res["host_over_device_median"] = round(res["host"]["median_ms"] / res["device"]["median_ms"], 1)
    res["spreads_overlap"] = not (res["device"]["max_ms"] < res["host"]["min_ms"] or res["host"]["max_ms"] < res["device"]["min_ms"])
    res["device_points_per_s"] = round(N / (res["device"]["median_ms"] * 1e-3))
    res["device_edge_tests_per_s"] = round(N * G * K / (res["device"]["median_ms"] * 1e-3))
    out[f"N{N}"] = res
print(json.dumps(out), flush=True)
