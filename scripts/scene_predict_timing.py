#!/usr/bin/env python3
"""END-TO-END times of scene inference on one MI355X, from a host uint16 array to a host array -- not kernel rates.

A seeded synthetic 4096 x 4096 uint16 scene (4 bands), once without nodata and once with a nodata half-plane; the 9-block generator at
the tiling of profiles/r06_next_rows_timings.txt (tile 512, margin 16, 8 tiles per model call, blended with the default overlap).
Two routes, each timed with a host clock between device synchronisations:
  float route   host astype(float32) / 10000, upload, predict_tiled(blend="blend"), download, .to(float16)
  uint16 route  upload uint16, predict_scene(out="uint16", nodata=0), download
One warm-up each, then ``--reps`` repeats ALTERNATING between the routes in one process; median, min and max are printed, with the
device-only time of the uint16 route (scene resident, event-timed, no download) and the share of tiles that ran beside them.
One JSON line per scene."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import numpy as np
import torch
from model import networks
from nirgan_hip.inference import predict_scene, predict_tiled

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ngf", type=int, default=64)
args = ap.parse_args()
assert args.reps >= 5 or args.size < 4096, "at least five repeats at the reported size"
dev = "cuda:0"
TILE, MARGIN, BATCH, DIVISOR = 512, 16, 8, 10000.0

torch.manual_seed(0)
net = networks.define_G(3, 1, args.ngf, "resnet_9blocks", "instance", False, "normal", 0.02).to(dev).eval()


class Counting:
    """the generator, counting the tiles it is given"""

    def __init__(self, model):
        self.model, self.tiles = model, 0

    def __call__(self, x):
        self.tiles += x.shape[0]
        return self.model(x)


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def float_route(a):
    t0 = clock()
    x = torch.from_numpy(a[:3].astype(np.float32) / np.float32(DIVISOR))[None].to(dev)
    y = predict_tiled(net, x, tile=TILE, margin=MARGIN, batch=BATCH, blend="blend")
    out = y[0, 0].cpu().to(torch.float16).numpy()
    return (clock() - t0) * 1e3, out


def uint16_route(a, nodata):
    t0 = clock()
    x = torch.from_numpy(a.view(np.int16)).to(dev)
    y = predict_scene(net, x, divisor=DIVISOR, nodata=nodata, tile=TILE, margin=MARGIN, batch=BATCH, out="uint16")
    out = y.cpu().numpy().view(np.uint16)
    return (clock() - t0) * 1e3, out


def device_only(a, nodata, reps):
    x = torch.from_numpy(a.view(np.int16)).to(dev)
    model = Counting(net)
    predict_scene(model, x, divisor=DIVISOR, nodata=nodata, tile=TILE, margin=MARGIN, batch=BATCH)
    ran, times = model.tiles, []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        predict_scene(net, x, divisor=DIVISOR, nodata=nodata, tile=TILE, margin=MARGIN, batch=BATCH)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return ran, times


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2)}


for name in ("no nodata", "nodata half-plane"):
    a = np.random.default_rng(1).integers(1, 10000, size=(4, args.size, args.size), dtype=np.uint16)
    if name != "no nodata":
        a[:, :, args.size // 2:] = 0
    with torch.no_grad():
        float_route(a), uint16_route(a, 0)                                       # warm-up: both routes, every batch size they use
        fl, u16 = [], []
        for _ in range(args.reps):
            fl.append(float_route(a)[0])
            u16.append(uint16_route(a, 0)[0])
        ran, dv = device_only(a, 0, args.reps)
        total = Counting(net)
        predict_scene(total, torch.from_numpy(a.view(np.int16)).to(dev), divisor=DIVISOR, nodata=None, tile=TILE, margin=MARGIN, batch=BATCH)
    row = {"scene": f"{args.size}x{args.size} uint16, {name}", "generator": f"resnet_9blocks ngf {args.ngf}", "tile": TILE, "margin": MARGIN,
           "batch": BATCH, "reps": args.reps, "tiles": total.tiles, "tiles_run": ran, "share_skipped": round(1 - ran / total.tiles, 4),
           "float_route_end_to_end": summary(fl), "uint16_route_end_to_end": summary(u16), "uint16_route_device_only": summary(dv)}
    print(json.dumps(row), flush=True)
