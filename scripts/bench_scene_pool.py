#!/usr/bin/env python3
"""What feeding the fused Pix2Pix step from a device-resident scene pool costs, in ONE process: the geometry of BASELINE.json
configs[1] (6 residual blocks, bs 16, 256 x 256, ngf = ndf = 64, fp32, L1 + GAN loss) through Pix2PixTrainer.step.

  fixed   the step on one fixed synthetic batch (what bench.py times)
  pool    every step draws its batch with ScenePool.loader: nirgan_scene_sample (draw + gather launches) in front of the step

The pool: `--scenes` uint16 scenes of 4 x `--extent` x `--extent` with nodata = 0 scattered in (the rejection test reads its table),
geotransforms given (coords are produced), augment "d4".  Warm-up, then `--steps` timed steps per arm between HIP events, the arms
interleaved over `--rounds` rounds; median, min and max of the rounds per arm.  `sample_ms` times the two launches of a batch alone,
back to back, and gives their rate against the bytes they move (uint16 in, float32 out).  Under a kernel trace (rocprofv3
--kernel-trace --stats -- python scripts/bench_scene_pool.py) the kernels are scene_draw_kernel<Scenes>, the draw all
sampling entries share, and scene_scaled_gather_kernel<uint16_t, 4> (profiles/scene_pool_timing.json is older: it names the two
kernels nirgan_scene_sample had to itself then).
Prints one JSON line.

    python scripts/bench_scene_pool.py [--rounds 3] [--steps 20] [--warmup 5] [--bs 16] [--size 256] [--scenes 8] [--extent 2048]
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--extent", type=int, default=2048)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_scene_pool.py measures on an MI355X"
dev = "cuda:0"

from model import networks
from nirgan_hip.data import ScenePool
from nirgan_hip.trainer import Pix2PixTrainer

B, S = args.bs, args.size
rng = np.random.default_rng(0)
scenes = []
for _ in range(args.scenes):
    x = rng.integers(200, 6000, size=(4, args.extent, args.extent), dtype=np.uint16)
    x[:, rng.integers(0, args.extent, 64), rng.integers(0, args.extent, 64)] = 0          # 64 nodata pixels per scene
    scenes.append(x)
geo = [(10.0 + i, 1e-4, 50.0, -1e-4) for i in range(args.scenes)]
pool = ScenePool(scenes, nodata=0, geotransforms=geo, device=dev)
del scenes

g = torch.Generator().manual_seed(0)
rgb = (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev)
nir = (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)
torch.manual_seed(0)
netG = networks.define_G(3, 1, 64, f"resnet_{args.blocks}blocks", "instance", False, "normal", 0.02).to(dev).train()
netD = networks.define_D(4, 64, "basic", 3, "instance", "normal", 0.02).to(dev).train()
tr = Pix2PixTrainer(netG, netD, n_blocks=args.blocks)


def timed(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(steps)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def fixed(steps):
    for _ in range(steps):
        tr.step(rgb, nir)


def from_pool(steps):
    for batch in pool.loader(B, S, steps, seed=1):
        tr.step(batch["rgb"], batch["nir"])


def sample_only(steps):
    for _ in pool.loader(B, S, steps, seed=2):
        pass


arms = {"fixed": fixed, "pool": from_pool}
for f in arms.values():
    timed(f, args.warmup)
times = {k: [] for k in arms}
for _ in range(args.rounds):
    for k, f in arms.items():
        times[k].append(timed(f, args.steps))
out = {"device": torch.cuda.get_device_name(0), "bs": B, "size": S, "blocks": args.blocks, "rounds": args.rounds, "steps_per_round": args.steps,
       "warmup": args.warmup, "pool": {"scenes": args.scenes, "extent": args.extent, "dtype": "uint16", "nodata": 0, "augment": "d4",
                                       "pool_mb": round(pool.pool_elems * 2 / 1e6, 1), "prefix_mb": round(pool.prefix_elems * 4 / 1e6, 1)}}
for k in arms:
    out[k] = stats(times[k])
out["pool_minus_fixed_median_ms"] = round(out["pool"]["median_ms"] - out["fixed"]["median_ms"], 4)
out["pool_over_fixed_median"] = round(out["pool"]["median_ms"] / out["fixed"]["median_ms"], 4)
timed(sample_only, 10)
ms = statistics.median(timed(sample_only, 50) for _ in range(5))
moved = B * 4 * S * S * (2 + 4)
out["sample_ms"] = {"one_batch": round(ms, 4), "share_of_fixed_step": round(ms / out["fixed"]["median_ms"], 5), "gb_per_s": round(moved / (ms * 1e-3) / 1e9, 1)}
last = pool.sample(B, S, seed=1, draw=0, return_windows=True)
out["last_batch"] = {"views": sorted(set((last["window"][:, 3] & 7).tolist())), "exhausted": int((last["window"][:, 3] < 0).sum()),
                     "rgb_mean": round(float(last["rgb"].mean()), 5)}
print(json.dumps(out), flush=True)
