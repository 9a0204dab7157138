#!/usr/bin/env python3
"""What carrying valid-pixel masks from the scene pool into the generator's losses costs, in ONE process: the geometry
of BASELINE.json configs[1] (6 residual blocks, bs 16, 256 x 256, ngf = ndf = 64, fp32, L1 + GAN loss) through Pix2PixTrainer.step,
every step drawing its batch from a pool of `--scenes` uint16 scenes of 4 x `--extent` x `--extent` with nodata.

  plain    ScenePool.loader(max_invalid = T*T/2) and the step as they were: nodata pixels are trained on
  masked   the same loader with return_valid=True (one nirgan_scene_valid launch per batch) and step(..., valid=batch["valid"])
           (one staging copy, one nirgan_valid_count, nirgan_pix_loss_masked in the place of nirgan_pix_loss)

Both arms draw the same windows.  The nodata of a scene: a solid corner wedge of about a fifth of it plus 0.1 % scattered pixels, so
accepted windows hold anything between none and half.  Warm-up, then `--steps` timed steps per arm between HIP events, the arms
interleaved over `--rounds` rounds; median, min and max of the rounds per arm.  The yardstick of `masked` is `plain` OF THIS RUN.
`entries_us` times each new entry alone, 200 calls back to back between two events (median [min, max] of five such windows), with the
bytes it has to move and the rate that gives.
Prints one JSON line.

    python scripts/bench_valid_mask.py [--rounds 5] [--steps 20] [--warmup 5] [--bs 16] [--size 256] [--scenes 8] [--extent 2048]
"""
import argparse
import ctypes as C
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
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--extent", type=int, default=2048)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_valid_mask.py measures on an MI355X"
dev = "cuda:0"

from model import networks
from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool, _scene_valid
from nirgan_hip.trainer import Pix2PixTrainer

B, S, E = args.bs, args.size, args.extent
rng = np.random.default_rng(0)
yy, xx = np.meshgrid(np.arange(E), np.arange(E), indexing="ij")
wedge = yy / E + xx / E < 0.63                                                   # 0.63^2 / 2 = a fifth of the scene
scenes = []
for _ in range(args.scenes):
    x = rng.integers(200, 6000, size=(4, E, E), dtype=np.uint16)
    x[:, wedge] = 0
    k = E * E // 1000
    x[:, rng.integers(0, E, k), rng.integers(0, E, k)] = 0
    scenes.append(x)
pool = ScenePool(scenes, nodata=0, device=dev)
del scenes, wedge, yy, xx

torch.manual_seed(0)
netG = networks.define_G(3, 1, 64, f"resnet_{args.blocks}blocks", "instance", False, "normal", 0.02).to(dev).train()
netD = networks.define_D(4, 64, "basic", 3, "instance", "normal", 0.02).to(dev).train()
tr = Pix2PixTrainer(netG, netD, n_blocks=args.blocks)
MOST = S * S // 2


def timed(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(steps)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def stats(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def plain(steps):
    for batch in pool.loader(B, S, steps, seed=1, max_invalid=MOST):
        tr.step(batch["rgb"], batch["nir"])


def masked(steps):
    for batch in pool.loader(B, S, steps, seed=1, max_invalid=MOST, return_valid=True):
        tr.step(batch["rgb"], batch["nir"], valid=batch["valid"])


arms = {"plain": plain, "masked": masked}
for f in arms.values():
    timed(f, args.warmup)
times = {k: [] for k in arms}
for _ in range(args.rounds):
    for k, f in arms.items():
        times[k].append(timed(f, args.steps))
out = {"device": torch.cuda.get_device_name(0), "bs": B, "size": S, "blocks": args.blocks, "rounds": args.rounds, "steps_per_round": args.steps,
       "warmup": args.warmup, "pool": {"scenes": args.scenes, "extent": E, "dtype": "uint16", "nodata": 0, "max_invalid": MOST,
                                       "pool_mb": round(pool.pool_elems * 2 / 1e6, 1), "prefix_mb": round(pool.prefix_elems * 4 / 1e6, 1)}}
for k in arms:
    out[k + "_step_ms"] = stats(times[k])
out["masked_minus_plain_median_ms"] = round(out["masked_step_ms"]["median"] - out["plain_step_ms"]["median"], 4)
out["plain_max_minus_min_ms"] = round(out["plain_step_ms"]["max"] - out["plain_step_ms"]["min"], 4)
out["masked_over_plain_median"] = round(out["masked_step_ms"]["median"] / out["plain_step_ms"]["median"], 5)

# ---- the three entries alone
batch = pool.sample(B, S, seed=1, draw=0, max_invalid=MOST, return_windows=True, return_valid=True)
valid, window = batch["valid"], batch["window"]
out["batch"] = {"valid_fraction": round(float(valid.mean()), 4), "exhausted": int((window[:, 3] < 0).sum())}
n = valid.numel()
st = torch.cuda.current_stream().cuda_stream
count = torch.zeros(1, dtype=torch.int32, device=dev)
pred = torch.rand(B, 1, S, S, device=dev)
sums, grad = torch.zeros(8, device=dev), torch.empty(B, 1, S, S, device=dev)
ws = torch.zeros(L.PIX_LOSS_WS_ELEMS, device=dev)
extra = torch.randn(B, 1, S, S, device=dev)


def loss_desc(cls):
    d = cls()
    d.rgb, d.nir, d.pred, d.B, d.H, d.W = batch["rgb"].data_ptr(), batch["nir"].data_ptr(), pred.data_ptr(), B, S, S
    d.w_l1, d.criterion, d.log_all = 100.0, 0, 0
    d.extra, d.extra_cs, d.extra_c, d.extra_scale = extra.data_ptr(), 1, 0, 1.0
    d.sums, d.grad_pred, d.ws, d.ws_elems = sums.data_ptr(), grad.data_ptr(), ws.data_ptr(), ws.numel()
    return d


dm, du = loss_desc(L.PixLossMaskedDesc), loss_desc(L.PixLossDesc)
dm.valid, dm.count = valid.data_ptr(), count.data_ptr()
entries = {
    # reads four int32 corners per pixel out of shared cache lines (counted once: 4 B per pixel) and writes one float
    "scene_valid": (lambda: _scene_valid(pool, S, window, None, B, 0, B, valid), n * 8),
    "valid_count": (lambda: L.call("nirgan_valid_count", valid.data_ptr(), n, count.data_ptr(), st), n * 4),
    # the step's shape of the call (L1 only, the GAN term as `extra`): the mask and extra in, grad out at every pixel, nir and pred in
    # at the kept ones; rgb is not read
    "pix_loss_masked": (lambda: L.call("nirgan_pix_loss_masked", C.byref(dm), st), int(n * 4 * (3 + 2 * float(valid.mean())))),
    "pix_loss": (lambda: L.call("nirgan_pix_loss", C.byref(du), st), n * 16),
}
out["entries_us"] = {}
for name, (fn, moved) in entries.items():
    def many(steps, fn=fn):
        for _ in range(steps):
            fn()
    timed(many, 20)
    v = [timed(many, 200) * 1e3 for _ in range(5)]
    s_ = stats(v, 2)
    s_["bytes"], s_["gb_per_s"] = moved, round(moved / (s_["median"] * 1e-6) / 1e9, 1)
    out["entries_us"][name] = s_
print(json.dumps(out), flush=True)
