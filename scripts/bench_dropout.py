#!/usr/bin/env python3
"""Step time of the fused Pix2Pix step with the generator's dropout off and on, in ONE process: the geometry of BASELINE.json
configs[1] (6 residual blocks, bs 16, 256 x 256, ngf = ndf = 64, fp32, L1 + GAN loss) through Pix2PixTrainer.step.

  off   define_G(..., use_dropout=False): the plans every earlier measurement ran (scripts/plan_signature.py pins them)
  on    define_G(..., use_dropout=True) in training mode: nirgan_dropout_advance in front of the forward plan, one nirgan_dropout_halo
        per residual block in the forward and in the backward plan, and the blocks' first convolutions without the three fusions the
        mask sits in the way of

Warm-up, then `--steps` timed steps per arm between HIP events, the arms interleaved over `--rounds` rounds; median, min and max of the
rounds per arm.  `dropout_kernel_ms` times the twelve mask launches of a step alone on the trunk's buffers (64 x 64 x 256 + halo at
bs 16) and gives their rate against the bytes they move.  Prints one JSON line.

    python scripts/bench_dropout.py [--rounds 3] [--steps 20] [--warmup 5] [--bs 16] [--size 256] [--blocks 6]
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--blocks", type=int, default=6)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_dropout.py measures on an MI355X"
dev = "cuda:0"

from model import networks
from nirgan_hip import dropout as HD
from nirgan_hip.trainer import Pix2PixTrainer

g = torch.Generator().manual_seed(0)
B, S = args.bs, args.size
rgb = (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev)
nir = (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)


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


def arm(drop):
    torch.manual_seed(0)
    netG = networks.define_G(3, 1, 64, f"resnet_{args.blocks}blocks", "instance", drop, "normal", 0.02).to(dev).train()
    netD = networks.define_D(4, 64, "basic", 3, "instance", "normal", 0.02).to(dev).train()
    tr = Pix2PixTrainer(netG, netD, n_blocks=args.blocks)
    return tr, (lambda: tr.step(rgb, nir))


arms = {"off": arm(False), "on": arm(True)}
for tr, f in arms.values():
    timed(f, args.warmup)
times = {k: [] for k in arms}
for _ in range(args.rounds):
    for k, (tr, f) in arms.items():
        times[k].append(timed(f, args.steps))
out = {"device": torch.cuda.get_device_name(0), "bs": B, "size": S, "blocks": args.blocks, "rounds": args.rounds,
       "steps_per_round": args.steps, "warmup": args.warmup}
for k in arms:
    out[k] = stats(times[k])
    out[k]["launches_per_step"] = {"G_fwd": len(arms[k][0].G.fwd.ops), "G_bwd": len(arms[k][0].G.bwd.ops)}
out["on_over_off_median"] = round(out["on"]["median_ms"] / out["off"]["median_ms"], 4)
out["last_losses_on"] = arms["on"][0].step(rgb, nir).as_dict()
out["dropout_state_on"] = list(arms["on"][0].netG.dropout_state())

# the mask launches alone: one residual block's halo'd map, 2 * blocks launches per step
Hq = S // 4
buf = torch.randn(B, Hq + 2, Hq + 2, 256, device=dev)
state = HD.state_words(1, 1).to(dev)
one = lambda: HD.apply_halo(buf, state, B, Hq, Hq, 256, 1, 0)        # noqa: E731
timed(one, 10)
ms = statistics.median(timed(one, 50) for _ in range(5))
out["dropout_kernel_ms"] = {"one_launch": round(ms, 4), "per_step": round(2 * args.blocks * ms, 4),
                            "gb_per_s": round(2 * buf.numel() * 4 / (ms * 1e-3) / 1e9, 1)}
print(json.dumps(out), flush=True)
