#!/usr/bin/env python3
"""One training step of the baseline models (model/baseline_models.py: MLP_NIR, Linear_NIR) at the shipped configuration -- bs 32,
256 x 256, fp32 (configs/config_baselines.yaml: train_batch_size 32, learning_rate 1e-3) -- on one MI355X, two ways in ONE process:

  fused   model.train_batch(batch): one nirgan_pixmlp_train (prediction, MSE, every gradient; csrc/pixmlp.hip) + one nirgan_adam
  stock   the reference's arithmetic as PyTorch-ROCm runs it: nn.Linear / nn.Sequential(Linear, ReLU, Linear, ReLU, Linear) on the
          permuted, reshaped input, F.mse_loss, backward, torch.optim.Adam.step (baseline_models.py:19-30, :88-100, :70, :139)

Warm-up, then interleaved rounds of `--steps` steps between HIP events; median, min and max of the rounds per arm.  Prints one JSON
line.  `floor_ms` is 3 x [pixels x 64 x 64] products at the 157.3 TFLOP/s fp32 MFMA peak; `fused_kernel_ms` times the train entry
alone (kernel + record merge, no Adam).

    python scripts/bench_baselines.py [--rounds 7] [--steps 20] [--bs 32] [--size 256]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import torch
import torch.nn as nn
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--bs", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_baselines.py measures on an MI355X"
dev = "cuda:0"

from model.baseline_models import Linear_NIR, MLP_NIR
from nirgan_hip import pixmlp as PX

ns = types.SimpleNamespace
cfg = ns(base_configs=ns(learning_rate=1e-3))
g = torch.Generator().manual_seed(0)
B, S = args.bs, args.size
batch = {"rgb": (0.02 + 0.58 * torch.rand(B, 3, S, S, generator=g)).to(dev), "nir": (0.05 + 0.75 * torch.rand(B, 1, S, S, generator=g)).to(dev)}
npix = B * S * S


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


def arms(kind):
    torch.manual_seed(0)
    fused = (MLP_NIR if kind == "MLP_NIR" else Linear_NIR)(cfg).to(dev).train()
    torch.manual_seed(0)
    body = nn.Linear(3, 1) if kind == "Linear_NIR" else nn.Sequential(nn.Linear(3, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 1))
    body = body.to(dev).train()
    opt = torch.optim.Adam(body.parameters(), lr=1e-3)

    def stock_step():
        x = batch["rgb"]
        Bb, _, H, W = x.shape
        pred = body(x.permute(0, 2, 3, 1).reshape(-1, 3)).reshape(Bb, 1, H, W)
        loss = F.mse_loss(pred, batch["nir"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    flat = fused._flat()
    ws, lossbuf = PX.workspace(batch["rgb"], fused.hidden), torch.zeros(1, device=dev)

    def kernel_only():
        PX.train(flat, fused.hidden, batch["rgb"], flat.grad, ws, nir=batch["nir"], loss=lossbuf)

    return {"fused": lambda: fused.train_batch(batch), "stock": stock_step, "fused_kernel": kernel_only}, fused, body


out = {"device": torch.cuda.get_device_name(0), "bs": B, "size": S, "pixels": npix, "rounds": args.rounds, "steps_per_round": args.steps}
for kind in ("MLP_NIR", "Linear_NIR"):
    fns, fused, body = arms(kind)
    # first step of both arms from the same weights on the same batch: the same loss
    l_f = fns["fused"]().as_dict()["train/loss"]
    l_s = float(fns["stock"]())
    for f in fns.values():                                       # warm-up of every arm
        timed(f, 5)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            times[k].append(timed(f, args.steps))
    res = {k: stats(v) for k, v in times.items()}
    res["first_step_loss"] = {"fused": l_f, "stock": l_s}
    res["stock_over_fused_median"] = round(res["stock"]["median_ms"] / res["fused"]["median_ms"], 3)
    res["spreads_overlap"] = not (res["fused"]["max_ms"] < res["stock"]["min_ms"] or res["stock"]["max_ms"] < res["fused"]["min_ms"])
    if kind == "MLP_NIR":
        floor = 3 * 2.0 * npix * 64 * 64 / 157.3e12 * 1e3
        res["floor_ms"] = round(floor, 4)
        res["fused_kernel_fraction_of_mfma_floor"] = round(floor / res["fused_kernel"]["median_ms"], 3)
    else:
        res["hbm_bytes"] = 16 * npix
        res["fused_kernel_gb_per_s"] = round(16 * npix / (res["fused_kernel"]["median_ms"] * 1e-3) / 1e9, 1)
    out[kind] = res
print(json.dumps(out), flush=True)
