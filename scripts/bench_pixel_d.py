#!/usr/bin/env python3
"""The pixel discriminator (netD 'pixel', model/networks.py::PixelDiscriminator) at the shipped batch -- bs 16, 256 x 256, fp32 -- on one
MI355X, two ways in ONE process:

  fused   nets.PixelDiscriminatorEngine: nirgan_pixdisc_fwd / _bwd (csrc/pixdisc.hip), the hidden activations never reach HBM
  stock   the reference's arithmetic as PyTorch-ROCm runs it: nn.Sequential(Conv2d(4,64,1), LeakyReLU, Conv2d(64,128,1),
          InstanceNorm2d(128), LeakyReLU, Conv2d(128,1,1)), out.backward(dout)

Two workloads, the discriminator's share of one fused train step:
  D pass   forward + parameter backward on [fake ; real] = 2B samples
  G pass   forward + backward to the prediction channel (mode PRED) on B samples (stock: the gradient wrt the whole input, parameters frozen)

Warm-up, then interleaved rounds of `--steps` steps between HIP events; median, min and max of the rounds per arm.  The fused passes are
also timed one by one (forward, backward per mode).  Prints one JSON line.

    python scripts/bench_pixel_d.py [--rounds 7] [--steps 10] [--bs 16] [--size 256]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import torch
import torch.nn as nn

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_pixel_d.py measures on an MI355X"
dev = "cuda:0"

from model import networks
from nirgan_hip.nets import PixelDiscriminatorEngine

B, S = args.bs, args.size
g = torch.Generator().manual_seed(0)
torch.manual_seed(0)
net = networks.define_D(4, 64, "pixel", norm="instance").to(dev)
flat = net._flat()
stock = nn.Sequential(nn.Conv2d(4, 64, 1), nn.LeakyReLU(0.2, True), nn.Conv2d(64, 128, 1), nn.InstanceNorm2d(128), nn.LeakyReLU(0.2, True),
                      nn.Conv2d(128, 1, 1)).to(dev)
stock.load_state_dict({k[4:]: v for k, v in net.state_dict().items()}, strict=True)


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


def workload(nb, frozen):
    x = (torch.rand(nb, 4, S, S, generator=g) * 2 - 1).to(dev)
    dout = (torch.randn(nb, 1, S, S, generator=g) / (nb * S * S)).to(dev)
    eng = PixelDiscriminatorEngine(flat.param_views(), flat.grad_views(), nb, S, S)
    eng.x_in.copy_(x)
    eng.in_plan.run()                                   # the trainer writes the input in place (torch.cat never materialises)
    eng.dout.copy_(dout)
    xs = x.clone().requires_grad_(frozen)
    for p in stock.parameters():
        p.requires_grad_(not frozen)

    def fused():
        eng.fwd.run()
        (eng.bwd_pred if frozen else eng.bwd).run()

    def stock_step():
        for p in stock.parameters():
            p.grad = None
        xs.grad = None
        stock(xs).backward(dout)

    fns = {"fused": fused, "stock": stock_step, "fused_fwd": eng.fwd.run, "fused_bwd": (eng.bwd_pred if frozen else eng.bwd).run}
    # same weights, same input: the same output
    with torch.no_grad():
        ref = stock(x)
    eng.fwd.run()
    err = ((eng.out - ref).abs().max() / ref.abs().max()).item()
    for f in fns.values():
        timed(f, 3)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            times[k].append(timed(f, args.steps))
    res = {k: stats(v) for k, v in times.items()}
    res["samples"], res["pixels"], res["out_max_rel_diff"] = nb, nb * S * S, err
    res["stock_over_fused_median"] = round(res["stock"]["median_ms"] / res["fused"]["median_ms"], 3)
    res["spreads_overlap"] = not (res["fused"]["max_ms"] < res["stock"]["min_ms"] or res["stock"]["max_ms"] < res["fused"]["min_ms"])
    # products of [pixels x 64 x 128] on the fp32 matrix pipe at 157.3 TFLOP/s: z2 four times (two forward, two backward passes), dh1,
    # and dW2 in the D pass
    nprod = 5 if frozen else 6
    res["mfma_floor_ms"] = round(nprod * 2.0 * nb * S * S * 64 * 128 / 157.3e12 * 1e3, 4)
    return res


out = {"device": torch.cuda.get_device_name(0), "bs": B, "size": S, "rounds": args.rounds, "steps_per_round": args.steps}
out["D_pass_fwd_params_2B"] = workload(2 * B, False)
out["G_pass_fwd_pred_B"] = workload(B, True)
print(json.dumps(out), flush=True)
