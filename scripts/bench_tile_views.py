#!/usr/bin/env python3
"""Timings of the dihedral test-time augmentation on one MI355X.

1. The two entries at tile 512, k = 8, n = 2 (expand C = 3, merge C = 1): warm-up, then the median of --runs event-timed single
   launches, next to a torch.Tensor.copy_ that moves the same number of bytes in the same process (the yardstick: a copy of
   b bytes reads b / 2 and writes b / 2).  Bytes of an entry = what it reads once + what it writes once.
2. predict_tiled on a --scene^2 scene with the 9-block generator, tta="d4" against tta="none", and the share of the d4 time that
   the expand and merge launches of one scene take (timed without the model).
Prints the lines and, with --out, appends them to that file."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nir-gan_amd"))
import torch
from model import networks
from nirgan_hip import lib as L
from nirgan_hip.inference import predict_tiled

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--scene", type=int, default=2048)
ap.add_argument("--scene-reps", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path and no CPU timing"
dev = "cuda:0"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def median_us(fn, runs, warm=5):
    """median over single event-timed calls, in microseconds"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    return statistics.median(times), min(times), max(times)


st = torch.cuda.current_stream().cuda_stream
T, K, N = 512, 8, 2
for name, Cc in (("nirgan_tile_views_expand", 3), ("nirgan_tile_views_merge", 1)):
    small, large = N * Cc * T * T, N * K * Cc * T * T
    a, b = torch.rand(small, device=dev), torch.rand(large, device=dev)
    d = L.TileViewsDesc()
    d.n, d.C, d.H, d.W, d.views = N, Cc, T, T, K
    d.src, d.dst = (a.data_ptr(), b.data_ptr()) if name.endswith("expand") else (b.data_ptr(), a.data_ptr())
    moved = (small + large) * 4
    half = (small + large) // 2
    ca, cb = torch.rand(half, device=dev), torch.empty(half, device=dev)
    us, lo, hi = median_us(lambda: L.call(name, C.byref(d), st), args.runs)
    cus, clo, chi = median_us(lambda: cb.copy_(ca), args.runs)
    say(f"{name[7:]:18s} tile {T}, C {Cc}, k {K}, n {N}: {us:7.1f} us median of {args.runs} (min {lo:.1f}, max {hi:.1f}) = "
        f"{moved / us / 1e6:6.2f} TB/s over {moved / 1e6:.1f} MB; copy_ of the same bytes {cus:7.1f} us (min {clo:.1f}, max {chi:.1f}) = "
        f"{moved / cus / 1e6:6.2f} TB/s; entry / copy = {us / cus:5.2f}")

# end to end: the 9-block generator on one scene, 512-pixel tiles with 16 pixels of context, at most 8 images per model call
torch.manual_seed(0)
net = networks.define_G(3, 1, 64, "resnet_9blocks", "instance", False, "normal", 0.02).to(dev).eval()
S = args.scene
scene = torch.rand(1, 3, S, S, device=dev)


def scene_ms(tta):
    predict_tiled(net, scene, tile=T, margin=16, batch=8, tta=tta)              # warm-up: engines for this batch size
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.scene_reps):
        predict_tiled(net, scene, tile=T, margin=16, batch=8, tta=tta)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / args.scene_reps


plain, d4 = scene_ms("none"), scene_ms("d4")
total = int(L.backend().nirgan_tile_count(1, S, S, T, 16))
tile3, views3 = torch.rand(1, 3, T, T, device=dev), torch.empty(K, 3, T, T, device=dev)
pred8, merged = torch.rand(K, 1, T, T, device=dev), torch.empty(1, 1, T, T, device=dev)
de, dm = L.TileViewsDesc(), L.TileViewsDesc()
de.n, de.C, de.H, de.W, de.views, de.src, de.dst = 1, 3, T, T, K, tile3.data_ptr(), views3.data_ptr()
dm.n, dm.C, dm.H, dm.W, dm.views, dm.src, dm.dst = 1, 1, T, T, K, pred8.data_ptr(), merged.data_ptr()


def views_of_a_scene():
    for _ in range(total):                                                       # batch 8, k 8: one tile per step
        L.call("nirgan_tile_views_expand", C.byref(de), st)
        L.call("nirgan_tile_views_merge", C.byref(dm), st)


vus, _, _ = median_us(views_of_a_scene, 10, warm=2)
say(f"predict_tiled {S}^2, 9-block fp32, tile {T}, margin 16, batch 8 ({total} tiles): tta none {plain:8.2f} ms, d4 {d4:8.2f} ms, "
    f"ratio {d4 / plain:5.2f}; the {total} expand + {total} merge launches of a d4 scene alone {vus / 1e3:6.3f} ms = "
    f"{vus / 1e3 / d4 * 100:5.2f} % of the d4 time")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
