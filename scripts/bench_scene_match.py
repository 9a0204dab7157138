#!/usr/bin/env python3
"""What matching a scene's histogram on the device costs, in ONE process on one MI355X, HIP events throughout.

Planes of `--side` x `--side` uint16 codes (default 4096: N = 2^24, the largest power of two both routes take), two distributions:
  uniform        every code equally likely
  concentrated   99 % of the pixels in 256 adjacent codes, 1 % anywhere (a vegetation-season scene in miniature)
Arms, buffers allocated once, interleaved over `--windows` windows of `--calls` calls back to back between two events:
  float_entry    the per-tile entry nirgan_hist_match on float32 planes of equal size (the route there was before)
  scene_route    clear two tables, nirgan_scene_hist(source), nirgan_scene_hist(reference), nirgan_scene_match_lut,
                 nirgan_scene_lut_apply
  scene_hist / scene_match_lut / scene_lut_apply   each new entry alone (the count into a table that is never cleared)
Median [min, max] of the windows per arm, the ratio float_entry / scene_route beside float_entry's own max - min, and the count and
apply passes as bytes over time (2 B per pixel read; 2 B read + 2 B written).

End to end (`--e2e-reps`, 0 skips it): the scene and tiling of scripts/scene_predict_timing.py (4096 x 4096 uint16, 4 bands, the 9-block
generator, tile 512, margin 16, 8 tiles per call), scene resident, predict_scene() against predict_scene(match=histogram), alternating.

Writes one JSON document to `--out` and prints it.

    python scripts/bench_scene_match.py [--side 4096] [--calls 200] [--windows 5] [--e2e-reps 5] [--out profiles/scene_match_timing.json]
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
ap.add_argument("--side", type=int, default=4096)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--e2e-reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_match_timing.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_scene_match.py measures on an MI355X"
dev = "cuda:0"

from nirgan_hip import lib as L
from nirgan_hip.inference import predict_scene, scene_histogram

N = args.side * args.side
st = torch.cuda.current_stream().cuda_stream


def planes(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 65536, size=N).astype(np.uint16)
    a = (3000 + 2000 * seed + rng.integers(0, 256, size=N)).astype(np.uint16)
    far = rng.random(N) < 0.01
    a[far] = rng.integers(0, 65536, size=int(far.sum())).astype(np.uint16)
    return a


def timed(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls * 1e3                                       # microseconds per call


def stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


out = {"device": torch.cuda.get_device_name(0), "pixels": N, "calls_per_window": args.calls, "windows": args.windows, "unit": "us per call",
       "distributions": {}}
for kind in ("uniform", "concentrated"):
    a, b = planes(kind, 0), planes(kind, 1)
    src, ref = (torch.from_numpy(x.view(np.int16)).to(dev) for x in (a, b))
    fsrc, fref = (torch.from_numpy(x.astype(np.float32)).to(dev) for x in (a, b))
    del a, b
    be = L.backend()
    ws = torch.empty(int(be.nirgan_hist_match_ws_bytes(1, N)) // 8, dtype=torch.int64, device=dev)
    fout = torch.empty_like(fsrc)
    h = L.HistMatchDesc()
    h.image, h.reference, h.B, h.N, h.ws, h.ws_bytes, h.out = fsrc.data_ptr(), fref.data_ptr(), 1, N, ws.data_ptr(), ws.numel() * 8, fout.data_ptr()
    tables = torch.zeros(2, 65536, dtype=torch.int64, device=dev)
    lut, res = torch.empty(65536, dtype=torch.int16, device=dev), torch.empty_like(src)
    ds, dr, dl, da = (L.SceneMatchDesc() for _ in range(4))
    ds.plane, ds.n, ds.hist = src.data_ptr(), N, tables[0].data_ptr()
    dr.plane, dr.n, dr.hist = ref.data_ptr(), N, tables[1].data_ptr()
    dl.src_hist, dl.ref_hist, dl.lut = tables[0].data_ptr(), tables[1].data_ptr(), lut.data_ptr()
    da.plane, da.n, da.lut, da.out = src.data_ptr(), N, lut.data_ptr(), res.data_ptr()

    def scene_route():
        tables.zero_()
        L.call("nirgan_scene_hist", C.byref(ds), st)
        L.call("nirgan_scene_hist", C.byref(dr), st)
        L.call("nirgan_scene_match_lut", C.byref(dl), st)
        L.call("nirgan_scene_lut_apply", C.byref(da), st)

    arms = {"float_entry": lambda: L.call("nirgan_hist_match", C.byref(h), st),
            "scene_route": scene_route,
            "scene_hist": lambda: L.call("nirgan_scene_hist", C.byref(ds), st),
            "scene_match_lut": lambda: L.call("nirgan_scene_match_lut", C.byref(dl), st),
            "scene_lut_apply": lambda: L.call("nirgan_scene_lut_apply", C.byref(da), st)}
    for fn in arms.values():
        timed(fn, 3)
    times = {k: [] for k in arms}
    for w in range(args.windows):
        for k, fn in arms.items():
            times[k].append(timed(fn, args.calls))
        print(f"# {kind}: window {w + 1} of {args.windows}", file=sys.stderr, flush=True)
    row = {k: stats(v) for k, v in times.items()}
    row["float_entry_over_scene_route_median"] = round(row["float_entry"]["median"] / row["scene_route"]["median"], 2)
    row["float_entry_max_minus_min"] = round(row["float_entry"]["max"] - row["float_entry"]["min"], 2)
    row["scene_hist"]["bytes"], row["scene_lut_apply"]["bytes"] = 2 * N, 4 * N
    for k in ("scene_hist", "scene_lut_apply"):
        row[k]["gb_per_s"] = round(row[k]["bytes"] / (row[k]["median"] * 1e-6) / 1e9, 1)
    out["distributions"][kind] = row
    del src, ref, fsrc, fref, ws, fout, res

if args.e2e_reps > 0:
    from model import networks
    torch.manual_seed(0)
    net = networks.define_G(3, 1, 64, "resnet_9blocks", "instance", False, "normal", 0.02).to(dev).eval()
    a = np.random.default_rng(1).integers(1, 10000, size=(4, 4096, 4096), dtype=np.uint16)
    scene = torch.from_numpy(a.view(np.int16)).to(dev)
    ref_hist = scene_histogram(scene[3], 0)
    kw = dict(divisor=10000.0, nodata=0, tile=512, margin=16, batch=8)

    def once(**extra):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        predict_scene(net, scene, **kw, **extra)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    with torch.no_grad():
        once(), once(match=ref_hist)
        plain, matched = [], []
        for _ in range(args.e2e_reps):
            plain.append(once())
            matched.append(once(match=ref_hist))
    out["end_to_end_ms"] = {"scene": "4096x4096 uint16, 4 bands, resnet_9blocks ngf 64, tile 512, margin 16, batch 8", "reps": args.e2e_reps,
                            "predict_scene": stats(plain), "predict_scene_match": stats(matched),
                            "match_minus_plain_median": round(statistics.median(matched) - statistics.median(plain), 3),
                            "plain_max_minus_min": round(max(plain) - min(plain), 3)}

text = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text, flush=True)
