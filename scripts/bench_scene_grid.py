#!/usr/bin/env python3
"""What cutting an explicit list of windows costs beside sampling them: nirgan_scene_gather against
nirgan_scene_sample_scaled with scales (f,), f = 1, 2, 4, on a uint16 pool of `--scenes` scenes of 5 x `--extent` x `--extent`,
B = `--bs`, T = `--size`, no nodata table, no coords.

The two arms of a factor cut the SAME windows: the sampler's arm runs draws 0 .. calls-1 ("d4"), the gather's arm cuts the window
rows those draws wrote, `--bs` rows per call from one list of calls * bs rows (only `first` changes).  A call of the sampler is its
draw launch plus the gather launch; a call of nirgan_scene_gather is the host's check of its `--bs` rows plus the gather launch.

Per arm: `--reps` repetitions, each `--calls` calls back to back between two HIP events after a warm-up; all arms interleaved within
a repetition.  Reported per arm: the median, min and max of the repetitions in microseconds per call, the bytes a call reads and
writes (B * 4 * T * T * (2 * f * f + 4)) and that rate as a fraction of the 8 TB/s HBM peak of DESIGN 5.  Prints one JSON line per
arm.

    python scripts/bench_scene_grid.py [--reps 7] [--calls 500] [--bs 16] [--size 256] [--scenes 4] [--extent 2048]
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--scenes", type=int, default=4)
ap.add_argument("--extent", type=int, default=2048)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_scene_grid.py measures on an MI355X"
dev = "cuda:0"

from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool, WindowList

HBM_PEAK = 8e12
B, T = args.bs, args.size
rng = np.random.default_rng(0)
pool = ScenePool([rng.integers(200, 6000, size=(5, args.extent, args.extent), dtype=np.uint16) for _ in range(args.scenes)], device=dev)
out = pool._outputs(B, T)
stream = torch.cuda.current_stream().cuda_stream
be = L.backend()


def sampler_arm(f):
    """nirgan_scene_sample_scaled on the descriptor ``ScenePool.sample`` would build, with only ``draw`` changing"""
    _, d = pool._describe(out, B, T, 3, 0, 0, "d4", 0, (f,), None)
    ref = C.byref(d)

    def run(n):
        for i in range(n):
            d.draw = i
            assert be.nirgan_scene_sample_scaled(ref, stream) == 0
    return run


def gather_arm(f):
    """nirgan_scene_gather on the rows that the sampler's arm draws, with only ``first`` changing"""
    rows = torch.cat([pool.sample(B, T, seed=3, draw=i, scales=(f,), return_windows=True)["window"] for i in range(args.calls)])
    wl = WindowList(rows, dev)
    table, table_host = pool._table(T)
    d = L.SceneGatherDesc()
    d.pool, d.pool_elems, d.dtype, d.S, d.C = pool.pool.data_ptr(), pool.pool_elems, pool.dtype, len(pool), pool.C
    d.table, d.table_host = table.data_ptr(), table_host.ctypes.data
    d.band = (C.c_int * 4)(*pool.bands)
    d.tile, d.divisor = T, pool.divisor
    d.window, d.window_host, d.n_windows, d.n = wl.device.data_ptr(), wl.host.ctypes.data, len(wl), B
    d.rgb, d.nir = out["rgb"].data_ptr(), out["nir"].data_ptr()
    ref = C.byref(d)

    def run(n):
        for i in range(n):
            d.first = i * B
            assert be.nirgan_scene_gather(ref, stream) == 0
    run.keep = (wl, table, table_host)
    return run


arms = {}
for f in (1, 2, 4):
    arms[f"scene_sample_scaled ({f},)"] = (sampler_arm(f), f)
    arms[f"scene_gather f={f}"] = (gather_arm(f), f)


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(n)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n


for fn, _ in arms.values():
    timed(fn, 20)
times = {k: [] for k in arms}
for r in range(args.reps):
    for k, (fn, _) in arms.items():
        times[k].append(timed(fn, args.calls))
for k, (fn, f) in arms.items():
    moved = B * 4 * T * T * (2 * f * f + 4)
    us = statistics.median(times[k])
    print(json.dumps({"arm": k, "device": torch.cuda.get_device_name(0), "bs": B, "size": T, "scenes": args.scenes, "extent": args.extent,
                      "reps": args.reps, "calls_per_rep": args.calls, "us_per_call": {"median": round(us, 2), "min": round(min(times[k]), 2),
                                                                                     "max": round(max(times[k]), 2)},
                      "mb_moved": round(moved / 1e6, 2), "tb_per_s": round(moved / (us * 1e-6) / 1e12, 3),
                      "share_of_hbm_peak": round(moved / (us * 1e-6) / HBM_PEAK, 4)}), flush=True)
