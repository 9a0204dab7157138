#!/usr/bin/env python3
"""What a multi-scale batch costs beside a native one: nirgan_scene_sample against nirgan_scene_sample_scaled with
scales (1,), (2,), (4,), (8,) and (1, 2, 3, 4), on a uint16 (`--dtype u16`) or float32 (`--dtype f32`, the same values) pool of
`--scenes` scenes of 5 x `--extent` x `--extent`, B = `--bs`, T = `--size`, augment "d4", no nodata table, no coords.

Per arm: `--reps` repetitions, each `--calls` calls back to back between two HIP events after a warm-up; the arms interleaved within
a repetition.  A call is the entry on a descriptor built once (the draw launch plus the gather launch; only `draw` changes).
Reported per arm: the median, min and max of the repetitions in microseconds per call, the bytes a call reads and writes
(B * 4 * T * T * (e * f * f + 4), e the bytes of a pool element, f * f averaged over the factors the batches drew), and that rate as a
fraction of the 8 TB/s HBM peak of DESIGN 5.  `--other-lib` names a second build of the library (the parent commit's, say): its
nirgan_scene_sample is timed as one more arm on the same descriptor.  Prints one JSON line per arm.

    python scripts/bench_scene_scale.py [--reps 5] [--calls 200] [--bs 16] [--size 256] [--scenes 4] [--extent 2048] [--dtype u16]
                                        [--other-lib PATH]
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--scenes", type=int, default=4)
ap.add_argument("--extent", type=int, default=2048)
ap.add_argument("--dtype", choices=("u16", "f32"), default="u16")
ap.add_argument("--other-lib", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_scene_scale.py measures on an MI355X"
dev = "cuda:0"

from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool

HBM_PEAK = 8e12
B, T = args.bs, args.size
rng = np.random.default_rng(0)
scenes = (rng.integers(200, 6000, size=(5, args.extent, args.extent), dtype=np.uint16) for _ in range(args.scenes))
pool = ScenePool([s if args.dtype == "u16" else s.astype(np.float32) for s in scenes], device=dev)
ELEM = 2 if args.dtype == "u16" else 4
out = pool._outputs(B, T)
stream = torch.cuda.current_stream().cuda_stream


def arm(scales, other=None):
    """the entry ``ScenePool.sample`` would call, on its descriptor, with only ``draw`` changing: no Python beyond the ctypes call.
    ``other``: nirgan_scene_sample of another build of the library instead"""
    entry, d = pool._describe(out, B, T, 3, 0, 0, "d4", 0, scales, None)
    fn = getattr(L.backend(), entry)
    if other:
        fn = C.CDLL(other).nirgan_scene_sample
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(L.SceneSampleDesc), C.c_void_p]
    ref = C.byref(d)

    def run(first, n):
        for i in range(n):
            d.draw = first + i
            assert fn(ref, stream) == 0
    return run


arms = {"scene_sample": (arm(None), (1,))}
if args.other_lib:
    arms["scene_sample, other build"] = (arm(None, args.other_lib), (1,))
for scales in ((1,), (2,), (4,), (8,), (1, 2, 3, 4)):
    arms[f"scaled {scales}"] = (arm(scales), scales)


def timed(fn, first, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(first, n)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n


for fn, _ in arms.values():
    timed(fn, 0, 20)
times = {k: [] for k in arms}
for r in range(args.reps):
    for k, (fn, _) in arms.items():
        times[k].append(timed(fn, r * args.calls, args.calls))
for k, (fn, scales) in arms.items():
    ff = [f * f for f in scales]
    if len(scales) > 1:                                                           # the factors these batches drew
        ff = []
        for i in range(args.reps * args.calls):
            w = pool.sample(B, T, seed=3, draw=i, out=out, scales=scales, return_windows=True)["window"]
            ff += (ScenePool.window_factor(w) ** 2).tolist()
    moved = B * 4 * T * T * (ELEM * statistics.mean(ff) + 4)
    us = statistics.median(times[k])
    print(json.dumps({"arm": k, "device": torch.cuda.get_device_name(0), "dtype": args.dtype, "bs": B, "size": T, "scenes": args.scenes,
                      "extent": args.extent, "reps": args.reps, "calls_per_rep": args.calls, "us_per_call": {"median": round(us, 2), "min": round(min(times[k]), 2),
                                                                                     "max": round(max(times[k]), 2)},
                      "mb_moved": round(moved / 1e6, 2), "tb_per_s": round(moved / (us * 1e-6) / 1e12, 3),
                      "share_of_hbm_peak": round(moved / (us * 1e-6) / HBM_PEAK, 4)}), flush=True)
