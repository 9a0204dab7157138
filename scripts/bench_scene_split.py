#!/usr/bin/env python3
"""What drawing from a table of origin rectangles costs beside drawing from whole scenes: nirgan_scene_sample_origins
against nirgan_scene_sample_scaled on a uint16 pool of `--scenes` scenes of 5 x `--extent` x `--extent`, B = `--bs`, T = `--size`,
"d4", no nodata table, no coords -- the set-up of DESIGN 3.14.

Arms, for the scales (1,) and (1, 2, 3, 4):
  scaled         nirgan_scene_sample_scaled: the yardstick
  origins whole  nirgan_scene_sample_origins on one row per scene: the same windows, the same bytes, the other draw kernel
  origins split  nirgan_scene_sample_origins on the table of ``split_blocks(--block, --fraction)``: some tens of rows to bisect, and
                 other windows (the same number of bytes)
  origins dense  the same on ``split_blocks(--dense-block, --fraction)``, scales (1,) only (a lattice that fine leaves no room for the
                 larger windows): a table of many hundreds of rows
A call is the draw launch plus the gather launch; only ``draw`` changes between calls.  `--other-lib` names a second build of the
library (the parent commit's, say): its nirgan_scene_sample_scaled is timed as one more arm per set of scales on the same descriptor.

Per arm: `--reps` repetitions, each `--calls` calls back to back between two HIP events after a warm-up; all arms interleaved within
a repetition, in one process.  Reported per arm: the median, min and max of the repetitions in microseconds per call and the rows R
of the origin table per scale.  One JSON line per arm, printed and written to `--out`.

    python scripts/bench_scene_split.py [--reps 7] [--calls 500] [--bs 16] [--size 256] [--scenes 4] [--extent 2048] [--block 512]
                                        [--dense-block 128] [--fraction 0.2] [--other-lib PATH]
                                        [--out profiles/scene_split_timing.jsonl]
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
ap.add_argument("--block", type=int, default=512)
ap.add_argument("--dense-block", type=int, default=128)
ap.add_argument("--fraction", type=float, default=0.2)
ap.add_argument("--other-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_split_timing.jsonl"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_scene_split.py measures on an MI355X"
dev = "cuda:0"

from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool

B, T = args.bs, args.size
rng = np.random.default_rng(0)
pool = ScenePool([rng.integers(200, 6000, size=(5, args.extent, args.extent), dtype=np.uint16) for _ in range(args.scenes)], device=dev)
whole, split = pool.split([]), pool.split_blocks(args.block, args.fraction, seed=3)
dense = pool.split_blocks(args.dense_block, args.fraction, seed=3)
out = pool._outputs(B, T)
stream = torch.cuda.current_stream().cuda_stream
be = L.backend()


def arm(source, scales, other=None):
    """the entry ``source.sample`` would call, on the descriptor it would build, with only ``draw`` changing; ``other``: the entry
    of that name in another build of the library instead"""
    entry, d = source._describe(out, B, T, 3, 0, 0, "d4", 0, scales, None)
    fn, ref = getattr(be, entry), C.byref(d)
    if other:
        fn = getattr(C.CDLL(other), entry)
        fn.restype, fn.argtypes = L.PROTOTYPES[entry]

    def run(n):
        for i in range(n):
            d.draw = i
            assert fn(ref, stream) == 0
    run.keep = d
    return run


arms = {}
for scales in ((1,), (1, 2, 3, 4)):
    arms[f"scene_sample_scaled {scales}"] = (arm(pool, scales), None, scales)
    if args.other_lib:
        arms[f"scene_sample_scaled {scales}, other build"] = (arm(pool, scales, args.other_lib), None, scales)
    arms[f"scene_sample_origins whole scenes {scales}"] = (arm(whole.train, scales), whole, scales)
    arms[f"scene_sample_origins split_blocks({args.block}, {args.fraction}) {scales}"] = (arm(split.train, scales), split, scales)
arms[f"scene_sample_origins split_blocks({args.dense_block}, {args.fraction}) (1,)"] = (arm(dense.train, (1,)), dense, (1,))


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(n)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n


for fn, _, _ in arms.values():
    timed(fn, 20)
times = {k: [] for k in arms}
for r in range(args.reps):
    for k, (fn, _, _) in arms.items():
        times[k].append(timed(fn, args.calls))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    for k, (fn, source, scales) in arms.items():
        rows = None if source is None else {str(f): len(source.train.origins(T, f)) for f in scales}
        line = json.dumps({"arm": k, "device": torch.cuda.get_device_name(0), "bs": B, "size": T, "scenes": args.scenes, "extent": args.extent,
                           "held_out_rectangles": None if source is None else len(source.rectangles), "origin_rows": rows,
                           "reps": args.reps, "calls_per_rep": args.calls,
                           "us_per_call": {"median": round(statistics.median(times[k]), 2), "min": round(min(times[k]), 2), "max": round(max(times[k]), 2)}})
        print(line, flush=True)
        fh.write(line + "\n")
