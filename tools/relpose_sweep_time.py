#!/usr/bin/env python3
"""Time the relative-pose threshold sweep (xfh_estimate_relpose_sweep) against the calls it replaces, in one process: the 1500 synthetic
MegaDepth-1500 pairs of tests/twoview_support.py (200-1024 matches, 0.5-1 px noise, 40 % outliers) at the twelve ScanNet-1500 RANSAC
thresholds and 10000 iterations -- one sweep call against twelve estimate_relative_pose_batch calls -- and checks that every slice of the
sweep equals its single call.   python tools/relpose_sweep_time.py [--pairs 1500] [--iters 10000] [--reps 2]
`--only single` / `--only sweep` runs one of the two paths alone: under `rocprofv3 --kernel-trace --stats -- python
tools/relpose_sweep_time.py --only sweep --reps 1` the kernel table is that path's time by launch (the solve, bound and select kernels
are shared by the two paths, so each needs a run of its own)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from accelerated_features_amd import _lib, pose  # noqa: E402
from twoview_support import fixture, megadepth_synthetic, timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1500)
ap.add_argument("--iters", type=int, default=10000)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--only", choices=("both", "single", "sweep"), default="both")
args = ap.parse_args()
P, iters, thr = args.pairs, args.iters, pose.SCANNET_THRESHOLDS
T = len(thr)

f = fixture()
a, b, c = (torch.from_numpy(v).cuda() for v in megadepth_synthetic(f, P, 1024, 1500, 200))
K0, K1 = f["K0"][:P], f["K1"][:P]
lib = _lib.load()
chunks = lambda per_pair: -(-P // max(1, min(P, pose.WORKSPACE_LIMIT // per_pair)))   # noqa: E731
print(f"P {P}, {T} thresholds {thr[0]}..{thr[-1]} px, max_iterations {iters}: workspace per pair {lib.xfh_relpose_workspace_bytes(1, iters) >> 10} KiB "
      f"({chunks(lib.xfh_relpose_workspace_bytes(1, iters))} chunks per single call), sweep {lib.xfh_relpose_sweep_workspace_bytes(1, iters, T) >> 10} KiB "
      f"({chunks(lib.xfh_relpose_sweep_workspace_bytes(1, iters, T))} chunks)", flush=True)

singles, total = [], 0.0
for v in thr if args.only != "sweep" else ():
    r, ms = timed(lambda: pose.estimate_relative_pose_batch(a, b, c, K0, K1, v, max_iterations=iters), 1, args.reps)
    info = r["info"].cpu().numpy()
    print(f"single call at {v:3.1f} px: {ms:9.3f} ms, found {int(info[:, 0].sum())}/{P}, loop iterations mean {info[:, 2].mean():.0f} max {info[:, 2].max()}",
          flush=True)
    singles.append(r)
    total += ms
if args.only == "single":
    print(f"{T} single calls: {total:9.3f} ms")
    sys.exit(0)
sweep, ms = timed(lambda: pose.estimate_relative_pose_sweep_batch(a, b, c, K0, K1, thr, max_iterations=iters), 1, args.reps)
if args.only == "sweep":
    print(f"one sweep call: {ms:9.3f} ms")
    sys.exit(0)
same = all(torch.equal(sweep[k][:, j], singles[j][k]) for j in range(T) for k in sweep)
print(f"{T} single calls: {total:9.3f} ms    one sweep call: {ms:9.3f} ms    ratio {ms / total:.3f}    every slice equals its single call: {same}", flush=True)
sys.exit(0 if same else 1)
