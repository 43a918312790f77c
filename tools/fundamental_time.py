#!/usr/bin/env python3
"""Time xfh_find_fundamental (USAC_MAGSAC) on synthetic correspondences built from the MegaDepth-1500 cameras and poses
(tests/golden/megadepth1500_poses.npz): one pair with 2000 matches at 1000 iterations, and the 1500 pairs (200-1024 matches, 0.5-1 px noise,
40 % outliers) at 1000 and at 10000 iterations; threshold 1.5 px.   python tools/fundamental_time.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from accelerated_features_amd.fundamental import find_fundamental_batch  # noqa: E402
import fundamental_reference as FR  # noqa: E402
import pose_reference as PR  # noqa: E402

f = dict(np.load(os.path.join(ROOT, "tests", "golden", "megadepth1500_poses.npz")))


def batch(P, nlo, nhi, seed):
    rng = np.random.default_rng(seed)
    cap = nhi
    pts0, pts1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    counts = rng.integers(nlo, nhi + 1, P).astype(np.int32)
    for p in range(P):
        a, b, _ = PR.synthetic_pair(f["K0"][p], f["K1"][p], f["T_0to1"][p], int(counts[p]), rng.uniform(0.5, 1.0), 0.4, tuple(f["size0_hw"][p]),
                                    tuple(f["size1_hw"][p]), rng)
        pts0[p, :counts[p]], pts1[p, :counts[p]] = a, b
    return torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.from_numpy(counts).cuda()


for P, nlo, nhi, iters, reps in ((1, 2000, 2000, 1000, 20), (1500, 200, 1024, 1000, 3), (1500, 200, 1024, 10000, 2)):
    a, b, c = batch(P, nlo, nhi, 1500)
    r = find_fundamental_batch(a, b, c, 1.5, iters)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        r = find_fundamental_batch(a, b, c, 1.5, iters)
    e1.record()
    torch.cuda.synchronize()
    info, F = r["info"].cpu().numpy(), r["F"].cpu().numpy()
    med = []
    for p in range(0, P, max(1, P // 100)):                  # held-out Sampson error of 100 sampled pairs
        if info[p, 0]:
            h0, h1, _ = PR.synthetic_pair(f["K0"][p], f["K1"][p], f["T_0to1"][p], 200, 0.0, 0.0, tuple(f["size0_hw"][p]), tuple(f["size1_hw"][p]),
                                          np.random.default_rng(p))
            med.append(np.median(FR.sampson_px(F[p], h0, h1)))
    print(f"P {P:4d} n {nlo}-{nhi} max_iters {iters:5d}: {e0.elapsed_time(e1) / reps:9.3f} ms per call, found {int(info[:, 0].sum())}/{P}, "
          f"loop iterations mean {info[:, 2].mean():.0f} max {info[:, 2].max()}, refinement steps {info[:, 4].mean():.1f}, "
          f"held-out Sampson error median {np.median(med):.3f} px", flush=True)
