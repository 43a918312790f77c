#!/usr/bin/env python3
"""Time xfh_estimate_abspose on synthetic 2D-3D correspondences built from the MegaDepth-1500 cameras and poses
(tests/golden/megadepth1500_poses.npz; tests/abspose_support.py): one pair with 2000 matches at 1000 iterations, and the 1500 pairs
(200-1024 matches, 0.5-1 px noise, 40 % outliers) at 1000 and at 10000 iterations, at max_reproj_error 3 px.   python tools/abspose_time.py [P,nlo,nhi,iters]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd.absolute_pose import estimate_absolute_pose_batch  # noqa: E402
from abspose_support import abspose_batch, pose_errors  # noqa: E402
from twoview_support import timed  # noqa: E402

CASES = ((1, 2000, 2000, 1000, 20), (1500, 200, 1024, 1000, 3), (1500, 200, 1024, 10000, 2))
if len(sys.argv) > 1:                      # one case "P,nlo,nhi,iters" (per-kernel profiles: rocprofv3 --kernel-trace --stats -- python tools/abspose_time.py 1500,200,1024,1000)
    CASES = (tuple(int(v) for v in sys.argv[1].split(",")) + (3,),)
for P, nlo, nhi, iters, reps in CASES:
    pts2d, pts3d, counts, K, T = abspose_batch(P, nhi, 1500, nlo)
    a, b, c = (torch.from_numpy(v).cuda() for v in (pts2d, pts3d, counts))
    r, ms = timed(lambda: estimate_absolute_pose_batch(a, b, c, K, 3.0, max_iterations=iters), 1, reps)
    info, R, t = r["info"].cpu().numpy(), r["R"].cpu().numpy(), r["t"].cpu().numpy()
    err = np.array([pose_errors(T[p], R[p], t[p]) if info[p, 0] else (np.inf, np.inf) for p in range(P)])
    print(f"P {P:4d} n {nlo}-{nhi} max_iterations {iters:5d}: {ms:9.3f} ms per call, found {int(info[:, 0].sum())}/{P}, "
          f"loop iterations mean {info[:, 2].mean():.0f} max {info[:, 2].max()}, refinement steps {info[:, 4].mean():.1f}, "
          f"worst rotation error {err[:, 0].max():.3f} deg, worst position error {100 * err[:, 1].max():.3f} %", flush=True)
