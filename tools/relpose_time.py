#!/usr/bin/env python3
"""Time xfh_estimate_relpose on synthetic correspondences built from the MegaDepth-1500 cameras and poses (tests/golden/megadepth1500_poses.npz):
one pair with 2000 matches at 1000 iterations, and the 1500 pairs (200-1024 matches, 0.5-1 px noise, 40 % outliers) at 1000 and at
10000 iterations.   python tools/relpose_time.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from accelerated_features_amd.pose import estimate_relative_pose_batch, pose_auc, relative_pose_error  # noqa: E402
from twoview_support import time_megadepth  # noqa: E402


def auc(f, P, r, info):
    R, t = r["R"].cpu().numpy(), r["t"].cpu().numpy()
    err = [max(relative_pose_error(f["T_0to1"][p], R[p], t[p])) if info[p, 0] else np.inf for p in range(P)]
    return f"AUC {pose_auc(err)}"


time_megadepth(lambda a, b, c, f, P, iters: estimate_relative_pose_batch(a, b, c, f["K0"][:P], f["K1"][:P], 1.0, max_iterations=iters),
               "max_iterations", auc)
