#!/usr/bin/env python3
"""Time xfh_find_fundamental (USAC_MAGSAC) on synthetic correspondences built from the MegaDepth-1500 cameras and poses
(tests/golden/megadepth1500_poses.npz): one pair with 2000 matches at 1000 iterations, and the 1500 pairs (200-1024 matches, 0.5-1 px noise,
40 % outliers) at 1000 and at 10000 iterations; threshold 1.5 px.   python tools/fundamental_time.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from accelerated_features_amd.fundamental import find_fundamental_batch  # noqa: E402
from twoview_support import holdout, sampson_px, time_megadepth  # noqa: E402


def holdout_error(f, P, r, info):
    F = r["F"].cpu().numpy()
    med = []
    for p in range(0, P, max(1, P // 100)):                  # held-out Sampson error of 100 sampled pairs
        if info[p, 0]:
            med.append(np.median(sampson_px(F[p], *holdout(f, p, 200))))
    return f"held-out Sampson error median {np.median(med):.3f} px"


time_megadepth(lambda a, b, c, f, P, iters: find_fundamental_batch(a, b, c, 1.5, iters), "max_iters", holdout_error)
