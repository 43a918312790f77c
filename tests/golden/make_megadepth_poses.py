#!/usr/bin/env python3
"""Camera data of the MegaDepth-1500 pair list -> tests/golden/megadepth1500_poses.npz (data only).

Reads the reference's assets/megadepth_1500.json (path given as the first argument) and keeps, per pair: K0, K1 (3x3), T_0to1 (4x4),
scale0 / scale1 (2,) and size0_hw / size1_hw (2,).  The images are not part of the repository; the tests build synthetic
correspondences from these real intrinsics and relative poses.
    python tests/golden/make_megadepth_poses.py <reference>/assets/megadepth_1500.json"""
import json
import os
import sys

import numpy as np

DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "megadepth1500_poses.npz")

if __name__ == "__main__":
    d = json.load(open(sys.argv[1]))
    assert len(d) == 1500
    arr = {k: np.array([e[k] for e in d], np.float64) for k in ("K0", "K1", "T_0to1", "scale0", "scale1")}
    arr.update({k: np.array([e[k] for e in d], np.int32) for k in ("size0_hw", "size1_hw")})
    np.savez_compressed(DST, **arr)
    print({k: v.shape for k, v in arr.items()}, "->", DST)
