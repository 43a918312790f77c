#!/usr/bin/env python3
"""Time xfh_triangulate_matches and xfh_recover_pose_matches on the synthetic MegaDepth-1500 set of the other time tools
(tests/twoview_support.megadepth_synthetic on tests/golden/megadepth1500_poses.npz: 0.5-1 px noise, 40 % outliers), under the true poses:
P pairs of `cap` matches on key-point lists of `cap` rows, and beside each time the bytes the call has to move and what they take at the
HBM rate a float4 copy reaches (6.3 TB/s).   python tools/structure_time.py [P,cap]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd.structure import recover_pose_matches, triangulate_matches  # noqa: E402
from twoview_support import essential_from_pose, fixture, megadepth_synthetic, timed  # noqa: E402

HBM = 6.3e12                               # bytes / s
CASES = ((32, 4096), (1, 4096), (1500, 1024))
if len(sys.argv) > 1:                      # one case "P,cap" (per-kernel profiles: rocprofv3 --kernel-trace --stats -- python tools/structure_time.py 32,4096)
    CASES = (tuple(int(v) for v in sys.argv[1].split(",")),)
f = fixture()
for P, cap in CASES:
    pts0, pts1, counts = megadepth_synthetic(f, P, cap, 1500, cap)      # every pair has cap matches
    rng = np.random.default_rng(0)
    idx0 = np.stack([rng.permutation(cap) for _ in range(P)]).astype(np.int64)      # the matches in a random order of the key-point rows
    idx1 = np.stack([rng.permutation(cap) for _ in range(P)]).astype(np.int64)
    k0, k1 = np.zeros_like(pts0), np.zeros_like(pts1)
    for p in range(P):
        k0[p, idx0[p]], k1[p, idx1[p]] = pts0[p], pts1[p]
    T = f["T_0to1"][:P]
    R, t = T[:, :3, :3].copy(), T[:, :3, 3] / np.linalg.norm(T[:, :3, 3], axis=1, keepdims=True)
    E = np.stack([essential_from_pose(R[p], t[p]) for p in range(P)])
    a, b, i0, i1, c = (torch.from_numpy(v).cuda() for v in (k0, k1, idx0, idx1, counts))
    K0, K1, Rd, td, Ed = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (f["K0"][:P], f["K1"][:P], R, t, E))
    n = P * cap
    r, ms = timed(lambda: triangulate_matches(a, b, i0, i1, c, K0, K1, Rd, td), 3, 20)
    # read: two indices, two key-points; written: point, status, error, the scattered point and the NaN fill of its row
    nbytes = n * (16 + 16 + 12 + 1 + 4 + 12 + 12)
    info = r["info"].cpu().numpy()
    print(f"P {P:4d} cap {cap}: triangulate_matches {1e3 * ms:8.1f} us per call (fill + kernel), {nbytes / 1e6:.1f} MB moved = {1e6 * nbytes / HBM:.1f} us at 6.3 TB/s; "
          f"status counts {info[:, 1:].sum(axis=0).tolist()} of {int(info[:, 0].sum())}", flush=True)
    r, ms = timed(lambda: recover_pose_matches(Ed, a, b, i0, i1, c, K0, K1), 3, 20)
    nbytes = n * (2 * (16 + 16) + 1 + 12)                  # two passes over the lists; mask and points written
    good = r["good"].cpu().numpy()
    print(f"P {P:4d} cap {cap}: recover_pose_matches {1e3 * ms:8.1f} us per call, {nbytes / 1e6:.1f} MB moved = {1e6 * nbytes / HBM:.1f} us at 6.3 TB/s; "
          f"found {int(r['info'][:, 0].sum())}/{P}, winner's share of the votes {good.max(axis=1).sum() / max(good.sum(), 1):.3f}", flush=True)
