#!/usr/bin/env python3
"""Time xfh_estimate_alignment on synthetic 3D-3D correspondences (tests/alignment_support.py: a cloud in a box, a similarity of scale
2.5, noise 0.01, 40 % outliers, 5 % NaN rows, max_error = 3 sqrt(3) sigma s): one pair with 2000 correspondences at 1000 iterations, and
1500 pairs (200-1024 correspondences) at 1000 iterations, whole calls between HIP events.   python tools/alignment_time.py [P,nlo,nhi,iters]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd.alignment import estimate_alignment_batch  # noqa: E402
from alignment_support import alignment_batch  # noqa: E402
from twoview_support import timed  # noqa: E402

CASES = ((1, 2000, 2000, 1000, 20), (1500, 200, 1024, 1000, 3))
if len(sys.argv) > 1:                      # one case "P,nlo,nhi,iters" (per-kernel profiles: rocprofv3 --kernel-trace --stats -- python tools/alignment_time.py 1500,200,1024,1000)
    CASES = (tuple(int(v) for v in sys.argv[1].split(",")) + (3,),)
for P, nlo, nhi, iters, reps in CASES:
    A, B, counts, gt, thr = alignment_batch(P, nhi, 1500, nlo)
    a, b, c = (torch.from_numpy(v).cuda() for v in (A, B, counts))
    for with_scale in (True, False):       # (the rigid fit of a cloud scaled by 2.5 finds nothing: it is timed, not judged)
        r, ms = timed(lambda: estimate_alignment_batch(a, b, c, thr, with_scale, max_iterations=iters), 1, reps)
        info, R, s = r["info"].cpu().numpy(), r["R"].cpu().numpy(), r["s"].cpu().numpy()
        line = f"P {P:4d} n {nlo}-{nhi} max_iterations {iters:5d} with_scale {int(with_scale)}: {ms:9.3f} ms per call, found {int(info[:, 0].sum())}/{P}, " \
               f"loop iterations mean {info[:, 2].mean():.0f} max {info[:, 2].max()}, refits {info[:, 4].mean():.1f}"
        if with_scale:
            rot = [np.rad2deg(np.arccos(np.clip((np.trace(gt[p][1].T @ R[p]) - 1.0) / 2.0, -1.0, 1.0))) if info[p, 0] else np.inf for p in range(P)]
            sc = [abs(s[p] / gt[p][0] - 1.0) if info[p, 0] else np.inf for p in range(P)]
            line += f", worst rotation error {max(rot):.3f} deg, worst relative scale error {max(sc):.2e}"
        print(line, flush=True)
