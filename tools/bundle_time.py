#!/usr/bin/env python3
"""Time xfh_bundle_adjust on S scenes of K tracks seen from V views (tests/bundle_support.scene: tests/multiview_support.arc_scene at 0.5 px of
noise, the free views perturbed by 0.2 degrees and 0.02 units, views 0 and 1 held), and beside it, for scale, triangulate_views_batch on the
same scenes.
    python tools/bundle_time.py [S,K,V]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd.multiview import bundle_adjust_batch, triangulate_views_batch  # noqa: E402
import bundle_support as BS  # noqa: E402
from twoview_support import timed  # noqa: E402

CASES = ((64, 4096, 3), (64, 4096, 8), (64, 4096, 32))
if len(sys.argv) > 1:                      # one case "S,K,V" (per-kernel profiles: rocprofv3 --kernel-trace --stats -- python tools/bundle_time.py 64,4096,8)
    CASES = (tuple(int(v) for v in sys.argv[1].split(",")),)
for S, K, V in CASES:
    base = [BS.scene(s, V, K, noise=0.5, fixed=3) for s in range(min(S, 4))]      # four draws, repeated over the batch
    scenes = [base[s % len(base)] for s in range(S)]
    kp, tr, Ks, Rs, ts = (torch.from_numpy(np.stack([sc[k] for sc in scenes])).cuda() for k in ("kpts", "tracks", "Ks", "Rs0", "ts0"))
    tri, ms_tri = timed(lambda: triangulate_views_batch(kp, tr, None, Ks, Rs, ts, max_reproj_error=BS.GATE), 3, 10)
    r, ms_ba = timed(lambda: bundle_adjust_batch(kp, tr, tri["inlier_views"], tri["points3d"], None, Ks, Rs, ts, fixed_views=3), 2, 5)
    info, cost = r["info"].cpu().numpy(), r["cost"].cpu().numpy()
    e0 = BS.pose_errors(base[0], base[0]["Rs0"], base[0]["ts0"])
    e1 = BS.pose_errors(base[0], r["Rs"][0].cpu().numpy(), r["ts"][0].cpu().numpy())
    print(f"S {S} K {K} V {V}: bundle_adjust_batch {ms_ba:8.2f} ms per call ({ms_ba / max(info[:, 3].max(), 1):.2f} ms per round of the longest scene; rounds "
          f"{info[:, 3].min()} - {info[:, 3].max()}, accepted {info[:, 4].min()} - {info[:, 4].max()}), triangulate_views_batch {1e3 * ms_tri:.1f} us; cost of scene 0 "
          f"{cost[0, 0]:.4e} -> {cost[0, 1]:.4e}; worst rotation / centre error of scene 0 {e0[0]:.3f} deg / {e0[1]:.1e} -> {e1[0]:.3f} deg / {e1[1]:.1e}", flush=True)
