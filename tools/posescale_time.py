#!/usr/bin/env python3
"""Time xfh_baseline_ratios and the pose graph with and without the ratio terms (FINDINGS.md 3.20) at S scenes of V = 32 views with K = 4096
key-points: all 496 pairs (14 880 wedges) and the chain of 31 pairs (30 wedges), on tests/posescale_support.scene (0.5 px, 0.5 degrees).  Whole
calls between HIP events, after two untimed ones.
    python tools/posescale_time.py [S,V,K]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd import multiview as mv  # noqa: E402
import posegraph_support as PS  # noqa: E402
import posescale_support as QS  # noqa: E402
from twoview_support import timed  # noqa: E402

CASES = ((1, 32, 4096), (64, 32, 4096))
if len(sys.argv) > 1:
    CASES = (tuple(int(x) for x in sys.argv[1].split(",")),)
for S, V, K in CASES:
    for graph, pairs in (("chain", PS.chain_pairs(V)), ("all pairs", PS.all_pairs(V))):
        sc = QS.scene(1, V, K, pairs)
        rep = lambda x: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[None], (S,) + x.shape))).cuda()      # noqa: E731
        a = [rep(sc[k]) for k in ("kpts", "tracks", "track_of", "pairs", "Rrel", "trel", "weight", "Ks")]
        r, ms_r = timed(lambda: mv.baseline_ratios_batch(*a, max_reproj_error=32.0), 2, 5)
        e = a[3:7]
        pg0, ms_0 = timed(lambda: mv.average_poses_batch(*e, V), 2, 5)
        pg1, ms_1 = timed(lambda: mv.average_poses_batch(*e, V, ratio=r["ratio"], ratio_count=r["count"]), 2, 5)
        info = r["info"][0].cpu().tolist()
        print(f"S {S} V {V} K {K} {graph} (P {len(pairs)}, wedges {info[0]}, with a ratio {info[1]}, tracks valid {info[3]} of {info[2]}): "
              f"baseline_ratios_batch {ms_r:9.3f} ms, average_poses_batch {ms_0:9.3f} ms without / {ms_1:9.3f} ms with ratios "
              f"({ms_1 / ms_0:.1f} x); status {pg0['info'][0, 6].item()} / {pg1['info'][0, 6].item()}", flush=True)
        del a, r, pg0, pg1
        torch.cuda.empty_cache()
