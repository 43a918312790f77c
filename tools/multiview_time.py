#!/usr/bin/env python3
"""Time xfh_build_tracks + xfh_triangulate_views on S scenes of K tracks seen from V views (tests/multiview_support.arc_scene on the
MegaDepth-1500 cameras of tests/golden/megadepth1500_poses.npz: 0.5 px of noise, one observation in 50 moved by 50 - 150 px), and beside it,
as a yardstick only, the V - 1 calls of triangulate_matches that give each pair (0, v) its own points from the same lists.
    python tools/multiview_time.py [S,K,V]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd.multiview import build_tracks, triangulate_views_batch, triangulate_views_matches  # noqa: E402
from accelerated_features_amd.structure import triangulate_matches  # noqa: E402
import multiview_reference as MR  # noqa: E402
import multiview_support as MS  # noqa: E402
from twoview_support import timed  # noqa: E402

CASES = ((64, 4096, 3), (64, 4096, 8))
if len(sys.argv) > 1:                      # one case "S,K,V" (per-kernel profiles: rocprofv3 --kernel-trace --stats -- python tools/multiview_time.py 64,4096,8)
    CASES = (tuple(int(v) for v in sys.argv[1].split(",")),)
for S, K, V in CASES:
    rng = np.random.default_rng(0)
    sc = MS.arc_scene(rng, V, K, noise=0.5)                # one set of cameras, S draws of the observations' rows and noise
    kpts, idx_ref, idx_view, n = np.zeros((S, V, K, 2), np.float32), np.zeros((S, V - 1, K), np.int64), np.zeros((S, V - 1, K), np.int64), np.zeros((S, V - 1), np.int32)
    for s in range(S):
        one = MS.arc_scene(np.random.default_rng(s), V, K, noise=0.5)
        MS.plant_outliers(np.random.default_rng(s), one, frac=0.1)
        kpts[s] = one["kpts"]
        idx_ref[s], idx_view[s], n[s] = MS.match_lists(rng, one["tracks"], cap=K)
        if s == 0:
            sc = one
    Ks, Rs, ts = (np.repeat(sc[k][None], S, axis=0) for k in ("Ks", "Rs", "ts"))
    kp, ia, ib, nm = (torch.from_numpy(v).cuda() for v in (kpts, idx_ref, idx_view, n))
    Kd, Rd, td = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Ks, Rs, ts))
    r, ms_all = timed(lambda: triangulate_views_matches(kp, ia, ib, nm, None, Kd, Rd, td), 3, 20)
    tracks = r["tracks"]
    _, ms_tab = timed(lambda: build_tracks(ia, ib, nm, K), 3, 20)
    _, ms_tri = timed(lambda: triangulate_views_batch(kp, tracks, None, Kd, Rd, td), 3, 20)
    info = r["info"].cpu().numpy()
    ok = r["status"][0].cpu().numpy() == 0
    err = np.median(MS.world_error(r["points3d"][0].cpu().numpy(), sc["X"])[ok])
    print(f"S {S} K {K} V {V}: triangulate_views_matches {1e3 * ms_all:8.1f} us per call (build_tracks {1e3 * ms_tab:.1f} us, triangulate_views_batch "
          f"{1e3 * ms_tri:.1f} us); status counts {info[:, 1:].sum(axis=0).tolist()} of {int(info[:, 0].sum())}; median error / depth of scene 0 {err:.2e}", flush=True)
    # the yardstick: every pair (0, v) on its own
    rel = [MR.stage_view(sc["Rs"][v], sc["ts"][v], sc["Ks"][v], sc["Rs"][0], sc["ts"][0]) for v in range(V)]
    pair = []
    for v in range(1, V):
        Rv, tv = np.array(rel[v]["Rrel"]).reshape(3, 3), np.array(rel[v]["trel"])
        pair.append((kp[:, 0].contiguous(), kp[:, v].contiguous(), ia[:, v - 1].contiguous(), ib[:, v - 1].contiguous(), nm[:, v - 1].contiguous(),
                     torch.from_numpy(sc["Ks"][0]).cuda(), torch.from_numpy(sc["Ks"][v]).cuda(), torch.from_numpy(Rv).cuda(), torch.from_numpy(tv).cuda()))
    torch.cuda.synchronize()
    _, ms_pairs = timed(lambda: [triangulate_matches(*p) for p in pair][-1], 3, 20)
    print(f"S {S} K {K} V {V}: {V - 1} calls of triangulate_matches {1e3 * ms_pairs:8.1f} us (yardstick: one point per pair, no track, no rejection)", flush=True)
