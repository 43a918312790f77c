#!/usr/bin/env python3
"""Time xfh_average_poses at S scenes of V views with all V (V - 1) / 2 pairs, the relative poses of those S P pairs that feed it
(``relative_poses_graph_matches`` on tests/multiview_support.arc_scene, K key-points, 0.5 px of noise, 1000 RANSAC iterations) in the same
run, and the stages of ``reconstruct_graph_matches`` one by one.  Whole calls between HIP events, after two untimed ones.
    python tools/posegraph_time.py [S,V,K]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd import multiview as mv  # noqa: E402
import multiview_support as MS  # noqa: E402
import posegraph_support as PS  # noqa: E402
import tracks_support as TKS  # noqa: E402
from twoview_support import timed  # noqa: E402

DRAWS = 2
CASES = ((64, 32, 512), (8, 8, 1024))
if len(sys.argv) > 1:
    CASES = (tuple(int(x) for x in sys.argv[1].split(",")),)
for S, V, K in CASES:
    pairs = TKS.all_pairs(V)
    P = len(pairs)
    # ---- the averaging alone, on synthetic edges with 0.5 degrees of noise and 15 % outlier edges
    scenes = [PS.scene(s, V, PS.all_pairs(V), 0.5, 0.15) for s in range(min(DRAWS, S))]
    b = PS.batch([scenes[s % len(scenes)] for s in range(S)])
    vp, Rr, tr, w = (torch.from_numpy(x).cuda() for x in b[:4])
    r, ms = timed(lambda: mv.average_poses_batch(vp, Rr, tr, w, V), 2, 10)
    info = r["info"].cpu().numpy()
    print(f"S {S} V {V} P {P}: average_poses_batch {1e3 * ms:9.1f} us per call (30 rounds, 10 redescending); status {sorted(set(info[:, 6].tolist()))}, "
          f"rotation outliers {info[:, 3].mean():.0f}, position outliers {info[:, 4].mean():.0f} of {int(scenes[0]['outlier'].sum())}", flush=True)
    # ---- the relative poses that feed it, and the chain by stage
    draws = []
    for s in range(min(DRAWS, S)):
        rng = np.random.default_rng(s)
        one = MS.arc_scene(rng, V, K, noise=0.5)
        draws.append((one, TKS.pair_lists(rng, one["tracks"], pairs, cap=K, kcap=K)))
    pick = [s % len(draws) for s in range(S)]
    kp = torch.from_numpy(np.stack([d[0]["kpts"] for d in draws])).cuda()[pick].contiguous()
    gp = torch.from_numpy(draws[0][1][0]).cuda()
    ia, ib, nm = (torch.from_numpy(np.stack([d[1][i] for d in draws])).cuda()[pick].contiguous() for i in (1, 2, 3))
    Kd = torch.from_numpy(np.ascontiguousarray(np.repeat(draws[0][0]["Ks"][None], S, axis=0))).cuda()
    ransac = dict(max_iterations=1000)
    rel, ms_rel = timed(lambda: mv.relative_poses_graph_matches(kp, gp, ia, ib, nm, Kd, **ransac), 1, 3)
    pg, ms_pg = timed(lambda: mv.average_poses_batch(gp, rel["R_rel"], rel["t_rel"], rel["weight"], V), 2, 10)
    tri, ms_tri = timed(lambda: mv.triangulate_graph_matches(kp, gp, ia, ib, nm, None, Kd, pg["Rs"], pg["ts"]), 1, 3)
    ba, ms_ba = timed(lambda: mv.bundle_adjust_batch(kp, tri["tracks"], tri["inlier_views"], tri["points3d"], None, Kd, pg["Rs"], pg["ts"]), 1, 3)
    fin, ms_fin = timed(lambda: mv.triangulate_views_batch(kp, tri["tracks"], None, Kd, ba["Rs"], ba["ts"], anchor="first"), 1, 3)
    out, ms_all = timed(lambda: mv.reconstruct_graph_matches(kp, gp, ia, ib, nm, None, Kd, ransac=ransac), 1, 3)
    info = pg["info"].cpu().numpy()
    print(f"S {S} V {V} K {K} ({S * P} pairs, {int(nm.sum())} matches): relative poses {ms_rel:9.3f} ms, average_poses_batch {ms_pg:9.3f} ms "
          f"({100.0 * ms_pg / ms_rel:.1f} % of the relative poses), tracks + triangulation {ms_tri:9.3f} ms, bundle adjustment {ms_ba:9.3f} ms, "
          f"second triangulation {ms_fin:9.3f} ms; reconstruct_graph_matches {ms_all:9.3f} ms; pose-graph status {sorted(set(info[:, 6].tolist()))}, "
          f"weights > 0: {int((rel['weight'] > 0).sum())}, valid points of scene 0: {int(out['valid'][0].sum())}", flush=True)
    del kp, ia, ib, nm, rel, pg, tri, ba, fin, out
    torch.cuda.empty_cache()
