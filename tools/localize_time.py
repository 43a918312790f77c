#!/usr/bin/env python3
"""Time build_map_batch and localize_map_batch (FINDINGS.md 3.21) at S scenes of V views with K key-points: the map of the views 0 .. V-1 of
tests/localization_support.descriptor_scene (0.5 px, sigma 0.05; one scene repeated S times), then Q = S queries (view V) against it, plain
and guided.  Whole calls between HIP events, after two untimed ones.  For the map the bytes it must move (the contributing descriptor rows, the
track tables, the rows written) over the call's time are given as a share of the 8 TB/s HBM peak: a whole-call figure (three launches and
the workspace allocation), not a kernel's.
    python tools/localize_time.py [S,V,K]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd import localization as loc, multiview as mv  # noqa: E402
import localization_support as LS  # noqa: E402
from twoview_support import timed  # noqa: E402

HBM_PEAK = 8.0e12
CASES = ((1, 8, 4096), (64, 8, 4096))
if len(sys.argv) > 1:
    CASES = (tuple(int(x) for x in sys.argv[1].split(",")),)
for S, V, K in CASES:
    sc = LS.descriptor_scene(np.random.default_rng(1), V + 1, K, 0.5, 0.05)
    rep = lambda x: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[None], (S,) + x.shape))).cuda()      # noqa: E731
    kpts, tracks, desc = rep(sc["kpts"][:V]), rep(sc["tracks"][:, :V]), rep(sc["desc"][:V])
    Ks, Rs, ts = (rep(sc[k][:V]) for k in ("Ks", "Rs", "ts"))
    tri = mv.triangulate_views_batch(kpts, tracks, None, Ks, Rs, ts)
    args = (desc, tracks, tri["points3d"], tri["status"], tri["inlier_views"])
    m, ms_map = timed(lambda: loc.build_map_batch(*args), 2, 10)
    info = m["info"][0].cpu().tolist()
    T, M = tracks.shape[1], m["desc"].shape[1]
    moved = S * (int(m["n_obs"][0].sum()) * 256 + T * (V * 4 + 12 + 1 + 4) + M * (256 + 128 + 12 + 4 + 1 + 4))
    q = (rep(sc["kpts"][V]), rep(sc["desc"][V]), torch.full((S,), K, dtype=torch.int32).cuda())
    Kq = rep(sc["Ks"][V])
    size = sc["sizes"][V][::-1]
    one, ms_plain = timed(lambda: loc.localize_map_batch(*q, m, Kq, min_cossim=0.8), 2, 5)
    two, ms_guided = timed(lambda: loc.localize_map_batch(*q, m, Kq, min_cossim=0.8, guided=True, image_size=size), 2, 5)
    er, ec = LS.truth_pose_errors(two["R"][0].cpu().numpy(), two["t"][0].cpu().numpy(), sc["Rs"][V], sc["ts"][V])
    print(f"S {S} V {V} K {K} (T {T}, map rows {info[1]}, skipped {info[2:6]}): build_map_batch {ms_map:9.3f} ms, {moved / 1e6:.1f} MB to move = "
          f"{moved / (ms_map * 1e-3) / 1e9:.0f} GB/s = {100 * moved / (ms_map * 1e-3) / HBM_PEAK:.1f} % of the HBM peak (whole call); "
          f"localize_map_batch Q {S}: plain {ms_plain:9.3f} ms ({int(one['n_matches'][0])} matches, {int(one['info'][0, 3])} inliers), "
          f"guided {ms_guided:9.3f} ms ({int(two['n_matches'][0])} matches, {int(two['info'][0, 3])} inliers, stage {int(two['stage'][0])}); "
          f"rotation error {er:.5f} degrees, centre error {ec:.5f}", flush=True)
    del kpts, tracks, desc, tri, args, m, q, one, two
    torch.cuda.empty_cache()
