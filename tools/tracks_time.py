#!/usr/bin/env python3
"""Time xfh_build_tracks_graph and, behind it, xfh_triangulate_tracks on S scenes of V views with K key-points each
(tests/multiview_support.arc_scene on the MegaDepth-1500 cameras of tests/golden/megadepth1500_poses.npz, 0.5 px of noise), for the matches
of the chain of pairs (v, v + 1) and of all V (V - 1) / 2 pairs.  Whole calls between HIP events.  The lists of DRAWS scenes are drawn and
repeated over the S scenes (the lists of all pairs at V = 32 hold 130 million matches).
    python tools/tracks_time.py [S,K,V,chain|all]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd.multiview import build_tracks_graph, triangulate_views_batch  # noqa: E402
import multiview_support as MS  # noqa: E402
import tracks_support as TKS  # noqa: E402
from twoview_support import timed  # noqa: E402

DRAWS = 4
CASES = ((64, 4096, 8, "chain"), (64, 4096, 8, "all"), (64, 4096, 32, "chain"), (64, 4096, 32, "all"))
if len(sys.argv) > 1:                      # one case "S,K,V,chain|all"
    c = sys.argv[1].split(",")
    CASES = ((int(c[0]), int(c[1]), int(c[2]), c[3]),)
for S, K, V, graph in CASES:
    pairs = TKS.chain_pairs(V) if graph == "chain" else TKS.all_pairs(V)
    P = len(pairs)
    draws = []
    for s in range(min(DRAWS, S)):
        rng = np.random.default_rng(s)
        one = MS.arc_scene(rng, V, K, noise=0.5)
        draws.append((one, TKS.pair_lists(rng, one["tracks"], pairs, cap=K, kcap=K)))
    sc = draws[0][0]
    pick = [s % len(draws) for s in range(S)]
    kp = torch.from_numpy(np.stack([d[0]["kpts"] for d in draws])).cuda()[pick].contiguous()
    vp = torch.from_numpy(draws[0][1][0]).cuda()
    ia, ib, nm = (torch.from_numpy(np.stack([d[1][i] for d in draws])).cuda()[pick].contiguous() for i in (1, 2, 3))
    Kd, Rd, td = (torch.from_numpy(np.ascontiguousarray(np.repeat(sc[k][None], S, axis=0))).cuda() for k in ("Ks", "Rs", "ts"))
    reps = 20 if graph == "chain" else 5
    (tracks, track_of, n_tracks, info), ms_graph = timed(lambda: build_tracks_graph(vp, ia, ib, nm, V, K), 2, reps)
    r, ms_tri = timed(lambda: triangulate_views_batch(kp, tracks, None, Kd, Rd, td, anchor="first"), 2, reps)
    info = info.cpu().numpy()
    n0 = int(n_tracks[0])
    ok = r["status"][0, :n0].cpu().numpy() == 0
    first = tracks[0, :n0].cpu().numpy()
    src = np.array([np.nonzero(sc["tracks"][:, v] == row)[0][0] for v, row in ((int(np.argmax(t >= 0)), t[np.argmax(t >= 0)]) for t in first)])
    err = np.median(MS.world_error(r["points3d"][0, :n0].cpu().numpy(), sc["X"][src])[ok])
    print(f"S {S} K {K} V {V} {graph} ({P} pairs, {int(nm.sum())} matches): build_tracks_graph {1e3 * ms_graph:9.1f} us per call, triangulate_views_batch"
          f"(anchor='first') over {tracks.shape[1]} rows {1e3 * ms_tri:9.1f} us; per scene: nodes {info[:, 0].mean():.0f}, tracks {info[:, 2].mean():.0f}, "
          f"inconsistent {info[:, 3].mean():.0f}, status {sorted(set(info[:, 6].tolist()))}; valid of scene 0 {int(ok.sum())}/{n0}, median error / depth {err:.2e}",
          flush=True)
    del kp, ia, ib, nm, tracks, track_of, r
    torch.cuda.empty_cache()
