#!/usr/bin/env python3
"""Time verify_matches_graph and filter_matches_batch beside the build_tracks_graph call they precede (FINDINGS.md 3.22) at S scenes of V
views with K key-points and all V (V - 1) / 2 pairs: the lists of tests/verification_support.wrong_scene (0.5 px, a share `wrong` of wrong
matches, cap = K; one scene repeated S times), verified under the scene's true poses at 1 px.  Whole calls between HIP events, after two
untimed ones.  The bytes a call must move over its time are given as a share of the 8 TB/s HBM peak: whole-call figures.
    python tools/verify_time.py [S,V,K[,wrong]]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd import multiview as mv, verification as ver  # noqa: E402
import verification_support as VS  # noqa: E402
from twoview_support import timed  # noqa: E402

HBM_PEAK = 8.0e12
CASES = ((1, 32, 4096, 0.2), (64, 32, 4096, 0.2))
if len(sys.argv) > 1:
    c = sys.argv[1].split(",")
    CASES = ((int(c[0]), int(c[1]), int(c[2]), float(c[3]) if len(c) > 3 else 0.2),)
for S, V, K, wrong in CASES:
    sc = VS.wrong_scene(1, V=V, K=K, wrong=wrong)
    rep = lambda x: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x[None], (S,) + x.shape))).cuda()      # noqa: E731
    kpts, Ks, Rs, ts = (rep(sc[k]) for k in ("kpts", "Ks", "Rs", "ts"))
    vp, ia, ib, n = (rep(x) for x in sc["lists"])
    P, cap = ia.shape[1:]
    (mask, err, info), ms_verify = timed(lambda: ver.verify_matches_graph(kpts, vp, ia, ib, n, None, Ks, Rs, ts), 2, 10)
    (fa, fb, fn, src, finfo), ms_filter = timed(lambda: ver.filter_matches_batch(ia, ib, n, mask, min_keep=15), 2, 10)
    raw, ms_raw = timed(lambda: mv.build_tracks_graph(vp, ia, ib, n, V, K), 2, 5)
    good, ms_good = timed(lambda: mv.build_tracks_graph(vp, fa, fb, fn, V, K), 2, 5)
    read, kept = int(n[0].sum()), int(fn[0].sum())
    # the verifier reads two indices and two key-points per entry read and writes a mask byte and an error per slot; the filter reads the mask
    # of the entries read and the indices of the kept ones and writes every slot of its three lists
    moved_v = S * (read * (16 + 16) + P * cap * 5)
    moved_f = S * (read * 1 + kept * 16 + P * cap * 20)
    share = lambda b, ms: f"{b / 1e6:.0f} MB = {b / (ms * 1e-3) / 1e9:.0f} GB/s = {100 * b / (ms * 1e-3) / HBM_PEAK:.1f} % of the HBM peak"      # noqa: E731
    print(f"S {S} V {V} K {K} P {P} cap {cap} wrong {wrong}: {read} entries per scene, {kept} kept; verify_matches_graph {ms_verify:9.3f} ms "
          f"({share(moved_v, ms_verify)}); filter_matches_batch {ms_filter:9.3f} ms ({share(moved_f, ms_filter)}); build_tracks_graph raw "
          f"{ms_raw:9.3f} ms ({int(raw[2][0])} tracks, {int(raw[3][0, 3])} components dropped), on the verified lists {ms_good:9.3f} ms "
          f"({int(good[2][0])} tracks, {int(good[3][0, 3])} dropped)", flush=True)
    del kpts, ia, ib, mask, err, fa, fb, src, raw, good
    torch.cuda.empty_cache()
