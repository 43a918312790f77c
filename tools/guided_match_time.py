#!/usr/bin/env python3
"""Time of the guided matcher beside the plain ones, whole calls between HIP events (warm-up, inputs resident): 32 pairs of 4096 x 4096 unit descriptors with
synthetic key-points on the MegaDepth-1500 fixture cameras (tests/guided_reference.py: 3/4 true correspondences, the rest clutter).
    python tools/guided_match_time.py [reps]
Lines: the ungated exact kernel (match_exact = 1), the shipped default matcher, the guided kernel with the F gate and with the H gate at 3 px, the guided / exact ratios.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures  # noqa: E402
import guided_reference as GR  # noqa: E402
import twoview_support as TS  # noqa: E402
from accelerated_features_amd import XFeat  # noqa: E402
from accelerated_features_amd.guided import match_guided_device  # noqa: E402

P, N, THR = 32, 4096, 3.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
xf = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=N)
t = lambda v, dt=None: (torch.from_numpy(np.ascontiguousarray(v)) if dt is None else torch.from_numpy(np.ascontiguousarray(v)).to(dt)).cuda()
nv = torch.full((P,), N, dtype=torch.int32).cuda()
res = {}
for kind in GR.KINDS:
    sc = [GR.epipolar_scene(p, N, N, 4000 + p) if kind == 'fundamental' else GR.planar_scene(N, N, 4000 + p) for p in range(P)]
    d1, k1, d2, k2 = (t(np.stack([s[k] for s in sc])) for k in ('d1', 'k1', 'd2', 'k2'))
    models = t(np.stack([s['model'] for s in sc]))
    if kind == 'fundamental':
        for name, exact in (("exact (match_exact = 1)", 1), ("default (fp16 filter + refine)", 0)):
            xf.set_option("match_exact", exact)
            r, ms = TS.timed(lambda: xf.match_sets_device(d1, nv, d2, nv, -1), 3, reps)
            xf.set_option("match_exact", 0)
            res[name] = ms
            print(f"{name:34s} {ms:8.3f} ms per call of {P} x {N} x {N}, matches {int(r[2].sum())}", flush=True)
    r, ms = TS.timed(lambda: match_guided_device(d1, k1, nv, d2, k2, nv, models, kind, THR, -1), 3, reps)
    res[kind] = ms
    true = sum(GR.true_matches(s, r[0][p, :int(r[2][p])].cpu().numpy(), r[1][p, :int(r[2][p])].cpu().numpy()) for p, s in enumerate(sc))
    print(f"guided, {kind:11s} gate at {THR} px  {ms:8.3f} ms per call, matches {int(r[2].sum())}, true {true} of {sum(len(s['truth']) for s in sc)}", flush=True)
ex = res["exact (match_exact = 1)"]
print(f"guided / exact: F {res['fundamental'] / ex:.3f}, H {res['homography'] / ex:.3f}")
