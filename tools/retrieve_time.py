#!/usr/bin/env python3
"""Time the retrieval stage (FINDINGS.md 3.23): global_descriptors_batch (xfh_vlad) at B = 64 images of K = 4096 descriptors over C = 64
centroids, and retrieve_topk (xfh_retrieve_topk) at Q = 64 queries against N = 1024 and N = 65536 database vectors of D = 4096 with k = 16,
beside torch.matmul + torch.topk on the same tensors (the yardstick: the parent has no retrieval).  Whole calls between HIP events, 20 runs
after 3 untimed ones.  The bytes a call must move over its time are given as a share of the 8 TB/s HBM peak: whole-call figures.
    python tools/retrieve_time.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd import retrieval as rt  # noqa: E402
from twoview_support import timed  # noqa: E402

HBM_PEAK = 8.0e12
WARM, RUNS = 3, 20
share = lambda b, ms: f"{b / 1e6:.0f} MB = {b / (ms * 1e-3) / 1e9:.0f} GB/s = {100 * b / (ms * 1e-3) / HBM_PEAK:.1f} % of the HBM peak"      # noqa: E731

torch.manual_seed(0)
B, K, C = 64, 4096, 64
desc = torch.nn.functional.normalize(torch.randn((B, K, 64), device="cuda"), dim=2)
book = rt.train_codebook(desc[:8], None, C, 5)["codebook"]
out, ms = timed(lambda: rt.global_descriptors_batch(desc, None, book), WARM, RUNS)
# the descriptors are read twice (assignment, sums), the assignment is written and read, the chunk sums written and read, the vectors written
moved = B * K * 64 * 4 * 2 + B * K * 4 * 2 + B * (K // 1024) * C * 256 * 2 + B * C * 256
print(f"xfh_vlad B {B} K {K} C {C}: {ms:9.3f} ms per call ({share(moved, ms)}); non-empty blocks mean {out['info'][:, 2].float().mean().item():.1f}", flush=True)

Q, D, k = 64, 4096, 16
for N in (1024, 65536):
    db = torch.nn.functional.normalize(torch.randn((N, D), device="cuda"), dim=1)
    q = torch.nn.functional.normalize(db[:Q] + 0.05 * torch.randn((Q, D), device="cuda"), dim=1)
    got, ms = timed(lambda: rt.retrieve_topk(q, db, k), WARM, RUNS)
    ref, ms_torch = timed(lambda: torch.topk(torch.matmul(q, db.t()), k, dim=1), WARM, RUNS)
    agree = (got["idx"].long() == ref.indices).float().mean().item()
    # both read the queries and the database once and write and read the Q x N scores
    moved = (Q + N) * D * 4 + Q * N * 4 * 2
    print(f"xfh_retrieve_topk Q {Q} N {N} D {D} k {k}: {ms:9.3f} ms per call ({share(moved, ms)}); torch.matmul + torch.topk {ms_torch:9.3f} ms "
          f"({share(moved, ms_torch)}); slots that agree {100 * agree:.2f} %", flush=True)
    del db, q
    torch.cuda.empty_cache()
