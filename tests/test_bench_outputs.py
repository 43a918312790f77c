"""bench.py's plain run and --dump-outputs: the arrays of the last timed step, their unspecified padding rows written as fixed values (host), and a
plain run on the GPU that times exactly --steps steps, prints the headline keys without the --full figures and leaves the outputs on disk."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DUMP_BYTES = 64 * 2 ** 20


def _dir_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def test_dump_outputs_fixes_padding_rows_and_stays_small(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    B, K = 64, 4096
    g = torch.Generator().manual_seed(5)
    nv = torch.randint(K // 2, K + 1, (B,), generator=g, dtype=torch.int32)
    nm = torch.randint(0, K // 2, (B // 2,), generator=g, dtype=torch.int32)
    r = {"keypoints": torch.rand(B, K, 2, generator=g) * 640, "scores": torch.rand(B, K, generator=g), "descriptors": torch.randn(B, K, 64, generator=g),
         "idx0": torch.randint(0, K, (B // 2, K), generator=g), "idx1": torch.randint(0, K, (B // 2, K), generator=g),
         "n_valid": nv, "n_candidates": nv + 100, "n_matches": nm}
    out = str(tmp_path / "a")
    names = bench.dump_outputs(out, r)
    assert sorted(f[:-4] for f in os.listdir(out)) == names
    assert _dir_bytes(out) <= MAX_DUMP_BYTES
    a = {n: np.load(os.path.join(out, n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    rows = a["descriptor_sample_rows"].astype(np.int64)
    for b in range(B):
        n = int(nv[b])
        assert np.array_equal(a["keypoints"][b, :n], r["keypoints"][b, :n].numpy()) and not a["keypoints"][b, n:].any()
        assert np.array_equal(a["scores"][b, :n], r["scores"][b, :n].numpy()) and not a["scores"][b, n:].any()
        assert np.array_equal(a["descriptors_sample"][b, rows < n], r["descriptors"][b, rows[rows < n]].numpy()) and not a["descriptors_sample"][b, rows >= n].any()
    for p in range(B // 2):
        n = int(nm[p])
        for k in ("idx0", "idx1"):
            assert np.array_equal(a[k][p, :n], r[k][p, :n].numpy()) and (a[k][p, n:] == -1).all()
    assert np.array_equal(a["n_valid"], nv.numpy()) and np.array_equal(a["n_matches"], nm.numpy())
    # the padding rows do not reach the files: other garbage there, the same files
    r2 = dict(r, keypoints=r["keypoints"].clone(), idx0=r["idx0"].clone())
    r2["keypoints"][0, int(nv[0]):] = -7.0
    r2["idx0"][0, int(nm[0]):] = 3
    out2 = str(tmp_path / "b")
    bench.dump_outputs(out2, r2)
    assert all(np.array_equal(np.load(os.path.join(out, n + ".npy")), np.load(os.path.join(out2, n + ".npy"))) for n in names)


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    out = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - d["config"]["batch_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert not {"roofline", "roofline_match", "cpu_baseline", "single_lane_synchronous_fps"} & d.keys() and "gpu_state" not in d["config"]
    assert _dir_bytes(out) <= MAX_DUMP_BYTES
    nv = np.load(os.path.join(out, "n_valid.npy"))
    nm = np.load(os.path.join(out, "n_matches.npy"))
    kp = np.load(os.path.join(out, "keypoints.npy"))
    i0 = np.load(os.path.join(out, "idx0.npy"))
    assert nv.shape == (64,) and kp.shape == (64, 4096, 2) and i0.shape == (32, 4096)
    assert round(float(nv.mean()), 1) == d["config"]["mean_keypoints"] and round(float(nm.mean()), 1) == d["config"]["mean_matches"]
    assert (nv > 0).all() and (nm > 0).all()
    for b in range(64):
        assert not kp[b, int(nv[b]):].any() and (kp[b, :int(nv[b])] >= 0).all()
    for p in range(32):
        n = int(nm[p])
        assert (i0[p, n:] == -1).all() and (i0[p, :n] >= 0).all() and (i0[p, :n] < nv[2 * p]).all()
