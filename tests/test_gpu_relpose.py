"""xfh_estimate_relpose (csrc/k_relpose.hip) on the MI355X against the numpy restatement tests/pose_reference.py: the winner, the
iteration count, the inlier count, the integer cost and the mask exactly; R, t and E to 1e-9."""
import numpy as np
import pytest
import torch

import pose_reference as PR
from twoview_support import check_common, fixture as _fixture, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pose():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import pose as m
    return m


def _check(got, want, p, n):
    check_common(got, want, p, n)
    for k in ("R", "t", "E"):
        g = got[k][p].cpu().numpy()
        assert np.isfinite(g).all()
        assert np.abs(g - want[k]).max() <= 1e-9, (k, g, want[k])


@pytest.mark.parametrize("n,outliers,thr,iters", [(5, 0.0, 1.0, 1000), (6, 0.0, 2.5, 1000), (300, 0.3, 1.0, 1000), (300, 0.8, 2.5, 10000),
                                                  (2000, 0.5, 1.0, 1000), (4096, 0.6, 2.5, 10000), (2000, 0.0, 1.0, 10000)])
def test_single_pair_equals_the_restatement(pose, n, outliers, thr, iters):
    p0, p1, _, K0, K1, _ = scene(7, n, 0.7, outliers, seed=n)
    got = pose.estimate_relative_pose_batch(torch.from_numpy(p0)[None].cuda(), torch.from_numpy(p1)[None].cuda(), None, K0, K1, thr,
                                            max_iterations=iters, seed=11)
    torch.cuda.synchronize()
    want = PR.estimate(p0, p1, K0, K1, thr, max_iterations=iters, seed=11)
    _check(got, want, 0, n)


def test_ragged_batch_equals_the_restatement_pair_by_pair(pose):
    ns = [300, 5, 0, 1200, 57, 4]
    P, cap = len(ns), max(ns)
    pts0, pts1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    K0, K1, sc = np.zeros((P, 3, 3)), np.zeros((P, 3, 3)), []
    for p, n in enumerate(ns):
        a, b, _, k0, k1, _ = scene(100 + p, max(n, 1), 0.5, 0.4, seed=p)
        pts0[p, :n], pts1[p, :n], K0[p], K1[p] = a[:n], b[:n], k0, k1
    got = pose.estimate_relative_pose_batch(torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.tensor(ns, dtype=torch.int32),
                                            K0, K1, 1.0, seed=5)
    torch.cuda.synchronize()
    for p, n in enumerate(ns):
        want = PR.estimate(pts0[p, :n], pts1[p, :n], K0[p], K1[p], 1.0, seed=5, pair=p)
        _check(got, want, p, n)


def test_index_list_entry_equals_gathered_points(pose):
    P, K, cap = 3, 700, 500
    rng = np.random.default_rng(3)
    kp0, kp1 = np.zeros((P, K, 2), np.float32), np.zeros((P, K, 2), np.float32)
    idx0, idx1 = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64)
    nm = np.array([500, 333, 20], np.int32)
    f = _fixture()
    for p in range(P):
        a, b, _, _, _, _ = scene(p, K, 0.5, 0.3, seed=p)
        kp0[p], kp1[p] = a, b[rng.permutation(K)]
        idx0[p] = rng.choice(K, cap, replace=False)
        idx1[p] = rng.choice(K, cap, replace=False)
    r1 = pose.estimate_relative_pose_matches(torch.from_numpy(kp0).cuda(), torch.from_numpy(kp1).cuda(), torch.from_numpy(idx0).cuda(),
                                             torch.from_numpy(idx1).cuda(), torch.from_numpy(nm).cuda(), f["K0"][:P], f["K1"][:P], 2.5, seed=9)
    pts0 = np.take_along_axis(kp0, idx0[:, :, None], 1)
    pts1 = np.take_along_axis(kp1, idx1[:, :, None], 1)
    r2 = pose.estimate_relative_pose_batch(torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.from_numpy(nm), f["K0"][:P],
                                           f["K1"][:P], 2.5, seed=9)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k


def test_degenerate_inputs_do_not_fault_or_nan(pose):
    f = _fixture()
    K = f["K0"][0]
    cap = 64
    pts0 = np.random.default_rng(0).uniform(0, 500, (5, cap, 2)).astype(np.float32)
    pts1 = pts0.copy()
    pts1[1] = pts1[1, :1]                       # all identical
    pts0[1] = pts0[1, :1]
    pts1[2] = pts0[2] + 3.0                     # pure translation in the image plane of identical cameras ~ rotation-free parallax
    Rz = np.array([[np.cos(0.1), -np.sin(0.1), 0], [np.sin(0.1), np.cos(0.1), 0], [0, 0, 1]])
    x = np.c_[(pts0[3] - K[:2, 2]) / K[0, 0], np.ones(cap)] @ Rz.T       # pure rotation
    pts1[3] = (x[:, :2] / x[:, 2:] * K[0, 0] + K[:2, 2]).astype(np.float32)
    pts0[4, ::3] = np.nan                        # NaN rows
    counts = torch.tensor([4, cap, cap, cap, cap], dtype=torch.int32)
    r = pose.estimate_relative_pose_batch(torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), counts, K, K, 1.0, seed=1)
    z = pose.estimate_relative_pose_batch(torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.zeros(5, dtype=torch.int32),
                                          K, K, 1.0, seed=1)
    torch.cuda.synchronize()
    for k in ("R", "t", "E"):
        assert torch.isfinite(r[k]).all() and torch.isfinite(z[k]).all()
    info = r["info"].cpu().numpy()
    assert info[0, 0] == 0 and info[1, 0] == 0
    assert (z["info"][:, 0] == 0).all() and not z["inliers"].any()
    assert not r["inliers"][4, ::3].any()
    for p in range(5):
        n = int(counts[p])
        want = PR.estimate(pts0[p, :n], pts1[p, :n], K, K, 1.0, seed=1, pair=p)
        assert list(info[p]) == list(want["info"])


def test_same_seed_same_bits(pose):
    p0, p1, _, K0, K1, _ = scene(3, 1500, 1.0, 0.5, seed=1)
    a = pose.estimate_relative_pose_batch(torch.from_numpy(p0)[None].cuda(), torch.from_numpy(p1)[None].cuda(), None, K0, K1, 1.0, seed=4)
    b = pose.estimate_relative_pose_batch(torch.from_numpy(p0)[None].cuda(), torch.from_numpy(p1)[None].cuda(), None, K0, K1, 1.0, seed=4)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_megadepth1500_synthetic_auc(pose):
    f = _fixture()
    P = 1500
    pts0, pts1, counts = PR.megadepth_synthetic(f)
    r = pose.estimate_relative_pose_batch(torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.from_numpy(counts), f["K0"],
                                          f["K1"], 1.0, max_iterations=1000, seed=0)
    info, R, t = r["info"].cpu().numpy(), r["R"].cpu().numpy(), r["t"].cpu().numpy()
    err = np.full(P, np.inf)
    for p in range(P):
        if info[p, 0]:
            err[p] = max(pose.relative_pose_error(f["T_0to1"][p], R[p], t[p]))
    auc = pose.pose_auc(err)
    print("synthetic MegaDepth-1500 AUC", auc)
    for k, v in PR.AUC_FLOORS.items():             # derived on the CPU: pose_reference.AUC_FLOORS
        assert auc[k] >= v, (k, auc)
    for p in range(0, P, 60):                    # 25 pairs exactly against the restatement
        want = PR.estimate(pts0[p, :counts[p]], pts1[p, :counts[p]], f["K0"][p], f["K1"][p], 1.0, max_iterations=1000, seed=0, pair=p)
        assert list(info[p]) == list(want["info"]), p
        assert np.abs(R[p] - want["R"]).max() <= 1e-9


def test_poselib_shaped_wrapper_equals_the_batch_entry(pose):
    p0, p1, _, K0, K1, _ = scene(11, 800, 0.5, 0.3, seed=2)
    cam = lambda K: {"model": "PINHOLE", "width": 1600, "height": 1200, "params": [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]}   # noqa: E731
    pz, det = pose.estimate_relative_pose(p0, p1, cam(K0), cam(K1), {"max_epipolar_error": 1.5}, {})
    r = pose.estimate_relative_pose_batch(torch.from_numpy(p0)[None].cuda(), torch.from_numpy(p1)[None].cuda(), None, K0, K1, 1.5,
                                          max_iterations=10000)
    assert np.array_equal(pz.R, r["R"][0].cpu().numpy()) and np.array_equal(pz.t, r["t"][0].cpu().numpy())
    assert det["inliers"] == [bool(v) for v in r["inliers"][0].cpu().tolist()] and det["num_inliers"] == sum(det["inliers"])
    with pytest.raises(Exception):
        pose.estimate_relative_pose(p0, p1, dict(cam(K0), model="OPENCV"), cam(K1))
    with pytest.raises(Exception):
        pose.estimate_relative_pose(p0, p1, cam(K0), cam(K1), {"max_reproj_error": 1.0})
    none, d = pose.estimate_relative_pose(p0[:4], p1[:4], cam(K0), cam(K1))
    assert none is None and d["inliers"] == [False] * 4


def test_pose_benchmark_equals_match_then_pose(pose):
    """pose_benchmark == batching.match_pairs, the rescaling, then the poselib-shaped estimate_relative_pose per pair (with the seed that
    gives pair p of a batch its draws), pose and inlier mask exactly."""
    import fixtures
    from accelerated_features_amd import XFeat, batching
    f = _fixture()
    xf = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=512, detection_threshold=0.05)
    pairs = []
    for i in range(3):
        a, b = fixtures.shifted_pair(1, 160, 224, seed=20 + i, shift=(3 + i, 5))
        pairs.append((a[0], b[0]))
    res = pose.pose_benchmark(xf, pairs, f["K0"][:3], f["K1"][:3], f["T_0to1"][:3], f["scale0"][:3], f["scale1"][:3], top_k=512)
    ref = batching.match_pairs(xf, pairs, top_k=512)
    cam = lambda K: {"model": "PINHOLE", "width": 1, "height": 1, "params": [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]}   # noqa: E731
    found = 0
    for p in range(3):
        m0 = np.asarray(ref[p][0], np.float32) * f["scale0"][p].astype(np.float32)
        m1 = np.asarray(ref[p][1], np.float32) * f["scale1"][p].astype(np.float32)
        n = len(m0)
        assert np.array_equal(res["matches"][0][p].numpy(), m0) and np.array_equal(res["matches"][1][p].numpy(), m1)
        pz, det = pose.estimate_relative_pose(m0, m1, cam(f["K0"][p]), cam(f["K1"][p]), {"max_epipolar_error": 2.5}, {},
                                              seed=pose.chunk_seed(0, p))
        assert (pz is None) == (res["info"][p, 0] == 0)
        assert det["inliers"] == [bool(v) for v in res["inliers"][p, :n]]
        if pz is not None:
            found += 1
            assert np.array_equal(pz.R, res["R"][p]) and np.array_equal(pz.t, res["t"][p])
    assert found > 0
