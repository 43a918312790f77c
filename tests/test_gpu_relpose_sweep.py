"""xfh_estimate_relpose_sweep (csrc/k_relpose.hip): relative pose at many RANSAC thresholds in one pass.  The specification is the
single-threshold one: slice j of a sweep must BE ``estimate_relative_pose_batch`` at thresholds[j] (torch.equal on every output), and,
independently of the device's single path, the numpy restatement tests/pose_reference.py (info words and mask exactly; R, t, E to 1e-9,
the bound of tests/test_gpu_relpose.py)."""
import numpy as np
import pytest
import torch

import pose_reference as PR
from twoview_support import check_common, fixture as _fixture, scene

pytestmark = pytest.mark.gpu
KEYS = ("R", "t", "E", "inliers", "info")


@pytest.fixture(scope="module")
def pose():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import pose as m
    return m


def _assert_slices_equal_single_calls(pose, pts0, pts1, counts, K0, K1, thresholds, sweep, **opt):
    """Every slice of `sweep` against the single call at its threshold; returns the single calls' info (T, P, 8)."""
    infos = []
    for j, thr in enumerate(thresholds):
        one = pose.estimate_relative_pose_batch(pts0, pts1, counts, K0, K1, thr, **opt)
        for k in KEYS:
            assert sweep[k].shape[:2] == (pts0.shape[0], len(thresholds))
            assert torch.equal(sweep[k][:, j], one[k]), (k, j, thr)
        infos.append(one["info"].cpu().numpy())
    return np.stack(infos)


def _ragged():
    """The ragged batch of test_gpu_relpose.py plus a 57-point scene whose loop passes the first 256 hypotheses at 0.5 px only."""
    ns = [300, 5, 0, 1200, 57, 4, 57]
    P, cap = len(ns), max(ns)
    pts0, pts1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    K0, K1 = np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
    for p, n in enumerate(ns[:6]):
        a, b, _, k0, k1, _ = scene(100 + p, max(n, 1), 0.5, 0.4, seed=p)
        pts0[p, :n], pts1[p, :n], K0[p], K1[p] = a[:n], b[:n], k0, k1
    a, b, _, K0[6], K1[6], _ = scene(7, 57, 0.7, 0.4, seed=57)
    pts0[6, :57], pts1[6, :57] = a, b
    return torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.tensor(ns, dtype=torch.int32), K0, K1


@pytest.fixture(scope="module")
def scene_b(pose):
    """Two 300-point scenes (60 % and 70 % outliers) at 10000 iterations, seed 11: the loops end beyond the first 256 hypotheses at a
    different place for almost every threshold.  (points, single-call-free sweep result)."""
    a0, b0, _, K0, K1, _ = scene(7, 300, 0.7, 0.6, seed=300)
    a1, b1, _, _, _, _ = scene(7, 300, 0.7, 0.7, seed=300)
    pts0, pts1 = torch.from_numpy(np.stack([a0, a1])).cuda(), torch.from_numpy(np.stack([b0, b1])).cuda()
    sweep = pose.estimate_relative_pose_sweep_batch(pts0, pts1, None, K0, K1, pose.SCANNET_THRESHOLDS, max_iterations=10000, seed=11)
    torch.cuda.synchronize()
    return pts0, pts1, K0, K1, sweep


def test_slices_equal_single_calls_on_the_ragged_batch(pose):
    pts0, pts1, counts, K0, K1 = _ragged()
    sweep = pose.estimate_relative_pose_sweep_batch(pts0, pts1, counts, K0, K1, pose.SCANNET_THRESHOLDS, max_iterations=1000, seed=5)
    info = _assert_slices_equal_single_calls(pose, pts0, pts1, counts, K0, K1, pose.SCANNET_THRESHOLDS, sweep, max_iterations=1000, seed=5)
    loops = info[:, 6, 2]
    print("57-point scene, loop lengths per threshold", loops.tolist())
    assert (loops > 256).any() and (loops <= 256).any()        # the sweep solves past what most of its thresholds visit


def test_slices_equal_single_calls_where_the_bounds_differ(pose, scene_b):
    pts0, pts1, K0, K1, sweep = scene_b
    info = _assert_slices_equal_single_calls(pose, pts0, pts1, None, K0, K1, pose.SCANNET_THRESHOLDS, sweep, max_iterations=10000, seed=11)
    for p in range(2):
        loops = info[:, p, 2]
        print("pair", p, "loop lengths per threshold", loops.tolist(), "winners", info[:, p, 1].tolist())
        assert len(set(loops[loops > 256].tolist())) >= 3, loops


@pytest.mark.parametrize("thr", [0.5, 6.0])
def test_scene_b_equals_the_restatement(pose, scene_b, thr):
    pts0, pts1, K0, K1, sweep = scene_b
    j = pose.SCANNET_THRESHOLDS.index(thr)
    want = PR.estimate(pts0[0].cpu().numpy(), pts1[0].cpu().numpy(), K0, K1, thr, max_iterations=10000, seed=11)
    _check_restatement({k: v[:, j] for k, v in sweep.items()}, want, 0, 300)


def test_short_and_long_loops_equal_the_restatement(pose):
    a, b, _, K0, K1, _ = scene(7, 57, 0.7, 0.4, seed=57)
    sweep = pose.estimate_relative_pose_sweep_batch(torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda(), None, K0, K1,
                                                    pose.SCANNET_THRESHOLDS, max_iterations=1000, seed=11)
    torch.cuda.synchronize()
    for thr in (0.5, 2.5):
        j = pose.SCANNET_THRESHOLDS.index(thr)
        want = PR.estimate(a, b, K0, K1, thr, max_iterations=1000, seed=11)
        _check_restatement({k: v[:, j] for k, v in sweep.items()}, want, 0, 57)


def _check_restatement(got, want, p, n):
    check_common(got, want, p, n)
    for k in ("R", "t", "E"):
        g = got[k][p].cpu().numpy()
        assert np.isfinite(g).all()
        assert np.abs(g - want[k]).max() <= 1e-9, (k, g, want[k])


def test_threshold_count_edges(pose):
    a, b, _, K0, K1, _ = scene(3, 400, 0.5, 0.5, seed=8)
    pts0, pts1 = torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda()
    one = pose.estimate_relative_pose_sweep_batch(pts0, pts1, None, K0, K1, [1.5], seed=2)
    _assert_slices_equal_single_calls(pose, pts0, pts1, None, K0, K1, [1.5], one, seed=2)
    sixteen = [0.25 * (k + 1) for k in range(16)]
    r16 = pose.estimate_relative_pose_sweep_batch(pts0, pts1, None, K0, K1, sixteen, seed=2)
    _assert_slices_equal_single_calls(pose, pts0, pts1, None, K0, K1, sixteen, r16, seed=2)
    mixed = [3.0, 0.5, 6.0, 0.5, 2.0, 3.0, 1.0]               # unsorted, two repeated values
    rm = pose.estimate_relative_pose_sweep_batch(pts0, pts1, None, K0, K1, mixed, seed=2)
    _assert_slices_equal_single_calls(pose, pts0, pts1, None, K0, K1, mixed, rm, seed=2)
    for k in KEYS:
        assert torch.equal(rm[k][:, 1], rm[k][:, 3]) and torch.equal(rm[k][:, 0], rm[k][:, 5]), k
    for bad in ([], [1.0] * 17, [1.0, float("nan")], [1.0, 0.0], [-2.0], [float("inf")]):
        with pytest.raises(Exception):
            pose.estimate_relative_pose_sweep_batch(pts0, pts1, None, K0, K1, bad, seed=2)


def test_the_library_refuses_bad_thresholds(pose):
    """The C entry itself (the Python wrapper checks first): T outside [1, 16], a NULL list, a NaN or non-positive threshold."""
    import ctypes as C
    from accelerated_features_amd import _lib
    lib = _lib.load()
    P, cap, iters = 1, 64, 256
    pts = torch.rand(P, cap, 2, device="cuda") * 400
    K = torch.tensor(_fixture()["K0"][:1]).cuda().contiguous()
    R, t, E = (torch.zeros(P, 16, n, dtype=torch.float64, device="cuda") for n in (9, 3, 9))
    mask, info = torch.zeros(P, 16, cap, dtype=torch.uint8, device="cuda"), torch.zeros(P, 16, 8, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.xfh_relpose_sweep_workspace_bytes(P, iters, 16) + 256, dtype=torch.uint8, device="cuda")
    ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731

    def call(thr, T):
        arr = (C.c_double * max(len(thr), 1))(*thr) if thr is not None else None
        return lib.xfh_estimate_relpose_sweep(ptr(pts), ptr(pts), None, cap, P, cap, ptr(K), ptr(K), arr, T, 20, iters, 0.999, 0, ptr(R), ptr(t),
                                              ptr(E), ptr(mask), ptr(info), ptr(ws), ws.numel(), None)
    assert call([1.0, 2.0], 2) == 0
    torch.cuda.synchronize()
    for thr, T in (([1.0], 0), ([1.0] * 17, 17), (None, 1), ([1.0, float("nan")], 2), ([0.0], 1), ([-1.0], 1), ([float("inf")], 1)):
        assert call(thr, T) != 0, (thr, T)


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
    thr = [0.5, 2.5, 6.0]
    r1 = pose.estimate_relative_pose_sweep_matches(torch.from_numpy(kp0).cuda(), torch.from_numpy(kp1).cuda(), torch.from_numpy(idx0).cuda(),
                                                   torch.from_numpy(idx1).cuda(), torch.from_numpy(nm).cuda(), f["K0"][:P], f["K1"][:P], thr, seed=9)
    pts0 = np.take_along_axis(kp0, idx0[:, :, None], 1)
    pts1 = np.take_along_axis(kp1, idx1[:, :, None], 1)
    r2 = pose.estimate_relative_pose_sweep_batch(torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda(), torch.from_numpy(nm), f["K0"][:P],
                                                 f["K1"][:P], thr, seed=9)
    torch.cuda.synchronize()
    for k in r1:
        assert r1[k].shape[:2] == (P, 3) and torch.equal(r1[k], r2[k]), k


def test_degenerate_inputs_do_not_fault_or_nan(pose):
    """The point sets of test_gpu_relpose.py's test of the same name, at every threshold."""
    f = _fixture()
    K = f["K0"][0]
    cap = 64
    pts0 = np.random.default_rng(0).uniform(0, 500, (5, cap, 2)).astype(np.float32)
    pts1 = pts0.copy()
    pts1[1] = pts1[1, :1]                       # all identical
    pts0[1] = pts0[1, :1]
    pts1[2] = pts0[2] + 3.0                     # pure translation in the image plane of identical cameras
    Rz = np.array([[np.cos(0.1), -np.sin(0.1), 0], [np.sin(0.1), np.cos(0.1), 0], [0, 0, 1]])
    x = np.c_[(pts0[3] - K[:2, 2]) / K[0, 0], np.ones(cap)] @ Rz.T       # pure rotation
    pts1[3] = (x[:, :2] / x[:, 2:] * K[0, 0] + K[:2, 2]).astype(np.float32)
    pts0[4, ::3] = np.nan                        # NaN rows
    a, b = torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda()
    thr = pose.SCANNET_THRESHOLDS
    for counts in (torch.tensor([4, cap, cap, cap, cap], dtype=torch.int32), torch.zeros(5, dtype=torch.int32)):
        r = pose.estimate_relative_pose_sweep_batch(a, b, counts, K, K, thr, seed=1)
        for k in ("R", "t", "E"):
            assert torch.isfinite(r[k]).all()
        info = _assert_slices_equal_single_calls(pose, a, b, counts, K, K, thr, r, seed=1)
        assert np.array_equal(r["info"][:, :, 0].cpu().numpy() == 0, info[:, :, 0].T == 0)
        assert (r["info"][0, :, 0] == 0).all()                                   # 4 or 0 points: never found
        if not counts.any():
            assert (r["info"][:, :, 0] == 0).all() and not r["inliers"].any()
        else:
            assert not r["inliers"][4, :, ::3].any()


def test_chunks_of_pairs_equal_one_call(pose, monkeypatch):
    from accelerated_features_amd import _lib
    P, cap, thr = 5, 200, [0.5, 1.0, 2.5, 6.0]
    pts0, pts1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    K0, K1 = np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
    for p in range(P):
        pts0[p], pts1[p], _, K0[p], K1[p], _ = scene(20 + p, cap, 0.6, 0.5, seed=p)
    a, b = torch.from_numpy(pts0).cuda(), torch.from_numpy(pts1).cuda()
    whole = pose.estimate_relative_pose_sweep_batch(a, b, None, K0, K1, thr, max_iterations=1000, seed=3)
    limit = _lib.load().xfh_relpose_sweep_workspace_bytes(2, 1000, 4)
    assert P > 2 * (limit // _lib.load().xfh_relpose_sweep_workspace_bytes(1, 1000, 4))          # at least three chunks
    monkeypatch.setattr(pose, "WORKSPACE_LIMIT", limit)
    parts = pose.estimate_relative_pose_sweep_batch(a, b, None, K0, K1, thr, max_iterations=1000, seed=3)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(whole[k], parts[k]), k
    assert (whole["info"][:, :, 0] == 1).any()


def test_scannet_benchmark_equals_pose_benchmark_per_threshold(pose):
    import fixtures
    from accelerated_features_amd import XFeat
    f = _fixture()
    xf = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=512, detection_threshold=0.05)
    pairs = []
    for i in range(3):
        a, b = fixtures.shifted_pair(1, 160, 224, seed=20 + i, shift=(3 + i, 5))
        pairs.append((a[0], b[0]))
    thr = (0.5, 2.5, 6.0)
    res = pose.scannet_benchmark(xf, pairs, f["K0"][:3], f["K1"][:3], f["T_0to1"][:3], ransac_thresholds=thr, top_k=512)
    assert res["err"].shape == (3, 3) and list(res["aucs_by_thresh"]) == list(thr) and list(res["accs_by_thresh"]) == list(thr)
    for j, v in enumerate(thr):
        one = pose.pose_benchmark(xf, pairs, f["K0"][:3], f["K1"][:3], f["T_0to1"][:3], ransac_thr=v, top_k=512)
        assert np.array_equal(res["err"][:, j], one["err"])
        assert np.array_equal(res["info"][:, j], one["info"]) and np.array_equal(res["inliers"][:, j], one["inliers"])
        auc = pose.pose_auc(res["err"][:, j])
        assert res["aucs_by_thresh"][v] == {k: 100.0 * auc[f"auc@{k}"] for k in (5, 10, 20)}
        assert res["accs_by_thresh"][v] == pose.pose_accuracy(res["err"][:, j])
    assert (res["info"][:, :, 0] == 1).any()


def test_estimate_pose_is_the_scannet_call_shape(pose):
    p0, p1, _, K0, K1, _ = scene(11, 800, 0.5, 0.3, seed=2)
    cam = lambda K: {"model": "PINHOLE", "width": 1600, "height": 1200, "params": [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]}   # noqa: E731
    R, t, inl = pose.estimate_pose(p0, p1, K0, K1, 1.5)
    pz, det = pose.estimate_relative_pose(p0, p1, cam(K0), cam(K1), {"max_epipolar_error": 1.5, "max_iterations": 10000}, {})
    assert np.array_equal(R, pz.R) and np.array_equal(t, pz.t) and inl == det["inliers"]
    assert pose.estimate_pose(p0[:4], p1[:4], K0, K1, 1.5) is None
    with pytest.raises(Exception):
        pose.estimate_pose(p0, p1, K0, K1, 1.5, type='opencv')
