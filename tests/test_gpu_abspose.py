"""xfh_estimate_abspose (csrc/k_abspose.hip) on the MI355X against the numpy restatement tests/abspose_reference.py: the winner, the
iteration count, the inlier count, the integer cost and the mask exactly; R and t to 1e-9 (t relative to max(1, |t|)): the refinement's
sums are taken in one fixed order on both sides, as for the relative pose."""
import numpy as np
import pytest
import torch

import abspose_reference as AR
import abspose_support as AS
from twoview_support import check_common

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ap():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import absolute_pose as m
    return m


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _check(got, want, p, n):
    check_common(got, want, p, n)
    R, t = got["R"][p].cpu().numpy(), got["t"][p].cpu().numpy()
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert np.abs(R - want["R"]).max() <= 1e-9, (R, want["R"])
    assert np.abs(t - want["t"]).max() <= 1e-9 * max(1.0, np.abs(want["t"]).max()), (t, want["t"])


@pytest.mark.parametrize("n,outliers,thr,iters", [(3, 0.0, 2.0, 1000), (4, 0.0, 2.0, 1000), (300, 0.3, 2.0, 1000), (300, 0.8, 4.0, 10000),
                                                  (1200, 0.5, 12.0, 1000)])
def test_single_pair_equals_the_restatement(ap, n, outliers, thr, iters):
    X, p, _, K, _ = AS.scene3d(7, n, 0.7, outliers, seed=n)
    a, b = _cuda(p[None], X[None])
    got = ap.estimate_absolute_pose_batch(a, b, None, K, thr, max_iterations=iters, seed=11)
    torch.cuda.synchronize()
    want = AR.estimate(p, X, K, thr, max_iterations=iters, seed=11)
    _check(got, want, 0, n)
    if n >= 300:
        assert want["info"][0] == 1


def test_loop_past_one_tile_of_the_select_kernel(ap):
    """At success_prob 0.9999 the 80 % outlier case above stops near 1100 hypotheses (log 1e-4 / log(1 - 0.2^3) = 1147), inside the first
    tile of 2048 list entries; 90 % outliers need log 1e-4 / log(1 - 0.1^3) = 9206, so the stopping rule walks five tiles."""
    X, p, _, K, _ = AS.scene3d(7, 300, 0.7, 0.9, seed=300)
    a, b = _cuda(p[None], X[None])
    got = ap.estimate_absolute_pose_batch(a, b, None, K, 4.0, max_iterations=10000, seed=11)
    torch.cuda.synchronize()
    want = AR.estimate(p, X, K, 4.0, max_iterations=10000, seed=11)
    _check(got, want, 0, 300)
    assert want["info"][2] > 2048 and want["info"][0] == 1


def _ragged(ns):
    P, cap = len(ns), max(ns)
    pts2, pts3, K = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 3), np.float32), np.zeros((P, 3, 3))
    for p, n in enumerate(ns):
        X, px, _, K[p], _ = AS.scene3d(100 + p, max(n, 1), 0.5, 0.4, seed=p)
        pts3[p, :n], pts2[p, :n] = X[:n], px[:n]
    return pts2, pts3, K


def test_ragged_batch_equals_the_restatement_pair_by_pair(ap):
    ns = [300, 3, 0, 1200, 57, 2]
    pts2, pts3, K = _ragged(ns)
    a, b = _cuda(pts2, pts3)
    got = ap.estimate_absolute_pose_batch(a, b, torch.tensor(ns, dtype=torch.int32), K, 3.0, seed=5)
    torch.cuda.synchronize()
    for p, n in enumerate(ns):
        want = AR.estimate(pts2[p, :n], pts3[p, :n], K[p], 3.0, seed=5, pair=p)
        _check(got, want, p, n)


def test_index_list_entry_equals_gathered_points(ap):
    P, cap2, cap3, cap = 3, 700, 900, 500
    rng = np.random.default_rng(3)
    kp, pt = np.zeros((P, cap2, 2), np.float32), np.zeros((P, cap3, 3), np.float32)
    idx2, idx3 = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64)
    nm = np.array([500, 333, 20], np.int32)
    K = np.zeros((P, 3, 3))
    for p in range(P):
        X, px, _, K[p], _ = AS.scene3d(p, cap3, 0.5, 0.3, seed=p)
        rows3 = rng.permutation(cap3)                       # correspondence i: 3D row rows3[i], 2D row rows2[i]
        rows2 = rng.permutation(cap2)
        pt[p, rows3] = X
        kp[p, rows2] = px[:cap2]
        idx3[p], idx2[p] = rows3[:cap], rows2[:cap]
    r1 = ap.estimate_absolute_pose_matches(*_cuda(kp, pt, idx2, idx3, nm), K, 3.0, seed=9)
    pts2 = np.take_along_axis(kp, idx2[:, :, None], 1)
    pts3 = np.take_along_axis(pt, idx3[:, :, None], 1)
    r2 = ap.estimate_absolute_pose_batch(*_cuda(pts2, pts3), torch.from_numpy(nm), K, 3.0, seed=9)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    assert r1["info"][:, 0].all()


def test_chunked_equals_unchunked(ap, monkeypatch):
    ns = [300, 3, 0, 1200, 57, 2]
    pts2, pts3, K = _ragged(ns)
    a, b = _cuda(pts2, pts3)
    counts = torch.tensor(ns, dtype=torch.int32)
    whole = ap.estimate_absolute_pose_batch(a, b, counts, K, 3.0, seed=5)
    from accelerated_features_amd import _lib
    per_pair = _lib.load().xfh_abspose_workspace_bytes(1, 1000)
    monkeypatch.setattr(ap, "WORKSPACE_LIMIT", 2 * per_pair + 1024)          # 2 pairs per library call: 3 chunks
    assert (2 * per_pair + 1024) // _lib.load().xfh_abspose_workspace_bytes(1, 1000) == 2
    split = ap.estimate_absolute_pose_batch(a, b, counts, K, 3.0, seed=5)
    torch.cuda.synchronize()
    for k in whole:
        assert torch.equal(whole[k], split[k]), k


def test_same_seed_same_bits(ap):
    X, p, _, K, _ = AS.scene3d(3, 1500, 1.0, 0.5, seed=1)
    a, b = _cuda(p[None], X[None])
    r1 = ap.estimate_absolute_pose_batch(a, b, None, K, 3.0, seed=4)
    r2 = ap.estimate_absolute_pose_batch(a, b, None, K, 3.0, seed=4)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    assert int(r1["info"][0, 0]) == 1


def test_degenerate_inputs_do_not_fault_or_nan(ap):
    K = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])
    rng = np.random.default_rng(5)
    cap = 64
    X = np.repeat(np.c_[rng.uniform(-1, 1, (cap, 2)), rng.uniform(2, 6, cap)].astype(np.float32)[None], 6, 0)
    X[0] = (np.array([0.25, -0.5, 3.0]) + np.arange(cap)[:, None] * np.array([0.125, 0.0625, 0.25])).astype(np.float32)      # collinear
    X[1] = X[1, :1]                                         # all identical
    X[2, :, 2] *= -1.0                                      # all behind the camera (pixels through the centre)
    p = (X[:, :, :2] / X[:, :, 2:] * 800.0 + K[:2, 2]).astype(np.float32)
    X[3, ::3] = np.nan                                      # NaN rows on either side
    p[3, 1::7] = np.nan
    p[4] = np.nan                                           # nothing finite
    counts = torch.tensor([cap, cap, cap, cap, cap, 2], dtype=torch.int32)
    a, b = _cuda(p, X)
    r = ap.estimate_absolute_pose_batch(a, b, counts, K, 2.0, max_iterations=300, seed=1)
    z = ap.estimate_absolute_pose_batch(a, b, torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32), K, 2.0, max_iterations=300, seed=1)      # n in {0, 1, 2}
    torch.cuda.synchronize()
    for k in ("R", "t"):
        assert torch.isfinite(r[k]).all() and torch.isfinite(z[k]).all()
    info = r["info"].cpu().numpy()
    assert (z["info"][:, 0] == 0).all() and not z["inliers"].any() and (z["info"][:, 2] == 0).all() and not z["R"].any() and not z["t"].any()
    assert z["info"][:, 5].tolist() == [0, 1, 2, 0, 1, 2] and (z["info"][:, 1] == -1).all()
    bad = np.isnan(X[3]).any(1) | np.isnan(p[3]).any(1)
    assert info[3, 0] == 1 and not r["inliers"][3].cpu().numpy()[bad].any()
    for q in range(6):
        n = int(counts[q])
        want = AR.estimate(p[q, :n], X[q, :n], K, 2.0, max_iterations=300, seed=1, pair=q)
        assert list(info[q]) == list(want["info"]), q
        assert np.array_equal(r["inliers"][q, :n].cpu().numpy(), want["mask"])
        if not want["info"][0]:
            assert info[q, 0] == 0 and not r["R"][q].any() and not r["t"][q].any() and not r["inliers"][q].any()
    assert [int(v) for v in info[[0, 1, 4, 5], 0]] == [0, 0, 0, 0]


def test_poselib_shaped_wrapper_equals_the_batch_entry(ap):
    X, p, _, K, _ = AS.scene3d(11, 800, 0.5, 0.3, seed=2)
    cam = {"model": "PINHOLE", "width": 1600, "height": 1200, "params": [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]}
    pz, det = ap.estimate_absolute_pose(p, X, cam, {"max_reproj_error": 4.0}, {})
    a, b = _cuda(p[None], X[None])
    r = ap.estimate_absolute_pose_batch(a, b, None, K, 4.0, max_iterations=10000)
    assert np.array_equal(pz.R, r["R"][0].cpu().numpy()) and np.array_equal(pz.t, r["t"][0].cpu().numpy())
    assert det["inliers"] == [bool(v) for v in r["inliers"][0].cpu().tolist()] and det["num_inliers"] == sum(det["inliers"])
    assert det["iterations"] == int(r["info"][0, 2]) and det["refinements"] == int(r["info"][0, 4])
    with pytest.raises(Exception):
        ap.estimate_absolute_pose(p, X, dict(cam, model="OPENCV"))
    with pytest.raises(Exception):
        ap.estimate_absolute_pose(p, X, cam, {"max_epipolar_error": 1.0})
    with pytest.raises(Exception):
        ap.estimate_absolute_pose(p, X, cam, {}, {"loss_scale": 1.0})
    none, d = ap.estimate_absolute_pose(p[:2], X[:2], cam)
    assert none is None and d["inliers"] == [False] * 2


def test_detect_match_unproject_then_pose_equals_the_gathered_points(ap):
    """_detect_device -> match_pairs_device -> unproject_keypoints on a synthetic positive depth map of image 0 ->
    estimate_absolute_pose_matches == estimate_absolute_pose_batch on the gathered points, exactly."""
    import fixtures
    from accelerated_features_amd import XFeat
    xf = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=512, detection_threshold=0.05)
    ims = []
    for i in range(3):
        a, b = fixtures.shifted_pair(1, 160, 224, seed=20 + i, shift=(3 + i, 5))
        ims += [a, b]
    kp, sc, de, nv, nc, dcap, hw = xf._detect_device(xf.parse_input(torch.cat(ims)), 512)
    idx0, idx1, nm = xf.match_pairs_device(de, nv, -1)
    kp0, kp1 = kp[0::2].contiguous(), kp[1::2].contiguous()
    vv, uu = torch.meshgrid(torch.arange(160.0), torch.arange(224.0), indexing="ij")
    depth = (4.0 + 0.01 * uu + 0.02 * vv + 0.5 * torch.sin(uu / 17.0)).cuda()[None].repeat(3, 1, 1)        # a smooth positive surface
    K = np.array([[200.0, 0, 112.0], [0, 200.0, 80.0], [0, 0, 1]])
    X0, valid = ap.unproject_keypoints(kp0, depth, K)
    assert X0.is_cuda and X0.shape == (3, kp0.shape[1], 3)
    r1 = ap.estimate_absolute_pose_matches(kp1, X0, idx1, idx0, nm, K, 2.0, seed=3)
    cap = idx0.shape[1]
    live = torch.arange(cap, device="cuda")[None, :] < nm[:, None]          # rows past n_matches hold no valid index
    g2 = torch.gather(kp1, 1, torch.where(live, idx1, 0)[:, :, None].expand(-1, -1, 2)).contiguous()
    g3 = torch.gather(X0, 1, torch.where(live, idx0, 0)[:, :, None].expand(-1, -1, 3)).contiguous()
    r2 = ap.estimate_absolute_pose_batch(g2, g3, nm, K, 2.0, seed=3)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    assert r1["inliers"].shape == (3, cap) and int(r1["info"][:, 0].sum()) >= 1
