"""The absolute-pose restatement (tests/abspose_reference.py) against ground truth, and the host side of
accelerated_features_amd.absolute_pose.  CPU only: the restatement is what the GPU tests hold the kernels to, so it is checked here on
its own.  Every bound is a condition on ground truth, not on the code under test; the restatement's own measured values are written beside
the assertions."""
import inspect

import numpy as np
import pytest
import torch

import abspose_reference as AR
import abspose_support as AS

K640 = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])


def test_every_candidate_is_a_pose_through_the_sample():
    rng = np.random.default_rng(0)
    x, y, X, _ = AS.true_samples(rng, 2000)
    cand, nc = AR.solve(x, y, X)
    assert (nc > 0).all() and nc.max() <= 4
    worst = 0.0
    for h in range(2000):
        for c in range(nc[h]):
            R, t = cand[h, c, :9].reshape(3, 3), cand[h, c, 9:]
            Y = X[h] @ R.T + t
            assert (Y[:, 2] > 0).all(), h
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-10 and abs(np.linalg.det(R) - 1.0) <= 1e-10, h
            worst = max(worst, np.abs(Y[:, 0] / Y[:, 2] - x[h]).max(), np.abs(Y[:, 1] / Y[:, 2] - y[h]).max())
    # measured: 9.0e-13 on these 2000 samples, 1.1e-11 on 20 000 (39 000 candidates)
    print("worst reprojection of a candidate", worst)
    assert worst <= 1e-9


def test_ground_truth_pose_is_among_the_candidates():
    rng = np.random.default_rng(1)
    x, y, X, gt = AS.true_samples(rng, 2000)
    cand, nc = AR.solve(x, y, X)
    best = np.array([min([np.abs(cand[h, c, :9] - gt[h][0].ravel()).max() + np.abs(cand[h, c, 9:] - gt[h][1]).max() for c in range(nc[h])] or [9.0])
                     for h in range(len(gt))])
    share = (best <= 1e-6).mean()
    print("share of samples whose true pose is among the candidates", share, "within 1e-10:", (best <= 1e-10).mean())
    # measured: 100.0 % within 1e-6 of the true (R, t) (2000 of 2000 here, 20 000 of 20 000 over five generators), 100 % within 1e-10 here;
    # asserted: the measured share minus 0.5 percentage points.  (Without the polish of (u, v): 99.85 % / 99.0 %.)
    assert share >= 0.995, np.sort(best)[-20:]


def _quartic(roots, quad=None, lead=1.0):
    p = np.array([lead])
    for r in roots:
        p = np.convolve(p, [1.0, -r])
    if quad is not None:
        p = np.convolve(p, [1.0, quad[0], quad[1]])
    return [np.array([c]) for c in p[::-1]]


@pytest.mark.parametrize("lead", [1.0, -3.7, 0.013])
def test_quartic_root_finder_on_known_roots(lead):
    """Every real root found, in ascending order.  Simple roots to 1e-10 (their condition is moderate), roots 1e-4 .. 1e-6 apart to 1e-8
    (a root d away from its neighbour moves by ~ eps |coefficients| / d), a double root to 1e-6: it moves with the square root of a
    perturbation of the coefficients, sqrt(1e-16 x 40) ~ 6e-8.  Measured worst errors: 2e-15, 4e-11, 3e-8."""
    cases = [([-1, 1, 2, 3], None, 1e-10), ([0.5, 0.7, 1.5, 4.0], None, 1e-10), ([0.3, 2.0], (0.0, 1.0), 1e-10), ([-2.5, 0.25], (1.0, 3.0), 1e-10),
             ([], (0.0, 1.0), 0.0), ([1, 1.0001, 2, 3], None, 1e-8), ([1, 1.000001, 2, 3], None, 1e-8), ([0.5, 2, 2.00001, 5], None, 1e-8),
             ([1, 1, 2, 3], None, 1e-6), ([0.5, 2, 2, 5], None, 1e-6), ([-1, 0.5, 3, 3], None, 1e-6), ([1.5, 1.5], (0.0, 2.0), 1e-6)]
    for roots, quad, tol in cases:
        p = _quartic(roots, quad, lead) if roots else [np.array([c * lead]) for c in np.convolve([1.0, 0.0, 1.0], [1.0, 1.0, 2.5])[::-1]]
        z, n, ok = AR.quartic_roots(p)
        got = z[0, :n[0]]
        assert ok[0] and (np.diff(got) >= 0).all()
        for r in roots:                                  # every true root has a found one next to it ...
            assert np.abs(got - r).min() <= tol, (roots, quad, got)
        for g in got:                                    # ... and nothing else is reported (a double root may be found twice)
            assert roots and np.abs(np.array(roots) - g).min() <= tol, (roots, quad, got)


def _check_recovery(i, n, noise, outliers, thr, worst):
    X, p, out, K, T = AS.scene3d(i, n, noise, outliers, seed=i)
    r = AR.estimate(p, X, K, thr, max_iterations=1000, seed=3)
    assert r["info"][0] == 1, i
    rot, pos = AS.pose_errors(T, r["R"], r["t"])
    diff = np.mean(r["mask"].astype(bool) != ~out)
    worst[:] = [max(worst[0], rot), max(worst[1], pos), max(worst[2], diff)]
    assert rot <= 0.5 and pos <= 0.01 and diff <= 0.10, (i, rot, pos, diff)


@pytest.mark.parametrize("n,noise,outliers,thr", [(300, 0.7, 0.4, 3.0), (300, 0.7, 0.7, 3.0), (60, 0.5, 0.3, 2.0)])
def test_estimator_recovers_every_25th_fixture_pose(n, noise, outliers, thr):
    """Every pair found, rotation error <= 0.5 degrees, |t - t_true| <= 1 % of max(1, 4 |t_true|), mask against the true inlier flags
    different on <= 10 % of the rows.  Measured worst values of this restatement over the 60 pairs:
    (300, 0.7, 0.4, 3): 0.037 degrees, 0.066 %, 0.33 %;  (300, 0.7, 0.7, 3): 0.072 degrees, 0.088 %, 0.33 %;
    (60, 0.5, 0.3, 2): 0.088 degrees, 0.097 %, 1.7 %."""
    worst = [0.0, 0.0, 0.0]
    for i in range(0, 1500, 25):
        _check_recovery(i, n, noise, outliers, thr, worst)
    print("worst rotation error (degrees), position error, mask difference:", worst)


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_estimator_recovers_fixture_poses_at_outlier_rates(outliers):
    """The same bounds at outlier rates 0, 0.3, 0.6 (300 correspondences, 0.7 px noise, 3 px threshold, every 150th pair).  Measured worst:
    0.014 / 0.018 / 0.017 degrees, 0.051 / 0.046 / 0.057 %, no mask difference."""
    worst = [0.0, 0.0, 0.0]
    for i in range(0, 1500, 150):
        _check_recovery(i, 300, 0.7, outliers, 3.0, worst)
    print("outliers", outliers, "worst:", worst)


def _nothing(r, n, iters=None):
    assert r["info"][0] == 0 and r["info"][1] == -1 and r["info"][3] == 0 and r["info"][5] == n
    assert not r["mask"].any() and np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all() and not r["R"].any() and not r["t"].any()
    if iters is not None:
        assert r["info"][2] == iters


def test_estimator_degenerate_inputs():
    rng = np.random.default_rng(5)
    n = 50
    X = np.c_[rng.uniform(-1, 1, (n, 2)), rng.uniform(2, 6, n)].astype(np.float32)
    p = (X[:, :2] / X[:, 2:] * 800.0 + K640[:2, 2]).astype(np.float32)        # the identity pose
    # n in {0, 1, 2}: the loop does not run
    for k in range(3):
        r = AR.estimate(p[:k], X[:k], K640)
        assert list(r["info"]) == [0, -1, 0, 0, 0, k, 0, 0]
        _nothing(r, k)
    # collinear 3D points (exactly: integer steps along one direction); the rotation about their line is free, so no sample gives a model
    line = (np.array([0.25, -0.5, 3.0]) + np.arange(n)[:, None] * np.array([0.125, 0.0625, 0.25])).astype(np.float32)
    pl = (line[:, :2] / line[:, 2:] * 800.0 + K640[:2, 2]).astype(np.float32)
    _nothing(AR.estimate(pl, line, K640, max_iterations=300), n, 300)
    # all points identical
    _nothing(AR.estimate(np.repeat(p[:1], n, 0), np.repeat(X[:1], n, 0), K640, max_iterations=300), n, 300)
    # NaN rows: never in a model, never inliers; the others still give the pose
    Xn, pn = X.copy(), p.copy()
    Xn[::3] = np.nan
    pn[1::7] = np.nan
    r = AR.estimate(pn, Xn, K640, 2.0, max_iterations=300)
    bad = np.isnan(Xn).any(1) | np.isnan(pn).any(1)
    assert r["info"][0] == 1 and not r["mask"][bad].any() and r["mask"][~bad].all() and np.isfinite(r["R"]).all()
    assert AS.pose_errors(np.eye(4)[:3], r["R"], r["t"])[0] <= 0.01
    _nothing(AR.estimate(np.full((n, 2), np.nan, np.float32), X, K640, max_iterations=300), n, 300)


def test_points_behind_the_camera_gather_no_consensus():
    """All points behind the camera, pixels through the centre of projection.  A triangle mirrored through the centre is congruent to
    itself, so P3P has a pose for every sample of three: "finds nothing" cannot hold for an estimator that returns a pose through n = 3
    points.  What must hold is that no consensus forms.  Such a pose reproduces the mirrored scene on the plane of its sample only: a
    point at distance d from that plane lands 2 d away from where its pixel wants it, which shows as 2 d sin(phi) / Z in the image (phi:
    the angle of its ray to the plane's normal, Z its depth <= 6), so an inlier at 2 px of f = 800 has d sin(phi) < 0.0075.  The 50 points
    are uniform in a 2 x 2 x 4 box: half of them inside one such slab does not happen.  So: no NaN, fewer than n / 2 inliers (measured:
    6 of 50), every inlier in front of the camera under the returned pose."""
    rng = np.random.default_rng(6)
    n = 50
    X = np.c_[rng.uniform(-1, 1, (n, 2)), -rng.uniform(2, 6, n)].astype(np.float32)
    p = (X[:, :2] / X[:, 2:] * 800.0 + K640[:2, 2]).astype(np.float32)
    r = AR.estimate(p, X, K640, 2.0, max_iterations=300)
    assert np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
    print("inliers of the behind-the-camera scene:", r["info"][3])
    assert r["info"][3] < n // 2 and r["mask"].sum() == (r["info"][3] if r["info"][0] else 0)
    Y = X.astype(np.float64) @ r["R"].T + r["t"]
    assert (Y[r["mask"].astype(bool), 2] > 0).all()


def test_three_points_give_a_pose_through_them():
    X, p, _, K, T = AS.scene3d(40, 3, 0.0, 0.0, seed=1)
    r = AR.estimate(p, X, K, 2.0)
    assert r["info"][0] == 1 and r["info"][3] == 3 and r["mask"].all()
    Y = X.astype(np.float64) @ r["R"].T + r["t"]
    px = np.c_[K[0, 0] * Y[:, 0] / Y[:, 2] + K[0, 2], K[1, 1] * Y[:, 1] / Y[:, 2] + K[1, 2]]
    assert (Y[:, 2] > 0).all() and np.abs(px - p).max() <= 1e-6            # pixels; the three points are fitted exactly


def test_poselib_shaped_wrapper_signature_and_no_cpu_path():
    from accelerated_features_amd import _lib, absolute_pose as m
    sig = inspect.signature(m.estimate_absolute_pose)
    assert list(sig.parameters) == ["points2D", "points3D", "camera", "ransac_opt", "bundle_opt", "seed"]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["ransac_opt"].default is None
    d = {k: v.default for k, v in inspect.signature(m.estimate_absolute_pose_batch).parameters.items()}
    assert (d["max_reproj_error"], d["success_prob"], d["min_iterations"], d["max_iterations"], d["seed"]) == (12.0, 0.9999, 20, 1000, 0)
    assert list(inspect.signature(m.estimate_absolute_pose_matches).parameters)[:6] == ["kpts_query", "points3d_ref", "idx_query", "idx_ref", "n_matches", "K"]
    assert m.INFO_FIELDS[0] == "found" and m.WORKSPACE_LIMIT == 512 << 20
    cam = {"model": "PINHOLE", "width": 640, "height": 480, "params": [800.0, 800.0, 320.0, 240.0]}
    pts2, pts3 = np.zeros((8, 2)), np.ones((8, 3))
    with pytest.raises(_lib.XFeatHipError):
        m.estimate_absolute_pose(pts2, pts3, dict(cam, model="SIMPLE_RADIAL"))
    with pytest.raises(_lib.XFeatHipError):
        m.estimate_absolute_pose(pts2, pts3, cam, {"max_epipolar_error": 1.0})
    with pytest.raises(_lib.XFeatHipError):
        m.estimate_absolute_pose(pts2, pts3, cam, {}, {"loss_scale": 1.0})
    none, det = m.estimate_absolute_pose(pts2[:2], pts3[:2], cam)
    assert none is None and det == {"inliers": [False, False], "num_inliers": 0, "iterations": 0, "refinements": 0}
    if not torch.cuda.is_available():
        with pytest.raises(_lib.XFeatHipError):
            m.estimate_absolute_pose(pts2, pts3, cam)
        with pytest.raises(_lib.XFeatHipError):
            m.estimate_absolute_pose_batch(torch.zeros(1, 8, 2), torch.zeros(1, 8, 3), None, K640)
        with pytest.raises(_lib.XFeatHipError):
            m.estimate_absolute_pose_matches(torch.zeros(1, 8, 2), torch.zeros(1, 8, 3), torch.zeros(1, 4, dtype=torch.int64),
                                             torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), K640)


def test_unproject_keypoints_on_a_hand_made_depth_map():
    from accelerated_features_amd.absolute_pose import unproject_keypoints
    depth = torch.arange(1.0, 17.0).reshape(1, 4, 4).clone()          # depth[v, u] = 1 + 4 v + u
    depth[0, 1, 2] = 0.0
    depth[0, 3, 0] = float("nan")
    depth[0, 0, 3] = -2.0
    K = np.array([[2.0, 0, 1.0], [0, 4.0, 2.0], [0, 0, 1]])
    kpts = torch.tensor([[[0.0, 0.0], [1.4, 2.4], [2.6, 2.6], [2.0, 1.0], [0.0, 3.0], [3.0, 0.0], [3.6, 1.0], [-0.6, 1.0], [1.0, 3.4],
                          [1.0, 3.6], [float("nan"), 1.0], [1.0, 1.0]]])
    X, valid = unproject_keypoints(kpts, depth, K, counts=torch.tensor([11]))
    assert X.dtype == torch.float32 and valid.dtype == torch.bool and X.shape == (1, 12, 3)
    #                  (0,0)  round->(1,2) round->(3,3) zero   nan    neg    u out  u out  (1,3)  v out  nan    beyond counts
    assert valid[0].tolist() == [True, True, True, False, False, False, False, False, True, False, False, False]
    assert torch.isnan(X[0][~valid[0]]).all() and torch.isfinite(X[0][valid[0]]).all()
    want = {0: (1.0, (0.0 - 1) / 2, (0.0 - 2) / 4), 1: (10.0, (1.4 - 1) / 2, (2.4 - 2) / 4), 2: (16.0, (2.6 - 1) / 2, (2.6 - 2) / 4), 8: (14.0, 0.0, (3.4 - 2) / 4)}
    for i, (d, x, y) in want.items():
        assert np.allclose(X[0, i].numpy(), np.float32([x * d, y * d, d]), rtol=1e-6, atol=0), (i, X[0, i])
    X2, v2 = unproject_keypoints(kpts, depth, torch.from_numpy(K)[None])
    assert v2[0, 11] and np.allclose(X2[0, 11].numpy(), [0.0, -1.5, 6.0])
