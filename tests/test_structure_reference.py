"""The numpy restatement of the two-view structure kernels (tests/structure_reference.py) against ground truth, on
twoview_support.motion / project scenes at f = 800: the quality of the correction and of the points, every status by a constructed case,
the pose of a scaled E, and the pose of an estimated F."""
import math

import numpy as np
import pytest

import fundamental_reference as FR
import structure_reference as SR
import structure_support as SS
import twoview_support as TS
from accelerated_features_amd.pose import relative_pose_error
from accelerated_features_amd.structure import essential_from_fundamental

K = SS.K


def _points(w):
    return np.stack([w["l0"] * w["y0"][0], w["l0"] * w["y0"][1], w["l0"]], axis=1)


def test_noise_free_points_are_recovered_to_1e_12():
    """Measured: 1.7e-14 relative over 50 motions of 100 points (float64 pixels: the function itself, not the float32 input format)."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(50):
        s = SS.scene(rng, 100)
        w = SR.triangulate(s["p0"], s["p1"], K, K, s["R"], s["t"], pixels64=True)
        assert np.isin(w["status"], (SR.VALID, SR.BEHIND, SR.PARALLAX)).all() and (w["status"] == SR.VALID).mean() > 0.5 or (s["X"] @ s["R"].T + s["t"])[:, 2].min() < 0
        worst = max(worst, float((np.linalg.norm(_points(w) - s["X"], axis=1) / np.linalg.norm(s["X"], axis=1)).max()))
    print("noise-free relative error", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("sigma", [0.5, 1.0, 3.0, 10.0])
def test_the_corrected_pair_is_on_the_constraint_and_optimal_to_first_order(sigma):
    """5000 samples (50 motions of 100 points) per noise level.  Measured (median / max): epipolar residual 1.8e-14 / 2.3e-13 px at 0.5 px,
    2.0e-14 / 1.6e-12 at 1 px, 1.6e-14 / 3.6e-13 at 3 px, 2.1e-14 / 2.6e-13 at 10 px; optimality residual 5.6e-9 / 2.9e-5, 1.7e-8 / 6.2e-5,
    2.6e-7 / 2.7e-3, 3.1e-6 / 2.6e-2.  (With niter2's closing step lambda <- lambda 2 d / (n.n + n'.n') in place of the second quadratic
    solve the residual was 2.7e-9 / 1.4e-2 px at 10 px on these samples, above the 1e-2 px bound: a pair near an epipole.)"""
    rng = np.random.default_rng(int(sigma * 10))
    res, opt = [], []
    for _ in range(50):
        s = SS.scene(rng, 100, noise=sigma)
        w = SR.triangulate(s["p0"], s["p1"], K, K, s["R"], s["t"], pixels64=True)
        E = TS.essential_from_pose(s["R"], s["t"])
        y0 = np.stack([w["y0"][0], w["y0"][1], np.ones(100)], axis=1)
        y1 = np.stack([w["y1"][0], w["y1"][1], np.ones(100)], axis=1)
        g = np.c_[(y1 @ E)[:, :2], (y0 @ E.T)[:, :2]]       # the constraint's gradient in (y0, y1) at the corrected point
        res.append(np.abs(np.einsum("ij,ij->i", y1, y0 @ E.T)) / np.linalg.norm(g, axis=1) * SS.F)
        d = np.c_[w["x0"][0] - w["y0"][0], w["x0"][1] - w["y0"][1], w["x1"][0] - w["y1"][0], w["x1"][1] - w["y1"][1]]
        gu = g / np.linalg.norm(g, axis=1)[:, None]
        opt.append(np.linalg.norm(d - np.einsum("ij,ij->i", d, gu)[:, None] * gu, axis=1) / np.linalg.norm(d, axis=1))
    res, opt = np.concatenate(res), np.concatenate(opt)
    print(f"sigma {sigma}: residual median {np.median(res):.3g} max {res.max():.3g} px, optimality median {np.median(opt):.3g} max {opt.max():.3g}")
    assert len(res) == 5000
    assert np.median(res) <= 1e-8 and res.max() <= 1e-2
    assert opt.max() <= 0.05


def _one(X, R, t, **kw):
    p0, p1 = SS.project_points(np.atleast_2d(np.asarray(X, np.float64)), R, t)
    return SR.triangulate(p0, p1, K, K, R, t, **kw)


def test_every_status_is_hit_by_a_constructed_case():
    R = TS.rotation(np.array([0.02, -0.1, 0.03]))
    t = np.array([0.5, 0.1, -0.5])
    X = np.array([[0.3, -0.2, 4.0]])
    assert list(_one(X, R, t)["status"]) == [SR.VALID]
    # a point behind camera 1: the camera moved 10 units forward, past the point
    tb = np.array([0.5, 0.1, -10.0])
    w = _one(X, R, tb)
    assert list(w["status"]) == [SR.BEHIND] and w["l0"][0] > 0 and w["l1"][0] < 0 and np.isnan(w["points3d"]).all() and np.isfinite(w["reproj_error"]).all()
    # max_depth just below and just above a known depth (camera 0 sees it at 4, camera 1 nearer)
    assert (R @ X[0] + t)[2] < 4.0
    assert list(_one(X, R, t, max_depth=4.0 * (1 - 1e-6), pixels64=True)["status"]) == [SR.FAR]
    assert list(_one(X, R, t, max_depth=4.0 * (1 + 1e-6), pixels64=True)["status"]) == [SR.VALID]
    # zero parallax: t along the ray (the point is on the baseline, beyond camera 1's centre as seen from camera 0)
    C1 = -R.T @ t
    tz = np.array([0.1, 0.05, -1.0])                       # camera 1 one unit ahead of camera 0, nearly on the axis
    w = _one(np.array([-R.T @ tz * 3.0]), R, tz)
    assert w["status"][0] != SR.VALID and np.isnan(w["points3d"]).all()      # (the depths are 0 / 0 up to rounding: any gate may catch it first)
    w = SR.triangulate(K[:2, 2][None], K[:2, 2][None], K, K, np.eye(3), np.array([0.0, 0.0, -1.0]))      # exactly: both rays are the axis, zz = 0
    assert list(w["status"]) == [SR.NOT_FINITE] and np.isnan(w["reproj_error"]).all()
    far = np.array([[300.0, -200.0, 4000.0]])              # 0.007 degrees of parallax: below the default 1 degree, fine at 0
    assert list(_one(far, R, t)["status"]) == [SR.PARALLAX] and list(_one(far, R, t, min_parallax_deg=0.0)["status"]) == [SR.VALID]
    assert C1 is not None
    # reprojection: one pixel moved 20 px off its epipolar line
    p0, p1 = SS.project_points(X, R, t)
    E = TS.essential_from_pose(R, t)
    line = E @ np.array([(p0[0, 0] - K[0, 2]) / SS.F, (p0[0, 1] - K[1, 2]) / SS.F, 1.0])
    p1 = p1 + 20.0 * line[:2] / np.linalg.norm(line[:2])
    w = SR.triangulate(p0, p1, K, K, R, t)
    assert list(w["status"]) == [SR.REPROJ] and 9.0 < w["reproj_error"][0] < 11.0        # the displacement is shared by the two images
    assert list(SR.triangulate(p0, p1, K, K, R, t, max_reproj_error=12.0)["status"]) == [SR.VALID]
    # NaN rows, a masked row, a zeroed pose
    s = SS.scene(np.random.default_rng(0), 6)
    p0, p1 = s["p0"].copy(), s["p1"].copy()
    p0[1, 0], p1[2, 1], p0[3] = np.nan, np.inf, np.nan
    w = SR.triangulate(p0, p1, K, K, s["R"], s["t"], mask=np.array([1, 1, 1, 1, 0, 1]))
    assert list(w["status"]) == [0, 2, 2, 2, 1, 0] and list(w["info"]) == [6, 2, 1, 3, 0, 0, 0, 0]
    assert np.isnan(w["points3d"][1:5]).all() and np.isfinite(w["points3d"][[0, 5]]).all()
    assert np.isnan(w["reproj_error"][1:5]).all() and np.isfinite(w["reproj_error"][[0, 5]]).all()
    w = SR.triangulate(s["p0"], s["p1"], K, K, np.zeros((3, 3)), np.zeros(3), mask=np.array([1, 1, 1, 1, 0, 1]))
    assert list(w["status"]) == [2, 2, 2, 2, 1, 2]
    assert list(SR.triangulate(s["p0"], s["p1"], K, K, s["R"], np.zeros(3))["status"]) == [2] * 6
    # the list form's index out of range: not finite
    assert list(SR.triangulate(s["p0"], s["p1"], K, K, s["R"], s["t"], in_range=np.arange(6) != 2)["status"]) == [0, 0, 2, 0, 0, 0]
    # no correspondence at all
    w = SR.triangulate(np.zeros((0, 2)), np.zeros((0, 2)), K, K, s["R"], s["t"])
    assert w["points3d"].shape == (0, 3) and list(w["info"]) == [0] * 8


@pytest.mark.parametrize("scale", SS.SCALES)
def test_recover_pose_finds_the_true_pose_of_a_scaled_E(scale):
    rng = np.random.default_rng(5)
    for k in range(8):
        s = SS.scene_in_front(rng, 60)
        tu = s["t"] / np.linalg.norm(s["t"])
        p0, p1 = s["p0"].copy(), s["p1"].copy()
        p0[7] = np.nan
        w = SR.recover_pose(scale * TS.essential_from_pose(s["R"], tu), p0, p1, K, K, 50.0, pixels64=True)
        assert w["found"] and np.abs(w["R"] - s["R"]).max() <= 1e-9 and np.abs(w["t"] - tu).max() <= 1e-9
        good = list(w["good"])
        assert good[w["pose"]] == 59 and sorted(good)[-2] < 59            # every finite point, and the other three get fewer
        assert w["mask"].sum() == 59 and w["mask"][7] == 0
        X = w["points3d"][w["mask"] != 0].astype(np.float64) * np.linalg.norm(s["t"])
        assert np.abs(X - s["X"][w["mask"] != 0]).max() < 1e-5           # float32 points
        assert np.abs(np.array(w["R"]) @ np.array(w["R"]).T - np.eye(3)).max() < 1e-14
    w = SR.recover_pose(np.zeros((3, 3)), p0, p1, K, K)
    assert not w["found"] and w["pose"] == -1 and not w["R"].any() and not w["t"].any() and not w["mask"].any() and list(w["info"]) == [0, -1, 0, 0, 0, 60, 0, 0]


def _svd_errors(E, T):
    """(t_err, R_err) of the textbook decomposition of E (U W V', U W' V', t = +-u3): the better of the two rotations."""
    U, _, Vt = np.linalg.svd(E)
    U, Vt = (U if np.linalg.det(U) > 0 else -U), (Vt if np.linalg.det(Vt) > 0 else -Vt)
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return min((relative_pose_error(T, Rs, U[:, 2]) for Rs in (U @ W @ Vt, U @ W.T @ Vt)), key=lambda e: e[1])


@pytest.mark.parametrize("pair", [0, 7, 33, 100, 250])
def test_recover_pose_of_an_estimated_F_is_as_good_as_the_F(pair):
    """E = K1' F K0 of the fundamental restatement's F (400 matches, 0.5 px noise, 20 % outliers): the winner is the pose on the true
    side, and its errors are the F estimate's own -- those of the textbook SVD decomposition of the same E, which no decomposition can
    beat by more than rounding -- + 1e-6 degrees.  Measured: equal to 1e-10 degrees (0.010 - 0.049 degrees of rotation, 0.012 - 0.045 of
    translation angle on these pairs); without tg_orthonormalise the rotation error was 0.012 - 0.022 degrees above the SVD's."""
    p0, p1, _, K0, K1, T = TS.scene(pair, 400, 0.5, 0.2, pair)
    r = FR.estimate(p0, p1, 1.5, 300, 0.99, seed=0)
    assert r["info"][0] == 1
    E = essential_from_fundamental(r["F"][0].reshape(3, 3), K0, K1)
    w = SR.recover_pose(E, p0, p1, K0, K1, 50.0, mask=r["mask"])
    assert w["found"]
    t_err, R_err = relative_pose_error(T, w["R"], w["t"])
    t_svd, R_svd = _svd_errors(E, T)
    print(f"pair {pair}: t_err {t_err:.6f} (svd {t_svd:.6f}) R_err {R_err:.6f} (svd {R_svd:.6f}) good {list(w['good'])}")
    assert float(np.dot(w["t"], T[:3, 3])) > 0.0           # the right side: not the mirrored translation
    assert R_err <= R_svd + 1e-6 and t_err <= t_svd + 1e-6
    assert w["good"][w["pose"]] >= 0.95 * r["mask"].sum() and sorted(w["good"])[-2] < 0.1 * r["mask"].sum()


def test_essential_from_fundamental_is_the_inverse_of_fundamental_from_pose():
    import torch
    from accelerated_features_amd.guided import fundamental_from_pose
    f = TS.fixture()
    T = f["T_0to1"][3]
    tu = T[:3, 3] / np.linalg.norm(T[:3, 3])
    F = fundamental_from_pose(torch.as_tensor(T[:3, :3]), torch.as_tensor(tu), torch.as_tensor(f["K0"][3]), torch.as_tensor(f["K1"][3])).numpy()
    E = essential_from_fundamental(F, f["K0"][3], f["K1"][3])
    assert np.abs(E - TS.essential_from_pose(T[:3, :3], tu)).max() < 1e-12
    assert essential_from_fundamental(np.stack([F, F]), f["K0"][3], f["K1"][3]).shape == (2, 3, 3)
    assert not essential_from_fundamental(np.zeros((3, 3)), f["K0"][3], f["K1"][3]).any()
    assert math.isclose(np.linalg.norm(E) ** 2 / 2, 1.0, rel_tol=1e-6)           # (the fixture's rotations are float32)
