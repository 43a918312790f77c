"""xfh_camera_points and xfh_undistort_images on the device against the numpy restatement tests/cameras_reference.py, by the rules of
tests/cameras_support.py: pinhole and Brown outputs bit for bit; fisheye points within one fp32 spacing with equal status; fisheye images
(fp32 only) within 2^-22 (max - min of src).  Two calls give the same bytes.  A ramp image ties the two kernels to one model.  Both entries
are held to the buffer contract of include/xfeat_hip.h (tests/guarded.py: guard bands, stale prefills, untouched inputs; there is no
workspace to be short of) with a table of their own, and the census of tests/test_host_api.py / tests/test_gpu_buffers.py is run for
include/xfeat_hip_cameras.h: every declared name exported, bound and driven.  Folding the two entries into include/xfeat_hip.h,
_lib.SIGNATURES and guarded.TABLE -- which three existing test files tie together -- is the maintainer's follow-up.

End to end: the synthetic two-view scene cameras_support.E2E seen through a Brown model (-0.28, 0.07) and through the fisheye set, estimated
by ``cameras.estimate_relative_pose``.  The bounds are twice what the restatement chain gives on the CPU (cameras_reference undistortion,
then pose_reference.estimate, the same seed), computed here; measured:
    model     chain t / R (deg)     raw pixels with the pinhole K, t / R (deg)
    brown     0.00767 / 0.00782     0.384 / 0.885
    fisheye   0.00767 / 0.00782     1.610 / 1.210"""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest
import torch

import cameras_reference as CR
import cameras_support as CS
import guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("pinhole", "brown", "fisheye")


def _cam():
    from accelerated_features_amd import cameras
    return cameras


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _k3(k4):
    """(C,4) fx, fy, cx, cy -> (C,3,3), or None."""
    if k4 is None:
        return None
    K = np.zeros((len(k4), 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = k4[:, 0], k4[:, 1], k4[:, 2], k4[:, 3], 1.0
    return K


def _points(c, direction):
    fn = _cam().undistort_keypoints if direction == 0 else _cam().distort_keypoints
    r = fn(dev(c["pts"]), (c["kind"], c["params"]), dev(c["counts"]), _k3(c["k_other"]))
    torch.cuda.synchronize()
    return r["kpts"].cpu().numpy(), r["status"].cpu().numpy()


def _reference(c, direction):
    return CR.camera_points(c["pts"], c["counts"], c["kind"], c["params"], c["k_other"], direction)


# ---- the points ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", CS.KS)
@pytest.mark.parametrize("P", [1, 3])
def test_points_equal_the_restatement(P, K, family):
    seen = set()
    for shared in ((True, False) if P > 1 else (True,)):
        c = CS.points_case(100 * P + K + (7 if shared else 0), P, K, family, shared, other=not shared)
        want = _reference(c, 0)
        got = _points(c, 0)
        CS.check_points(got, want, family == "fisheye")
        assert CS.same_bits(_points(c, 0)[0], got[0]) and CS.same_bits(_points(c, 0)[1], got[1])     # two calls: the same bytes
        seen |= set(want[1].reshape(-1).tolist())
        und = np.where(np.isnan(want[0]) & ~np.isnan(c["pts"]), c["pts"], want[0])                   # points of the ideal image, the bad rows kept
        d = dict(c, pts=np.where(np.isfinite(c["pts"]), und, c["pts"]).astype(np.float32))
        CS.check_points(_points(d, 1), _reference(d, 1), family == "fisheye")
    if P == 3 and K >= 63:
        assert {CR.OK, CR.ROW, CR.POINT} <= seen
        bad = CS.points_case(K, P, K, family, False, bad_camera=True)
        want = _reference(bad, 0)
        assert (want[1][-1] == CR.CAMERA).all() and (want[1][1] == CR.OK).sum() > 0
        CS.check_points(_points(bad, 0), want, family == "fisheye")
        bad = dict(CS.points_case(K + 1, P, K, family, True, other=True))
        bad["k_other"][0, 1] = -1.0
        want = _reference(bad, 1)
        assert set(want[1].reshape(-1).tolist()) == {CR.ROW, CR.CAMERA}
        CS.check_points(_points(bad, 1), want, family == "fisheye")


def test_points_beyond_the_fold_outside_the_field_of_view_and_not_converging():
    cam = CS.brown_camera(0)                                            # k1 = -0.12: folds at r = 1 / 0.6
    kind, params = CS.packed([cam])
    f, cx, cy = cam["params"][0], cam["params"][2], cam["params"][3]
    rd_fold = (1.0 / 0.6) * (1 - 0.12 / 0.36)
    pts = np.array([[[cx + f * rd_fold * 1.01, cy], [cx + f * rd_fold * 0.99, cy], [cx + 10.0, cy + 20.0], [cx + f * 5.0, cy]]], np.float32)
    c = dict(pts=pts, counts=None, kind=kind, params=params, k_other=None)
    want = _reference(c, 0)
    assert want[1][0].tolist() == [CR.FOLD, CR.OK, CR.OK, CR.FOLD]
    CS.check_points(_points(c, 0), want, False)
    cam = CS.fisheye_camera()
    kind, params = CS.packed([cam])
    f, cx, cy = cam["params"][0], cam["params"][2], cam["params"][3]
    thd = 1.6 * CR.fisheye_poly(np.array(CS.FISHEYE_SET), 1.6 ** 2)
    pts = np.array([[[cx + f * thd, cy], [cx + 100.0, cy - 50.0], [cx, cy], [cx - f * thd * 0.7, cy]]], np.float32)
    c = dict(pts=pts, counts=None, kind=kind, params=params, k_other=None)
    want = _reference(c, 0)
    assert want[1][0].tolist() == [CR.OUTSIDE, CR.OK, CR.OK, CR.OK]
    CS.check_points(_points(c, 0), want, True)
    c = CS.not_converging_case()
    want = _reference(c, 0)
    assert want[1].tolist() == [[CR.NOT_CONVERGED, CR.OK]] * 2
    CS.check_points(_points(c, 0), want, False)


def test_key_points_of_one_image_and_camera_dicts():
    cams = _cam()
    cam = CS.brown_camera(3)
    c = CS.points_case(9, 1, 65, "brown", True, ragged=False)
    kind, params = CS.packed([cam])
    c = dict(c, kind=kind, params=params)
    r = cams.undistort_keypoints(c["pts"][0], cam)                       # (K, 2) numpy in, one dict
    assert r["kpts"].shape == (65, 2) and r["status"].shape == (65,) and r["kpts"].is_cuda
    want = _reference(c, 0)
    CS.check_points((r["kpts"].cpu().numpy()[None], r["status"].cpu().numpy()[None]), want, False)
    assert torch.equal(r["K"].cpu(), cams.camera_matrix(cam))
    back = cams.distort_keypoints(r["kpts"], cam)
    ok = r["status"].cpu().numpy() == 0
    assert np.abs(back["kpts"].cpu().numpy()[ok] - c["pts"][0][ok]).max() < 2e-4     # the fp32 rounding of the ideal pixels


# ---- the images ---------------------------------------------------------------------------------------------------------------------------
def _images(c, k_new, Ho, Wo, fill, with_valid):
    r = _cam().undistort_images(dev(c["src"]), (c["kind"], c["params"]), _k3(k_new), (Ho, Wo), fill, with_valid)
    torch.cuda.synchronize()
    return (r[0].cpu().numpy(), r[1].cpu().numpy()) if with_valid else (r.cpu().numpy(), None)


def _check_images(c, k_new, Ho, Wo, fill, with_valid, fisheye):
    dst, valid = _images(c, k_new, Ho, Wo, fill, with_valid)
    w_dst, w_valid, exact = CR.undistort_images(c["src"], c["kind"], c["params"], k_new, Ho, Wo, fill)
    if with_valid:
        assert CS.same_bits(valid, w_valid)
    if not fisheye:
        assert CS.same_bits(dst, w_dst)
    else:
        CS.check_fisheye_f32(dst, exact, c["src"], fill)
    again = _images(c, k_new, Ho, Wo, fill, with_valid)
    assert CS.same_bits(again[0], dst) and (not with_valid or CS.same_bits(again[1], valid))          # two calls: the same bytes
    return w_valid


@pytest.mark.parametrize("family,dtype", [(f, d) for f in FAMILIES for d in (np.uint8, np.float32) if (f, d) != ("fisheye", np.uint8)])
@pytest.mark.parametrize("C_", [1, 3])
def test_images_equal_the_restatement(C_, family, dtype):
    c = CS.image_case(10 * C_ + (1 if dtype == np.uint8 else 2), 2, C_, 37, 53, dtype, family)
    _check_images(c, None, 29, 41, 0.0, False, family == "fisheye")
    v = _check_images(c, CS.new_k(c, 0.5), 29, 41, 7.25 if dtype == np.uint8 else 0.25, True, family == "fisheye")
    assert v.min() == 0 and v.max() == 1
    one = CS.image_case(3, 2, C_, 1, 1, dtype, family, shared=True)
    _check_images(one, None, 1, 1, 3.0 if dtype == np.uint8 else 0.5, True, family == "fisheye")
    if C_ == 3 and family == "brown":                                   # an unusable camera in the batch: `fill`, valid 0
        bad = dict(c, params=c["params"].copy())
        bad["params"][1, 0] = 0.0
        v = _check_images(bad, None, 29, 41, 200.5, True, False)
        assert not v[1].any() and v[0].any()
        wide = CS.image_case(4, 1, 4, 5, 130, dtype, family)             # more than one workgroup along x, four channels
        _check_images(wide, None, 7, 131, 1.0, True, False)


@pytest.mark.parametrize("family", ["brown", "fisheye"])
def test_a_ramp_image_ties_the_two_kernels_to_one_model(family):
    """Bilinear sampling reproduces a x + b y + c, so every valid pixel of the rectified ramp equals the ramp at the raw position of its own
    coordinate, which distort_keypoints gives.  Tolerance: the fp32 rounding of that position (half a spacing of each coordinate, times the
    slopes) plus the fp32 rounding of the value; both kernels evaluate the same fp64 expressions on the same fp64 inputs."""
    cams = _cam()
    a, b, c0 = 0.5, 0.25, 3.0                                           # every ramp value is exact in fp32
    H, W = 72, 96
    cam = CS.image_case(0, 1, 1, H, W, np.float32, family, shared=True)
    y, x = np.mgrid[0:H, 0:W]
    src = (a * x + b * y + c0).astype(np.float32)[None, None]
    dst, valid = cams.undistort_images(dev(src), (cam["kind"], cam["params"]), return_valid=True)
    grid = np.stack([x, y], axis=2).reshape(1, H * W, 2).astype(np.float32)
    raw = cams.distort_keypoints(dev(grid), (cam["kind"], cam["params"]))
    torch.cuda.synchronize()
    assert not raw["status"].any()
    xy = raw["kpts"].cpu().numpy().reshape(H, W, 2).astype(np.float64)
    want = a * xy[..., 0] + b * xy[..., 1] + c0
    tol = (a * np.spacing(np.abs(xy[..., 0]).astype(np.float32)) / 2 + b * np.spacing(np.abs(xy[..., 1]).astype(np.float32)) / 2
           + np.spacing(np.abs(want).astype(np.float32)) / 2).astype(np.float64) * (1 + 1e-6)
    ok = valid.cpu().numpy()[0] == 1
    assert 0.5 * H * W < ok.sum()
    assert (np.abs(dst.cpu().numpy()[0, 0].astype(np.float64) - want)[ok] <= tol[ok]).all()


# ---- the buffer contract and the census of the new header ------------------------------------------------------------------------------------
TABLE = {"xfh_camera_points": guarded.Entry((9, 10)), "xfh_undistort_images": guarded.Entry((13, 14))}
CASES = {}


class Case:
    def __init__(self, inputs, call):
        self.inputs, self.call = [t for t in inputs if t is not None], call


def _points_case(direction):
    def make(seed, small):
        P, K = (2, 75) if small else (3, 77)
        c = CS.points_case(3000 + seed, P, K, "brown" if direction == 0 else "fisheye", False, other=True)
        a = [dev(c["pts"]), dev(c["kind"]), dev(c["params"]), dev(c["counts"]), dev(_k3(c["k_other"]))]
        fn = _cam().undistort_keypoints if direction == 0 else _cam().distort_keypoints
        return Case(a, lambda: fn(a[0], (a[1], a[2]), a[3], a[4]))
    return make


def _images_case(dtype):
    def make(seed, small):
        B, Ch, H, W, Ho, Wo = (1, 2, 31, 47, 23, 37) if small else (2, 3, 37, 53, 29, 41)
        c = CS.image_case(3100 + seed, B, Ch, H, W, dtype, "brown")
        a = [dev(c["src"]), dev(c["kind"]), dev(c["params"]), dev(_k3(CS.new_k(c, 0.5)))]
        return Case(a, lambda: _cam().undistort_images(a[0], (a[1], a[2]), a[3], (Ho, Wo), 9.0, True))
    return make


CASES["xfh_camera_points[undistort]"] = ("xfh_camera_points", _points_case(0))
CASES["xfh_camera_points[distort]"] = ("xfh_camera_points", _points_case(1))
CASES["xfh_undistort_images[u8]"] = ("xfh_undistort_images", _images_case(np.uint8))
CASES["xfh_undistort_images[f32]"] = ("xfh_undistort_images", _images_case(np.float32))


def test_every_declared_name_is_exported_bound_and_driven():
    cams = _cam()
    from accelerated_features_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip_cameras.h")).read()
    declared = set(re.findall(r"\b(xfh_[a-z_0-9]+)\s*\(", hdr[hdr.index("#ifndef"):]))
    raw = C.CDLL(_lib.LIB_PATH)
    assert declared and all(hasattr(raw, n) for n in declared)
    assert declared == set(cams.SIGNATURES) == set(TABLE) == {e for e, _ in CASES.values()}
    assert not any(guarded.Proxy.has_workspace(args) for _, args in cams.SIGNATURES.values())        # no workspace: nothing to be short of


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_holds_the_buffer_contract(name):
    cams = _cam()
    from accelerated_features_amd import _lib
    entry, make = CASES[name]
    t0 = time.perf_counter()
    problems, _ = guarded.hold(make, cams, TABLE, "cuda", entry, error=_lib.XFeatHipError)
    print(f"{name}: {time.perf_counter() - t0:.2f} s")
    assert not problems, "\n".join(problems)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(CS.E2E_MODELS))
def test_relative_pose_through_distorting_cameras(which):
    cams = _cam()
    from accelerated_features_amd import pose
    raw0, raw1, cam0, cam1, K0, K1, T, _ = CS.distorted_scene(which)
    chain, keep = CS.restatement_chain(raw0, raw1, cam0, cam1, K0, K1)
    assert chain["info"][0] == 1 and keep.all()
    t_chain, r_chain = pose.relative_pose_error(T, chain["R"], chain["t"])
    opt = {"max_iterations": CS.E2E["max_iterations"]}
    model, details = cams.estimate_relative_pose(raw0, raw1, cam0, cam1, opt, seed=CS.E2E["pose_seed"])
    assert model is not None and len(details["inliers"]) == len(raw0)
    t_err, r_err = pose.relative_pose_error(T, model.R, model.t)
    print(f"{which}: device t {t_err:.5f} R {r_err:.5f} deg; chain t {t_chain:.5f} R {r_chain:.5f} deg; inliers {details['num_inliers']} / {chain['info'][3]}")
    assert t_err <= 2 * t_chain and r_err <= 2 * r_chain
    # the raw pixels with the pinhole K of the same fx, fy, cx, cy: worse than that bound -- the undistortion is what makes the pose
    pin = [{"model": "PINHOLE", "width": 0, "height": 0, "params": c["params"][:4]} for c in (cam0, cam1)]
    naive, _ = pose.estimate_relative_pose(raw0, raw1, pin[0], pin[1], opt, seed=CS.E2E["pose_seed"])
    if naive is not None:
        t_raw, r_raw = pose.relative_pose_error(T, naive.R, naive.t)
        print(f"{which}: raw pixels with the pinhole K t {t_raw:.5f} R {r_raw:.5f} deg")
        assert t_raw > 2 * t_chain and r_raw > 2 * r_chain


def test_poselib_shaped_wrappers_drop_rows_and_pass_pinhole_through():
    cams = _cam()
    from accelerated_features_amd import absolute_pose, pose
    raw0, raw1, cam0, cam1, K0, K1, T, (p0, p1) = CS.distorted_scene("fisheye")
    opt = {"max_iterations": 500}
    # PINHOLE and SIMPLE_PINHOLE inputs: the existing wrapper's result
    pin0 = {"model": "PINHOLE", "width": 0, "height": 0, "params": cam0["params"][:4]}
    pin1 = {"model": "PINHOLE", "width": 0, "height": 0, "params": cam1["params"][:4]}
    a, da = cams.estimate_relative_pose(p0, p1, pin0, pin1, opt, seed=2)
    b, db = pose.estimate_relative_pose(p0, p1, pin0, pin1, opt, seed=2)
    assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and da == db
    # rows without a pinhole image (not finite, outside the fisheye's field of view) are dropped and come back as False
    bad0 = raw0.copy()
    bad0[5] = np.nan
    bad0[9] = [cam0["params"][2] + cam0["params"][0] * 1.7, cam0["params"][3]]
    m, d = cams.estimate_relative_pose(bad0, raw1, cam0, cam1, opt, seed=2)
    keep = np.ones(len(raw0), bool)
    keep[[5, 9]] = False
    m2, d2 = cams.estimate_relative_pose(raw0[keep], raw1[keep], cam0, cam1, opt, seed=2)
    assert m is not None and np.array_equal(m.R, m2.R) and len(d["inliers"]) == len(raw0) and not d["inliers"][5] and not d["inliers"][9]
    assert [v for v, k in zip(d["inliers"], keep) if k] == d2["inliers"] and d["num_inliers"] == d2["num_inliers"] == sum(d["inliers"])
    # absolute pose: points in front of camera 0 at known depths, seen through the fisheye
    rng = np.random.default_rng(4)
    z = rng.uniform(2.0, 6.0, len(p0))
    X = np.c_[(p0[:, 0] - K0[0, 2]) / K0[0, 0] * z, (p0[:, 1] - K0[1, 2]) / K0[1, 1] * z, z]
    Rw, tw = _rotation(rng), rng.normal(size=3)
    Xw = (X - tw) @ Rw                                                   # X_cam = Rw X_world + tw
    bad0[9] = raw0[9]
    m, d = cams.estimate_absolute_pose(bad0, Xw, cam0, {"max_iterations": 500, "max_reproj_error": 2.0}, seed=1)
    assert m is not None and not d["inliers"][5] and len(d["inliers"]) == len(raw0) and d["num_inliers"] > 0.9 * len(raw0)
    assert np.abs(m.R - Rw).max() < 1e-3 and np.abs(m.t - tw).max() < 2e-2
    with pytest.raises(Exception):
        absolute_pose.estimate_absolute_pose(raw0, Xw, cam0)             # the existing wrapper keeps refusing the model


def _rotation(rng):
    import twoview_support as TS
    return TS.rotation(rng.normal(size=3) * 0.4)
