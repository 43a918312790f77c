"""Two-view structure on MI355X: the 3D points that the matches of a pair see, and the pose of an essential matrix.

    n, R, t, mask = cv2.recoverPose(E, points1, points2, cameraMatrix)          # modules/eval/scannet1500.py:84 (estimate_pose, 'opencv')

``triangulate_batch`` / ``triangulate_matches`` turn the correspondences of P pairs and a relative pose (``estimate_relative_pose_*``'s
``R``, ``t``) into points in camera 0's frame, with a status per correspondence (cheirality, depth, reprojection error, parallax);
``triangulate_matches`` can scatter them to image 0's key-point rows, which is what ``estimate_absolute_pose_matches`` takes as
``points3d_ref``: detect -> match -> relative pose -> points -> absolute pose of the next image stays in HBM.  ``recover_pose_batch`` /
``recover_pose_matches`` decompose an E (any scale or sign; ``essential_from_fundamental`` makes one of an F) into its four poses and
keep the one that puts most points in front of both cameras; ``recover_pose`` has ``cv2.recoverPose``'s shape.  The kernels behind
``xfh_triangulate`` / ``xfh_recover_pose`` (include/xfeat_hip.h, csrc/k_triangulate.hip) run Lindstrom's optimal correction (niter2) and the
closed-form depths of the corrected rays per correspondence; DESIGN.md 3.14 is the specification.  OpenCV is not a dependency and is not
available here, so the results agree with it as estimates of the same geometry, not bit for bit.  There is no CPU path: without the HIP
library and a gfx950 device the functions raise.
"""
import math

import numpy as np
import torch

from . import _lib, _twoview
from ._twoview import ptr as _ptr

STATUS = ("valid", "masked", "not_finite", "behind", "far", "reproj", "parallax")      # the status codes 0 .. 6
INFO_FIELDS = ("n", "valid", "masked", "not_finite", "behind", "far", "reproj", "parallax")
RECOVER_INFO_FIELDS = ("found", "pose", "unused2", "n_good", "unused4", "n", "unused6", "unused7")
MAX_PAIRS = 65535                            # of one library call; larger batches are split into chunks of pairs
_WHAT = "two-view structure"


def _f64(x, shape, P, dev, name):
    x = torch.as_tensor(x, dtype=torch.float64)
    if x.shape == shape:
        x = x.expand(P, *shape)
    if x.shape != (P, *shape):
        raise RuntimeError(f'{name} must be {shape} or {(P, *shape)}')
    return x.to(dev).contiguous()


def _mask(mask, P, cap, dev):
    if mask is None:
        return None
    mask = torch.as_tensor(mask).to(dev)
    if mask.shape != (P, cap):
        raise RuntimeError('mask must be (P, cap)')
    return (mask != 0).to(torch.uint8).contiguous()


def _positive(who, name, v, inf_ok):
    v = float(v)
    if not v > 0.0 or (math.isinf(v) and not inf_ok) or math.isnan(v):
        raise _lib.XFeatHipError(f"{who}: {name} {v} must be positive{'' if inf_ok else ' and finite'}")
    return v


def _chunks(P):
    return [(a, min(P, a + MAX_PAIRS)) for a in range(0, P, MAX_PAIRS)]


def _triangulate(who, pts0, pts1, index, counts, n_const, P, cap, K0, K1, R, t, max_reproj_error, min_parallax_deg, max_depth, mask, scatter, dev):
    """Shared driver: outputs, one library call per chunk of 65535 pairs.  index = (idx0, idx1, kcap) or None."""
    thr = _positive(who, "max_reproj_error", max_reproj_error, False)
    depth = _positive(who, "max_depth", max_depth, True)
    deg = float(min_parallax_deg)
    if not 0.0 <= deg <= 180.0:
        raise _lib.XFeatHipError(f"{who}: min_parallax_deg {deg} outside [0, 180]")
    cos_min = math.cos(math.radians(deg))
    K0, K1 = _f64(K0, (3, 3), P, dev, 'intrinsics'), _f64(K1, (3, 3), P, dev, 'intrinsics')
    R, t = _f64(R, (3, 3), P, dev, 'R'), _f64(t, (3,), P, dev, 't')
    mask = _mask(mask, P, cap, dev)
    X = torch.empty((P, cap, 3), dtype=torch.float32, device=dev)
    status = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    err = torch.empty((P, cap), dtype=torch.float32, device=dev)
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    out = {'points3d': X, 'status': status, 'reproj_error': err, 'info': info}
    ref = None
    if scatter:
        ref = torch.empty((P, index[2], 3), dtype=torch.float32, device=dev)
        out['points3d_ref'] = ref
    if P == 0 or cap == 0:                    # no correspondence at all: every element written like the kernel writes it
        X.fill_(float('nan')); err.fill_(float('nan')); status.fill_(1); info.zero_()
        if ref is not None:
            ref.fill_(float('nan'))
    else:
        lib = _lib.load()
        stream = torch.cuda.current_stream(dev).cuda_stream
        for a, b in _chunks(P):
            head = _twoview.list_args(pts0, pts1, index, counts, n_const, a, b, cap)
            tail = (_ptr(K0[a:b]), _ptr(K1[a:b]), _ptr(R[a:b]), _ptr(t[a:b]), _ptr(mask[a:b]) if mask is not None else None, thr, cos_min, depth,
                    _ptr(X[a:b]), _ptr(status[a:b]), _ptr(err[a:b]), _ptr(info[a:b]))
            if index is None:
                rc = lib.xfh_triangulate(*head, *tail, stream)
            else:
                rc = lib.xfh_triangulate_matches(*head, *tail, _ptr(ref[a:b]) if ref is not None else None, stream)
            _lib.check(rc, who)
    out['valid'] = status == 0
    return out


def triangulate_batch(pts0, pts1, counts, K0, K1, R, t, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=float('inf'), mask=None):
    """The 3D points of the correspondences of P pairs under their relative poses, in one call.

    pts0, pts1 : (P, cap, 2) float32 pixel coordinates (row i of pts0 matches row i of pts1)
    counts     : (P,) int32, pair p uses its first counts[p] rows; None = all cap rows
    K0, K1     : (P, 3, 3) or (3, 3) float64 PINHOLE intrinsics;  R (P,3,3) / (3,3), t (P,3) / (3,) float64 with X1 = R X0 + t (the 'R',
                 't' of estimate_relative_pose_batch; a pair that found no pose carries zeros and gets status 2 everywhere)
    mask       : (P, cap) or None; a zero masks the correspondence out (for instance the estimator's 'inliers')
    Each correspondence is moved onto the epipolar constraint by the least displacement (Lindstrom, niter2), then X = depth * ray in
    camera 0's frame and t's unit.  status (STATUS): 0 valid, 1 masked (also rows beyond the count), 2 not finite, 3 behind a camera,
    4 deeper than max_depth in a camera, 5 displaced by more than max_reproj_error pixels in an image, 6 rays closer than
    min_parallax_deg.  Returns a dict of CUDA tensors: 'points3d' (P,cap,3) float32, NaN unless valid (unproject_keypoints'
    convention: the points go into estimate_absolute_pose_* as they are), 'status' (P,cap) uint8, 'reproj_error' (P,cap) float32 pixels
    (NaN for status 1 and 2), 'info' (P,8) int32 (INFO_FIELDS: the count and the number of its rows per status), 'valid' (P,cap) bool.
    Asynchronous."""
    pts0, pts1, counts, dev = _twoview.check_points(_WHAT, pts0, pts1, counts)
    P, cap = pts0.shape[0], pts0.shape[1]
    return _triangulate("xfh_triangulate", pts0, pts1, None, counts, cap, P, cap, K0, K1, R, t, max_reproj_error, min_parallax_deg, max_depth,
                        mask, False, dev)


def triangulate_matches(kpts0, kpts1, idx0, idx1, n_matches, K0, K1, R, t, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=float('inf'),
                        mask=None, scatter=True):
    """triangulate_batch straight on the matcher's output: correspondence i of pair p is (kpts0[p, idx0[p, i]], kpts1[p, idx1[p, i]]) for
    i < n_matches[p] (kpts (P,K,2) float32, idx (P,cap) int64, n_matches (P,) int32 CUDA tensors).  Same result dict; with ``scatter`` also
    'points3d_ref' (P,K,3) float32: the valid points at image 0's key-point rows, NaN elsewhere -- ``points3d_ref`` of
    ``estimate_absolute_pose_matches`` for a third image matched against image 0.  One-to-one index lists (as the matchers produce them)
    are the contract: with duplicate rows in idx0 a row holds one of its candidates.  An index outside [0, K) gives status 2."""
    dev, P, cap = _twoview.check_matches("triangulate_matches", kpts0, kpts1, idx0, idx1, n_matches)
    return _triangulate("xfh_triangulate_matches", kpts0, kpts1, (idx0, idx1, kpts0.shape[1]), n_matches, 0, P, cap, K0, K1, R, t,
                        max_reproj_error, min_parallax_deg, max_depth, mask, bool(scatter), dev)


def _recover(who, E, pts0, pts1, index, counts, n_const, P, cap, K0, K1, distance_thresh, mask, dev):
    thr = _positive(who, "distance_thresh", distance_thresh, True)
    K0, K1 = _f64(K0, (3, 3), P, dev, 'intrinsics'), _f64(K1, (3, 3), P, dev, 'intrinsics')
    E = _f64(E, (3, 3), P, dev, 'E')
    mask = _mask(mask, P, cap, dev)
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((P, 3), dtype=torch.float64, device=dev)
    good = torch.empty((P, 4), dtype=torch.int32, device=dev)
    inl = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    X = torch.empty((P, cap, 3), dtype=torch.float32, device=dev)
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    out = {'R': R, 't': t, 'good': good, 'inliers': inl, 'points3d': X, 'info': info}
    if P == 0 or cap == 0:                    # no correspondence at all: nothing found, every element written like the kernel writes it
        for v in (R, t, good, inl, info):
            v.zero_()
        info[:, 1] = -1
        X.fill_(float('nan'))
        return out
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn = lib.xfh_recover_pose if index is None else lib.xfh_recover_pose_matches
    for a, b in _chunks(P):
        _lib.check(fn(*_twoview.list_args(pts0, pts1, index, counts, n_const, a, b, cap), _ptr(K0[a:b]), _ptr(K1[a:b]), _ptr(E[a:b]),
                      _ptr(mask[a:b]) if mask is not None else None, thr, _ptr(R[a:b]), _ptr(t[a:b]), _ptr(good[a:b]), _ptr(inl[a:b]), _ptr(X[a:b]),
                      _ptr(info[a:b]), stream), who)
    return out


def recover_pose_batch(E, pts0, pts1, counts, K0, K1, distance_thresh=50.0, mask=None):
    """The pose of P essential matrices, chosen by the points: E (P,3,3) / (3,3) float64 at any scale or sign with x1' E x0 = 0 in
    calibrated coordinates; the other inputs as for triangulate_batch.  E = s [t]x R decomposes into (Ra, t) (Ra, -t) (Rb, t) (Rb, -t);
    every correspondence votes for the poses under which its depth is in (0, distance_thresh) in both cameras (the unit is |t| = 1;
    inf: in front of both is enough), the most votes win, ties go to the first.  Returns a dict of CUDA tensors: 'R' (P,3,3), 't' (P,3)
    unit float64, 'good' (P,4) int32 (the four counts), 'inliers' (P,cap) uint8 (mask and passes under the winner), 'points3d' (P,cap,3)
    float32 (the winner's points, NaN where 'inliers' is 0), 'info' (P,8) int32 (RECOVER_INFO_FIELDS).  An E that cannot be decomposed
    (not finite, zero) or that no correspondence votes for: found = 0 and zeros.  Asynchronous."""
    pts0, pts1, counts, dev = _twoview.check_points(_WHAT, pts0, pts1, counts)
    P, cap = pts0.shape[0], pts0.shape[1]
    return _recover("xfh_recover_pose", E, pts0, pts1, None, counts, cap, P, cap, K0, K1, distance_thresh, mask, dev)


def recover_pose_matches(E, kpts0, kpts1, idx0, idx1, n_matches, K0, K1, distance_thresh=50.0, mask=None):
    """recover_pose_batch straight on the matcher's output (the list arguments of triangulate_matches)."""
    dev, P, cap = _twoview.check_matches("recover_pose_matches", kpts0, kpts1, idx0, idx1, n_matches)
    return _recover("xfh_recover_pose_matches", E, kpts0, kpts1, (idx0, idx1, kpts0.shape[1]), n_matches, 0, P, cap, K0, K1, distance_thresh,
                    mask, dev)


def recover_pose(E, points1, points2, cameraMatrix=None, distanceThresh=None, mask=None):
    """``cv2.recoverPose(E, points1, points2, cameraMatrix[, distanceThresh][, mask])``: returns (n, R (3,3), t (3,1), mask (N,1) uint8 with
    255 for the points in front of both cameras under the pose) as numpy arrays, and with ``distanceThresh`` also triangulatedPoints (4,N)
    float64 (w = 1; NaN columns for the rejected points).  cameraMatrix None is the identity (points already calibrated), as cv2's default;
    without distanceThresh cv2 uses 50, and so does this.  ``mask`` (N,) / (N,1): only its non-zero points vote.  NOT pinned against cv2,
    which is absent here: the decomposition and the vote are cv2's by its documentation, the points come from this module's optimal
    triangulation, so a point near a gate can differ.  No pose (found = 0): n = 0, zeros."""
    a, b = _twoview.as_points(points1), _twoview.as_points(points2)
    if a.shape != b.shape:
        raise RuntimeError('points1 and points2 must hold the same number of points')
    N = a.shape[0]
    K = np.eye(3) if cameraMatrix is None else np.asarray(cameraMatrix, np.float64).reshape(3, 3)
    E = np.asarray(E.cpu() if torch.is_tensor(E) else E, np.float64)
    if E.shape != (3, 3):
        raise RuntimeError('E must be (3,3)')
    dev = _twoview.device(_WHAT)
    m = None if mask is None else torch.as_tensor(np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)).reshape(1, -1)
    if m is not None and m.shape[1] != N:
        raise RuntimeError('mask must hold one entry per point')
    r = recover_pose_batch(E, a.to(dev).float()[None], b.to(dev).float()[None], None, K, K, 50.0 if distanceThresh is None else distanceThresh, m)
    inl = r['inliers'][0].cpu().numpy()
    out = (int(r['info'][0, 3]), r['R'][0].cpu().numpy(), r['t'][0].cpu().numpy().reshape(3, 1), (inl * 255).astype(np.uint8).reshape(N, 1))
    if distanceThresh is None:
        return out
    X = r['points3d'][0].cpu().numpy().astype(np.float64)
    return out + (np.concatenate([X.T, np.where(inl[None, :] != 0, 1.0, np.nan)], axis=0),)


def essential_from_fundamental(F, K0, K1):
    """E = K1' F K0 (float64 numpy, (3,3) or (P,3,3)) of a fundamental matrix with p1' F p0 = 0 in pixels (``find_fundamental_mat``'s) and
    the two PINHOLE intrinsics: the counterpart of ``guided.fundamental_from_pose``.  A zero F (no model) gives a zero E."""
    as64 = lambda v: np.asarray(v.cpu() if torch.is_tensor(v) else v, np.float64)      # noqa: E731
    F, K0, K1 = as64(F), as64(K0), as64(K1)
    return np.swapaxes(K1, -1, -2) @ F @ K0
