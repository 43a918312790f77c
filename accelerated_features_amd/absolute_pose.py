"""Absolute camera pose from 2D-3D correspondences on MI355X: localisation of a query image against 3D points.

    pose, info = poselib.estimate_absolute_pose(points2D, points3D, camera, ransac_opt, bundle_opt)     # what hloc runs for Aachen

``estimate_absolute_pose`` has that call's shape (a PINHOLE camera dict, the option dicts, a pose with ``R`` / ``t`` and an info dict with
``inliers``); ``estimate_absolute_pose_batch`` is the same estimator over P point lists resident in HBM and
``estimate_absolute_pose_matches`` runs it straight on the matcher's index lists, with the reference image's key-points lifted to 3D
(``unproject_keypoints``: the depth read at the rounded pixel, as modules/dataset/megadepth/megadepth_warper.py::warp_kpts reads it).
The kernels behind ``xfh_estimate_abspose`` (include/xfeat_hip.h, csrc/k_abspose.hip) build and score every hypothesis at once and
apply RANSAC's stopping rule to the cost list afterwards.  poselib is not a dependency and its source is not available here: the estimator
is the published one (P3P RANSAC, MSAC on the reprojection error, Gauss-Newton refinement), so the pose agrees with poselib's as an
estimate of the same camera, not in its random stream.  There is no CPU path: without the HIP library and a gfx950 device the estimators
raise.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, _twoview
from ._twoview import WORKSPACE_LIMIT, chunk_seed, intrinsics as _intrinsics, ptr as _ptr      # chunk_seed is public here: chunk_seed(seed, p) = the seed of pair p alone

INFO_FIELDS = ("found", "best_it", "iters", "n_inliers", "lo_accepted", "n", "cost_lo", "cost_hi")
MAX_ITERATIONS = 16384                       # the kernel's limit; more is an error
_WHAT = "absolute pose estimation"
RANSAC_DEFAULTS = {"max_reproj_error": 12.0, "success_prob": 0.9999, "min_iterations": 20, "max_iterations": 10000}


def _run(who, pts2d, pts3d, index, counts, n_const, P, cap, K, max_reproj_error, success_prob, min_iterations, max_iterations, seed, dev):
    """Shared driver: outputs, chunks of pairs under WORKSPACE_LIMIT, one library call per chunk.  index = (idx2d, idx3d) or None."""
    K = _intrinsics(K, P, dev)
    if not 1 <= int(max_iterations) <= MAX_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: max_iterations {max_iterations} outside [1, {MAX_ITERATIONS}]")
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((P, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    out = {'R': R, 't': t, 'inliers': mask, 'info': info}
    if P == 0 or cap == 0:                    # no correspondence at all: nothing found, every element written like the kernel writes it
        for v in (R, t, mask, info):
            v.zero_()
        info[:, 1] = -1
        return out
    lib = _lib.load()
    tail = (float(max_reproj_error), int(min_iterations), int(max_iterations), float(success_prob))

    def call(a, b, *ws_and_stream):
        if index is None:
            head = (_ptr(pts2d[a:b]), _ptr(pts3d[a:b]), _ptr(counts[a:b]) if counts is not None else None, n_const, b - a, cap)
            fn = lib.xfh_estimate_abspose
        else:
            head = (_ptr(pts2d[a:b]), pts2d.shape[1], _ptr(pts3d[a:b]), pts3d.shape[1], _ptr(index[0][a:b]), _ptr(index[1][a:b]),
                    _ptr(counts[a:b]), b - a, cap)
            fn = lib.xfh_estimate_abspose_matches
        return fn(*head, _ptr(K[a:b]), *tail, chunk_seed(seed, a), _ptr(R[a:b]), _ptr(t[a:b]), _ptr(mask[a:b]), _ptr(info[a:b]), *ws_and_stream)

    _twoview.run_chunked(who, P, WORKSPACE_LIMIT, lambda n: lib.xfh_abspose_workspace_bytes(n, int(max_iterations)), dev, call)
    return out


def estimate_absolute_pose_batch(pts2d, pts3d, counts, K, max_reproj_error=12.0, success_prob=0.9999, min_iterations=20, max_iterations=1000,
                                 seed=0):
    """P absolute poses in one call (split internally into chunks of pairs whose workspace stays under 512 MiB).

    pts2d  : (P, cap, 2) float32 pixel coordinates in the query image
    pts3d  : (P, cap, 3) float32 points in any world frame (row i of pts2d sees row i of pts3d)
    counts : (P,) int32, pair p uses its first counts[p] rows; None = all cap rows
    K      : (P, 3, 3) or (3, 3) float64 PINHOLE intrinsics of the query camera
    max_reproj_error is in pixels (converted with the camera's mean focal length).
    Returns a dict of CUDA tensors: 'R' (P,3,3) float64, 't' (P,3) float64 with X_cam = R X_world + t (t in the world's unit),
    'inliers' (P,cap) uint8, 'info' (P,8) int32 (INFO_FIELDS).  Rows with a coordinate that is not finite are never sampled into a model
    and never inliers.  Asynchronous."""
    pts2d, pts3d, counts, dev = _twoview.check_points_2d3d(_WHAT, pts2d, pts3d, counts)
    P, cap = pts2d.shape[0], pts2d.shape[1]
    return _run("xfh_estimate_abspose", pts2d, pts3d, None, counts, cap, P, cap, K, max_reproj_error, success_prob, min_iterations,
                max_iterations, seed, dev)


def estimate_absolute_pose_matches(kpts_query, points3d_ref, idx_query, idx_ref, n_matches, K, max_reproj_error=12.0, success_prob=0.9999,
                                   min_iterations=20, max_iterations=1000, seed=0):
    """The same estimator straight on the matcher's output: correspondence i of pair p is (kpts_query[p, idx_query[p, i]],
    points3d_ref[p, idx_ref[p, i]]) for i < n_matches[p].  kpts_query (P,K2,2) float32, points3d_ref (P,K3,3) float32 (for instance
    ``unproject_keypoints`` of the reference image's key-points), idx (P,cap) int64, n_matches (P,) int32 CUDA tensors, as
    ``XFeat._detect_device`` and ``XFeat.match_pairs_device`` / ``match_sets_device`` return them.  Same result dict as
    estimate_absolute_pose_batch."""
    dev, P, cap = _twoview.check_matches_2d3d("estimate_absolute_pose_matches", kpts_query, points3d_ref, idx_query, idx_ref, n_matches)
    return _run("xfh_estimate_abspose_matches", kpts_query, points3d_ref, (idx_query, idx_ref), n_matches, 0, P, cap, K, max_reproj_error,
                success_prob, min_iterations, max_iterations, seed, dev)


def _camera_K(cam):
    if not isinstance(cam, dict) or cam.get("model") != "PINHOLE":
        raise _lib.XFeatHipError(f"estimate_absolute_pose: only PINHOLE cameras are supported, got {cam!r}")
    fx, fy, cx, cy = (float(v) for v in cam["params"])
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def estimate_absolute_pose(points2D, points3D, camera, ransac_opt=None, bundle_opt=None, *, seed=0):
    """``poselib.estimate_absolute_pose(points2D, points3D, camera, ransac_opt, bundle_opt)``.

    camera dict {"model": "PINHOLE", "width", "height", "params": [fx, fy, cx, cy]}; ransac_opt keys max_reproj_error (12.0),
    success_prob (0.9999), min_iterations (20), max_iterations (10000 -- poselib's default is 100000; this estimator stops at 16384);
    bundle_opt must be None or {} (the refinement is the estimator's own).
    Returns (pose, info): pose.R (3,3), pose.t (3,) float64 numpy arrays (X_cam = R X_world + t), info {"inliers": list of bool,
    "num_inliers", "iterations", "refinements"}; pose is None when fewer than 3 points are given or no model is found."""
    opt = dict(RANSAC_DEFAULTS)
    for k, v in (ransac_opt or {}).items():
        if k not in opt:
            raise _lib.XFeatHipError(f"estimate_absolute_pose: unknown ransac option {k!r} (known: {sorted(opt)})")
        opt[k] = v
    if bundle_opt not in (None, {}):
        raise _lib.XFeatHipError("estimate_absolute_pose: bundle options are not supported")
    K = _camera_K(camera)
    a = _twoview.as_points(points2D)
    b = torch.as_tensor(np.asarray(points3D) if not torch.is_tensor(points3D) else points3D).reshape(-1, 3)
    if a.shape[0] != b.shape[0]:
        raise RuntimeError('points2D and points3D must hold the same number of points')
    n = a.shape[0]
    if n < 3:
        return None, {"inliers": [False] * n, "num_inliers": 0, "iterations": 0, "refinements": 0}
    dev = _twoview.device(_WHAT)
    r = estimate_absolute_pose_batch(a.to(dev).float()[None], b.to(dev).float()[None], None, K, opt["max_reproj_error"], opt["success_prob"],
                                     opt["min_iterations"], opt["max_iterations"], seed)
    info = r['info'][0].cpu().tolist()
    details = {"inliers": [bool(v) for v in r['inliers'][0].cpu().tolist()], "num_inliers": info[3] if info[0] else 0,
               "iterations": info[2], "refinements": info[4]}
    if not info[0]:
        return None, details
    return SimpleNamespace(R=r['R'][0].cpu().numpy(), t=r['t'][0].cpu().numpy()), details


def unproject_keypoints(kpts, depth, K, counts=None):
    """Key-points lifted through a depth map: X = depth[round(v), round(u)] K^-1 (u, v, 1), in the camera frame of the image the map
    belongs to -- the lift of modules/dataset/megadepth/megadepth_warper.py::warp_kpts (depth at the rounded pixel).

    kpts (B,N,2) float32 pixels (x, y), depth (B,H,W) float, K (B,3,3) or (3,3) PINHOLE intrinsics, counts (B,) or None: rows at or beyond
    counts[b] are invalid.  Returns (points3d (B,N,3) float32, valid (B,N) bool) on kpts' device.  A depth <= 0 or not finite, a pixel
    outside the map or a key-point that is not finite gives NaN coordinates and valid = False; the estimators never sample such a row
    into a model and never count it as an inlier, so the result can go into estimate_absolute_pose_matches as it is.  Plain tensor
    indexing on whatever device the inputs are on (no kernel of its own)."""
    kpts = torch.as_tensor(kpts)
    dev = kpts.device
    depth = torch.as_tensor(depth).to(dev)
    if kpts.dim() != 3 or kpts.shape[2] != 2 or depth.dim() != 3 or depth.shape[0] != kpts.shape[0]:
        raise RuntimeError('expected kpts (B,N,2) and depth (B,H,W)')
    B, N = kpts.shape[:2]
    H, W = depth.shape[1:]
    K = torch.as_tensor(K, dtype=torch.float64).to(dev)
    if K.shape == (3, 3):
        K = K.expand(B, 3, 3)
    if K.shape != (B, 3, 3):
        raise RuntimeError('intrinsics must be (3,3) or (B,3,3)')
    k64 = kpts.to(torch.float64)
    fin = torch.isfinite(k64).all(dim=2)
    px = torch.round(torch.where(fin[..., None], k64, torch.zeros_like(k64))).long()
    inside = fin & (px[..., 0] >= 0) & (px[..., 0] < W) & (px[..., 1] >= 0) & (px[..., 1] < H)
    if counts is not None:
        inside &= torch.arange(N, device=dev)[None, :] < torch.as_tensor(counts).to(dev)[:, None]
    flat = px[..., 1].clamp(0, H - 1) * W + px[..., 0].clamp(0, W - 1)
    d = torch.gather(depth.reshape(B, H * W).to(torch.float64), 1, flat)
    valid = inside & torch.isfinite(d) & (d > 0)
    x = (k64[..., 0] - K[:, None, 0, 2]) / K[:, None, 0, 0]
    y = (k64[..., 1] - K[:, None, 1, 2]) / K[:, None, 1, 1]
    X = torch.stack([x * d, y * d, d], dim=2)
    X = torch.where(valid[..., None], X, torch.full_like(X, float('nan')))
    return X.to(torch.float32), valid
