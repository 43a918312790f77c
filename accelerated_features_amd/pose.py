"""Relative camera pose from the matches on MI355X: the step after matching in the reference's evaluation.

    pose, details = poselib.estimate_relative_pose(kpts0, kpts1, cam0, cam1, ransac_opt, bundle_opt)   # modules/eval/megadepth1500.py

``estimate_relative_pose`` has that call's shape (PINHOLE camera dicts, the option dicts the evaluation passes, a pose with ``R`` / ``t``
and an info dict with ``inliers``); ``estimate_relative_pose_batch`` is the same estimator over P point lists resident in HBM and
``estimate_relative_pose_matches`` runs it straight on the matcher's index lists.  The kernels behind ``xfh_estimate_relpose``
(include/xfeat_hip.h, csrc/k_relpose.hip) build and score every hypothesis at once and apply RANSAC's stopping rule to the cost list
afterwards.  poselib is not a dependency and its source is not available here: the estimator is the published one (five-point essential
RANSAC, MSAC on the Sampson error, Gauss-Newton refinement), so the pose agrees with poselib's as an estimate of the same motion, not in
its random stream.  ``relative_pose_error``, ``pose_auc`` and ``pose_benchmark`` are the evaluation's metrics, written from their
definitions.  There is no CPU path: without the HIP library and a gfx950 device the estimators raise.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, _twoview
from ._twoview import chunk_seed, ptr as _ptr           # chunk_seed is public here: pose.chunk_seed(seed, p) = the seed of pair p alone

INFO_FIELDS = ("found", "best_it", "iters", "n_inliers", "lo_accepted", "n", "cost_lo", "cost_hi")
MAX_ITERATIONS = 16384                       # the kernel's limit; more is an error
WORKSPACE_LIMIT = 512 << 20                  # bytes of workspace per library call: larger batches are split into chunks of pairs
_WHAT = "relative pose estimation"
RANSAC_DEFAULTS = {"max_epipolar_error": 1.0, "success_prob": 0.99999, "min_iterations": 20, "max_iterations": 10000}


def _intrinsics(K, P, dev):
    K = torch.as_tensor(K, dtype=torch.float64)
    if K.shape == (3, 3):
        K = K.expand(P, 3, 3)
    if K.shape != (P, 3, 3):
        raise RuntimeError('intrinsics must be (3,3) or (P,3,3)')
    return K.to(dev).contiguous()


def _run(who, pts0, pts1, index, counts, n_const, P, cap, K0, K1, max_epipolar_error, success_prob, min_iterations, max_iterations, seed, dev):
    """Shared driver: outputs, chunks of pairs under WORKSPACE_LIMIT, one library call per chunk.  index = (idx0, idx1, kcap) or None."""
    K0, K1 = _intrinsics(K0, P, dev), _intrinsics(K1, P, dev)
    if not 1 <= int(max_iterations) <= MAX_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: max_iterations {max_iterations} outside [1, {MAX_ITERATIONS}]")
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((P, 3), dtype=torch.float64, device=dev)
    E = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    out = {'R': R, 't': t, 'E': E, 'inliers': mask, 'info': info}
    if P == 0 or cap == 0:                    # no correspondence at all: nothing found, every element written like the kernel writes it
        for v in (R, t, E, mask, info):
            v.zero_()
        info[:, 1] = -1
        return out
    lib = _lib.load()
    fn = lib.xfh_estimate_relpose if index is None else lib.xfh_estimate_relpose_matches

    def call(a, b, *ws_and_stream):
        return fn(*_twoview.list_args(pts0, pts1, index, counts, n_const, a, b, cap), _ptr(K0[a:b]), _ptr(K1[a:b]), float(max_epipolar_error),
                  int(min_iterations), int(max_iterations), float(success_prob), chunk_seed(seed, a), _ptr(R[a:b]), _ptr(t[a:b]), _ptr(E[a:b]),
                  _ptr(mask[a:b]), _ptr(info[a:b]), *ws_and_stream)

    _twoview.run_chunked(who, P, WORKSPACE_LIMIT, lambda n: lib.xfh_relpose_workspace_bytes(n, int(max_iterations)), dev, call)
    return out


def estimate_relative_pose_batch(pts0, pts1, counts, K0, K1, max_epipolar_error=1.0, success_prob=0.99999, min_iterations=20,
                                 max_iterations=1000, seed=0):
    """P relative poses in one call (split internally into chunks of pairs whose workspace stays under 512 MiB).

    pts0, pts1 : (P, cap, 2) float32 pixel coordinates (row i of pts0 matches row i of pts1)
    counts     : (P,) int32, pair p uses its first counts[p] rows; None = all cap rows
    K0, K1     : (P, 3, 3) or (3, 3) float64 PINHOLE intrinsics of the two cameras
    max_epipolar_error is in pixels (Sampson error; converted with the mean focal length of the two cameras).
    Returns a dict of CUDA tensors: 'R' (P,3,3) float64, 't' (P,3) unit, 'E' (P,3,3) = [t]x R, 'inliers' (P,cap) uint8, 'info' (P,8) int32
    (INFO_FIELDS).  x1 in camera 0 maps to camera 1 as X1 = R X0 + t.  Asynchronous."""
    pts0, pts1, counts, dev = _twoview.check_points(_WHAT, pts0, pts1, counts)
    P, cap = pts0.shape[0], pts0.shape[1]
    return _run("xfh_estimate_relpose", pts0, pts1, None, counts, cap, P, cap, K0, K1, max_epipolar_error, success_prob, min_iterations,
                max_iterations, seed, dev)


def estimate_relative_pose_matches(kpts0, kpts1, idx0, idx1, n_matches, K0, K1, max_epipolar_error=1.0, success_prob=0.99999,
                                   min_iterations=20, max_iterations=1000, seed=0):
    """The same estimator straight on the matcher's output: correspondence i of pair p is (kpts0[p, idx0[p, i]], kpts1[p, idx1[p, i]])
    for i < n_matches[p].  kpts (P,K,2) float32, idx (P,cap) int64, n_matches (P,) int32 CUDA tensors, as ``XFeat._detect_device`` and
    ``XFeat.match_pairs_device`` return them.  Same result dict as estimate_relative_pose_batch."""
    dev, P, cap = _twoview.check_matches("estimate_relative_pose_matches", kpts0, kpts1, idx0, idx1, n_matches)
    return _run("xfh_estimate_relpose_matches", kpts0, kpts1, (idx0, idx1, kpts0.shape[1]), n_matches, 0, P, cap, K0, K1,
                max_epipolar_error, success_prob, min_iterations, max_iterations, seed, dev)


def _camera_K(cam):
    if not isinstance(cam, dict) or cam.get("model") != "PINHOLE":
        raise _lib.XFeatHipError(f"estimate_relative_pose: only PINHOLE cameras are supported, got {cam!r}")
    fx, fy, cx, cy = (float(v) for v in cam["params"])
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def estimate_relative_pose(kpts0, kpts1, camera0, camera1, ransac_opt=None, bundle_opt=None, *, seed=0):
    """``poselib.estimate_relative_pose(kpts0, kpts1, camera0, camera1, ransac_opt, bundle_opt)`` as the reference's evaluation calls it
    (modules/eval/megadepth1500.py, scannet1500.py).

    camera dicts {"model": "PINHOLE", "width", "height", "params": [fx, fy, cx, cy]}; ransac_opt keys max_epipolar_error (1.0),
    success_prob (0.99999), min_iterations (20), max_iterations (10000 -- poselib's default is 100000; this estimator stops at 16384);
    bundle_opt must be None or {} (what the evaluation passes: the refinement is the estimator's own).
    Returns (pose, info): pose.R (3,3), pose.t (3,) float64 numpy arrays (X1 = R X0 + t, |t| = 1), info {"inliers": list of bool,
    "num_inliers", "iterations", "refinements"}; pose is None when fewer than 5 points are given or no model is found."""
    opt = dict(RANSAC_DEFAULTS)
    for k, v in (ransac_opt or {}).items():
        if k not in opt:
            raise _lib.XFeatHipError(f"estimate_relative_pose: unknown ransac option {k!r} (known: {sorted(opt)})")
        opt[k] = v
    if bundle_opt not in (None, {}):
        raise _lib.XFeatHipError("estimate_relative_pose: bundle options are not supported (the evaluation passes {})")
    K0, K1 = _camera_K(camera0), _camera_K(camera1)
    a, b = _twoview.as_points(kpts0), _twoview.as_points(kpts1)
    if a.shape != b.shape:
        raise RuntimeError('kpts0 and kpts1 must hold the same number of points')
    n = a.shape[0]
    if n < 5:
        return None, {"inliers": [False] * n, "num_inliers": 0, "iterations": 0, "refinements": 0}
    dev = _twoview.device(_WHAT)
    r = estimate_relative_pose_batch(a.to(dev).float()[None], b.to(dev).float()[None], None, K0, K1, opt["max_epipolar_error"],
                                     opt["success_prob"], opt["min_iterations"], opt["max_iterations"], seed)
    info = r['info'][0].cpu().tolist()
    details = {"inliers": [bool(v) for v in r['inliers'][0].cpu().tolist()], "num_inliers": info[3] if info[0] else 0,
               "iterations": info[2], "refinements": info[4]}
    if not info[0]:
        return None, details
    return SimpleNamespace(R=r['R'][0].cpu().numpy(), t=r['t'][0].cpu().numpy()), details


# ---- evaluation metrics ------------------------------------------------------------------------------------------------------------------
def relative_pose_error(T_0to1, R, t, ignore_gt_t_thr=0.0):
    """(t_err, R_err) in degrees.  t_err: angle between the estimated and the true translation direction, folded by min(e, 180 - e)
    (the direction's sign is not observable); 0 when |t_gt| < ignore_gt_t_thr.  R_err: rotation angle of R_gt' R from its trace."""
    T = np.asarray(T_0to1, np.float64)
    R_gt, t_gt = T[:3, :3], T[:3, 3]
    t = np.asarray(t, np.float64)
    n = np.linalg.norm(t) * np.linalg.norm(t_gt)
    c = np.clip(np.dot(t, t_gt) / n, -1.0, 1.0) if n > 0 else 1.0
    t_err = np.rad2deg(np.arccos(c))
    t_err = min(t_err, 180.0 - t_err)
    if np.linalg.norm(t_gt) < ignore_gt_t_thr:
        t_err = 0.0
    cr = np.clip((np.trace(R_gt.T @ np.asarray(R, np.float64)) - 1.0) / 2.0, -1.0, 1.0)
    return float(t_err), float(np.rad2deg(np.abs(np.arccos(cr))))


def pose_auc(errors, thresholds=(5, 10, 20)):
    """Area under the recall-vs-error curve up to each threshold, normalised by the threshold: the curve starts at (0, 0), steps to recall
    i/N at the i-th smallest error, and is closed with a point at the threshold (recall held)."""
    e = np.sort(np.asarray(errors, np.float64))
    recall = (np.arange(len(e)) + 1) / len(e)
    e = np.concatenate([[0.0], e])
    recall = np.concatenate([[0.0], recall])
    out = {}
    for thr in thresholds:
        last = np.searchsorted(e, thr)
        r = np.concatenate([recall[:last], [recall[last - 1]]])
        x = np.concatenate([e[:last], [thr]])
        out[f"auc@{thr}"] = float(np.sum((x[1:] - x[:-1]) * (r[1:] + r[:-1]) * 0.5) / thr)
    return out


def pose_benchmark(xfeat, pairs, K0, K1, T_0to1, scale0=None, scale1=None, ransac_thr=2.5, star=False, max_pairs=32, top_k=4096, seed=0):
    """The evaluation loop of modules/eval/megadepth1500.py on the device: ``batching.match_pairs`` (``match_pairs_star`` with star=True) on
    `pairs` (a list of (img0, img1)), key-points rescaled by scale0 / scale1 ((P,2) factors, points * scale), one batched pose call at
    max_epipolar_error = ransac_thr, errors against T_0to1.  Returns {"t_err", "R_err", "err" (max of the two, inf when no pose), "auc",
    "info", "R", "t", "inliers" (P, cap), "matches" (the rescaled point lists)}.  Pair p draws as pair p of a batch: the single-pair
    ``estimate_relative_pose`` with ``seed=chunk_seed(seed, p)`` makes the same draws."""
    pairs = list(pairs)[:max_pairs]
    P = len(pairs)
    from . import batching
    res = batching.match_pairs_star(xfeat, pairs) if star else batching.match_pairs(xfeat, pairs, top_k=top_k)
    m0 = [torch.as_tensor(np.asarray(r[0]) if not torch.is_tensor(r[0]) else r[0]).float().reshape(-1, 2) for r in res]
    m1 = [torch.as_tensor(np.asarray(r[1]) if not torch.is_tensor(r[1]) else r[1]).float().reshape(-1, 2) for r in res]
    for p in range(P):
        if scale0 is not None:
            m0[p] = m0[p].cpu() * torch.as_tensor(np.asarray(scale0[p], np.float32))
        if scale1 is not None:
            m1[p] = m1[p].cpu() * torch.as_tensor(np.asarray(scale1[p], np.float32))
    cap = max(1, max(len(m) for m in m0))
    pts0, pts1 = torch.zeros((P, cap, 2)), torch.zeros((P, cap, 2))
    counts = torch.zeros(P, dtype=torch.int32)
    for p in range(P):
        k = len(m0[p])
        pts0[p, :k], pts1[p, :k], counts[p] = m0[p].cpu(), m1[p].cpu(), k
    r = estimate_relative_pose_batch(pts0, pts1, counts, np.asarray(K0)[:P], np.asarray(K1)[:P], ransac_thr,
                                     RANSAC_DEFAULTS["success_prob"], RANSAC_DEFAULTS["min_iterations"], RANSAC_DEFAULTS["max_iterations"], seed)
    info, R, t = r['info'].cpu().numpy(), r['R'].cpu().numpy(), r['t'].cpu().numpy()
    t_err, R_err = np.full(P, np.inf), np.full(P, np.inf)
    for p in range(P):
        if info[p, 0]:
            t_err[p], R_err[p] = relative_pose_error(np.asarray(T_0to1)[p], R[p], t[p])
    err = np.maximum(t_err, R_err)
    return {"t_err": t_err, "R_err": R_err, "err": err, "auc": pose_auc(err), "info": info, "R": R, "t": t,
            "inliers": r['inliers'].cpu().numpy(), "matches": (m0, m1)}
