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

modules/eval/scannet1500.py estimates every pair at twelve RANSAC thresholds.  ``estimate_relative_pose_sweep_batch`` /
``estimate_relative_pose_sweep_matches`` do that in one pass (``xfh_estimate_relpose_sweep``): a hypothesis does not depend on the
threshold, so it is solved once and every Sampson error is evaluated once; slice j of the result is the single call at thresholds[j],
bit for bit.  ``estimate_pose``, ``pose_accuracy``, ``relative_transform`` and ``scannet_benchmark`` are that script's call shape,
metrics and loop.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, _twoview
from ._twoview import WORKSPACE_LIMIT, chunk_seed, intrinsics as _intrinsics, ptr as _ptr      # chunk_seed is public here: pose.chunk_seed(seed, p) = the seed of pair p alone

INFO_FIELDS = ("found", "best_it", "iters", "n_inliers", "lo_accepted", "n", "cost_lo", "cost_hi")
MAX_ITERATIONS = 16384                       # the kernel's limit; more is an error
MAX_THRESHOLDS = 16                          # of one sweep call; more is an error
SCANNET_THRESHOLDS = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0)   # 'ransac_thresholds' of modules/eval/scannet1500.py
_WHAT = "relative pose estimation"
RANSAC_DEFAULTS = {"max_epipolar_error": 1.0, "success_prob": 0.99999, "min_iterations": 20, "max_iterations": 10000}


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


def _run_sweep(who, pts0, pts1, index, counts, n_const, P, cap, K0, K1, thresholds, success_prob, min_iterations, max_iterations, seed, dev):
    """_run with a threshold axis after the pair axis: one library call per chunk of pairs runs all the thresholds."""
    K0, K1 = _intrinsics(K0, P, dev), _intrinsics(K1, P, dev)
    if not 1 <= int(max_iterations) <= MAX_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: max_iterations {max_iterations} outside [1, {MAX_ITERATIONS}]")
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    T = len(thr)
    if not 1 <= T <= MAX_THRESHOLDS:
        raise _lib.XFeatHipError(f"{who}: {T} thresholds outside [1, {MAX_THRESHOLDS}]")
    if not (np.isfinite(thr) & (thr > 0)).all():
        raise _lib.XFeatHipError(f"{who}: thresholds must be finite and positive, got {thr.tolist()}")
    R = torch.empty((P, T, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((P, T, 3), dtype=torch.float64, device=dev)
    E = torch.empty((P, T, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((P, T, cap), dtype=torch.uint8, device=dev)
    info = torch.empty((P, T, 8), dtype=torch.int32, device=dev)
    out = {'R': R, 't': t, 'E': E, 'inliers': mask, 'info': info}
    if P == 0 or cap == 0:                    # no correspondence at all: nothing found, every element written like the kernel writes it
        for v in (R, t, E, mask, info):
            v.zero_()
        info[:, :, 1] = -1
        return out
    lib = _lib.load()
    fn = lib.xfh_estimate_relpose_sweep if index is None else lib.xfh_estimate_relpose_sweep_matches
    thr_host = (C.c_double * T)(*thr.tolist())

    def call(a, b, *ws_and_stream):
        return fn(*_twoview.list_args(pts0, pts1, index, counts, n_const, a, b, cap), _ptr(K0[a:b]), _ptr(K1[a:b]), thr_host, T,
                  int(min_iterations), int(max_iterations), float(success_prob), chunk_seed(seed, a), _ptr(R[a:b]), _ptr(t[a:b]), _ptr(E[a:b]),
                  _ptr(mask[a:b]), _ptr(info[a:b]), *ws_and_stream)

    _twoview.run_chunked(who, P, WORKSPACE_LIMIT, lambda n: lib.xfh_relpose_sweep_workspace_bytes(n, int(max_iterations), T), dev, call)
    return out


def estimate_relative_pose_sweep_batch(pts0, pts1, counts, K0, K1, thresholds, success_prob=0.99999, min_iterations=20, max_iterations=1000,
                                       seed=0):
    """estimate_relative_pose_batch at every max_epipolar_error of `thresholds` (1 to 16 values in pixels, any order, repeats allowed) in
    one pass over the hypotheses.  Returns the same dict with a threshold axis after the pair axis: 'R' (P,T,3,3), 't' (P,T,3),
    'E' (P,T,3,3), 'inliers' (P,T,cap), 'info' (P,T,8); [:, j] equals estimate_relative_pose_batch(..., thresholds[j], same other
    arguments) bit for bit (the threshold does not enter the draws)."""
    pts0, pts1, counts, dev = _twoview.check_points(_WHAT, pts0, pts1, counts)
    P, cap = pts0.shape[0], pts0.shape[1]
    return _run_sweep("xfh_estimate_relpose_sweep", pts0, pts1, None, counts, cap, P, cap, K0, K1, thresholds, success_prob, min_iterations,
                      max_iterations, seed, dev)


def estimate_relative_pose_sweep_matches(kpts0, kpts1, idx0, idx1, n_matches, K0, K1, thresholds, success_prob=0.99999, min_iterations=20,
                                         max_iterations=1000, seed=0):
    """The sweep straight on the matcher's output (the arguments of estimate_relative_pose_matches, the result of
    estimate_relative_pose_sweep_batch)."""
    dev, P, cap = _twoview.check_matches("estimate_relative_pose_sweep_matches", kpts0, kpts1, idx0, idx1, n_matches)
    return _run_sweep("xfh_estimate_relpose_sweep_matches", kpts0, kpts1, (idx0, idx1, kpts0.shape[1]), n_matches, 0, P, cap, K0, K1,
                      thresholds, success_prob, min_iterations, max_iterations, seed, dev)


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


def estimate_pose(kpts0, kpts1, K0, K1, thresh, conf=0.99999, type='poselib', *, seed=0):
    """``estimate_pose(kpts0, kpts1, K0, K1, thresh, conf)`` of modules/eval/scannet1500.py: (R, t, inliers) at max_iterations 10000
    through estimate_relative_pose, or None (fewer than 5 points, no model).  K0, K1 are 3x3 intrinsics; type='opencv' is not offered."""
    if type != 'poselib':
        raise _lib.XFeatHipError(f"estimate_pose: type {type!r} is not supported (only 'poselib': the five-point estimator of this module)")
    cam = lambda K: {"model": "PINHOLE", "width": 0, "height": 0, "params": [K[0][0], K[1][1], K[0][2], K[1][2]]}   # noqa: E731
    pose, details = estimate_relative_pose(kpts0, kpts1, cam(np.asarray(K0)), cam(np.asarray(K1)),
                                           {"max_iterations": 10000, "success_prob": conf, "max_epipolar_error": thresh}, {}, seed=seed)
    return None if pose is None else (pose.R, pose.t, details["inliers"])


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


def pose_accuracy(errors, thresholds=(5, 10, 20)):
    """{threshold: percentage of the pairs whose error is below it}."""
    e = np.asarray(errors, np.float64)
    return {thr: float(np.mean(e < thr) * 100.0) for thr in thresholds}


def relative_transform(pose0, pose1):
    """T_0to1 (..., 3, 4) of two camera-to-world poses (..., 3|4, 4): X1 = R1' R0 X0 + R1' (t0 - t1)."""
    pose0, pose1 = np.asarray(pose0, np.float64), np.asarray(pose1, np.float64)
    R1t = np.swapaxes(pose1[..., :3, :3], -1, -2)
    return np.concatenate([R1t @ pose0[..., :3, :3], R1t @ (pose0[..., :3, 3:4] - pose1[..., :3, 3:4])], axis=-1)


def _match_and_pack(xfeat, pairs, scale0, scale1, star, top_k):
    """Match the pairs and pack the (rescaled) point lists: (m0, m1) lists of (n_p, 2) tensors, pts0, pts1 (P, cap, 2), counts (P,)."""
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
    return m0, m1, pts0, pts1, counts


def pose_benchmark(xfeat, pairs, K0, K1, T_0to1, scale0=None, scale1=None, ransac_thr=2.5, star=False, max_pairs=32, top_k=4096, seed=0):
    """The evaluation loop of modules/eval/megadepth1500.py on the device: ``batching.match_pairs`` (``match_pairs_star`` with star=True) on
    `pairs` (a list of (img0, img1)), key-points rescaled by scale0 / scale1 ((P,2) factors, points * scale), one batched pose call at
    max_epipolar_error = ransac_thr, errors against T_0to1.  Returns {"t_err", "R_err", "err" (max of the two, inf when no pose), "auc",
    "info", "R", "t", "inliers" (P, cap), "matches" (the rescaled point lists)}.  Pair p draws as pair p of a batch: the single-pair
    ``estimate_relative_pose`` with ``seed=chunk_seed(seed, p)`` makes the same draws."""
    pairs = list(pairs)[:max_pairs]
    P = len(pairs)
    m0, m1, pts0, pts1, counts = _match_and_pack(xfeat, pairs, scale0, scale1, star, top_k)
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


def scannet_benchmark(xfeat, pairs, K0, K1, T_0to1, ransac_thresholds=SCANNET_THRESHOLDS, pose_thresholds=(5, 10, 20), star=False, max_pairs=32,
                      top_k=4096, seed=0):
    """The evaluation loop of modules/eval/scannet1500.py (``Scannet1500.run_benchmark``) on the device: the pairs are matched once
    (as pose_benchmark matches them; ScanNet's key-points need no rescaling), ONE sweep call estimates every pair at every RANSAC threshold
    (RANSAC_DEFAULTS otherwise: 10000 iterations), and the errors against T_0to1 give an AUC and an accuracy per threshold.
    Returns {"aucs_by_thresh": {ransac threshold: {pose threshold: AUC x 100}}, "accs_by_thresh": {...: {...: percentage}}, "err" (P, T)
    (max of the translation and rotation error, inf when no pose), "info" (P,T,8), "R", "t", "inliers" (P,T,cap), "matches"}.  Column j
    equals pose_benchmark(..., ransac_thr=ransac_thresholds[j]) with the same seed."""
    pairs = list(pairs)[:max_pairs]
    P = len(pairs)
    thresholds = [float(v) for v in ransac_thresholds]
    m0, m1, pts0, pts1, counts = _match_and_pack(xfeat, pairs, None, None, star, top_k)
    r = estimate_relative_pose_sweep_batch(pts0, pts1, counts, np.asarray(K0)[:P], np.asarray(K1)[:P], thresholds, RANSAC_DEFAULTS["success_prob"],
                                           RANSAC_DEFAULTS["min_iterations"], RANSAC_DEFAULTS["max_iterations"], seed)
    info, R, t = r['info'].cpu().numpy(), r['R'].cpu().numpy(), r['t'].cpu().numpy()
    err = np.full((P, len(thresholds)), np.inf)
    for p in range(P):
        for j in range(len(thresholds)):
            if info[p, j, 0]:
                err[p, j] = max(relative_pose_error(np.asarray(T_0to1)[p], R[p, j], t[p, j]))
    aucs, accs = {}, {}
    for j, thr in enumerate(thresholds):
        auc = pose_auc(err[:, j], pose_thresholds)
        aucs[thr] = {k: 100.0 * auc[f"auc@{k}"] for k in pose_thresholds}
        accs[thr] = pose_accuracy(err[:, j], pose_thresholds)
    return {"aucs_by_thresh": aucs, "accs_by_thresh": accs, "err": err, "info": info, "R": R, "t": t, "inliers": r['inliers'].cpu().numpy(),
            "matches": (m0, m1)}
