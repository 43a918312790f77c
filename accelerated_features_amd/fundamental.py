"""Fundamental matrix from the matches on MI355X: match verification for uncalibrated, non-planar image pairs.

    F, mask = cv2.findFundamentalMat(points1, points2, cv2.USAC_MAGSAC, ransacReprojThreshold, confidence, maxIters)

``find_fundamental_mat`` has that call's parameter names and order and its results (F (3,3) float64 and an (N,1) uint8 mask, or
``(None, None)``); ``find_fundamental_batch`` is the same estimator over P point lists resident in HBM and ``find_fundamental_matches``
runs it straight on the matcher's index lists (``XFeat.match_pairs_device``), without leaving the device.  The kernels behind
``xfh_find_fundamental`` (include/xfeat_hip.h, csrc/k_fundamental.hip) build and score every hypothesis at once and apply RANSAC's
stopping rule to the score list afterwards.  OpenCV is not a dependency: the estimator is the published one (7-point RANSAC with the
oriented epipolar constraint, the MAGSAC++ quality and sigma-consensus++ refinement), so F agrees with cv2's as an estimate of the same
epipolar geometry, not in its random stream; parity with cv2 is not pinned.  A planar scene (or a pure rotation) does not determine F:
use ``homography.find_homography`` there.  There is no CPU path: without the HIP library and a gfx950 device these functions raise.
"""
import torch

from . import _lib, _twoview
from ._twoview import WORKSPACE_LIMIT, ptr as _ptr

FM_7POINT = 1             # cv2.FM_7POINT: exactly 7 points, every real solution (up to 3, stacked)
FM_8POINT = 2             # cv2.FM_8POINT: one least-squares fit on all points (at least 8)
USAC_MAGSAC = 38          # cv2.USAC_MAGSAC: the robust estimator, and this module's default method
METHODS = (FM_7POINT, FM_8POINT, USAC_MAGSAC)
INFO_FIELDS = ("found", "best_it", "iters", "n_inliers", "lo_accepted", "n", "score_lo", "score_hi")
MAX_ITERATIONS = 16384                       # the kernel's limit; more is an error
_WHAT = "fundamental matrix estimation"


def _check_method(who, method):
    if method not in METHODS:
        raise _lib.XFeatHipError(f"{who}: method {method} is not implemented (USAC_MAGSAC {USAC_MAGSAC}, FM_7POINT {FM_7POINT} and "
                                 f"FM_8POINT {FM_8POINT} are; FM_RANSAC / FM_LMEDS / other USAC flags are not)")


def _run(who, pts0, pts1, index, counts, n_const, P, cap, method, ransac_thr, max_iters, confidence, seed, dev):
    """Shared driver: outputs, chunks of pairs under WORKSPACE_LIMIT, one library call per chunk.  index = (idx0, idx1, kcap) or None."""
    _check_method(who, method)
    if not 1 <= int(max_iters) <= MAX_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: max_iters {max_iters} outside [1, {MAX_ITERATIONS}]")
    F = torch.empty((P, 3, 9), dtype=torch.float64, device=dev)
    mask = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    if P == 0 or cap == 0:                    # no correspondence at all: nothing found, every element written like the kernel writes it
        for v in (F, mask, info):
            v.zero_()
        info[:, 1] = -1
    else:
        lib = _lib.load()
        iters = int(max_iters) if method == USAC_MAGSAC else 1
        fn = lib.xfh_find_fundamental if index is None else lib.xfh_find_fundamental_matches

        def call(a, b, *ws_and_stream):
            return fn(*_twoview.list_args(pts0, pts1, index, counts, n_const, a, b, cap), int(method), float(ransac_thr), iters, float(confidence),
                      _twoview.chunk_seed(seed, a), _ptr(F[a:b]), _ptr(mask[a:b]), _ptr(info[a:b]), *ws_and_stream)

        _twoview.run_chunked(who, P, WORKSPACE_LIMIT, lambda n: lib.xfh_fundamental_workspace_bytes(n, iters), dev, call)
    return {'F': (F.view(P, 3, 3, 3) if method == FM_7POINT else F[:, 0].view(P, 3, 3)), 'inliers': mask, 'info': info}


def find_fundamental_batch(pts0, pts1, counts=None, ransac_thr=3.0, max_iters=1000, confidence=0.99, seed=0, method=USAC_MAGSAC):
    """P fundamental matrices in one call (split internally into chunks of pairs whose workspace stays under 512 MiB; the draws are those
    of the whole batch).

    pts0, pts1 : (P, cap, 2) float32 pixel coordinates (row i of pts0 matches row i of pts1; x1' F x0 = 0)
    counts     : (P,) int32, pair p uses its first counts[p] rows; None = all cap rows
    ransac_thr is in pixels (Sampson error); max_iters <= 16384.
    Returns a dict of CUDA tensors: 'F' (P,3,3) float64 ((P,3,3,3) for FM_7POINT: up to 3 solutions, zeros beyond info 'iters'),
    'inliers' (P,cap) uint8, 'info' (P,8) int32 (INFO_FIELDS; for FM_7POINT / FM_8POINT 'iters' holds the number of models).
    F is scaled to F[2,2] = 1 (unit Frobenius norm when |F[2,2]| <= FLT_EPSILON) and is zero where nothing was found.  Asynchronous."""
    pts0, pts1, counts, dev = _twoview.check_points(_WHAT, pts0, pts1, counts)
    P, cap = pts0.shape[0], pts0.shape[1]
    return _run("xfh_find_fundamental", pts0, pts1, None, counts, cap, P, cap, method, ransac_thr, max_iters, confidence, seed, dev)


def find_fundamental_matches(kpts0, kpts1, idx0, idx1, n_matches, ransac_thr=3.0, max_iters=1000, confidence=0.99, seed=0,
                             method=USAC_MAGSAC):
    """The same estimator straight on the matcher's output: correspondence i of pair p is (kpts0[p, idx0[p, i]], kpts1[p, idx1[p, i]])
    for i < n_matches[p].  kpts (P,K,2) float32, idx (P,cap) int64, n_matches (P,) int32 CUDA tensors, as ``XFeat._detect_device`` and
    ``XFeat.match_pairs_device`` return them.  Same result dict as find_fundamental_batch."""
    dev, P, cap = _twoview.check_matches("find_fundamental_matches", kpts0, kpts1, idx0, idx1, n_matches)
    return _run("xfh_find_fundamental_matches", kpts0, kpts1, (idx0, idx1, kpts0.shape[1]), n_matches, 0, P, cap, method, ransac_thr,
                max_iters, confidence, seed, dev)


def find_fundamental_mat(points1, points2, method=USAC_MAGSAC, ransacReprojThreshold=3.0, confidence=0.99, maxIters=1000, mask=None, *,
                         seed=0, return_info=False):
    """``cv2.findFundamentalMat(points1, points2, method, ransacReprojThreshold, confidence, maxIters)`` for one pair: cv2's parameter
    names and order (``mask`` is cv2's optional output argument: accepted and ignored).  The default method is USAC_MAGSAC, not cv2's
    FM_RANSAC, as ``find_homography`` defaults to the method it implements; FM_7POINT and FM_8POINT are supported, FM_RANSAC, FM_LMEDS
    and the other USAC flags raise XFeatHipError.  OpenCV is not used: this is an estimate of the same F, not cv2's random stream.

    points1, points2 : (N,2) or (N,1,2) arrays / tensors (numpy, CPU or CUDA torch), any float type; x2' F x1 = 0
    Returns (F, mask): F (3,3) float64 numpy array ((3k,3) for FM_7POINT: the k solutions stacked, like cv2), mask (N,1) uint8 -- or
    (None, None) like cv2 when too few points are given or no model is found.  ``seed`` fixes the sample sequence (same arguments, same
    bits).  A planar scene does not determine F: use ``find_homography`` for it."""
    _check_method("find_fundamental_mat", method)
    dev = _twoview.device(_WHAT)
    a, b = _twoview.as_points(points1), _twoview.as_points(points2)
    if a.shape != b.shape:
        raise RuntimeError('points1 and points2 must hold the same number of points')
    n = a.shape[0]
    if n < 7 or (method == FM_8POINT and n < 8) or (method == FM_7POINT and n != 7):
        return (None, None, dict.fromkeys(INFO_FIELDS, 0)) if return_info else (None, None)
    r = find_fundamental_batch(a.to(dev).float()[None], b.to(dev).float()[None], None, ransacReprojThreshold, maxIters, confidence, seed,
                               method)
    info = dict(zip(INFO_FIELDS, r['info'][0].cpu().tolist()))
    if not info['found']:
        return (None, None, info) if return_info else (None, None)
    F = r['F'][0].cpu().numpy()
    if method == FM_7POINT:
        F = F[:info['iters']].reshape(-1, 3)
    out = (F, r['inliers'][0].cpu().numpy().reshape(-1, 1))
    return out + (info,) if return_info else out
