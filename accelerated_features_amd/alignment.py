"""3D-3D alignment on MI355X: the similarity (or rigid) transform between two sets of corresponding 3D points,

    B ~= s R A + t,    R a proper rotation, s > 0    (with_scale=False: s = 1)

-- the metric relative pose of an RGB-D pair (``estimate_relative_pose_rgbd_matches``: both key-point sets lifted through their depth
maps, no essential matrix and none of its degeneracies), the scale between two reconstructions triangulated under baselines of their own,
the registration of a reconstruction to a metric frame.  ``estimate_alignment_batch`` takes P gathered point lists resident in HBM,
``estimate_alignment_matches`` works straight on index lists into two point tables (``unproject_keypoints``' output, the triangulation's
scattered ``points3d_ref``), NaN rows meaning "no point".  The kernels behind ``xfh_estimate_alignment`` (include/xfeat_hip.h,
csrc/k_align.hip) build and score every hypothesis at once and apply RANSAC's stopping rule to the cost list afterwards;
the consensus set is refitted in closed form (Horn's quaternion method).  There is no CPU path: without the HIP library and a gfx950
device the estimators raise.
"""
import math

import torch

from . import _lib, _twoview
from ._twoview import WORKSPACE_LIMIT, chunk_seed, ptr as _ptr      # chunk_seed is public here: chunk_seed(seed, p) = the seed of pair p alone
from .absolute_pose import unproject_keypoints

INFO_FIELDS = ("found", "best_it", "iters", "n_inliers", "lo_accepted", "n", "cost_lo", "cost_hi")
MAX_ITERATIONS = 16384                       # the kernel's limit; more is an error
_WHAT = "3D-3D alignment"


def _run(who, pts_a, pts_b, index, counts, n_const, P, cap, max_error, with_scale, success_prob, min_iterations, max_iterations, seed, dev):
    """Shared driver: outputs, chunks of pairs under WORKSPACE_LIMIT, one library call per chunk.  index = (idx_a, idx_b) or None."""
    if not 1 <= int(max_iterations) <= MAX_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: max_iterations {max_iterations} outside [1, {MAX_ITERATIONS}]")
    if not (float(max_error) > 0.0 and math.isfinite(float(max_error))):
        raise _lib.XFeatHipError(f"{who}: max_error {max_error} must be positive and finite")
    R = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((P, 3), dtype=torch.float64, device=dev)
    s = torch.empty((P,), dtype=torch.float64, device=dev)
    mask = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    info = torch.empty((P, 8), dtype=torch.int32, device=dev)
    out = {'R': R, 't': t, 's': s, 'inliers': mask, 'info': info}
    if P == 0 or cap == 0:                    # no correspondence at all: nothing found, every element written like the kernel writes it
        for v in (R, t, s, mask, info):
            v.zero_()
        info[:, 1] = -1
        return out
    lib = _lib.load()
    tail = (1 if with_scale else 0, float(max_error), int(min_iterations), int(max_iterations), float(success_prob))

    def call(a, b, *ws_and_stream):
        if index is None:
            head = (_ptr(pts_a[a:b]), _ptr(pts_b[a:b]), _ptr(counts[a:b]) if counts is not None else None, n_const, b - a, cap)
            fn = lib.xfh_estimate_alignment
        else:
            head = (_ptr(pts_a[a:b]), pts_a.shape[1], _ptr(pts_b[a:b]), pts_b.shape[1], _ptr(index[0][a:b]), _ptr(index[1][a:b]),
                    _ptr(counts[a:b]), b - a, cap)
            fn = lib.xfh_estimate_alignment_matches
        return fn(*head, *tail, chunk_seed(seed, a), _ptr(R[a:b]), _ptr(t[a:b]), _ptr(s[a:b]), _ptr(mask[a:b]), _ptr(info[a:b]), *ws_and_stream)

    _twoview.run_chunked(who, P, WORKSPACE_LIMIT, lambda n: lib.xfh_align_workspace_bytes(n, int(max_iterations)), dev, call)
    return out


def estimate_alignment_batch(pts_a, pts_b, counts, max_error, with_scale=True, success_prob=0.9999, min_iterations=20, max_iterations=1000,
                             seed=0):
    """P alignments B ~= s R A + t in one call (split internally into chunks of pairs whose workspace stays under 512 MiB).

    pts_a  : (P, cap, 3) float32 points
    pts_b  : (P, cap, 3) float32 points (row i of pts_a corresponds to row i of pts_b); NaN rows on either side mean "no point"
    counts : (P,) int32, pair p uses its first counts[p] rows; None = all cap rows
    max_error is a distance in B's unit; with_scale=False fixes s = 1 (the rigid case).
    Returns a dict of CUDA tensors: 'R' (P,3,3) float64 (a proper rotation), 't' (P,3) float64, 's' (P,) float64, 'inliers' (P,cap) uint8,
    'info' (P,8) int32 (INFO_FIELDS).  Nothing found: zeros.  Asynchronous."""
    pts_a, pts_b, counts, dev = _twoview.check_points_3d3d(_WHAT, pts_a, pts_b, counts)
    P, cap = pts_a.shape[0], pts_a.shape[1]
    return _run("xfh_estimate_alignment", pts_a, pts_b, None, counts, cap, P, cap, max_error, with_scale, success_prob, min_iterations,
                max_iterations, seed, dev)


def estimate_alignment_matches(points3d_a, points3d_b, idx_a, idx_b, n_matches, max_error, with_scale=True, success_prob=0.9999,
                               min_iterations=20, max_iterations=1000, seed=0):
    """The same estimator straight on index lists into two point tables: correspondence i of pair p is (points3d_a[p, idx_a[p, i]],
    points3d_b[p, idx_b[p, i]]) for i < n_matches[p].  points3d_a (P,Ka,3), points3d_b (P,Kb,3) float32 (for instance
    ``unproject_keypoints`` of both images' key-points, or the ``points3d_ref`` tables of two triangulations), idx (P,cap) int64,
    n_matches (P,) int32 CUDA tensors.  An index outside its table makes the correspondence "no point".  Same result dict as
    estimate_alignment_batch."""
    dev, P, cap = _twoview.check_matches_3d3d("estimate_alignment_matches", points3d_a, points3d_b, idx_a, idx_b, n_matches)
    return _run("xfh_estimate_alignment_matches", points3d_a, points3d_b, (idx_a, idx_b), n_matches, 0, P, cap, max_error, with_scale,
                success_prob, min_iterations, max_iterations, seed, dev)


def estimate_relative_pose_rgbd_matches(kpts0, depth0, K0, kpts1, depth1, K1, idx0, idx1, n_matches, max_error, success_prob=0.9999,
                                        min_iterations=20, max_iterations=1000, seed=0):
    """The metric relative pose of an RGB-D pair from the matcher's lists: both key-point sets are lifted through their depth maps
    (``unproject_keypoints``: kpts (P,K,2) float32 pixels, depth (P,H,W), K (P,3,3) or (3,3)) and the rigid transform between the two
    lifted tables is estimated, X1 = R X0 + t in the depth maps' unit; max_error is a distance in that unit.  Key-points without a valid
    depth are "no point" on their side.  Same result dict as estimate_alignment_batch ('s' is 1 where a pose was found)."""
    X0, _ = unproject_keypoints(kpts0, depth0, K0)
    X1, _ = unproject_keypoints(kpts1, depth1, K1)
    return estimate_alignment_matches(X0.contiguous(), X1.contiguous(), idx0, idx1, n_matches, max_error, False, success_prob, min_iterations,
                                      max_iterations, seed)


def apply_alignment(points, s, R, t):
    """s R X + t on a point table: points (P,N,3) with s (P,), R (P,3,3), t (P,3), or (N,3) with a scalar s, R (3,3), t (3,).  The result
    has the points' dtype; NaN rows stay NaN.  Plain tensor arithmetic on whatever device the inputs are on (no kernel of its own)."""
    points = torch.as_tensor(points)
    dev = points.device
    s, R, t = (torch.as_tensor(v, dtype=torch.float64).to(dev) for v in (s, R, t))
    if points.shape[-1] != 3 or R.shape[-2:] != (3, 3) or t.shape[-1] != 3 or R.shape[:-2] != t.shape[:-1] or s.shape != t.shape[:-1] \
            or points.dim() != R.dim() or (points.dim() == 3 and points.shape[0] != R.shape[0]):
        raise RuntimeError('expected points (P,N,3) with s (P,), R (P,3,3), t (P,3), or points (N,3) with a scalar s, R (3,3), t (3,)')
    Y = s[..., None, None] * (points.to(torch.float64) @ R.transpose(-1, -2)) + t[..., None, :]
    return Y.to(points.dtype if points.is_floating_point() else torch.float64)
