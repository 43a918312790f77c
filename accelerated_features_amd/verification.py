"""Geometric verification of match lists on MI355X: what stands between two-view geometry and the track graph.

``build_tracks_graph`` merges everything a match touches, so one wrong match joins two 3D points into one component, which then holds two
key-points of one view and is dropped whole.  A mutual-nearest-neighbour list carries tens of percent of wrong matches; given raw, it leaves
almost no track (DESIGN.md 3.22 has the measurements).  ``filter_matches_batch`` compacts match lists by a mask -- the inlier mask of the
homography, fundamental, relative-pose or absolute-pose estimator, or the one of ``verify_matches_graph`` -- keeping their order, and
``verify_matches_graph`` tests every match of a pair graph against the epipolar geometry of the world poses of its two views: for a pair
whose own RANSAC failed but whose views are registered, and for a new selection under bundle-adjusted poses.
``reconstruct_graph_matches(verified=True)`` compacts the lists with the relative poses' inlier masks before anything else reads them.
The kernels behind ``xfh_filter_matches`` / ``xfh_verify_matches`` (include/xfeat_hip.h, csrc/k_matchfilter.hip, csrc/k_triangulate.hip) are
specified in DESIGN.md 3.22.  There is no CPU path: without the HIP library and a gfx950 device the functions raise.
"""
import ctypes as C
import math

import torch

from . import _lib, _scenes
from ._scenes import MAX_SCENES, MAX_VIEWS      # noqa: F401 (public here)
from ._twoview import ptr as _ptr

FILTER_INFO_FIELDS = ("read", "set", "emptied", "spare")
EMPTIED = ("no", "keep", "min_keep")                       # filter info[..., 2]
VERIFY_INFO_FIELDS = ("status", "read", "kept", "spare")
VERIFY_STATUS = ("ok", "illegal_pair", "pose_not_usable", "zero_baseline")       # verify info[..., 0]
MAX_PAIRS = 65535
MAX_LISTS = (1 << 31) - 1                    # of one xfh_filter_matches call; larger batches are split into chunks of lists
MAX_CAP = 1 << 24


def filter_matches_batch(idx_a, idx_b, n_matches, mask, keep=None, min_keep=0):
    """Match lists compacted by a mask, their order kept.

    idx_a, idx_b : (P, cap) or (S, P, cap) int64 CUDA tensors;  n_matches (P,) / (S, P) int32, read clamped to [0, cap]
    mask         : (P, cap) / (S, P, cap) uint8 or bool: non-zero keeps entry i < n_matches (the 'inliers' of any estimator of this package,
                   the mask of ``verify_matches_graph``)
    keep         : (P,) / (S, P) uint8 or bool, or None: zero empties the list;  min_keep >= 0: a list that keeps fewer entries is emptied
    Returns (idx_a, idx_b, n_matches, src, info) in the input's shape: the kept entries first, in their original order, then -1; src int32
    = the original position of each kept entry, then -1 (gather scores, refined coordinates or a second mask with it); info (..., 4) int32:
    FILTER_INFO_FIELDS = entries read, entries whose mask is set, the reason the list was emptied (EMPTIED), 0.  Two calls give the same
    bytes.  Asynchronous: nothing synchronises with the host."""
    who = "filter_matches_batch"
    _scenes.tensors(who, idx_a, idx_b, n_matches, mask)
    if idx_a.dim() not in (2, 3) or idx_b.shape != idx_a.shape or mask.shape != idx_a.shape or n_matches.shape != idx_a.shape[:-1]:
        raise RuntimeError('expected idx_a, idx_b, mask (P,cap) or (S,P,cap) and n_matches (P,) or (S,P)')
    if keep is not None:
        _scenes.tensors(who, keep)
        if keep.shape != n_matches.shape:
            raise RuntimeError('keep must have one entry per list')
    if isinstance(min_keep, bool) or int(min_keep) != min_keep or int(min_keep) < 0:
        raise _lib.XFeatHipError(f"{who}: min_keep {min_keep} must be an integer >= 0")
    lead, cap = tuple(idx_a.shape[:-1]), idx_a.shape[-1]
    if cap > MAX_CAP:
        raise _lib.XFeatHipError(f"{who}: cap {cap} above {MAX_CAP}")
    L = math.prod(lead)
    empty = L == 0 or cap == 0
    if not idx_a.is_cuda and not empty:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    dev = idx_a.device
    for t, dts, name in ((idx_a, (torch.int64,), 'idx_a'), (idx_b, (torch.int64,), 'idx_b'), (n_matches, (torch.int32,), 'n_matches'),
                         (mask, (torch.uint8, torch.bool), 'mask'), (keep, (torch.uint8, torch.bool), 'keep')):
        if t is not None and (t.dtype not in dts or t.device != dev):
            raise RuntimeError(f'{who}: {name} must be a {" or ".join(str(d) for d in dts)} tensor on the device of idx_a')
    out_a = torch.empty(lead + (cap,), dtype=torch.int64, device=dev)
    out_b = torch.empty(lead + (cap,), dtype=torch.int64, device=dev)
    src = torch.empty(lead + (cap,), dtype=torch.int32, device=dev)
    n_out = torch.empty(lead, dtype=torch.int32, device=dev)
    info = torch.empty(lead + (4,), dtype=torch.int32, device=dev)
    if empty:                                 # no entry: nothing is read, nothing is kept
        n_out.zero_(); info.zero_()
        if L and keep is not None:
            info[..., 2] = (keep == 0).to(torch.int32)
        if L and int(min_keep) > 0:
            info[..., 2] = torch.where(info[..., 2] == 0, torch.full_like(info[..., 2], 2), info[..., 2])
        return out_a, out_b, n_out, src, info
    ia, ib, nm = idx_a.contiguous().view(L, cap), idx_b.contiguous().view(L, cap), n_matches.contiguous().view(L)
    mk = mask.contiguous().view(L, cap).view(torch.uint8)           # (a bool tensor holds 0 / 1 bytes)
    kp = keep.contiguous().view(L).view(torch.uint8) if keep is not None else None
    oa, ob, sr, no, inf = out_a.view(L, cap), out_b.view(L, cap), src.view(L, cap), n_out.view(L), info.view(L, 4)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for a in range(0, L, MAX_LISTS):
        b = min(L, a + MAX_LISTS)
        _lib.check(lib.xfh_filter_matches(_ptr(ia[a:b]), _ptr(ib[a:b]), _ptr(nm[a:b]), _ptr(mk[a:b]), _ptr(kp[a:b]) if kp is not None else None, b - a, cap,
                                          int(min_keep), _ptr(oa[a:b]), _ptr(ob[a:b]), _ptr(sr[a:b]), _ptr(no[a:b]), _ptr(inf[a:b]), stream),
                   "xfh_filter_matches")
    return out_a, out_b, n_out, src, info


def verify_matches_graph(kpts, view_pairs, idx_a, idx_b, n_matches, n_views, Ks, Rs, ts, max_epipolar_error=1.0):
    """The epipolar test of every match of a pair graph under the world poses of the views.

    kpts (S,V,K,2) float32, view_pairs (S,P,2) or (P,2) int32, idx_a / idx_b (S,P,cap) int64, n_matches (S,P) int32 CUDA tensors as for
    ``build_tracks_graph``; n_views (S,) int32 or None = all V <= 32; Ks, Rs (S,V,3,3), ts (S,V,3) float64 with x_v = R_v X + t_v (what
    ``average_poses_batch`` / ``bundle_adjust_batch`` return); max_epipolar_error in pixels, positive and finite.
    Per pair (a, b): status (VERIFY_STATUS) 1 when a == b or a view is outside [0, n_views), 2 when a pose is not usable (an entry that is
    not finite, an all-zero R: the NaN pose of a view that the pose graph did not register), 3 when t_rel is zero (exactly, as the triangulation has it); otherwise
    E = [t_rel]x R_rel of the pair and the threshold max_epipolar_error over the mean of the four focal lengths, as
    ``estimate_relative_pose_matches`` has it.  A match whose rows are in [0, K) and whose pixels are finite is evaluated: mask = its Sampson
    error (float64, normalised coordinates) is finite and below the threshold (strictly).  No cheirality test: the triangulation has its gates.
    Returns (mask (S,P,cap) uint8, 0 wherever nothing was evaluated;  err (S,P,cap) float32, the Sampson error in pixels, NaN wherever
    nothing was evaluated;  info (S,P,4) int32: VERIFY_INFO_FIELDS = status, entries read, entries kept, 0).  Asynchronous."""
    who = "verify_matches_graph"
    _scenes.tensors(who, kpts, view_pairs, idx_a, idx_b, n_matches)
    if kpts.dim() != 4 or kpts.shape[3] != 2:
        raise RuntimeError('expected kpts (S,V,K,2)')
    S, V, K = kpts.shape[:3]
    _scenes.views(who, V)
    if idx_a.dim() != 3 or idx_a.shape[0] != S or idx_b.shape != idx_a.shape or n_matches.shape != idx_a.shape[:2]:
        raise RuntimeError('expected idx_a, idx_b (S,P,cap) and n_matches (S,P) for kpts (S,V,K,2)')
    P, cap = idx_a.shape[1:]
    _scenes.check_view_pairs(view_pairs, S, P)
    if P > MAX_PAIRS:
        raise _lib.XFeatHipError(f"{who}: {P} pairs, more than {MAX_PAIRS}")
    if cap > MAX_CAP or K > MAX_CAP:
        raise _lib.XFeatHipError(f"{who}: cap {cap} or K {K} above {MAX_CAP}")
    thr = float(max_epipolar_error)
    if not thr > 0.0 or math.isinf(thr):
        raise _lib.XFeatHipError(f"{who}: max_epipolar_error {thr} must be positive and finite")
    empty = S == 0 or P == 0 or cap == 0 or K == 0
    if not kpts.is_cuda and not empty:
        raise _lib.XFeatHipError(f"{who} works on device-resident key-points and match lists")
    dev = kpts.device
    for t, dt, name in ((kpts, torch.float32, 'kpts'), (idx_a, torch.int64, 'idx_a'), (idx_b, torch.int64, 'idx_b'), (n_matches, torch.int32, 'n_matches')):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f'{who}: {name} must be a contiguous {dt} tensor on the device of kpts')
    n_views = _scenes.n_views_arg(n_views, S, dev)
    Ks, Rs, ts = _scenes.f64(Ks, (S, V, 3, 3), dev, 'Ks'), _scenes.f64(Rs, (S, V, 3, 3), dev, 'Rs'), _scenes.f64(ts, (S, V, 3), dev, 'ts')
    view_pairs = _scenes.view_pairs_arg(view_pairs, S, P, dev)
    mask = torch.empty((S, P, cap), dtype=torch.uint8, device=dev)
    err = torch.empty((S, P, cap), dtype=torch.float32, device=dev)
    info = torch.empty((S, P, 4), dtype=torch.int32, device=dev)
    if empty:                                 # no entry, or no key-point row: nothing is evaluated (the statuses are not worked out)
        mask.zero_(); err.fill_(float('nan')); info.zero_()
        info[..., 1] = n_matches.clamp(0, cap)
        return mask, err, info
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    step = min(MAX_SCENES, MAX_LISTS // P)    # chunks of at most 65535 scenes whose pairs one launch holds
    for c in range(0, S, step):
        d = min(S, c + step)
        _lib.check(lib.xfh_verify_matches(_ptr(kpts[c:d]), _ptr(view_pairs[c:d]), _ptr(idx_a[c:d]), _ptr(idx_b[c:d]), _ptr(n_matches[c:d]),
                                          _ptr(n_views[c:d]) if n_views is not None else None, d - c, P, cap, V, K, _ptr(Ks[c:d]), _ptr(Rs[c:d]),
                                          _ptr(ts[c:d]), thr, _ptr(mask[c:d]), _ptr(err[c:d]), _ptr(info[c:d]), stream), "xfh_verify_matches")
    return mask, err, info
