"""Multi-view triangulation of key-point tracks on MI355X: the point of every key-point of a reference view from all the views that see it.

The chain detect -> match -> relative pose -> two-view points (``triangulate_matches``) -> absolute pose of further images
(``estimate_absolute_pose_matches``) leaves one reference frame, V - 1 further frames matched against it and a pose for every frame.
``build_tracks`` turns the matcher's lists of the pairs (reference view, view v) into a track table, ``triangulate_views_batch`` triangulates
every track from all its views -- exhaustive two-view hypotheses of the pairs (0, v) scored by MSAC over the views, the inlier views of the
best one, a Gauss-Newton refit on them, the gates of the two-view triangulation -- and ``triangulate_views_matches`` does both.  The points
come out in the world frame, at the reference view's key-point rows: ``points3d_ref`` of ``estimate_absolute_pose_matches`` for the next
image, so "map from k views -> localise view k + 1 -> extend the map" never leaves HBM.  The kernels behind ``xfh_build_tracks`` /
``xfh_triangulate_views`` (include/xfeat_hip.h, csrc/k_triangulate.hip) are specified in DESIGN.md 3.16.  There is no CPU path: without the
HIP library and a gfx950 device the functions raise.
"""
import math

import torch

from . import _lib, _twoview
from ._twoview import ptr as _ptr

STATUS = ("valid", "unobserved", "not_finite", "behind", "far", "reproj", "parallax")      # the status codes 0 .. 6
INFO_FIELDS = ("n", "valid", "unobserved", "not_finite", "behind", "far", "reproj", "parallax")
MAX_VIEWS = 32
MAX_SCENES = 65535                           # of one library call; larger batches are split into chunks of scenes
_WHAT = "multi-view triangulation"


def _chunks(S):
    return [(a, min(S, a + MAX_SCENES)) for a in range(0, S, MAX_SCENES)]


def _views(who, V):
    if not 2 <= V <= MAX_VIEWS:
        raise _lib.XFeatHipError(f"{who}: V {V} outside [2, {MAX_VIEWS}]")


def build_tracks(idx_ref, idx_view, n_matches, K):
    """The track table of S scenes from the matcher's lists of the pairs (view 0, view v), v = 1 .. V-1.

    idx_ref, idx_view : (S, V-1, cap) int64 CUDA tensors: match i of the pair (0, v) is (row idx_ref[s, v-1, i] of view 0, row
                        idx_view[s, v-1, i] of view v) for i < n_matches[s, v-1];  n_matches (S, V-1) int32;  K: rows of the key-point tables
    Returns tracks (S, K, V) int32: [s, k, 0] = k, [s, k, v] = the row of view v that reference row k is matched to, or -1.  An index
    outside [0, K) is ignored; of duplicate reference rows the largest candidate row stays (the table is reproducible).  Asynchronous."""
    who = "build_tracks"
    for t in (idx_ref, idx_view, n_matches):
        if not torch.is_tensor(t):
            raise RuntimeError(f'{who}: tensors expected')
    if idx_ref.dim() != 3 or idx_view.shape != idx_ref.shape or n_matches.shape != idx_ref.shape[:2]:
        raise RuntimeError('expected idx_ref, idx_view (S,V-1,cap) and n_matches (S,V-1)')
    S, V, cap = idx_ref.shape[0], idx_ref.shape[1] + 1, idx_ref.shape[2]
    K = int(K)
    if K < 0:
        raise RuntimeError(f'{who}: K {K} is negative')
    _views(who, V)
    if not idx_ref.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    for t, dt in ((idx_ref, torch.int64), (idx_view, torch.int64), (n_matches, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != idx_ref.device:
            raise RuntimeError(f'{who}: contiguous int64 indices and int32 counts on one device expected')
    dev = idx_ref.device
    tracks = torch.empty((S, K, V), dtype=torch.int32, device=dev)
    if S == 0 or K == 0:                      # no track at all
        return tracks
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for a, b in _chunks(S):
        _lib.check(lib.xfh_build_tracks(_ptr(idx_ref[a:b]) if cap else None, _ptr(idx_view[a:b]) if cap else None, _ptr(n_matches[a:b]) if cap else None,
                                        b - a, V, cap, K, K, _ptr(tracks[a:b]), stream), "xfh_build_tracks")
    return tracks


def _f64(x, shape, dev, name):
    x = torch.as_tensor(x, dtype=torch.float64)
    if x.shape != shape:
        raise RuntimeError(f'{name} must be {tuple(shape)}')
    return x.to(dev).contiguous()


def _gates(who, max_reproj_error, min_parallax_deg, max_depth, min_views):
    thr, depth, deg = float(max_reproj_error), float(max_depth), float(min_parallax_deg)
    if not thr > 0.0 or math.isinf(thr):
        raise _lib.XFeatHipError(f"{who}: max_reproj_error {thr} must be positive and finite")
    if not depth > 0.0:
        raise _lib.XFeatHipError(f"{who}: max_depth {depth} must be positive")
    if not 0.0 <= deg <= 180.0:
        raise _lib.XFeatHipError(f"{who}: min_parallax_deg {deg} outside [0, 180]")
    if not 2 <= int(min_views) <= MAX_VIEWS:
        raise _lib.XFeatHipError(f"{who}: min_views {min_views} outside [2, {MAX_VIEWS}]")
    return thr, math.cos(math.radians(deg)), depth, int(min_views)


def triangulate_views_batch(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=float('inf'), min_views=2):
    """The 3D points of the tracks of S scenes from all the views that see them, in one call.

    kpts    : (S, V, Kcap, 2) float32 pixel coordinates, the key-point tables of the V <= 32 views; view 0 is the reference view
    tracks  : (S, K, V) int32, [s, k, v] = the row of view v's table that track k sees, or -1 (``build_tracks``)
    n_views : (S,) int32, scene s uses its first n_views[s] views; None = all V
    Ks, Rs  : (S, V, 3, 3) float64 PINHOLE intrinsics and rotations, ts (S, V, 3) float64, world -> camera: x_v = R_v X + t_v (what
              ``estimate_absolute_pose_*`` returns; (I, 0) and ``estimate_relative_pose_*``'s R, t are the two-view case)
    Per track: the views O that observe it (an entry in range, a finite pixel, a usable pose); for every v in O but 0 the optimal two-view
    point of the pair (0, v) (``triangulate_batch``'s), scored by MSAC over O at max_reproj_error pixels; the inlier views I of the best; a
    Gauss-Newton refit of the point on I; the gates.  status (STATUS): 0 valid, 1 unobserved (view 0 or every other view does not see it),
    2 not finite (also: no pair with a baseline), 3 behind an inlier view, 4 deeper than max_depth in one, 5 fewer than min_views inlier views,
    view 0 not among them, or an inlier error above max_reproj_error after the refit, 6 every ray closer than min_parallax_deg to view 0's.
    Returns a dict of CUDA tensors: 'points3d' (S,K,3) float32 in the world frame, NaN unless valid (``points3d_ref`` of
    ``estimate_absolute_pose_matches`` as it is, with its ``idx_ref`` the reference rows), 'status' (S,K) uint8, 'n_inliers' (S,K) uint8,
    'inlier_views' (S,K) int32 (bit v = view v), 'reproj_error' (S,K) float32 pixels (the largest inlier error; NaN for status 1 and 2),
    'info' (S,8) int32 (INFO_FIELDS: K and the number of tracks per status), 'valid' (S,K) bool.  Asynchronous."""
    who = "triangulate_views_batch"
    thr, cos_min, depth, min_views = _gates(who, max_reproj_error, min_parallax_deg, max_depth, min_views)
    kpts, tracks = torch.as_tensor(kpts), torch.as_tensor(tracks)
    if kpts.dim() != 4 or kpts.shape[3] != 2 or tracks.dim() != 3 or tracks.shape[0] != kpts.shape[0] or tracks.shape[2] != kpts.shape[1]:
        raise RuntimeError('expected kpts (S,V,Kcap,2) and tracks (S,K,V)')
    S, V, kcap = kpts.shape[:3]
    K = tracks.shape[1]
    _views(who, V)
    dev = kpts.device if kpts.is_cuda else _twoview.device(_WHAT)
    kpts, tracks = kpts.to(dev).float().contiguous(), tracks.to(dev).to(torch.int32).contiguous()
    if n_views is not None:
        n_views = torch.as_tensor(n_views)
        if n_views.shape != (S,):
            raise RuntimeError('n_views must have one entry per scene')
        n_views = n_views.to(dev).to(torch.int32).contiguous()
    Ks, Rs, ts = _f64(Ks, (S, V, 3, 3), dev, 'Ks'), _f64(Rs, (S, V, 3, 3), dev, 'Rs'), _f64(ts, (S, V, 3), dev, 'ts')
    X = torch.empty((S, K, 3), dtype=torch.float32, device=dev)
    status = torch.empty((S, K), dtype=torch.uint8, device=dev)
    ninl = torch.empty((S, K), dtype=torch.uint8, device=dev)
    inl = torch.empty((S, K), dtype=torch.int32, device=dev)
    err = torch.empty((S, K), dtype=torch.float32, device=dev)
    info = torch.empty((S, 8), dtype=torch.int32, device=dev)
    if S == 0 or K == 0:                      # no track at all: info written like the kernel writes it
        info.zero_()
    elif kcap == 0:                           # no key-point at all: nothing observes any track
        X.fill_(float('nan')); err.fill_(float('nan')); status.fill_(1); ninl.zero_(); inl.zero_(); info.zero_()
        info[:, 0] = K; info[:, 2] = K
    else:
        lib = _lib.load()
        stream = torch.cuda.current_stream(dev).cuda_stream
        for a, b in _chunks(S):
            _lib.check(lib.xfh_triangulate_views(_ptr(kpts[a:b]), kcap, _ptr(tracks[a:b]), _ptr(n_views[a:b]) if n_views is not None else None, b - a, K, V,
                                                 _ptr(Ks[a:b]), _ptr(Rs[a:b]), _ptr(ts[a:b]), thr, cos_min, depth, min_views, _ptr(X[a:b]), _ptr(status[a:b]),
                                                 _ptr(ninl[a:b]), _ptr(inl[a:b]), _ptr(err[a:b]), _ptr(info[a:b]), stream), "xfh_triangulate_views")
    return {'points3d': X, 'status': status, 'n_inliers': ninl, 'inlier_views': inl, 'reproj_error': err, 'info': info, 'valid': status == 0}


def triangulate_views_matches(kpts, idx_ref, idx_view, n_matches, n_views, Ks, Rs, ts, max_reproj_error=4.0, min_parallax_deg=1.0,
                              max_depth=float('inf'), min_views=2):
    """``build_tracks`` on the matcher's lists, then ``triangulate_views_batch`` on the table: kpts (S,V,K,2), idx_ref / idx_view (S,V-1,cap)
    int64, n_matches (S,V-1) int32 CUDA tensors.  Same result dict, with 'tracks' (S,K,V) int32 added."""
    _gates("triangulate_views_matches", max_reproj_error, min_parallax_deg, max_depth, min_views)
    if not torch.is_tensor(kpts) or kpts.dim() != 4 or kpts.shape[3] != 2:
        raise RuntimeError('expected kpts (S,V,K,2)')
    if torch.is_tensor(idx_ref) and idx_ref.dim() == 3 and (idx_ref.shape[0] != kpts.shape[0] or idx_ref.shape[1] + 1 != kpts.shape[1]):
        raise RuntimeError('expected idx_ref, idx_view (S,V-1,cap) for kpts (S,V,K,2)')
    tracks = build_tracks(idx_ref, idx_view, n_matches, kpts.shape[2])
    out = triangulate_views_batch(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error, min_parallax_deg, max_depth, min_views)
    out['tracks'] = tracks
    return out
