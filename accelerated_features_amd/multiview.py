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

With the matches of arbitrary pairs of views (a sequence's (v, v + 1), an unordered set) ``build_tracks_graph`` makes the tables from the
connected components of the match graph, ``triangulate_views_batch(anchor='first')`` triangulates each track from its lowest observing
view, ``triangulate_graph_matches`` does both and ``view_points`` hands the map to ``estimate_absolute_pose_matches`` at any view's rows
(``xfh_build_tracks_graph`` / ``xfh_triangulate_tracks``, csrc/k_tracks.hip).

``average_poses_batch`` supplies the poses when nobody gives them: from the relative poses of the pairs (``relative_poses_graph_matches``
runs ``estimate_relative_pose_matches`` over a pair graph) it estimates the world poses of all views -- a spanning tree, robust rotation
averaging, robust position averaging on the directions (``xfh_average_poses``, csrc/k_triangulate.hip) -- and
``reconstruct_graph_matches`` chains matches -> relative poses -> global poses -> tracks -> triangulation -> bundle adjustment.
"""
import math

import torch

from . import _lib, _scenes, _twoview
from ._scenes import MAX_SCENES, MAX_VIEWS, WORKSPACE_LIMIT      # noqa: F401 (public here)
from ._twoview import ptr as _ptr

STATUS = ("valid", "unobserved", "not_finite", "behind", "far", "reproj", "parallax")      # the status codes 0 .. 6
INFO_FIELDS = ("n", "valid", "unobserved", "not_finite", "behind", "far", "reproj", "parallax")
_WHAT = "multi-view triangulation"


def build_tracks(idx_ref, idx_view, n_matches, K):
    """The track table of S scenes from the matcher's lists of the pairs (view 0, view v), v = 1 .. V-1.

    idx_ref, idx_view : (S, V-1, cap) int64 CUDA tensors: match i of the pair (0, v) is (row idx_ref[s, v-1, i] of view 0, row
                        idx_view[s, v-1, i] of view v) for i < n_matches[s, v-1];  n_matches (S, V-1) int32;  K: rows of the key-point tables
    Returns tracks (S, K, V) int32: [s, k, 0] = k, [s, k, v] = the row of view v that reference row k is matched to, or -1.  An index
    outside [0, K) is ignored; of duplicate reference rows the largest candidate row stays (the table is reproducible).  Asynchronous."""
    who = "build_tracks"
    _scenes.tensors(who, idx_ref, idx_view, n_matches)
    if idx_ref.dim() != 3 or idx_view.shape != idx_ref.shape or n_matches.shape != idx_ref.shape[:2]:
        raise RuntimeError('expected idx_ref, idx_view (S,V-1,cap) and n_matches (S,V-1)')
    S, V, cap = idx_ref.shape[0], idx_ref.shape[1] + 1, idx_ref.shape[2]
    K = int(K)
    if K < 0:
        raise RuntimeError(f'{who}: K {K} is negative')
    _scenes.views(who, V)
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
    for a, b in _scenes.chunks(S):
        _lib.check(lib.xfh_build_tracks(_ptr(idx_ref[a:b]) if cap else None, _ptr(idx_view[a:b]) if cap else None, _ptr(n_matches[a:b]) if cap else None,
                                        b - a, V, cap, K, K, _ptr(tracks[a:b]), stream), "xfh_build_tracks")
    return tracks


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


ANCHORS = {'reference': 'xfh_triangulate_views', 'first': 'xfh_triangulate_tracks'}


def _anchor(who, anchor):
    if anchor not in ANCHORS:
        raise _lib.XFeatHipError(f"{who}: anchor {anchor!r} is neither 'reference' nor 'first'")
    return ANCHORS[anchor]


def triangulate_views_batch(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=float('inf'), min_views=2,
                            anchor='reference'):
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
    'info' (S,8) int32 (INFO_FIELDS: K and the number of tracks per status), 'valid' (S,K) bool.  Asynchronous.
    anchor='first' (the tables of ``build_tracks_graph``): "view 0" above is the lowest view that observes the track, status 1
    is fewer than two observing views alone; a track whose lowest observing view is 0 gets the same bits either way."""
    who = "triangulate_views_batch"
    thr, cos_min, depth, min_views = _gates(who, max_reproj_error, min_parallax_deg, max_depth, min_views)
    entry = _anchor(who, anchor)
    kpts, tracks = torch.as_tensor(kpts), torch.as_tensor(tracks)
    S, V, kcap, K = _scenes.kpts_tracks(kpts, tracks)
    _scenes.views(who, V)
    dev = kpts.device if kpts.is_cuda else _twoview.device(_WHAT)
    kpts, tracks = kpts.to(dev).float().contiguous(), tracks.to(dev).to(torch.int32).contiguous()
    n_views = _scenes.n_views_arg(n_views, S, dev)
    Ks, Rs, ts = _scenes.f64(Ks, (S, V, 3, 3), dev, 'Ks'), _scenes.f64(Rs, (S, V, 3, 3), dev, 'Rs'), _scenes.f64(ts, (S, V, 3), dev, 'ts')
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
        for a, b in _scenes.chunks(S):
            _lib.check(getattr(lib, entry)(_ptr(kpts[a:b]), kcap, _ptr(tracks[a:b]), _ptr(n_views[a:b]) if n_views is not None else None, b - a, K, V,
                                           _ptr(Ks[a:b]), _ptr(Rs[a:b]), _ptr(ts[a:b]), thr, cos_min, depth, min_views, _ptr(X[a:b]), _ptr(status[a:b]),
                                           _ptr(ninl[a:b]), _ptr(inl[a:b]), _ptr(err[a:b]), _ptr(info[a:b]), stream), entry)
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


# ---- bundle adjustment -----------------------------------------------------------------------------------------------------
BA_STATUS = ("ok", "nothing_to_refine", "not_finite")       # info[:, 5]
BA_INFO_FIELDS = ("refined_points", "observations", "free_views", "iterations", "accepted_steps", "status", "spare0", "spare1")
MIN_VIEW_OBS = 6                             # ba::MIN_VIEW_OBS: a view with fewer observations is held
MAX_BA_ITERATIONS = 1000


def _ba_settings(who, fixed_views, max_iterations, huber_px):
    if isinstance(fixed_views, bool) or not isinstance(fixed_views, int):
        raise _lib.XFeatHipError(f"{who}: fixed_views must be an int bit mask of views")
    if not 0 <= fixed_views < (1 << 32):
        raise _lib.XFeatHipError(f"{who}: fixed_views {fixed_views} outside [0, 2^32)")
    iters, c = int(max_iterations), float(huber_px)
    if not 0 <= iters <= MAX_BA_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: max_iterations {iters} outside [0, {MAX_BA_ITERATIONS}]")
    if not c > 0.0:
        raise _lib.XFeatHipError(f"{who}: huber_px {c} must be positive (inf: plain squares)")
    return fixed_views, iters, c


def bundle_adjust_batch(kpts, tracks, inlier_views, points3d, n_views, Ks, Rs, ts, fixed_views=1, max_iterations=10, huber_px=1.0):
    """Bundle adjustment of S scenes in one call: the poses of the free views and the points of the valid tracks, refined together.

    kpts, tracks, n_views, Ks, Rs, ts : as for ``triangulate_views_batch``;  inlier_views (S,K) int32 and points3d (S,K,3) float32: its result
    fixed_views    : int bit mask of the views held constant (default 1: view 0; bit 0 need not be set)
    max_iterations : Levenberg-Marquardt rounds at the most;  huber_px: the Huber loss's corner in pixels, inf = plain squares
    The observations are fixed at the input state: (k, w) with bit w of inlier_views[k], w < n_views, a table entry in range, a finite pixel,
    a usable pose, a finite point, depth > 0 and a finite error.  A track with fewer than 2 of them is not refined; a view is free when it is
    not in fixed_views and keeps at least MIN_VIEW_OBS observations, every other view is held and still constrains the points.  Gauge: with
    only view 0 held the global scale is free -- the damping keeps it where the start put it, nothing pins it; hold two views
    (fixed_views=3) for a pinned gauge.
    Returns a dict of CUDA tensors: 'Rs' (S,V,3,3), 'ts' (S,V,3) float64 (held views: the input's bits), 'points3d' (S,K,3) float32 (refined
    tracks rounded once at the end, every other row the input's bits), 'refined' (S,K) bool, 'free_views' (S,) int32 mask, 'cost' (S,2)
    float64 (the robust cost before and after), 'info' (S,8) int32 (BA_INFO_FIELDS; status: BA_STATUS).  Asynchronous."""
    who = "bundle_adjust_batch"
    fixed_views, iters, huber = _ba_settings(who, fixed_views, max_iterations, huber_px)
    kpts, tracks = torch.as_tensor(kpts), torch.as_tensor(tracks)
    inlier_views, points3d = torch.as_tensor(inlier_views), torch.as_tensor(points3d)
    S, V, kcap, K = _scenes.kpts_tracks(kpts, tracks)
    if inlier_views.shape != (S, K) or points3d.shape != (S, K, 3):
        raise RuntimeError('expected inlier_views (S,K) and points3d (S,K,3)')
    _scenes.views(who, V)
    dev = kpts.device if kpts.is_cuda else _twoview.device("bundle adjustment")
    kpts, tracks = kpts.to(dev).float().contiguous(), tracks.to(dev).to(torch.int32).contiguous()
    inlier_views, points3d = inlier_views.to(dev).to(torch.int32).contiguous(), points3d.to(dev).float().contiguous()
    n_views = _scenes.n_views_arg(n_views, S, dev)
    Ks, Rs, ts = _scenes.f64(Ks, (S, V, 3, 3), dev, 'Ks'), _scenes.f64(Rs, (S, V, 3, 3), dev, 'Rs'), _scenes.f64(ts, (S, V, 3), dev, 'ts')
    if S == 0 or K == 0 or kcap == 0:         # no observation at all: nothing to refine
        info = torch.zeros((S, 8), dtype=torch.int32, device=dev)
        info[:, 5] = 1
        return {'Rs': Rs.clone(), 'ts': ts.clone(), 'points3d': points3d.clone(), 'refined': torch.zeros((S, K), dtype=torch.bool, device=dev),
                'free_views': torch.zeros((S,), dtype=torch.int32, device=dev), 'cost': torch.zeros((S, 2), dtype=torch.float64, device=dev),
                'info': info}
    Ro, to, Xo = torch.empty_like(Rs), torch.empty_like(ts), torch.empty_like(points3d)
    refined = torch.empty((S, K), dtype=torch.uint8, device=dev)
    free = torch.empty((S,), dtype=torch.int32, device=dev)
    cost = torch.empty((S, 2), dtype=torch.float64, device=dev)
    info = torch.empty((S, 8), dtype=torch.int32, device=dev)
    lib = _lib.load()

    def call(a, b, ws, ws_bytes, stream):
        return lib.xfh_bundle_adjust(_ptr(kpts[a:b]), kcap, _ptr(tracks[a:b]), _ptr(inlier_views[a:b]), _ptr(points3d[a:b]),
                                     _ptr(n_views[a:b]) if n_views is not None else None, b - a, K, V, _ptr(Ks[a:b]), _ptr(Rs[a:b]), _ptr(ts[a:b]),
                                     fixed_views, iters, huber, _ptr(Ro[a:b]), _ptr(to[a:b]), _ptr(Xo[a:b]), _ptr(refined[a:b]), _ptr(free[a:b]),
                                     _ptr(cost[a:b]), _ptr(info[a:b]), ws, ws_bytes, stream)
    _scenes.run_scenes("xfh_bundle_adjust", S, lambda n: lib.xfh_bundle_workspace_bytes(n, K, V), dev, call)
    return {'Rs': Ro, 'ts': to, 'points3d': Xo, 'refined': refined.bool(), 'free_views': free, 'cost': cost, 'info': info}


def refine_views_batch(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=float('inf'), min_views=2,
                       fixed_views=1, max_iterations=10, huber_px=1.0, anchor='reference'):
    """``triangulate_views_batch`` -> ``bundle_adjust_batch`` -> ``triangulate_views_batch`` again under the refined poses, so the status and
    the gates describe the refined map (the inlier views are selected anew; the points are the second triangulation's).  Returns the second
    triangulation's dict ('points3d' feeds ``estimate_absolute_pose_matches`` as before) with 'Rs', 'ts' (the refined poses), 'refined',
    'free_views', 'cost' and 'ba_info' of the adjustment added.  anchor: of both triangulations.  Asynchronous."""
    who = "refine_views_batch"
    _gates(who, max_reproj_error, min_parallax_deg, max_depth, min_views)
    _ba_settings(who, fixed_views, max_iterations, huber_px)
    _anchor(who, anchor)
    first = triangulate_views_batch(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error, min_parallax_deg, max_depth, min_views, anchor)
    ba = bundle_adjust_batch(kpts, tracks, first['inlier_views'], first['points3d'], n_views, Ks, Rs, ts, fixed_views, max_iterations, huber_px)
    out = triangulate_views_batch(kpts, tracks, n_views, Ks, ba['Rs'], ba['ts'], max_reproj_error, min_parallax_deg, max_depth, min_views, anchor)
    out.update(Rs=ba['Rs'], ts=ba['ts'], refined=ba['refined'], free_views=ba['free_views'], cost=ba['cost'], ba_info=ba['info'])
    return out


# ---- tracks over a graph of view pairs ---------------------------------------------------------------------------------------
TRACK_STATUS = ("ok", "unused", "bound_reached")           # track_info[:, 6]
TRACK_INFO_FIELDS = ("nodes", "components", "tracks", "inconsistent", "short", "over_capacity", "status", "spare")
MAX_PAIRS = 65535


def build_tracks_graph(view_pairs, idx_a, idx_b, n_matches, n_views, K, min_length=2, max_tracks=None):
    """The track tables of S scenes from the matcher's lists of any pairs of views: the connected components of the match graph.

    view_pairs   : (S, P, 2) or (P, 2) int32: pair p matches view view_pairs[..., p, 0] against view view_pairs[..., p, 1]
    idx_a, idx_b : (S, P, cap) int64 CUDA tensors: match i of pair p = (a, b) is (row idx_a[s, p, i] of view a, row idx_b[s, p, i] of view b)
                   for i < n_matches[s, p];  n_matches (S, P) int32;  n_views: V <= 32;  K: rows of the key-point tables
    A pair with a == b or a view outside [0, V) and an index outside [0, K) are ignored; a pair may occur more than once.  A track is a
    component with at most one key-point per view (any other component is dropped whole) that spans at least min_length views.  Its id is
    the rank of its smallest node (lowest view, then row) within the scene; ids from max_tracks (None: (V K) // 2, more cannot exist) on are
    dropped and counted.  The tables do not depend on the order of the lists: two calls give the same bytes.
    Returns (tracks (S, T, V) int32: a row or -1, rows >= n_tracks[s] all -1;  track_of (S, V, K) int32: the track of a key-point or -1;
    n_tracks (S,) int32;  info (S, 8) int32: TRACK_INFO_FIELDS, status: TRACK_STATUS).  Asynchronous."""
    who = "build_tracks_graph"
    _scenes.tensors(who, view_pairs, idx_a, idx_b, n_matches)
    V, K = int(n_views), int(K)
    if K < 0:
        raise RuntimeError(f'{who}: K {K} is negative')
    _scenes.views(who, V)
    if idx_a.dim() != 3 or idx_b.shape != idx_a.shape or n_matches.shape != idx_a.shape[:2]:
        raise RuntimeError('expected idx_a, idx_b (S,P,cap) and n_matches (S,P)')
    S, P, cap = idx_a.shape
    _scenes.check_view_pairs(view_pairs, S, P)
    if P > MAX_PAIRS:
        raise _lib.XFeatHipError(f"{who}: {P} pairs, more than {MAX_PAIRS}")
    if not 2 <= int(min_length) <= MAX_VIEWS:
        raise _lib.XFeatHipError(f"{who}: min_length {min_length} outside [2, {MAX_VIEWS}]")
    T = (V * K) // 2 if max_tracks is None else int(max_tracks)
    if max_tracks is not None and not 1 <= T <= max(V * K, 1):
        raise _lib.XFeatHipError(f"{who}: max_tracks {T} outside [1, V K = {V * K}]")
    if not idx_a.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    for t, dt in ((view_pairs, torch.int32), (idx_a, torch.int64), (idx_b, torch.int64), (n_matches, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != idx_a.device:
            raise RuntimeError(f'{who}: contiguous int32 pairs, int64 indices and int32 counts on one device expected')
    dev = idx_a.device
    if view_pairs.dim() == 2:
        view_pairs = view_pairs.expand(S, P, 2).contiguous()
    tracks = torch.empty((S, T, V), dtype=torch.int32, device=dev)
    track_of = torch.empty((S, V, K), dtype=torch.int32, device=dev)
    n_tracks = torch.empty((S,), dtype=torch.int32, device=dev)
    info = torch.empty((S, 8), dtype=torch.int32, device=dev)
    if S == 0 or K == 0 or P == 0 or cap == 0:                # no match at all: written like the kernels write it
        tracks.fill_(-1); track_of.fill_(-1); n_tracks.zero_(); info.zero_()
        return tracks, track_of, n_tracks, info
    lib = _lib.load()

    def call(a, b, ws, ws_bytes, stream):
        return lib.xfh_build_tracks_graph(_ptr(view_pairs[a:b]), _ptr(idx_a[a:b]), _ptr(idx_b[a:b]), _ptr(n_matches[a:b]), b - a, P, cap, V, K,
                                          int(min_length), T, _ptr(tracks[a:b]), _ptr(track_of[a:b]), _ptr(n_tracks[a:b]), _ptr(info[a:b]), ws,
                                          ws_bytes, stream)
    _scenes.run_scenes("xfh_build_tracks_graph", S, lambda n: lib.xfh_track_graph_workspace_bytes(n, V, K), dev, call)
    return tracks, track_of, n_tracks, info


def triangulate_graph_matches(kpts, view_pairs, idx_a, idx_b, n_matches, n_views, Ks, Rs, ts, max_reproj_error=4.0, min_parallax_deg=1.0,
                              max_depth=float('inf'), min_views=2, min_length=2, max_tracks=None):
    """``build_tracks_graph`` on the matcher's lists of any pairs of views, then ``triangulate_views_batch(anchor='first')`` on its table:
    kpts (S,V,K,2), view_pairs (S,P,2) or (P,2) int32, idx_a / idx_b (S,P,cap) int64, n_matches (S,P) int32 CUDA tensors; n_views (S,) int32
    or None as for ``triangulate_views_batch`` (the tracks are built over all V views).  The result dict of the triangulation over the T
    rows of the table (rows >= n_tracks are unobserved), with 'tracks' (S,T,V), 'track_of' (S,V,K), 'n_tracks' (S,) and 'track_info' (S,8)
    added."""
    who = "triangulate_graph_matches"
    _gates(who, max_reproj_error, min_parallax_deg, max_depth, min_views)
    if not torch.is_tensor(kpts) or kpts.dim() != 4 or kpts.shape[3] != 2:
        raise RuntimeError('expected kpts (S,V,K,2)')
    if torch.is_tensor(idx_a) and idx_a.dim() == 3 and idx_a.shape[0] != kpts.shape[0]:
        raise RuntimeError('expected idx_a, idx_b (S,P,cap) for kpts (S,V,K,2)')
    tracks, track_of, n_tracks, info = build_tracks_graph(view_pairs, idx_a, idx_b, n_matches, kpts.shape[1], kpts.shape[2], min_length, max_tracks)
    out = triangulate_views_batch(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error, min_parallax_deg, max_depth, min_views, anchor='first')
    out.update(tracks=tracks, track_of=track_of, n_tracks=n_tracks, track_info=info)
    return out


def view_points(points3d, track_of, view):
    """The points of the tracks at the key-point rows of one view: points3d (S,T,3) float32 and track_of (S,V,K) int32 of
    ``triangulate_graph_matches`` -> (S,K,3) float32, NaN where the key-point has no track (or its track no point).  It is
    ``points3d_ref`` of ``estimate_absolute_pose_matches`` for an image matched against that view."""
    points3d, track_of = torch.as_tensor(points3d), torch.as_tensor(track_of)
    if points3d.dim() != 3 or points3d.shape[2] != 3 or track_of.dim() != 3 or track_of.shape[0] != points3d.shape[0]:
        raise RuntimeError('expected points3d (S,T,3) and track_of (S,V,K)')
    view = int(view)
    if not 0 <= view < track_of.shape[1]:
        raise RuntimeError(f'view {view} outside [0, {track_of.shape[1]})')
    t = track_of[:, view].to(points3d.device).long()
    T = points3d.shape[1]
    has = (t >= 0) & (t < T)
    out = torch.full(t.shape + (3,), float('nan'), dtype=torch.float32, device=points3d.device)
    if T:
        got = torch.gather(points3d.float(), 1, t.clamp(0, T - 1).unsqueeze(-1).expand(-1, -1, 3))
        out = torch.where(has.unsqueeze(-1), got, out)
    return out


# ---- pose-graph initialisation -----------------------------------------------------------------------------------------------
PG_STATUS = ("ok", "nothing_at_view_0", "rotations_only", "not_finite")       # info[:, 6]
PG_INFO_FIELDS = ("valid_edges", "registered_views", "direction_edges", "rotation_outliers", "position_outliers", "unknowns", "status", "spare")
MAX_PG_ITERATIONS = 1000
MAX_PG_PAIRS = 1 << 20
# the geometric mean of the lowest pivot ratio of the rigid families (2.4e-2) and the highest of the non-rigid ones (1.8e-15)
# on NOISE-FREE input.  At 0.5 degrees of noise the two families come within a factor of 1.3 (1.4e-3 against 1.1e-3): no value separates
# them there, and two triangles that share one view pass as rigid.
MIN_PIVOT_RATIO = 6.5e-9
# baseline scales from shared tracks
MAX_RATIO_PAIRS = 512                        # ps::MAX_PAIRS: all 496 pairs of 32 views fit
MAX_RATIO_KPTS = 4096                        # ps::MAX_K: the values of a wedge are selected in LDS
SCALE_TOL = 0.1                              # measured on the restatement at 0.5 px / 0.5 degrees
PS_INFO_FIELDS = ("wedges", "ratios", "tracks_examined", "tracks_valid", "status", "spare0", "spare1", "spare2")


def _pg_settings(who, iterations, redescend, rot_scale_deg, pos_scale_deg, min_pivot_ratio):
    it, rd = int(iterations), int(redescend)
    if not 1 <= it <= MAX_PG_ITERATIONS:
        raise _lib.XFeatHipError(f"{who}: iterations {it} outside [1, {MAX_PG_ITERATIONS}]")
    if not 0 <= rd <= it:
        raise _lib.XFeatHipError(f"{who}: redescend {rd} outside [0, iterations = {it}]")
    rot, pos, piv = float(rot_scale_deg), float(pos_scale_deg), float(min_pivot_ratio)
    if not 0.0 < rot <= 180.0:
        raise _lib.XFeatHipError(f"{who}: rot_scale_deg {rot} outside (0, 180]")
    if not 0.0 < pos <= 90.0:
        raise _lib.XFeatHipError(f"{who}: pos_scale_deg {pos} outside (0, 90]")
    if not 0.0 <= piv < 1.0:
        raise _lib.XFeatHipError(f"{who}: min_pivot_ratio {piv} outside [0, 1)")
    return it, rd, math.radians(rot), math.sin(math.radians(pos)), piv


def average_poses_batch(view_pairs, R_rel, t_rel, weight, n_views, iterations=30, redescend=10, rot_scale_deg=2.0, pos_scale_deg=2.0,
                        min_pivot_ratio=MIN_PIVOT_RATIO, V=None, ratio=None, ratio_count=None, scale_weight=1.0, scale_tol=SCALE_TOL):
    """The world -> camera poses of the views of S scenes from the relative poses of P pairs of views per scene, in one call.

    view_pairs   : (S, P, 2) or (P, 2) int32: edge p = (a, b)
    R_rel, t_rel : (S, P, 3, 3), (S, P, 3) float64 with x_b = R_rel x_a + t_rel: what ``estimate_relative_pose_*`` returns with image 0 = a;
                   only the direction of t_rel is used;  weight (S, P) >= 0, for example the inlier count
    n_views      : V <= 32 as an int, or (S,) int32 (scene s uses its first n_views[s] views) with V given by the keyword
    An edge is valid when a != b, both views are in [0, n_views), the weight is finite and > 0 and R_rel is finite; it has a direction when
    t_rel is finite and not zero.  Duplicate pairs and pairs given as (b, a) are edges of their own.  A spanning tree from view 0 (largest
    weight first) starts the rotations; `iterations` rounds of rotation averaging and as many of position averaging follow, the last
    `redescend` of them with Cauchy's factor, the others with Huber's, at rot_scale_deg / pos_scale_deg.  Gauge: R_0 = I, c_0 = 0, the
    weighted mean of the baselines projected on their directions is 1.  A view that the valid edges do not connect to view 0 is
    unregistered: NaN pose, bit clear.  When the graph is not parallel-rigid (a chain of pairs (v, v + 1) is not: its baselines have no
    common scale) the positions are not determined: status 2, 'Rs' valid, 'ts' NaN but for view 0.
    ratio, ratio_count: (S, P, P) float64 / int32 of ``baseline_ratios_batch`` (both or neither; P <= 512): the baseline ratios of the edge
    pairs that share a view join the position rounds with the weight scale_weight ratio_count and the robust scale scale_tol (the relative
    disagreement |u_p - r u_q| / (u_p + r u_q) of the two baselines at which the factor starts to fall), which gives a chain positions.
    None: the call and the bytes of the pose graph without them.
    Returns a dict of CUDA tensors: 'Rs' (S,V,3,3), 'ts' (S,V,3) float64, 'registered' (S,) int32 mask, 'edge_factor' (S,P,2) float64 (the
    final rotation and position factors; 0 for an edge that took no part), 'info' (S,8) int32 (PG_INFO_FIELDS; status: PG_STATUS) and, with
    ratios, 'ratio_factor' (S,P,P) float64 (the final factor of every wedge that took part, else 0).  Asynchronous."""
    who = "average_poses_batch"
    it, rd, crot, cpos, piv = _pg_settings(who, iterations, redescend, rot_scale_deg, pos_scale_deg, min_pivot_ratio)
    if (ratio is None) != (ratio_count is None):
        raise RuntimeError('ratio and ratio_count come together')
    if ratio is not None:
        sw, stol = float(scale_weight), float(scale_tol)
        if not 0.0 < sw < 1e300:
            raise _lib.XFeatHipError(f"{who}: scale_weight {sw} must be positive and finite")
        if not 0.0 < stol <= 1.0:
            raise _lib.XFeatHipError(f"{who}: scale_tol {stol} outside (0, 1]")
    view_pairs, R_rel, t_rel, weight = torch.as_tensor(view_pairs), torch.as_tensor(R_rel), torch.as_tensor(t_rel), torch.as_tensor(weight)
    if R_rel.dim() != 4 or R_rel.shape[2:] != (3, 3):
        raise RuntimeError('expected R_rel (S,P,3,3)')
    S, P = R_rel.shape[:2]
    _scenes.check_edges(view_pairs, t_rel, weight, S, P)
    per_scene = torch.is_tensor(n_views)
    if per_scene:
        if V is None:
            raise RuntimeError('n_views per scene needs the keyword V')
        if n_views.shape != (S,):
            raise RuntimeError('n_views must have one entry per scene')
    V = int(n_views) if not per_scene else int(V)
    _scenes.views(who, V)
    if P > MAX_PG_PAIRS:
        raise _lib.XFeatHipError(f"{who}: {P} pairs, more than {MAX_PG_PAIRS}")
    dev = R_rel.device if R_rel.is_cuda else _twoview.device("pose-graph initialisation")
    view_pairs, R_rel, t_rel, weight = _scenes.edges_arg(view_pairs, R_rel, t_rel, weight, S, P, dev)
    n_views = n_views.to(dev).to(torch.int32).contiguous() if per_scene else None
    Rs = torch.empty((S, V, 3, 3), dtype=torch.float64, device=dev)
    ts = torch.empty((S, V, 3), dtype=torch.float64, device=dev)
    registered = torch.empty((S,), dtype=torch.int32, device=dev)
    factor = torch.empty((S, P, 2), dtype=torch.float64, device=dev)
    info = torch.empty((S, 8), dtype=torch.int32, device=dev)
    out = {'Rs': Rs, 'ts': ts, 'registered': registered, 'edge_factor': factor, 'info': info}
    if ratio is not None:
        ratio, ratio_count = torch.as_tensor(ratio), torch.as_tensor(ratio_count)
        if ratio.shape != (S, P, P) or ratio_count.shape != (S, P, P):
            raise RuntimeError('expected ratio and ratio_count (S,P,P)')
        if P > MAX_RATIO_PAIRS:
            raise _lib.XFeatHipError(f"{who}: {P} pairs with ratios, more than {MAX_RATIO_PAIRS}")
        ratio, ratio_count = ratio.to(dev).to(torch.float64).contiguous(), ratio_count.to(dev).to(torch.int32).contiguous()
        out['ratio_factor'] = rfactor = torch.zeros((S, P, P), dtype=torch.float64, device=dev)
    if S == 0 or P == 0:                      # no edge at all: written like the kernel writes a scene without a valid edge
        Rs.fill_(float('nan')); ts.fill_(float('nan')); registered.fill_(1); info.zero_()
        Rs[:, 0] = torch.eye(3, dtype=torch.float64, device=dev); ts[:, 0] = 0.0
        info[:, 1] = 1; info[:, 6] = 1
        return out
    lib = _lib.load()

    def call(a, b, ws, ws_bytes, stream):
        return lib.xfh_average_poses(_ptr(view_pairs[a:b]), _ptr(R_rel[a:b]), _ptr(t_rel[a:b]), _ptr(weight[a:b]),
                                     _ptr(n_views[a:b]) if n_views is not None else None, b - a, P, V, it, rd, crot, cpos, piv, _ptr(Rs[a:b]),
                                     _ptr(ts[a:b]), _ptr(registered[a:b]), _ptr(factor[a:b]), _ptr(info[a:b]), ws, ws_bytes, stream)
    def call_ratios(a, b, ws, ws_bytes, stream):
        return lib.xfh_average_poses_ratios(_ptr(view_pairs[a:b]), _ptr(R_rel[a:b]), _ptr(t_rel[a:b]), _ptr(weight[a:b]),
                                            _ptr(n_views[a:b]) if n_views is not None else None, _ptr(ratio[a:b]), _ptr(ratio_count[a:b]), b - a, P, V,
                                            it, rd, crot, cpos, piv, sw, stol, _ptr(Rs[a:b]), _ptr(ts[a:b]), _ptr(registered[a:b]), _ptr(factor[a:b]),
                                            _ptr(rfactor[a:b]), _ptr(info[a:b]), ws, ws_bytes, stream)
    name, run, size = "xfh_average_poses", call, lib.xfh_pose_graph_workspace_bytes
    if ratio is not None:
        name, run, size = "xfh_average_poses_ratios", call_ratios, lib.xfh_pose_graph_ratios_workspace_bytes
    _scenes.run_scenes(name, S, lambda n: size(n, P, V), dev, run)
    return out


def baseline_ratios_batch(kpts, tracks, track_of, view_pairs, R_rel, t_rel, weight, Ks, n_views=None, max_reproj_error=4.0, min_parallax_deg=1.0,
                          max_depth=float('inf'), min_common=8):
    """The ratios of the baselines of the edge pairs that share a view, from the tracks: what ties the scales of a chain's relative poses.

    kpts (S,V,K,2) float32; tracks (S,T,V), track_of (S,V,K) int32 as ``build_tracks_graph`` returns them; view_pairs (S,P,2) or (P,2) int32,
    R_rel (S,P,3,3), t_rel (S,P,3), weight (S,P) as for ``average_poses_batch`` (P <= 512, K <= 4096); Ks (S,V,3,3); n_views (S,) int32 or
    None = V; the gates of ``triangulate_views_batch``.  A wedge is a pair of edges p < q, both valid and with a direction, whose view sets
    share exactly one view v.  Every track with a key-point in v and in the other view of either edge is triangulated under both edges; where
    both are valid the quotient of its two depths in v is a value, and the wedge's ratio |baseline p| / |baseline q| is the lower median
    of its n values when n >= min_common.  A selection, no average: two calls give the same bytes whatever the order of the rows.
    Returns a dict of CUDA tensors, all fully written: 'ratio' (S,P,P) float64 (NaN: none), 'count' (S,P,P) int32 (n; 0: no wedge),
    'shared_view' (S,P,P) int32 (-1: no wedge), 'info' (S,8) int32 (PS_INFO_FIELDS); entries with p >= q are (NaN, 0, -1), and so is every
    entry when there is no edge, no key-point row or no track row (written without a library call, info 0).  Asynchronous."""
    who = "baseline_ratios_batch"
    thr, cos_min, depth, _ = _gates(who, max_reproj_error, min_parallax_deg, max_depth, 2)
    _scenes.tensors(who, kpts, tracks, track_of)
    if kpts.dim() != 4 or kpts.shape[3] != 2:
        raise RuntimeError('expected kpts (S,V,K,2)')
    S, V, K = kpts.shape[:3]
    _scenes.views(who, V)
    if tracks.dim() != 3 or tracks.shape[0] != S or tracks.shape[2] != V or track_of.shape != (S, V, K):
        raise RuntimeError('expected tracks (S,T,V) and track_of (S,V,K) for kpts (S,V,K,2)')
    T = tracks.shape[1]
    view_pairs, R_rel, t_rel, weight = torch.as_tensor(view_pairs), torch.as_tensor(R_rel), torch.as_tensor(t_rel), torch.as_tensor(weight)
    if R_rel.dim() != 4 or R_rel.shape[0] != S or R_rel.shape[2:] != (3, 3):
        raise RuntimeError('expected R_rel (S,P,3,3)')
    P = R_rel.shape[1]
    _scenes.check_edges(view_pairs, t_rel, weight, S, P)
    if P > MAX_RATIO_PAIRS:
        raise _lib.XFeatHipError(f"{who}: {P} pairs, more than {MAX_RATIO_PAIRS}")
    if K > MAX_RATIO_KPTS:
        raise _lib.XFeatHipError(f"{who}: {K} key-points per view, more than {MAX_RATIO_KPTS}")
    if int(min_common) < 1:
        raise _lib.XFeatHipError(f"{who}: min_common {min_common} below 1")
    dev = kpts.device
    for t, dt, name in ((kpts, torch.float32, 'kpts'), (tracks, torch.int32, 'tracks'), (track_of, torch.int32, 'track_of')):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f'{who}: {name} must be a contiguous {dt} tensor on the device of kpts')
    n_views = _scenes.n_views_arg(n_views, S, dev)
    Ks = _scenes.f64(Ks, (S, V, 3, 3), dev, 'Ks')
    view_pairs, R_rel, t_rel, weight = _scenes.edges_arg(view_pairs, R_rel, t_rel, weight, S, P, dev)
    ratio = torch.empty((S, P, P), dtype=torch.float64, device=dev)
    count = torch.empty((S, P, P), dtype=torch.int32, device=dev)
    shared = torch.empty((S, P, P), dtype=torch.int32, device=dev)
    info = torch.empty((S, 8), dtype=torch.int32, device=dev)
    out = {'ratio': ratio, 'count': count, 'shared_view': shared, 'info': info}
    if S == 0 or P == 0 or K == 0 or T == 0:  # no edge or no track: no candidate is examined, every entry is (NaN, 0, -1), info 0
        ratio.fill_(float('nan')); count.zero_(); shared.fill_(-1); info.zero_()
        return out
    if not kpts.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident key-points and tracks")
    lib = _lib.load()

    def call(a, b, ws, ws_bytes, stream):
        return lib.xfh_baseline_ratios(_ptr(kpts[a:b]), _ptr(tracks[a:b]), _ptr(track_of[a:b]), _ptr(view_pairs[a:b]), _ptr(R_rel[a:b]), _ptr(t_rel[a:b]),
                                       _ptr(weight[a:b]), _ptr(Ks[a:b]), _ptr(n_views[a:b]) if n_views is not None else None, b - a, P, V, K, T, thr,
                                       cos_min, depth, int(min_common), _ptr(ratio[a:b]), _ptr(count[a:b]), _ptr(shared[a:b]), _ptr(info[a:b]), ws,
                                       ws_bytes, stream)
    _scenes.run_scenes("xfh_baseline_ratios", S, lambda n: lib.xfh_baseline_ratios_workspace_bytes(n, P, V, K), dev, call)
    return out


def relative_poses_graph_matches(kpts, view_pairs, idx_a, idx_b, n_matches, Ks, min_inliers=15, **ransac):
    """The relative poses of the pairs of a pair graph: ``estimate_relative_pose_matches`` once over the S P pairs of S scenes.

    kpts (S,V,K,2) float32, view_pairs (S,P,2) or (P,2) int32, idx_a / idx_b (S,P,cap) int64, n_matches (S,P) int32 CUDA tensors as for
    ``build_tracks_graph``; Ks (S,V,3,3) float64; **ransac: the estimator's settings (max_epipolar_error, success_prob, min_iterations,
    max_iterations, seed).  The key-point tables and intrinsics of each pair are gathered by indexing (2 S P K points: choose S to fit).
    Returns a dict: 'R_rel' (S,P,3,3), 't_rel' (S,P,3) float64 with x_b = R_rel x_a + t_rel, 'weight' (S,P) float64 = the inlier count where
    a pose was found with at least min_inliers inliers, else 0 (also for a pair with a == b or a view outside [0, V)), 'inliers' (S,P,cap)
    uint8, 'info' (S,P,8) int32 (pose.INFO_FIELDS): the arguments of ``average_poses_batch``.  Asynchronous."""
    from . import pose
    who = "relative_poses_graph_matches"
    _scenes.tensors(who, kpts, view_pairs, idx_a, idx_b, n_matches)
    if kpts.dim() != 4 or kpts.shape[3] != 2:
        raise RuntimeError('expected kpts (S,V,K,2)')
    S, V, K = kpts.shape[:3]
    _scenes.views(who, V)
    if idx_a.dim() != 3 or idx_a.shape[0] != S or idx_b.shape != idx_a.shape or n_matches.shape != idx_a.shape[:2]:
        raise RuntimeError('expected idx_a, idx_b (S,P,cap) and n_matches (S,P) for kpts (S,V,K,2)')
    P, cap = idx_a.shape[1:]
    _scenes.check_view_pairs(view_pairs, S, P)
    if int(min_inliers) < 0:
        raise _lib.XFeatHipError(f"{who}: min_inliers {min_inliers} is negative")
    if not kpts.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    dev = kpts.device
    Ks = _scenes.f64(Ks, (S, V, 3, 3), dev, 'Ks')
    vp = (view_pairs.expand(S, P, 2) if view_pairs.dim() == 2 else view_pairs).to(dev).long()
    a, b = vp[..., 0], vp[..., 1]
    legal = (a != b) & (a >= 0) & (a < V) & (b >= 0) & (b < V)
    a, b = a.clamp(0, V - 1), b.clamp(0, V - 1)
    sc = torch.arange(S, device=dev).unsqueeze(1).expand(S, P)
    r = pose.estimate_relative_pose_matches(kpts[sc, a].reshape(S * P, K, 2).float().contiguous(), kpts[sc, b].reshape(S * P, K, 2).float().contiguous(),
                                            idx_a.reshape(S * P, cap).contiguous(), idx_b.reshape(S * P, cap).contiguous(),
                                            n_matches.reshape(S * P).contiguous(), Ks[sc, a].reshape(S * P, 3, 3), Ks[sc, b].reshape(S * P, 3, 3), **ransac)
    info = r['info'].reshape(S, P, 8)
    found = legal & (info[..., 0] != 0) & (info[..., 3] >= int(min_inliers))
    weight = torch.where(found, info[..., 3].double(), torch.zeros((), dtype=torch.float64, device=dev))
    return {'R_rel': r['R'].reshape(S, P, 3, 3), 't_rel': r['t'].reshape(S, P, 3), 'weight': weight, 'inliers': r['inliers'].reshape(S, P, cap),
            'info': info}


def reconstruct_graph_matches(kpts, view_pairs, idx_a, idx_b, n_matches, n_views, Ks, min_inliers=15, ransac=None, iterations=30, redescend=10,
                              rot_scale_deg=2.0, pos_scale_deg=2.0, min_pivot_ratio=MIN_PIVOT_RATIO, max_reproj_error=4.0, min_parallax_deg=1.0,
                              max_depth=float('inf'), min_views=2, min_length=2, max_tracks=None, fixed_views=1, max_iterations=10, huber_px=1.0,
                              track_scales=False, min_common=8, scale_weight=1.0, scale_tol=SCALE_TOL, verified=False):
    """From the matches of an unordered set of images to a map: ``relative_poses_graph_matches`` -> ``average_poses_batch`` ->
    ``triangulate_graph_matches`` -> ``bundle_adjust_batch`` -> ``triangulate_views_batch(anchor='first')`` under the refined poses.
    track_scales=True builds the tracks first and gives the pose graph the baseline ratios of ``baseline_ratios_batch`` (P <= 512,
    K <= 4096): the way to positions for a sequence's pairs (v, v + 1), whose relative poses alone leave every baseline's length open
    (pose-graph status 2, an empty map).  The result then has 'ratio', 'ratio_count', 'ratio_factor' and 'ratio_info' added.
    verified=True compacts the lists to each pair's RANSAC inliers right after the relative poses (``filter_matches_batch`` with
    rel['inliers'], a pair without a pose emptied) and gives the compacted lists to every later stage: one wrong match
    joins two tracks into a component that is dropped whole, so raw mutual-nearest-neighbour lists leave almost no track.  The result then
    has 'idx_a_verified', 'idx_b_verified', 'n_verified', 'match_src' and 'filter_info' added.

    kpts (S,V,K,2), view_pairs (S,P,2) or (P,2), idx_a / idx_b (S,P,cap), n_matches (S,P) CUDA tensors; n_views (S,) int32 or None = all V;
    Ks (S,V,3,3); ransac: a dict of the relative-pose settings; the other keywords are those of the stages.
    The NaN pose of a view that the pose graph did not register (and every pose but view 0's of a scene with status 2) passes through
    untouched: both triangulations treat such a view as one that observes nothing (a pose that is not usable), the adjustment holds it.
    Returns the second triangulation's dict with 'Rs', 'ts' (the refined poses), 'refined', 'free_views', 'cost', 'ba_info' of the
    adjustment, 'tracks', 'track_of', 'n_tracks', 'track_info' of the tables, 'Rs_init', 'ts_init', 'registered', 'edge_factor', 'pg_info' of
    the pose graph and 'R_rel', 't_rel', 'weight', 'rel_info' of the pairs added.  Asynchronous: nothing synchronises with the host."""
    who = "reconstruct_graph_matches"
    _pg_settings(who, iterations, redescend, rot_scale_deg, pos_scale_deg, min_pivot_ratio)
    _gates(who, max_reproj_error, min_parallax_deg, max_depth, min_views)
    _ba_settings(who, fixed_views, max_iterations, huber_px)
    rel = relative_poses_graph_matches(kpts, view_pairs, idx_a, idx_b, n_matches, Ks, min_inliers, **(ransac or {}))
    V = kpts.shape[1]
    vp = view_pairs.to(kpts.device).to(torch.int32).contiguous()
    if verified:
        from . import verification
        idx_a, idx_b, n_matches, match_src, filter_info = verification.filter_matches_batch(idx_a, idx_b, n_matches, rel['inliers'], rel['weight'] > 0)
    if track_scales:
        tracks, track_of, n_tracks, track_info = build_tracks_graph(vp, idx_a, idx_b, n_matches, V, kpts.shape[2], min_length, max_tracks)
        br = baseline_ratios_batch(kpts.float().contiguous(), tracks, track_of, vp, rel['R_rel'], rel['t_rel'], rel['weight'], Ks, n_views, max_reproj_error,
                                   min_parallax_deg, max_depth, min_common)
        pg = average_poses_batch(view_pairs, rel['R_rel'], rel['t_rel'], rel['weight'], V if n_views is None else torch.as_tensor(n_views), iterations,
                                 redescend, rot_scale_deg, pos_scale_deg, min_pivot_ratio, V=V, ratio=br['ratio'], ratio_count=br['count'],
                                 scale_weight=scale_weight, scale_tol=scale_tol)
        first = triangulate_views_batch(kpts, tracks, n_views, Ks, pg['Rs'], pg['ts'], max_reproj_error, min_parallax_deg, max_depth, min_views,
                                        anchor='first')
        first.update(tracks=tracks, track_of=track_of, n_tracks=n_tracks, track_info=track_info)
    else:
        pg = average_poses_batch(view_pairs, rel['R_rel'], rel['t_rel'], rel['weight'], V if n_views is None else torch.as_tensor(n_views), iterations,
                                 redescend, rot_scale_deg, pos_scale_deg, min_pivot_ratio, V=V)
        first = triangulate_graph_matches(kpts, vp, idx_a, idx_b, n_matches, n_views, Ks, pg['Rs'], pg['ts'], max_reproj_error, min_parallax_deg, max_depth,
                                          min_views, min_length, max_tracks)
    ba = bundle_adjust_batch(kpts, first['tracks'], first['inlier_views'], first['points3d'], n_views, Ks, pg['Rs'], pg['ts'], fixed_views,
                             max_iterations, huber_px)
    out = triangulate_views_batch(kpts, first['tracks'], n_views, Ks, ba['Rs'], ba['ts'], max_reproj_error, min_parallax_deg, max_depth, min_views,
                                  anchor='first')
    out.update(Rs=ba['Rs'], ts=ba['ts'], refined=ba['refined'], free_views=ba['free_views'], cost=ba['cost'], ba_info=ba['info'],
               tracks=first['tracks'], track_of=first['track_of'], n_tracks=first['n_tracks'], track_info=first['track_info'],
               Rs_init=pg['Rs'], ts_init=pg['ts'], registered=pg['registered'], edge_factor=pg['edge_factor'], pg_info=pg['info'],
               R_rel=rel['R_rel'], t_rel=rel['t_rel'], weight=rel['weight'], rel_info=rel['info'])
    if track_scales:
        out.update(ratio=br['ratio'], ratio_count=br['count'], ratio_factor=pg['ratio_factor'], ratio_info=br['info'])
    if verified:
        out.update(idx_a_verified=idx_a, idx_b_verified=idx_b, n_verified=n_matches, match_src=match_src, filter_info=filter_info)
    return out
