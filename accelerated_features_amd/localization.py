"""Localisation against the map on MI355X: descriptors for the tracks, 2D-3D matching, the pose of a new image.

``reconstruct_graph_matches`` leaves refined poses and triangulated tracks; ``view_points`` hands them to the P3P estimator at the rows of ONE
view, so a query can only be localised against a reference image it was matched with.  ``build_map_batch`` gives every usable track a
descriptor -- the normalised sum of the descriptors of the views that the triangulation kept as inliers -- and packs point, descriptor and
track id into map rows; ``localize_map_batch`` matches query images against those rows with the exact mutual-nearest-neighbour matcher, runs
``estimate_absolute_pose_matches`` on the 2D-3D lists and, with ``guided=True``, matches again among the candidates that agree with that pose
(the map projected by ``xfh_map_project``, the forward-transfer gate of ``match_guided_device`` under the identity) and estimates once more.
``resect_views_batch`` is ``view_points`` for all views at once with one P3P RANSAC per (scene, view): the poses of the views a pose graph
left unregistered, whose key-points already sit in tracks that have points.  The kernels behind ``xfh_build_map`` / ``xfh_map_project``
(include/xfeat_hip.h, csrc/k_map.hip) are specified in DESIGN.md 3.21.  There is no CPU path: without the HIP library and a gfx950 device the
functions raise.
"""
import ctypes as C

import torch

from . import _lib, _scenes, _twoview, absolute_pose, guided as _guided
from ._scenes import MAX_SCENES, MAX_VIEWS, WORKSPACE_LIMIT      # noqa: F401 (public here)
from ._twoview import ptr as _ptr

MAP_INFO_FIELDS = ("tracks", "written", "skipped_status", "skipped_point", "skipped_views", "skipped_norm", "over_capacity", "spare")
_WHAT = "map building"


def build_map_batch(desc, tracks, points3d, status, inlier_views, min_views=2, max_points=None):
    """The map rows of S scenes from a triangulation's outputs: a point, a descriptor and the track id for every usable track.

    desc         : (S, V, Kcap, 64) float32, the L2-normalised descriptor tables of the V <= 32 views (``XFeat._detect_device`` per image)
    tracks       : (S, T, V) int32;  points3d (S, T, 3) float32;  status (S, T) uint8;  inlier_views (S, T) int32: what
                   ``triangulate_views_batch`` / ``triangulate_graph_matches`` / ``reconstruct_graph_matches`` return
    min_views    : a track needs that many contributing views (1 .. 32);  max_points: the rows M of the map per scene, None = T
    View v contributes to track t iff bit v of inlier_views[t] is set, tracks[t, v] is a row of the table and that row is finite.  A track is
    selected unless (in this order) its status is not 0, its point is not finite, fewer than min_views views contribute or the sum of the
    contributing rows has a squared norm that is not finite or below FLT_MIN (two antipodal observations).  The selected tracks fill the rows
    in ascending track id; those beyond max_points are dropped and counted.  Two calls give the same bytes.
    Returns a dict of CUDA tensors: 'points' (S,M,3) float32, 'desc' (S,M,64) float32 (unit rows), 'desc_f16' (S,M,64) float16 (256 * desc
    rounded to nearest even: ``d2_f16`` of ``xfh_match_mnn``), 'track' (S,M) int32, 'n_obs' (S,M) uint8, 'coherence' (S,M) float32 (the norm
    of the sum over n_obs: 1 when all observations agree, 0 when they cancel), 'n_points' (S,) int32, 'info' (S,8) int32 (MAP_INFO_FIELDS).
    Rows from n_points on hold a NaN point, zero descriptors, track -1, n_obs 0, coherence 0.  Asynchronous."""
    who = "build_map_batch"
    desc, tracks, points3d = torch.as_tensor(desc), torch.as_tensor(tracks), torch.as_tensor(points3d)
    status, inlier_views = torch.as_tensor(status), torch.as_tensor(inlier_views)
    if desc.dim() != 4 or desc.shape[3] != 64:
        raise RuntimeError('expected desc (S,V,Kcap,64)')
    S, V, kcap = desc.shape[:3]
    if tracks.dim() != 3 or tracks.shape[0] != S or tracks.shape[2] != V:
        raise RuntimeError('expected tracks (S,T,V) for desc (S,V,Kcap,64)')
    T = tracks.shape[1]
    if points3d.shape != (S, T, 3) or status.shape != (S, T) or inlier_views.shape != (S, T):
        raise RuntimeError('expected points3d (S,T,3), status (S,T) and inlier_views (S,T)')
    if not 1 <= V <= MAX_VIEWS:
        raise _lib.XFeatHipError(f"{who}: V {V} outside [1, {MAX_VIEWS}]")
    if isinstance(min_views, bool) or not 1 <= int(min_views) <= MAX_VIEWS:
        raise _lib.XFeatHipError(f"{who}: min_views {min_views} outside [1, {MAX_VIEWS}]")
    M = T if max_points is None else int(max_points)
    if max_points is not None and M < 1:
        raise _lib.XFeatHipError(f"{who}: max_points {M} below 1")
    empty = S == 0 or T == 0 or kcap == 0
    dev = desc.device if desc.is_cuda or empty else _twoview.device(_WHAT)
    desc, tracks, points3d = desc.to(dev).float().contiguous(), tracks.to(dev).to(torch.int32).contiguous(), points3d.to(dev).float().contiguous()
    status, inlier_views = status.to(dev).to(torch.uint8).contiguous(), inlier_views.to(dev).to(torch.int32).contiguous()
    out = {'points': torch.empty((S, M, 3), dtype=torch.float32, device=dev), 'desc': torch.empty((S, M, 64), dtype=torch.float32, device=dev),
           'desc_f16': torch.empty((S, M, 64), dtype=torch.float16, device=dev), 'track': torch.empty((S, M), dtype=torch.int32, device=dev),
           'n_obs': torch.empty((S, M), dtype=torch.uint8, device=dev), 'coherence': torch.empty((S, M), dtype=torch.float32, device=dev),
           'n_points': torch.empty((S,), dtype=torch.int32, device=dev), 'info': torch.empty((S, 8), dtype=torch.int32, device=dev)}
    if empty:                                 # nothing can be selected: written like the kernels write it
        out['points'].fill_(float('nan')); out['desc'].zero_(); out['desc_f16'].zero_(); out['track'].fill_(-1); out['n_obs'].zero_()
        out['coherence'].zero_(); out['n_points'].zero_(); out['info'].zero_()
        if T and S:                           # no key-point row: the tracks are skipped by status, by their point, or for want of views
            bad_point = ~torch.isfinite(points3d).all(dim=2)
            by_status = status != 0
            out['info'][:, 0] = T
            out['info'][:, 2] = by_status.sum(dim=1)
            out['info'][:, 3] = (~by_status & bad_point).sum(dim=1)
            out['info'][:, 4] = (~by_status & ~bad_point).sum(dim=1)
        return out
    lib = _lib.load()

    def call(a, b, ws, ws_bytes, stream):
        return lib.xfh_build_map(_ptr(desc[a:b]), kcap, _ptr(tracks[a:b]), _ptr(points3d[a:b]), _ptr(status[a:b]), _ptr(inlier_views[a:b]), b - a, T, V,
                                 int(min_views), M, _ptr(out['points'][a:b]), _ptr(out['desc'][a:b]), _ptr(out['desc_f16'][a:b]), _ptr(out['track'][a:b]),
                                 _ptr(out['n_obs'][a:b]), _ptr(out['coherence'][a:b]), _ptr(out['n_points'][a:b]), _ptr(out['info'][a:b]), ws, ws_bytes,
                                 stream)
    _scenes.run_scenes("xfh_build_map", S, lambda n: lib.xfh_map_workspace_bytes(n, T, V), dev, call)
    return out


def project_map(points, n_points, R, t, K, image_size=None, margin=0.0):
    """The pixels of map rows under Q poses (``xfh_map_project``): points (Q,M,3) float32, n_points (Q,) int32 or None = M, R (Q,3,3), t (Q,3),
    K (Q,3,3) or (3,3) float64 with x = K (R X + t).  Returns uv (Q,M,2) float32: fp64 arithmetic rounded once; NaN for a row >= n_points, a
    depth that is not finite or not > 0 and, with image_size = (W, H), a pixel more than `margin` outside the image.  Asynchronous."""
    who = "project_map"
    points = torch.as_tensor(points)
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError('expected points (Q,M,3)')
    Q, M = points.shape[:2]
    W = H = 0.0
    if image_size is not None:
        W, H = float(image_size[0]), float(image_size[1])
        if not (0.0 < W < float('inf') and 0.0 < H < float('inf')):
            raise _lib.XFeatHipError(f"{who}: image_size {image_size} must be positive and finite")
    margin = float(margin)
    if not 0.0 <= margin < float('inf'):
        raise _lib.XFeatHipError(f"{who}: margin {margin} must be finite and not negative")
    dev = points.device if points.is_cuda else _twoview.device("map projection")
    points = points.to(dev).float().contiguous()
    if n_points is not None:
        n_points = torch.as_tensor(n_points)
        if n_points.shape != (Q,):
            raise RuntimeError('n_points must have one entry per query')
        n_points = n_points.to(dev).to(torch.int32).contiguous()
    R, t = torch.as_tensor(R, dtype=torch.float64), torch.as_tensor(t, dtype=torch.float64)
    if R.shape != (Q, 3, 3) or t.shape != (Q, 3):
        raise RuntimeError('expected R (Q,3,3) and t (Q,3)')
    R, t, K = R.to(dev).contiguous(), t.to(dev).contiguous(), _twoview.intrinsics(K, Q, dev)
    uv = torch.empty((Q, M, 2), dtype=torch.float32, device=dev)
    if Q == 0 or M == 0:
        return uv
    _lib.check(_lib.load().xfh_map_project(_ptr(points), _ptr(n_points), Q, M, _ptr(R), _ptr(t), _ptr(K), W, H, margin, _ptr(uv),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "xfh_map_project")
    return uv


_MAP_KEYS = ('points', 'desc', 'desc_f16', 'track', 'n_points')


def _match_map(desc_q, q16, n_q, mdesc, m16, n_map, min_cossim):
    """xfh_match_mnn without a handle (the way ``guided._plain_mnn`` calls it): query = side 1, map = side 2 with n_points as its counts."""
    Q, nv = _guided._check_sets("localize_map_batch", desc_q, n_q, mdesc, n_map)
    N1, N2, dev = desc_q.shape[1], mdesc.shape[1], desc_q.device
    idx0, idx1, n = _guided._outputs(Q, N1, dev)
    if Q == 0 or N1 == 0 or N2 == 0:
        n.zero_()
        return idx0, idx1, n
    lib = _lib.load()
    ws, nb, _keep = _guided._workspace(lib.xfh_match_workspace_bytes(Q, N1, N2), dev)
    both = q16 is not None and m16 is not None
    _lib.check(lib.xfh_match_mnn(None, _ptr(desc_q), N1 * 64, _ptr(mdesc), N2 * 64, _ptr(q16) if both else None, _ptr(m16) if both else None, _ptr(nv),
                                 _ptr(nv), 1, Q, Q, N1, N2, float(min_cossim), _ptr(idx0), _ptr(idx1), _ptr(n), ws, nb,
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "xfh_match_mnn")
    return idx0, idx1, n


def localize_map_batch(kpts_q, desc_q, n_q, map, K, scene_of=None, min_cossim=0.82, guided=False, guide_thr=None, image_size=None, desc_q_f16=None,
                       **ransac):
    """The poses of Q query images against the maps of ``build_map_batch``.

    kpts_q, desc_q, n_q : (Q,Kq,2) float32 pixels, (Q,Kq,64) float32 unit descriptors, (Q,) int32 valid rows (``XFeat._detect_device``);
                          desc_q_f16 (Q,Kq,64) float16: the detector's fp16 copy, or None
    map                 : the dict of ``build_map_batch`` (S scenes, M rows);  K (Q,3,3) or (3,3) float64 PINHOLE intrinsics of the queries
    scene_of            : (Q,) int64, the scene whose map query q uses; None = arange, which needs Q == S.  The map rows of every query are
                          gathered by indexing (Q M rows: choose Q to fit)
    min_cossim          : the matcher's similarity test (the reference's ``match`` default);  **ransac: the settings of
                          ``estimate_absolute_pose_matches`` (max_reproj_error = 12 px by default)
    Stage 1: mutual nearest neighbours of the query's descriptors and the map's, then P3P RANSAC on the 2D-3D lists.  guided=True adds stage
    2: the map's points projected under stage 1's pose, mutual nearest neighbours among the candidates within guide_thr pixels (None: the
    estimator's max_reproj_error) of their projection -- image_size = (W, H) also drops the rows that project more than guide_thr outside
    the image -- and P3P again.  A query keeps its stage-1 result when stage 1 found nothing or stage 2 has fewer inliers.
    Returns the absolute-pose dict ('R' (Q,3,3), 't' (Q,3) float64, 'inliers' (Q,cap) uint8, 'info' (Q,8) int32) with 'idx_query', 'idx_map'
    (Q,cap) int64 and 'n_matches' (Q,) int32 (the lists the pose was estimated on, cap = min(Kq, M)), 'track' (Q,cap) int32 (the track id of
    each match, -1 beyond the count) and 'stage' (Q,) uint8 added.  Asynchronous: nothing synchronises with the host."""
    who = "localize_map_batch"
    if not isinstance(map, dict) or any(k not in map for k in _MAP_KEYS):
        raise RuntimeError(f'{who}: map must be the dict of build_map_batch')
    _scenes.tensors(who, kpts_q, desc_q, n_q, *(map[k] for k in _MAP_KEYS))
    if desc_q.dim() != 3 or desc_q.shape[2] != 64 or kpts_q.shape != desc_q.shape[:2] + (2,) or n_q.shape != desc_q.shape[:1]:
        raise RuntimeError('expected kpts_q (Q,Kq,2), desc_q (Q,Kq,64) and n_q (Q,)')
    Q, Kq = desc_q.shape[:2]
    mp, md, m16, mt, mn = (map[k] for k in _MAP_KEYS)
    if md.dim() != 3 or md.shape[2] != 64 or mp.shape != md.shape[:2] + (3,) or m16.shape != md.shape or mt.shape != md.shape[:2] or mn.shape != md.shape[:1]:
        raise RuntimeError('expected map points (S,M,3), desc and desc_f16 (S,M,64), track (S,M) and n_points (S,)')
    S, M = md.shape[:2]
    if desc_q_f16 is not None and (not torch.is_tensor(desc_q_f16) or desc_q_f16.shape != desc_q.shape or desc_q_f16.dtype != torch.float16):
        raise RuntimeError('desc_q_f16 must be a (Q,Kq,64) float16 tensor')
    if scene_of is None:
        if Q != S:
            raise RuntimeError(f'{who}: {Q} queries for {S} maps need scene_of')
    else:
        scene_of = torch.as_tensor(scene_of)
        if scene_of.shape != (Q,) or scene_of.dtype != torch.int64:
            raise RuntimeError('scene_of must be (Q,) int64')
    thr = float(ransac.get('max_reproj_error', absolute_pose.RANSAC_DEFAULTS['max_reproj_error'])) if guide_thr is None else float(guide_thr)
    if guided and not 0.0 < thr < float('inf'):
        raise _lib.XFeatHipError(f"{who}: guide_thr {thr} must be positive and finite")
    if image_size is not None and not (0.0 < float(image_size[0]) < float('inf') and 0.0 < float(image_size[1]) < float('inf')):
        raise _lib.XFeatHipError(f"{who}: image_size {image_size} must be positive and finite")
    if not desc_q.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident key-points, descriptors and maps")
    dev = desc_q.device
    for t, dt in ((kpts_q, torch.float32), (desc_q, torch.float32), (n_q, torch.int32), (mp, torch.float32), (md, torch.float32), (m16, torch.float16),
                  (mt, torch.int32), (mn, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f'{who}: contiguous float32 points and descriptors, float16 copies, int32 tracks and counts on one device expected')
    if scene_of is not None:
        sc = scene_of.to(dev).clamp(0, max(S - 1, 0))
        mp, md, m16, mt, mn = (x[sc].contiguous() for x in (mp, md, m16, mt, mn))
    cap = min(Kq, M)
    K = _twoview.intrinsics(K, Q, dev)

    def lists(i_q, i_m, n):
        """The first cap entries (no list is longer) and the track of every match."""
        i_q, i_m = i_q[:, :cap].contiguous(), i_m[:, :cap].contiguous()
        inside = torch.arange(cap, device=dev)[None, :] < n[:, None]
        trk = torch.gather(mt, 1, i_m.clamp(0, max(M - 1, 0))) if M else torch.empty((Q, 0), dtype=torch.int32, device=dev)
        return i_q, i_m, torch.where(inside, trk, torch.full_like(trk, -1))

    i_q, i_m, n = _match_map(desc_q, desc_q_f16, n_q, md, m16, mn, min_cossim)
    i_q, i_m, trk = lists(i_q, i_m, n)
    out = absolute_pose.estimate_absolute_pose_matches(kpts_q, mp, i_q, i_m, n, K, **ransac)
    stage = torch.ones((Q,), dtype=torch.uint8, device=dev)
    if guided and Q and cap:
        uv = project_map(mp, mn, out['R'], out['t'], K, image_size, thr if image_size is not None else 0.0)
        eye = torch.eye(3, dtype=torch.float64, device=dev).expand(Q, 3, 3)
        g_m, g_q, g_n = _guided.match_guided_device(md, uv, mn, desc_q, kpts_q, n_q, eye, 'homography', thr, min_cossim)
        g_q, g_m, g_trk = lists(g_q, g_m, g_n)
        second = absolute_pose.estimate_absolute_pose_matches(kpts_q, mp, g_q, g_m, g_n, K, **ransac)
        use = (out['info'][:, 0] != 0) & (second['info'][:, 0] != 0) & (second['info'][:, 3] >= out['info'][:, 3])
        pick = lambda a, b: torch.where(use.reshape((Q,) + (1,) * (a.dim() - 1)), b, a)
        out = {k: pick(out[k], second[k]) for k in out}
        i_q, i_m, trk, n = pick(i_q, g_q), pick(i_m, g_m), pick(trk, g_trk), pick(n, g_n)
        stage = torch.where(use, torch.full_like(stage, 2), stage)
    out.update(idx_query=i_q, idx_map=i_m, n_matches=n, track=trk, stage=stage)
    return out


def resect_views_batch(kpts, track_of, points3d, Ks, **ransac):
    """The poses of all V views of S scenes from the map's points at their own key-points: ``view_points`` for every view with one gather,
    then ``estimate_absolute_pose_batch`` over the S V (scene, view) problems.

    kpts (S,V,K,2) float32; track_of (S,V,K) int32 and points3d (S,T,3) float32 of ``triangulate_graph_matches`` /
    ``reconstruct_graph_matches``; Ks (S,V,3,3) float64; **ransac: the estimator's settings.  A key-point without a track, or whose track has no
    point, is a NaN row: never sampled, never an inlier.  Returns a dict: 'Rs' (S,V,3,3), 'ts' (S,V,3) float64 (zeros where nothing was
    found), 'inliers' (S,V,K) uint8, 'info' (S,V,8) int32 (absolute_pose.INFO_FIELDS).  The caller fills the NaN poses of the views a pose
    graph left out with the poses it gets for them.  Asynchronous."""
    kpts, track_of, points3d = torch.as_tensor(kpts), torch.as_tensor(track_of), torch.as_tensor(points3d)
    if kpts.dim() != 4 or kpts.shape[3] != 2:
        raise RuntimeError('expected kpts (S,V,K,2)')
    S, V, K = kpts.shape[:3]
    if track_of.shape != (S, V, K) or points3d.dim() != 3 or points3d.shape[0] != S or points3d.shape[2] != 3:
        raise RuntimeError('expected track_of (S,V,K) and points3d (S,T,3) for kpts (S,V,K,2)')
    Ks = torch.as_tensor(Ks, dtype=torch.float64)
    if Ks.shape != (S, V, 3, 3):
        raise RuntimeError('Ks must be (S,V,3,3)')
    dev = kpts.device if kpts.is_cuda else _twoview.device("view resection")
    T = points3d.shape[1]
    t = track_of.to(dev).long().reshape(S, V * K)
    has = (t >= 0) & (t < T)
    X = torch.full((S, V * K, 3), float('nan'), dtype=torch.float32, device=dev)
    if T:
        got = torch.gather(points3d.to(dev).float(), 1, t.clamp(0, T - 1).unsqueeze(-1).expand(-1, -1, 3))
        X = torch.where(has.unsqueeze(-1), got, X)
    r = absolute_pose.estimate_absolute_pose_batch(kpts.to(dev).float().reshape(S * V, K, 2), X.reshape(S * V, K, 3), None, Ks.reshape(S * V, 3, 3), **ransac)
    return {'Rs': r['R'].reshape(S, V, 3, 3), 'ts': r['t'].reshape(S, V, 3), 'inliers': r['inliers'].reshape(S, V, K), 'info': r['info'].reshape(S, V, 8)}
