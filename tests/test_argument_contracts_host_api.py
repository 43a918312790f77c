"""The argument contracts that the geometry entries of the C ABI and the scene-batched Python wrappers (multiview.py, verification.py,
localization.py) have in common, pinned to the byte: the return code and the whole ``xfh_last_error()`` text of every check that several
entries share, which of two violated checks is reported, and the type and full message of the wrappers' shared exceptions.  Every call
below fails an argument check, which returns before any launch: the pointers are never dereferenced and no GPU is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

ARG, UNSUPPORTED, WORKSPACE = -1, -4, -3                     # XFH_ERR_ARG, XFH_ERR_UNSUPPORTED, XFH_ERR_WORKSPACE
INF, NAN = float("inf"), float("nan")
X = C.c_void_p(256)                                         # never dereferenced
THRESHOLDS = (C.c_double * 2)(1.0, 2.0)                     # the one argument an entry reads on the host (the sweep's thresholds)

# entry -> (the order of its arguments, the values that pass every check); a name without a value is the pointer X, `stream` is NULL and
# `nbytes` (of the workspace) is large
_RANSAC = dict(n=0, P=2, cap=64, kcap=128, cap2=128, cap3=96, thr=1.0, min_iters=20, iters=100, prob=0.999, conf=0.99, seed=1, T=2, method=1, with_scale=1,
               thrs=C.cast(THRESHOLDS, C.c_void_p))
_SCENES = dict(S=2, P=3, V=3, K=16, T=8, cap=8, kcap=16, thr=4.0, cos_min=0.5, max_depth=INF, min_views=2, min_length=2, max_tracks=24, fixed=1, iters=10,
               huber=1.0, it=30, rd=10, rot=0.03, pos=0.03, piv=1e-8, sw=1.0, stol=0.1, min_common=8, max_points=8)
ENTRIES = {
    "xfh_find_homography": ("pts0 pts1 counts n P cap thr iters conf seed H mask info ws nbytes stream", _RANSAC),
    "xfh_find_homography_matches": ("kpts0 kpts1 kcap idx0 idx1 nm P cap thr iters conf seed H mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_relpose": ("pts0 pts1 counts n P cap K0 K1 thr min_iters iters prob seed R t E mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_relpose_matches": ("kpts0 kpts1 kcap idx0 idx1 nm P cap K0 K1 thr min_iters iters prob seed R t E mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_relpose_sweep": ("pts0 pts1 counts n P cap K0 K1 thrs T min_iters iters prob seed R t E mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_relpose_sweep_matches": ("kpts0 kpts1 kcap idx0 idx1 nm P cap K0 K1 thrs T min_iters iters prob seed R t E mask info ws nbytes stream",
                                           _RANSAC),
    "xfh_estimate_abspose": ("pts2d pts3d counts n P cap K thr min_iters iters prob seed R t mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_abspose_matches": ("kpts2d cap2 points3d cap3 idx2d idx3d nm P cap K thr min_iters iters prob seed R t mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_alignment": ("a b counts n P cap with_scale thr min_iters iters prob seed R t s mask info ws nbytes stream", _RANSAC),
    "xfh_estimate_alignment_matches": ("pa cap2 pb cap3 idx_a idx_b nm P cap with_scale thr min_iters iters prob seed R t s mask info ws nbytes stream",
                                       _RANSAC),
    "xfh_find_fundamental": ("pts0 pts1 counts n P cap method thr iters conf seed F mask info ws nbytes stream", _RANSAC),
    "xfh_find_fundamental_matches": ("kpts0 kpts1 kcap idx0 idx1 nm P cap method thr iters conf seed F mask info ws nbytes stream", _RANSAC),
    "xfh_triangulate": ("pts0 pts1 counts n P cap K0 K1 R t mask thr cos_min max_depth X status reproj info stream", dict(_SCENES, n=0)),
    "xfh_triangulate_matches": ("kpts0 kpts1 kcap idx0 idx1 nm P cap K0 K1 R t mask thr cos_min max_depth X status reproj info Xref stream", _SCENES),
    "xfh_triangulate_views": ("kpts kcap tracks n_views S K V Ks Rs ts thr cos_min max_depth min_views X status ninl inl reproj info stream", _SCENES),
    "xfh_triangulate_tracks": ("kpts kcap tracks n_views S K V Ks Rs ts thr cos_min max_depth min_views X status ninl inl reproj info stream", _SCENES),
    "xfh_build_tracks": ("idx_ref idx_view nm S V cap K kcap tracks stream", _SCENES),
    "xfh_build_tracks_graph": ("vp idx_a idx_b nm S P cap V K min_length max_tracks tracks track_of n_tracks info ws nbytes stream", _SCENES),
    "xfh_bundle_adjust": ("kpts kcap tracks inl X n_views S K V Ks Rs ts fixed iters huber Ro to Xo refined free cost info ws nbytes stream", _SCENES),
    "xfh_average_poses": ("vp R t w n_views S P V it rd rot pos piv Ro to reg fac info ws nbytes stream", _SCENES),
    "xfh_baseline_ratios": ("kpts tracks track_of vp R t w Ks n_views S P V K T thr cos_min max_depth min_common ratio count shared info ws nbytes stream",
                            _SCENES),
    "xfh_average_poses_ratios": ("vp R t w n_views ratio rcount S P V it rd rot pos piv sw stol Ro to reg fac rfac info ws nbytes stream", _SCENES),
    "xfh_build_map": ("desc kcap tracks X status inl S T V min_views max_points points mdesc m16 track n_obs coh n_points info ws nbytes stream", _SCENES),
    "xfh_verify_matches": ("kpts vp idx_a idx_b nm n_views S P cap V K Ks Rs ts thr mask err info stream", _SCENES),
}
ESTIMATORS = [e for e in ENTRIES if ENTRIES[e][1] is _RANSAC]
LISTS = [e for e in ESTIMATORS if not e.endswith("_matches")]           # (P, cap) point lists with counts or one constant count
SCENES = ["xfh_build_tracks", "xfh_triangulate_views", "xfh_triangulate_tracks", "xfh_build_tracks_graph", "xfh_bundle_adjust", "xfh_average_poses",
          "xfh_baseline_ratios", "xfh_average_poses_ratios", "xfh_build_map", "xfh_verify_matches"]
VIEWS = SCENES[:8]                                          # (the map and the verification word their view counts differently: below)
MAX_ITERS = [e for e in ESTIMATORS if "homography" not in e]            # (the homography's limit is 4096)
GATES = ["xfh_triangulate", "xfh_triangulate_matches", "xfh_triangulate_views", "xfh_triangulate_tracks"]
POSE_GRAPH = ["xfh_average_poses", "xfh_average_poses_ratios"]


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def answer(lib, entry, **kw):
    """(return code, the text of xfh_last_error()) of one call of `entry` with the passing values but for `kw`."""
    order, values = ENTRIES[entry]
    given = dict({"stream": None, "nbytes": 1 << 40}, **values)
    given.update(kw)
    rc = getattr(lib, entry)(*[given.get(name, X) for name in order.split()])
    return rc, lib.xfh_last_error().decode()


def test_the_scene_count_is_checked_with_one_text(lib):
    assert len(SCENES) == 10
    for e in SCENES:
        assert answer(lib, e, S=0) == (ARG, "%s: S 0 outside [1, 65535]" % e), e
        assert answer(lib, e, S=65536) == (ARG, "%s: S 65536 outside [1, 65535]" % e), e
        assert answer(lib, e, S=-3, V=40) == (ARG, "%s: S -3 outside [1, 65535]" % e), e           # the scenes come before the views


def test_the_view_count_is_checked_with_one_text(lib):
    for e in VIEWS:
        assert answer(lib, e, V=1) == (ARG, "%s: V 1 outside [2, 32]" % e), e
        assert answer(lib, e, V=33) == (ARG, "%s: V 33 outside [2, 32]" % e), e
    # the views come before the shapes and the settings that follow them
    assert answer(lib, "xfh_build_tracks", V=33, K=0) == (ARG, "xfh_build_tracks: V 33 outside [2, 32]")
    assert answer(lib, "xfh_triangulate_views", V=33, K=0) == (ARG, "xfh_triangulate_views: V 33 outside [2, 32]")
    assert answer(lib, "xfh_build_tracks_graph", V=33, P=0) == (ARG, "xfh_build_tracks_graph: V 33 outside [2, 32]")
    assert answer(lib, "xfh_bundle_adjust", V=33, K=0) == (ARG, "xfh_bundle_adjust: V 33 outside [2, 32]")
    assert answer(lib, "xfh_average_poses", V=33, P=0) == (ARG, "xfh_average_poses: V 33 outside [2, 32]")
    assert answer(lib, "xfh_baseline_ratios", V=33, P=0) == (ARG, "xfh_baseline_ratios: V 33 outside [2, 32]")
    assert answer(lib, "xfh_average_poses_ratios", V=33, P=0) == (ARG, "xfh_average_poses_ratios: V 33 outside [2, 32]")
    # the two entries that say something else keep their words and their codes
    assert answer(lib, "xfh_build_map", V=0) == (ARG, "xfh_build_map: V 0 below 1")
    assert answer(lib, "xfh_build_map", V=33) == (UNSUPPORTED, "xfh_build_map: V 33 above 32")
    assert answer(lib, "xfh_build_map", V=1, T=0) == (ARG, "xfh_build_map: bad shape (T 0, key-point capacity 16)")      # one view is a map
    assert answer(lib, "xfh_verify_matches", V=1) == (ARG, "xfh_verify_matches: V 1 below 2")
    assert answer(lib, "xfh_verify_matches", V=33) == (UNSUPPORTED, "xfh_verify_matches: V 33 above 32")


def test_the_shapes_that_follow_the_views_keep_their_texts(lib):
    big = (1 << 24) + 1
    assert answer(lib, "xfh_build_tracks", K=big) == (ARG, "xfh_build_tracks: bad shape (cap 8, K 16777217, key-point capacity 16)")
    assert answer(lib, "xfh_build_tracks", cap=big) == (ARG, "xfh_build_tracks: bad shape (cap 16777217, K 16, key-point capacity 16)")
    for e in ("xfh_triangulate_views", "xfh_triangulate_tracks", "xfh_bundle_adjust"):
        assert answer(lib, e, K=big) == (ARG, "%s: bad shape (K 16777217, key-point capacity 16)" % e), e
    for e in ("xfh_build_tracks_graph", "xfh_verify_matches"):
        assert answer(lib, e, P=65536) == (ARG, "%s: bad shape (P 65536, cap 8, K 16)" % e), e
        assert answer(lib, e, cap=big) == (ARG, "%s: bad shape (P 3, cap 16777217, K 16)" % e), e
        assert answer(lib, e, K=big) == (ARG, "%s: bad shape (P 3, cap 8, K 16777217)" % e), e
    assert answer(lib, "xfh_average_poses", P=(1 << 20) + 1) == (ARG, "xfh_average_poses: P 1048577 outside [1, 2^20]")
    assert answer(lib, "xfh_build_map", T=big) == (ARG, "xfh_build_map: bad shape (T 16777217, key-point capacity 16)")
    assert answer(lib, "xfh_build_map", max_points=big) == (ARG, "xfh_build_map: max_points 16777217 outside [1, 2^24]")
    assert answer(lib, "xfh_triangulate_views", min_views=33) == (ARG, "xfh_triangulate_views: min_views 33 outside [2, 32]")
    assert answer(lib, "xfh_build_tracks_graph", min_length=33) == (ARG, "xfh_build_tracks_graph: min_length 33 outside [2, 32]")
    assert answer(lib, "xfh_build_map", min_views=33) == (ARG, "xfh_build_map: min_views 33 outside [1, 32]")
    for e in ("xfh_triangulate", "xfh_triangulate_matches"):
        assert answer(lib, e, P=65536) == (ARG, "%s: P 65536 outside [1, 65535]" % e), e
    assert answer(lib, "xfh_triangulate", cap=big) == (ARG, "xfh_triangulate: bad shape (cap 16777217, key-point capacity 16777217, n 0)")
    assert answer(lib, "xfh_triangulate_matches", cap=big) == (ARG, "xfh_triangulate_matches: bad shape (cap 16777217, key-point capacity 16, n 0)")


def test_the_workspace_sizes_are_zero_beyond_the_same_limits(lib):
    big = (1 << 24) + 1
    f = lib.xfh_track_graph_workspace_bytes
    assert f(65535, 32, 16) > 0 and f(65536, 32, 16) == 0 and f(2, 33, 16) == 0 and f(2, 1, 16) == 0 and f(2, 3, big) == 0 and f(1, 2, 1 << 24) > 0
    f = lib.xfh_bundle_workspace_bytes
    assert f(65535, 16, 32) > 0 and f(65536, 16, 32) == 0 and f(2, 16, 33) == 0 and f(2, 16, 1) == 0 and f(2, big, 3) == 0
    f = lib.xfh_pose_graph_workspace_bytes
    assert f(65535, 3, 32) > 0 and f(65536, 3, 32) == 0 and f(2, 3, 33) == 0 and f(2, 3, 1) == 0
    f = lib.xfh_baseline_ratios_workspace_bytes
    assert f(65535, 3, 32, 16) == 256 and f(65536, 3, 32, 16) == 0 and f(2, 3, 33, 16) == 0 and f(2, 3, 1, 16) == 0
    f = lib.xfh_pose_graph_ratios_workspace_bytes
    assert f(65535, 3, 32) > 0 and f(65536, 3, 32) == 0 and f(2, 3, 33) == 0 and f(2, 3, 1) == 0
    f = lib.xfh_map_workspace_bytes
    assert f(65535, 8, 32) > 0 and f(65536, 8, 32) == 0 and f(2, 8, 33) == 0 and f(2, 8, 1) > 0 and f(2, 8, 0) == 0 and f(2, big, 3) == 0


def test_the_estimators_check_their_shapes_with_one_text(lib):
    big = (1 << 24) + 1
    assert len(ESTIMATORS) == 12 and len(LISTS) == 6
    for e in ESTIMATORS:
        assert answer(lib, e, P=0) == (ARG, "%s: bad shape (P 0, cap 64, n 0)" % e), e
        assert answer(lib, e, P=65536) == (ARG, "%s: bad shape (P 65536, cap 64, n 0)" % e), e
        assert answer(lib, e, cap=0) == (ARG, "%s: bad shape (P 2, cap 0, n 0)" % e), e
        assert answer(lib, e, cap=big) == (ARG, "%s: bad shape (P 2, cap 16777217, n 0)" % e), e
        assert answer(lib, e, P=65535, cap=1 << 24, iters=0)[1].startswith("%s: max_iters 0 outside [1, " % e), e      # both limits are inside
        # the shape comes before the settings and the iteration limit
        assert answer(lib, e, P=0, thr=0.0, iters=0) == (ARG, "%s: bad shape (P 0, cap 64, n 0)" % e), e
    for e in LISTS:                                         # one constant count for every pair: within [0, cap]
        assert answer(lib, e, counts=None, n=65) == (ARG, "%s: bad shape (P 2, cap 64, n 65)" % e), e
        assert answer(lib, e, counts=None, n=-1) == (ARG, "%s: bad shape (P 2, cap 64, n -1)" % e), e
        assert answer(lib, e, n=65, iters=0)[1].startswith("%s: max_iters 0 outside [1, " % e), e      # with counts the constant is not read
    for e in ("xfh_find_homography_matches", "xfh_estimate_relpose_matches", "xfh_estimate_relpose_sweep_matches", "xfh_find_fundamental_matches"):
        assert answer(lib, e, kcap=0) == (ARG, "%s: bad shape (P 2, cap 64, n 0)" % e), e
    for e in ("xfh_estimate_abspose_matches", "xfh_estimate_alignment_matches"):       # two tables, two capacities
        assert answer(lib, e, cap2=0) == (ARG, "%s: bad shape (P 2, cap 64, n 0)" % e), e
        assert answer(lib, e, cap3=0) == (ARG, "%s: bad shape (P 2, cap 64, n 0)" % e), e
        assert answer(lib, e, cap2=1, cap3=1, iters=0) == (UNSUPPORTED, "%s: max_iters 0 outside [1, 16384]" % e), e


def test_the_iteration_limit_is_checked_with_one_text(lib):
    assert len(MAX_ITERS) == 10
    for e in MAX_ITERS:
        assert answer(lib, e, iters=0) == (UNSUPPORTED, "%s: max_iters 0 outside [1, 16384]" % e), e
        assert answer(lib, e, iters=16385) == (UNSUPPORTED, "%s: max_iters 16385 outside [1, 16384]" % e), e
        rc, text = answer(lib, e, iters=16384, ws=None)     # the limit itself is inside: the next check answers
        assert rc == WORKSPACE and text.startswith("workspace is NULL (need "), e
        # the settings come before the iteration limit
        rc, text = answer(lib, e, iters=0, prob=1.0, conf=1.0)
        assert rc == ARG and "max_iters" not in text and text.startswith(e + ": "), e
    for e in ("xfh_find_homography", "xfh_find_homography_matches"):
        assert answer(lib, e, iters=4097) == (UNSUPPORTED, "%s: max_iters 4097 outside [1, 4096]" % e), e


def test_the_gates_of_the_triangulations_are_checked_in_one_order(lib):
    for e in GATES:
        for v, s in ((0.0, "0"), (-1.0, "-1"), (INF, "inf"), (NAN, "nan")):
            assert answer(lib, e, thr=v) == (ARG, "%s: max_reproj_error %s must be positive and finite" % (e, s)), (e, v)
        for v, s in ((0.0, "0"), (-2.0, "-2"), (NAN, "nan")):
            assert answer(lib, e, max_depth=v) == (ARG, "%s: max_depth %s must be positive (+inf: no limit)" % (e, s)), (e, v)
        for v, s in ((1.5, "1.5"), (-1.5, "-1.5"), (NAN, "nan")):
            assert answer(lib, e, cos_min=v) == (ARG, "%s: cos_min %s outside [-1, 1]" % (e, s)), (e, v)
        # error, depth, parallax: in that order
        assert answer(lib, e, thr=0.0, max_depth=0.0, cos_min=2.0) == (ARG, "%s: max_reproj_error 0 must be positive and finite" % e), e
        assert answer(lib, e, max_depth=0.0, cos_min=2.0) == (ARG, "%s: max_depth 0 must be positive (+inf: no limit)" % e), e
    for e in GATES[2:]:                                     # the shapes and min_views come first
        assert answer(lib, e, min_views=1, thr=0.0) == (ARG, "%s: min_views 1 outside [2, 32]" % e), e
        assert answer(lib, e, K=0, thr=0.0) == (ARG, "%s: bad shape (K 0, key-point capacity 16)" % e), e
    for e in GATES[:2]:
        assert answer(lib, e, P=0, thr=0.0) == (ARG, "%s: P 0 outside [1, 65535]" % e), e
    # the baseline ratios word the first gate differently (no upper limit) and have depth and parallax the other way round
    e = "xfh_baseline_ratios"
    assert answer(lib, e, thr=0.0) == (ARG, "xfh_baseline_ratios: max_reproj_error 0 must be positive")
    assert answer(lib, e, thr=NAN) == (ARG, "xfh_baseline_ratios: max_reproj_error nan must be positive")
    assert answer(lib, e, thr=INF, min_common=0) == (ARG, "xfh_baseline_ratios: min_common 0 below 1")
    assert answer(lib, e, cos_min=2.0, max_depth=0.0) == (ARG, "xfh_baseline_ratios: cos_min 2 outside [-1, 1]")
    assert answer(lib, e, max_depth=0.0) == (ARG, "xfh_baseline_ratios: max_depth 0 must be positive (+inf: no limit)")


def test_the_settings_of_the_pose_graph_are_checked_in_one_order(lib):
    for e in POSE_GRAPH:
        for kw, text in ((dict(it=0), "iterations 0 outside [1, 1000]"), (dict(it=1001), "iterations 1001 outside [1, 1000]"),
                         (dict(rd=-1), "redescend -1 outside [0, iterations]"), (dict(rd=31), "redescend 31 outside [0, iterations]"),
                         (dict(rot=0.0), "rot_scale_rad 0 outside (0, 4)"), (dict(rot=4.0), "rot_scale_rad 4 outside (0, 4)"),
                         (dict(rot=NAN), "rot_scale_rad nan outside (0, 4)"), (dict(pos=0.0), "pos_scale_sin 0 outside (0, 1]"),
                         (dict(pos=1.5), "pos_scale_sin 1.5 outside (0, 1]"), (dict(pos=NAN), "pos_scale_sin nan outside (0, 1]"),
                         (dict(piv=-0.5), "min_pivot_ratio -0.5 outside [0, 1)"), (dict(piv=1.0), "min_pivot_ratio 1 outside [0, 1)"),
                         (dict(piv=NAN), "min_pivot_ratio nan outside [0, 1)"),
                         # iterations, redescend, rotation scale, position scale, pivot ratio: in that order
                         (dict(it=0, rd=-1), "iterations 0 outside [1, 1000]"), (dict(rd=-1, rot=0.0), "redescend -1 outside [0, iterations]"),
                         (dict(rot=0.0, pos=0.0), "rot_scale_rad 0 outside (0, 4)"), (dict(pos=0.0, piv=1.0), "pos_scale_sin 0 outside (0, 1]"),
                         (dict(it=0, piv=1.0), "iterations 0 outside [1, 1000]")):
            assert answer(lib, e, **kw) == (ARG, "%s: %s" % (e, text)), (e, kw)
        assert answer(lib, e, P=0, it=0) == (ARG, "%s: P 0 outside [1, %s]" % (e, "2^20" if e == "xfh_average_poses" else "512")), e
    e = "xfh_average_poses_ratios"                          # its own two settings follow the shared five
    assert answer(lib, e, piv=1.0, sw=0.0) == (ARG, "xfh_average_poses_ratios: min_pivot_ratio 1 outside [0, 1)")
    assert answer(lib, e, sw=0.0, stol=0.0) == (ARG, "xfh_average_poses_ratios: scale_weight 0 must be positive and finite")
    assert answer(lib, e, stol=1.5) == (ARG, "xfh_average_poses_ratios: scale_tol 1.5 outside (0, 1]")


# ---- the Python wrappers: everything that is raised before the device is asked for ----------------------------------------------------------
def raises(kind, text, fn, *args, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind and str(e.value) == text, (str(e.value), text)


def _graph(S=2, V=3, K=8, P=4, cap=5):
    """kpts, view_pairs, idx_a, idx_b, n_matches of a pair graph."""
    return [torch.zeros((S, V, K, 2)), torch.zeros((P, 2), dtype=torch.int32), torch.zeros((S, P, cap), dtype=torch.int64),
            torch.zeros((S, P, cap), dtype=torch.int64), torch.zeros((S, P), dtype=torch.int32)]


def _edges(S=2, P=4):
    """view_pairs, R_rel, t_rel, weight."""
    return [np.zeros((S, P, 2), np.int32), np.tile(np.eye(3), (S, P, 1, 1)), np.ones((S, P, 3)), np.ones((S, P))]


def test_the_wrappers_ask_for_tensors_with_one_text():
    from accelerated_features_amd import localization as loc, multiview as mv, verification as ver
    k, vp, ia, ib, nm = _graph()
    for i in range(3):
        a = [ia[:, :2], ib[:, :2], nm[:, :2]]
        a[i] = a[i].numpy()
        raises(RuntimeError, "build_tracks: tensors expected", mv.build_tracks, *a, 8)
    for i in range(4):
        a = [vp, ia, ib, nm]
        a[i] = a[i].numpy()
        raises(RuntimeError, "build_tracks_graph: tensors expected", mv.build_tracks_graph, *a, 3, 8)
    for i in range(5):
        a = _graph()
        a[i] = a[i].numpy()
        raises(RuntimeError, "relative_poses_graph_matches: tensors expected", mv.relative_poses_graph_matches, *a, np.zeros((2, 3, 3, 3)))
        raises(RuntimeError, "verify_matches_graph: tensors expected", ver.verify_matches_graph, *a, None, *[np.zeros((2, 3, 3, 3))] * 3)
    tracks, track_of = torch.zeros((2, 6, 3), dtype=torch.int32), torch.zeros((2, 3, 8), dtype=torch.int32)
    for i in range(3):
        a = [k, tracks, track_of]
        a[i] = a[i].numpy()
        raises(RuntimeError, "baseline_ratios_batch: tensors expected", mv.baseline_ratios_batch, *a, *_edges(), np.zeros((2, 3, 3, 3)))
    mask = torch.ones((2, 4, 5), dtype=torch.uint8)
    for i in range(4):
        a = [ia, ib, nm, mask]
        a[i] = a[i].numpy()
        raises(RuntimeError, "filter_matches_batch: tensors expected", ver.filter_matches_batch, *a)
    raises(RuntimeError, "filter_matches_batch: tensors expected", ver.filter_matches_batch, ia, ib, nm, mask, keep=np.ones((2, 4), np.uint8))
    q = [torch.zeros((2, 8, 2)), torch.zeros((2, 8, 64)), torch.zeros((2,), dtype=torch.int32)]
    m = {'points': torch.zeros((2, 6, 3)), 'desc': torch.zeros((2, 6, 64)), 'desc_f16': torch.zeros((2, 6, 64), dtype=torch.float16),
         'track': torch.zeros((2, 6), dtype=torch.int32), 'n_points': torch.zeros((2,), dtype=torch.int32)}
    for i in range(3):
        a = list(q)
        a[i] = a[i].numpy()
        raises(RuntimeError, "localize_map_batch: tensors expected", loc.localize_map_batch, *a, m, np.eye(3))
    for key in m:
        raises(RuntimeError, "localize_map_batch: tensors expected", loc.localize_map_batch, *q, dict(m, **{key: m[key].numpy()}), np.eye(3))
    raises(RuntimeError, "localize_map_batch: map must be the dict of build_map_batch", loc.localize_map_batch, *q, {'points': m['points']}, np.eye(3))


def test_the_wrappers_check_key_points_and_tracks_with_one_text():
    from accelerated_features_amd import multiview as mv
    text = "expected kpts (S,V,Kcap,2) and tracks (S,K,V)"
    P = [np.zeros((2, 3, 3, 3)), np.zeros((2, 3, 3, 3)), np.zeros((2, 3, 3))]
    for k, t in ((np.zeros((2, 3, 8, 3), np.float32), np.zeros((2, 6, 3), np.int32)), (np.zeros((2, 3, 8), np.float32), np.zeros((2, 6, 3), np.int32)),
                 (np.zeros((2, 3, 8, 2), np.float32), np.zeros((2, 6), np.int32)), (np.zeros((2, 3, 8, 2), np.float32), np.zeros((1, 6, 3), np.int32)),
                 (np.zeros((2, 3, 8, 2), np.float32), np.zeros((2, 6, 4), np.int32))):
        raises(RuntimeError, text, mv.triangulate_views_batch, k, t, None, *P)
        raises(RuntimeError, text, mv.bundle_adjust_batch, k, t, np.zeros((2, 6), np.int32), np.zeros((2, 6, 3), np.float32), None, *P)
    k, t = np.zeros((2, 33, 8, 2), np.float32), np.zeros((2, 6, 33), np.int32)
    P33 = [np.zeros((2, 33, 3, 3)), np.zeros((2, 33, 3, 3)), np.zeros((2, 33, 3))]
    raises(mv._lib.XFeatHipError, "triangulate_views_batch: V 33 outside [2, 32]", mv.triangulate_views_batch, k, t, None, *P33)
    raises(mv._lib.XFeatHipError, "bundle_adjust_batch: V 33 outside [2, 32]", mv.bundle_adjust_batch, k, t, np.zeros((2, 6), np.int32),
           np.zeros((2, 6, 3), np.float32), None, *P33)
    # the settings come before the shapes, and the shapes of the adjustment's own inputs after the shared ones
    raises(mv._lib.XFeatHipError, "triangulate_views_batch: max_reproj_error 0.0 must be positive and finite", mv.triangulate_views_batch,
           np.zeros((2, 3, 8, 3), np.float32), np.zeros((2, 6, 3), np.int32), None, *P, max_reproj_error=0.0)
    raises(RuntimeError, "expected inlier_views (S,K) and points3d (S,K,3)", mv.bundle_adjust_batch, np.zeros((2, 3, 8, 2), np.float32),
           np.zeros((2, 6, 3), np.int32), np.zeros((2, 5), np.int32), np.zeros((2, 6, 3), np.float32), None, *P)
    if not torch.cuda.is_available():                      # the device is asked for before n_views and the poses are looked at
        for fn, what, extra in ((mv.triangulate_views_batch, "multi-view triangulation", ()),
                                (mv.bundle_adjust_batch, "bundle adjustment", (np.zeros((2, 6), np.int32), np.zeros((2, 6, 3), np.float32)))):
            raises(mv._lib.XFeatHipError, what + " needs an AMD MI355X (gfx950) GPU; no CPU fallback exists", fn, np.zeros((2, 3, 8, 2), np.float32),
                   np.zeros((2, 6, 3), np.int32), *extra, np.zeros((3,), np.int32), *P[:2], np.zeros((2, 3, 4)))


def test_the_wrappers_check_the_view_pairs_with_one_text():
    from accelerated_features_amd import multiview as mv, verification as ver
    text = "expected view_pairs (S,P,2) or (P,2)"
    Ks = np.zeros((2, 3, 3, 3))
    for bad in (torch.zeros((3, 2), dtype=torch.int32), torch.zeros((2, 4, 3), dtype=torch.int32), torch.zeros((1, 4, 2), dtype=torch.int32),
                torch.zeros((4,), dtype=torch.int32)):
        k, _, ia, ib, nm = _graph()
        raises(RuntimeError, text, mv.build_tracks_graph, bad, ia, ib, nm, 3, 8)
        raises(RuntimeError, text, mv.relative_poses_graph_matches, k, bad, ia, ib, nm, Ks)
        raises(RuntimeError, text, ver.verify_matches_graph, k, bad, ia, ib, nm, None, Ks, Ks, np.zeros((2, 3, 3)))
        raises(RuntimeError, text, mv.average_poses_batch, bad.numpy(), *_edges()[1:], 3)
        raises(RuntimeError, text, mv.baseline_ratios_batch, k, torch.zeros((2, 6, 3), dtype=torch.int32), torch.zeros((2, 3, 8), dtype=torch.int32),
               bad.numpy(), *_edges()[1:], Ks)
    # what is checked before the pairs, and what after them
    k, vp, ia, ib, nm = _graph()
    bad = torch.zeros((3, 2), dtype=torch.int32)
    raises(RuntimeError, "expected idx_a, idx_b (S,P,cap) and n_matches (S,P)", mv.build_tracks_graph, bad, ia, ib[:, :3], nm, 3, 8)
    raises(mv._lib.XFeatHipError, "build_tracks_graph: V 33 outside [2, 32]", mv.build_tracks_graph, bad, ia, ib, nm, 33, 8)
    raises(mv._lib.XFeatHipError, "build_tracks_graph: min_length 1 outside [2, 32]", mv.build_tracks_graph, vp, ia, ib, nm, 3, 8, min_length=1)
    raises(RuntimeError, "expected idx_a, idx_b (S,P,cap) and n_matches (S,P) for kpts (S,V,K,2)", mv.relative_poses_graph_matches, k, bad, ia, ib[:, :3],
           nm, Ks)
    raises(mv._lib.XFeatHipError, "relative_poses_graph_matches: min_inliers -1 is negative", mv.relative_poses_graph_matches, k, vp, ia, ib, nm, Ks,
           min_inliers=-1)
    raises(RuntimeError, "expected idx_a, idx_b (S,P,cap) and n_matches (S,P) for kpts (S,V,K,2)", ver.verify_matches_graph, k, bad, ia, ib[:, :3], nm, None,
           Ks, Ks, np.zeros((2, 3, 3)))
    raises(mv._lib.XFeatHipError, "verify_matches_graph: max_epipolar_error 0.0 must be positive and finite", ver.verify_matches_graph, k, vp, ia, ib, nm, None,
           Ks, Ks, np.zeros((2, 3, 3)), max_epipolar_error=0.0)


def test_the_wrappers_check_the_edges_with_one_text():
    from accelerated_features_amd import multiview as mv
    k, tracks, track_of = torch.zeros((2, 3, 8, 2)), torch.zeros((2, 6, 3), dtype=torch.int32), torch.zeros((2, 3, 8), dtype=torch.int32)
    Ks = np.zeros((2, 3, 3, 3))
    for i, bad, text in ((1, np.zeros((2, 4, 3, 2)), "expected R_rel (S,P,3,3)"), (1, np.zeros((2, 4, 3)), "expected R_rel (S,P,3,3)"),
                         (2, np.zeros((2, 4, 2)), "expected t_rel (S,P,3) and weight (S,P)"), (2, np.zeros((2, 5, 3)), "expected t_rel (S,P,3) and weight (S,P)"),
                         (3, np.zeros((2, 5)), "expected t_rel (S,P,3) and weight (S,P)"), (3, np.zeros((1, 4)), "expected t_rel (S,P,3) and weight (S,P)")):
        a = _edges()
        a[i] = bad
        raises(RuntimeError, text, mv.average_poses_batch, *a, 3)
        raises(RuntimeError, text, mv.baseline_ratios_batch, k, tracks, track_of, *a, Ks)
    # rotations before translations and weights, those before the pairs; the ratios also want the scenes of the key-points
    a = _edges()
    a[0], a[1], a[2] = np.zeros((3, 2), np.int32), np.zeros((2, 4, 2, 3)), np.zeros((2, 4, 2))
    raises(RuntimeError, "expected R_rel (S,P,3,3)", mv.average_poses_batch, *a, 3)
    raises(RuntimeError, "expected R_rel (S,P,3,3)", mv.baseline_ratios_batch, k, tracks, track_of, *a, Ks)
    a[1] = np.zeros((2, 4, 3, 3))
    raises(RuntimeError, "expected t_rel (S,P,3) and weight (S,P)", mv.average_poses_batch, *a, 3)
    raises(RuntimeError, "expected t_rel (S,P,3) and weight (S,P)", mv.baseline_ratios_batch, k, tracks, track_of, *a, Ks)
    raises(RuntimeError, "expected R_rel (S,P,3,3)", mv.baseline_ratios_batch, k, tracks, track_of, *_edges(S=3), Ks)
    raises(RuntimeError, "n_views per scene needs the keyword V", mv.average_poses_batch, *_edges(), torch.zeros(2, dtype=torch.int32))
    raises(RuntimeError, "n_views must have one entry per scene", mv.average_poses_batch, *_edges(), torch.zeros(3, dtype=torch.int32), V=3)
    raises(mv._lib.XFeatHipError, "average_poses_batch: V 33 outside [2, 32]", mv.average_poses_batch, *_edges(), 33)
    raises(mv._lib.XFeatHipError, "average_poses_batch: iterations 0 outside [1, 1000]", mv.average_poses_batch, np.zeros((3, 2), np.int32), *_edges()[1:], 3,
           iterations=0)


def test_the_wrappers_check_the_views_per_scene_and_the_cameras_with_one_text():
    """Where the tensors decide the device (the baseline ratios, the verification of an empty graph) the checks behind it are reached here."""
    from accelerated_features_amd import multiview as mv, verification as ver
    k, tracks, track_of = torch.zeros((2, 3, 8, 2)), torch.zeros((2, 6, 3), dtype=torch.int32), torch.zeros((2, 3, 8), dtype=torch.int32)
    Ks, ts = np.zeros((2, 3, 3, 3)), np.zeros((2, 3, 3))
    for nv in (torch.zeros(3, dtype=torch.int32), np.zeros((2, 1), np.int32)):
        raises(RuntimeError, "n_views must have one entry per scene", mv.baseline_ratios_batch, k, tracks, track_of, *_edges(), Ks, nv)
        raises(RuntimeError, "n_views must have one entry per scene", ver.verify_matches_graph, *_graph(cap=0), nv, Ks, Ks, ts)
    raises(RuntimeError, "Ks must be (2, 3, 3, 3)", mv.baseline_ratios_batch, k, tracks, track_of, *_edges(), np.zeros((2, 3, 3)), [3, 3])
    raises(RuntimeError, "Ks must be (2, 3, 3, 3)", ver.verify_matches_graph, *_graph(cap=0), [3, 3], np.zeros((3, 3)), Ks, ts)
    raises(RuntimeError, "Rs must be (2, 3, 3, 3)", ver.verify_matches_graph, *_graph(cap=0), None, Ks, ts, ts)
    raises(RuntimeError, "ts must be (2, 3, 3)", ver.verify_matches_graph, *_graph(cap=0), None, Ks, Ks, Ks)
    # the views per scene come before the cameras, the dtype of the tables before both
    raises(RuntimeError, "n_views must have one entry per scene", ver.verify_matches_graph, *_graph(cap=0), [3], np.zeros((3, 3)), Ks, ts)
    raises(RuntimeError, "n_views must have one entry per scene", mv.baseline_ratios_batch, k, tracks, track_of, *_edges(), np.zeros((3, 3)), [3])
    raises(RuntimeError, "baseline_ratios_batch: tracks must be a contiguous torch.int32 tensor on the device of kpts", mv.baseline_ratios_batch, k,
           tracks.long(), track_of, *_edges(), Ks, [3])
    raises(RuntimeError, "verify_matches_graph: kpts must be a contiguous torch.float32 tensor on the device of kpts", ver.verify_matches_graph,
           *([_graph(cap=0)[0].double()] + _graph(cap=0)[1:]), [3], Ks, Ks, ts)
    # with every argument in order the shapes that need no library call come out on the host
    out = mv.baseline_ratios_batch(k, tracks[:, :0], track_of, *_edges(), Ks, [3, 2])
    assert out['ratio'].shape == (2, 4, 4) and bool(torch.isnan(out['ratio']).all()) and not out['count'].any() and bool((out['shared_view'] == -1).all())
    mask, err, info = ver.verify_matches_graph(*_graph(cap=0), [3, 2], Ks, Ks, ts)
    assert mask.shape == (2, 4, 0) and err.shape == (2, 4, 0) and info.shape == (2, 4, 4) and not info.any()


def test_the_limits_have_one_value_wherever_they_are_read():
    from accelerated_features_amd import absolute_pose, alignment, fundamental, localization as loc, multiview as mv, pose, verification as ver
    assert mv.MAX_VIEWS == ver.MAX_VIEWS == loc.MAX_VIEWS == 32 and mv.MAX_SCENES == ver.MAX_SCENES == loc.MAX_SCENES == 65535
    for m in (mv, loc, pose, absolute_pose, alignment, fundamental):
        assert m.WORKSPACE_LIMIT == 512 << 20, m.__name__
