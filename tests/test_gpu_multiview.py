"""xfh_build_tracks / xfh_triangulate_views (csrc/k_triangulate.hip) on the MI355X against the numpy restatement tests/multiview_reference.py
on the same inputs: status, n_inliers, inlier_views, info and tracks exactly, the points and the reprojection error as float32 bits (fp
contraction is off and fp64 division and square root are correctly rounded on both sides).  Through the restatement every comparison first
asserts that no track of its scene lies within relative 1e-9 of a gate or of a tie of its two best scores (multiview_reference.gate_margin),
so a last-bit difference could not flip a discrete output."""
import math

import numpy as np
import pytest
import torch

import abspose_reference as AR
import multiview_reference as MR
import multiview_support as MS
from twoview_support import check_common

pytestmark = pytest.mark.gpu
GATES = dict(max_reproj_error=2.0, min_parallax_deg=4.0, max_depth=1.3 * MS.DEPTH, min_views=2)


@pytest.fixture(scope="module")
def mv():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import multiview as m
    return m


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _same_f32(got, want):
    """float32 arrays equal as bits, any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _want(sc, gates):
    return MR.triangulate_views(sc["kpts"], sc["tracks"], sc["n_views"], sc["Ks"], sc["Rs"], sc["ts"], **gates)


def _scene(seed, V, K, gates=GATES, kcap=None):
    """A noisy scene (0.5 px) with planted outliers (also in the reference view: status 5), holes in the table and rows past it (tracks left
    with the 3 degrees of view 1 alone: status 6), a max_depth inside it (status 4), whose tracks are all clear of every gate and tie."""
    rng = np.random.default_rng(seed)
    for _ in range(50):
        sc = MS.arc_scene(rng, V, max(K, 1), noise=0.5, cam=seed, kcap=kcap)
        MS.plant_outliers(rng, sc, frac=0.4)
        off = rng.random(max(K, 1)) < 0.05
        sc["kpts"][0, :max(K, 1)][off] += 3.5              # (far more would saturate every score of the track: an exact tie)
        holes = rng.random(sc["tracks"].shape) < 0.06
        sc["tracks"][holes] = np.where(rng.random(holes.sum()) < 0.5, -1, sc["kpts"].shape[1] + 3)
        sc["tracks"] = sc["tracks"][:K]
        w = _want(sc, gates)
        if MR.gate_margin(w, gates["max_depth"]) > 1e-9:
            return sc, w
    raise AssertionError("no scene clear of its gates in 50 draws")


def _check(got, s, want):
    K = want["status"].shape[0]
    for k in ("status", "n_inliers", "inlier_views"):
        g = got[k][s].cpu().numpy()
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (k, np.nonzero(g != want[k])[0][:8])
    assert list(got["info"][s].cpu().numpy()) == list(want["info"]), (got["info"][s], want["info"])
    X, err, status = got["points3d"][s].cpu().numpy(), got["reproj_error"][s].cpu().numpy(), want["status"]
    assert X.shape == (K, 3) and _same_f32(X, want["points3d"]) and _same_f32(err, want["reproj_error"])
    assert np.isfinite(X[status == 0]).all() and np.isnan(X[status != 0]).all()
    assert np.array_equal(got["valid"][s].cpu().numpy(), status == 0)


def _batch(mv, scenes, gates=GATES, n_views=None):
    kp, tr, Ks, Rs, ts = (np.stack([sc[k] for sc in scenes]) for k in ("kpts", "tracks", "Ks", "Rs", "ts"))
    return mv.triangulate_views_batch(*_cuda(kp, tr), n_views, Ks, Rs, ts, **gates)


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 300])
def test_single_scene_equals_the_restatement(mv, K):
    """The wave and workgroup edges of a thread-per-track kernel and the ballot counts around them, at V = 3."""
    sc, want = _scene(100 + K, 3, K)
    got = _batch(mv, [sc])
    torch.cuda.synchronize()
    _check(got, 0, want)
    assert got["info"][0, 0] == K and got["points3d"].shape == (1, K, 3)
    if K == 300:
        assert (np.bincount(want["status"], minlength=7) > 0).sum() >= 4


@pytest.mark.parametrize("V", [2, 32])
def test_view_counts_at_both_ends(mv, V):
    """LDS staging with 2 and with 32 views; at 32 the mask's top bit (a negative inlier_views)."""
    gates = dict(GATES, min_parallax_deg=1.0) if V == 2 else GATES      # (view 1 is 3 degrees from view 0)
    sc, want = _scene(200 + V, V, 65, gates)
    got = _batch(mv, [sc], gates)
    torch.cuda.synchronize()
    _check(got, 0, want)
    assert (want["status"] == 0).sum() > 30
    if V == 32:
        assert (want["inlier_views"] < 0).any() and want["n_inliers"].max() >= 20
        assert (want["status"] == 0).sum() > 40


def test_ragged_batch_two_calls_and_n_views(mv):
    """S = 3 with different n_views and per-view key-point counts in tables of one capacity; n_views = None uses all V; two calls, equal bits."""
    V, K, kcap = 5, 130, 160
    nv, Ks_ = [3, 5, 2], [130, 70, 1]
    scenes, wants = [], []
    for s in range(3):
        sc, _ = _scene(300 + s, V, K, kcap=kcap)
        sc["tracks"][Ks_[s]:] = -1                         # this scene has fewer key-points
        sc["n_views"] = nv[s]
        scenes.append(sc)
        wants.append(_want(sc, GATES))
        assert MR.gate_margin(wants[-1], GATES["max_depth"]) > 1e-9
    got = _batch(mv, scenes, n_views=np.array(nv, np.int32))
    again = _batch(mv, scenes, n_views=np.array(nv, np.int32))
    torch.cuda.synchronize()
    for s in range(3):
        _check(got, s, wants[s])
        assert (wants[s]["status"][Ks_[s]:] == MR.UNOBSERVED).all() and (wants[s]["inlier_views"] >> nv[s] == 0).all()
    for k in got:
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), again[k].cpu().numpy().view(np.uint8)), k
    full = _batch(mv, scenes, n_views=None)
    for s in range(3):
        scenes[s]["n_views"] = V
        w = _want(scenes[s], GATES)
        if MR.gate_margin(w, GATES["max_depth"]) > 1e-9:
            _check(full, s, w)
    assert list(full["info"][1].cpu().numpy()) == list(wants[1]["info"])      # (scene 1 used all five views already)


def test_build_tracks_is_a_maximum_scatter(mv):
    rng = np.random.default_rng(7)
    for V, K, cap, dup in ((4, 300, 340, 40), (2, 65, 64, 0), (32, 70, 300, 20), (3, 1, 5, 4)):
        S = 3
        a, b, n = np.zeros((S, V - 1, cap), np.int64), np.zeros((S, V - 1, cap), np.int64), np.zeros((S, V - 1), np.int32)
        for s in range(S):
            sc = MS.arc_scene(rng, V, K)
            ia, ib, nn = MS.match_lists(rng, sc["tracks"], cap=max(cap, K + dup), dup=dup)
            a[s], b[s], n[s] = ia[:, :cap], ib[:, :cap], np.minimum(nn, cap)
            bad = rng.random((V - 1, cap)) < 0.05          # indices out of range on either side, duplicates of every kind
            a[s][bad] = rng.choice([-1, K, K + 7, -(1 << 40), 1 << 40], bad.sum())
            bad = rng.random((V - 1, cap)) < 0.05
            b[s][bad] = rng.choice([-1, K, 1 << 33], bad.sum())
            dupl = rng.random((V - 1, cap)) < 0.1
            a[s][dupl] = rng.integers(0, K, dupl.sum())
        n[S - 1, 0] = 0
        got = mv.build_tracks(*_cuda(a, b, n), K)
        again = mv.build_tracks(*_cuda(a, b, n), K)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and got.shape == (S, K, V) and torch.equal(got, again)
        for s in range(S):
            assert np.array_equal(got[s].cpu().numpy(), MR.build_tracks(a[s], b[s], n[s], K)), (V, K, s)
    e = mv.build_tracks(*_cuda(np.zeros((2, 2, 0), np.int64), np.zeros((2, 2, 0), np.int64), np.zeros((2, 2), np.int32)), 5)      # no match at all
    assert np.array_equal(e.cpu().numpy(), np.stack([MR.build_tracks(np.zeros((2, 0)), np.zeros((2, 0)), [0, 0], 5)] * 2))
    assert mv.build_tracks(*_cuda(a, b, n), 0).shape == (3, 0, 3) and mv.build_tracks(*_cuda(a[:0], b[:0], n[:0]), 4).shape == (0, 4, 3)


def test_matches_form_equals_the_batch_form_on_its_table(mv):
    rng = np.random.default_rng(11)
    V, K = 4, 300
    sc, want = _scene(400, V, K)
    a, b, n = MS.match_lists(rng, np.where(sc["tracks"] < K, sc["tracks"], -1), dup=30)
    table = MR.build_tracks(a, b, n, K)
    kp, = _cuda(sc["kpts"][None])
    args = (np.array([V], np.int32), sc["Ks"][None], sc["Rs"][None], sc["ts"][None])
    got = mv.triangulate_views_matches(kp, *_cuda(a[None], b[None], n[None]), *args, **GATES)
    ref = mv.triangulate_views_batch(kp, got["tracks"], *args, **GATES)
    torch.cuda.synchronize()
    assert np.array_equal(got["tracks"][0].cpu().numpy(), table)
    for k in ref:
        assert np.array_equal(got[k].cpu().numpy().view(np.uint8), ref[k].cpu().numpy().view(np.uint8)), k
    sc["tracks"] = table
    w = _want(sc, GATES)
    assert MR.gate_margin(w, GATES["max_depth"]) > 1e-9
    _check(got, 0, w)


def test_degenerate_scenes(mv):
    """Every pose the same motionless one (R = I, t = 0): no pair has a baseline, status 2 everywhere.  Poses of zeros (what an estimator
    that found nothing returns) are not poses: nothing observes the track, status 1 everywhere (the rule of the observed set).  NaN
    key-points, an empty table: no fault, info consistent, no NaN outside rows of status != 0."""
    rng = np.random.default_rng(5)
    V, K = 4, 200
    base = MS.arc_scene(rng, V, K, noise=0.5)
    copy = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}      # noqa: E731
    still, zeros, nans, empty = copy(), copy(), copy(), copy()
    still["Rs"][:], still["ts"][:] = np.eye(3), 0.0
    zeros["Rs"][:], zeros["ts"][:] = 0.0, 0.0
    nans["kpts"][:] = np.nan
    empty["tracks"][:] = -1
    scenes = [still, zeros, nans, empty, base]
    got = _batch(mv, scenes)
    torch.cuda.synchronize()
    for s, sc in enumerate(scenes):
        _check(got, s, _want(sc, GATES))
    info = got["info"].cpu().numpy()
    assert list(info[0]) == [K, 0, 0, K, 0, 0, 0, 0] and (got["status"][0] == 2).all() and not got["n_inliers"][0].any()
    for s in (1, 2, 3):
        assert list(info[s]) == [K, 0, K, 0, 0, 0, 0, 0]
    assert (info[:, 1:].sum(axis=1) == K).all() and info[4, 1] > K // 2
    # nothing to do: fully written outputs without a library call
    e = mv.triangulate_views_batch(torch.zeros((0, 3, 4, 2)).cuda(), torch.zeros((0, 5, 3), dtype=torch.int32).cuda(), None, np.zeros((0, 3, 3, 3)),
                                   np.zeros((0, 3, 3, 3)), np.zeros((0, 3, 3)))
    assert e["points3d"].shape == (0, 5, 3) and e["info"].shape == (0, 8) and e["inlier_views"].dtype == torch.int32
    e = mv.triangulate_views_batch(torch.zeros((2, 3, 4, 2)).cuda(), torch.zeros((2, 0, 3), dtype=torch.int32).cuda(), None, np.zeros((2, 3, 3, 3)),
                                   np.zeros((2, 3, 3, 3)), np.zeros((2, 3, 3)))
    assert e["status"].shape == (2, 0) and e["info"].shape == (2, 8) and not e["info"].any()
    e = mv.triangulate_views_batch(torch.zeros((2, 3, 0, 2)).cuda(), torch.zeros((2, 6, 3), dtype=torch.int32).cuda(), None, np.zeros((2, 3, 3, 3)),
                                   np.zeros((2, 3, 3, 3)), np.zeros((2, 3, 3)))
    assert (e["status"] == 1).all() and list(e["info"][1].cpu().numpy()) == [6, 0, 6, 0, 0, 0, 0, 0] and torch.isnan(e["points3d"]).all()
    from accelerated_features_amd import _lib
    kp, tr = _cuda(base["kpts"][None], base["tracks"][None])
    with pytest.raises(_lib.XFeatHipError):
        mv.triangulate_views_batch(kp, tr, None, base["Ks"][None], base["Rs"][None], base["ts"][None], min_views=1)
    with pytest.raises(RuntimeError):
        mv.triangulate_views_batch(kp, tr, None, base["Ks"][None], base["Rs"][None, :3], base["ts"][None])
    with pytest.raises(RuntimeError):
        mv.triangulate_views_batch(kp, tr, np.array([4, 4], np.int32), base["Ks"][None], base["Rs"][None], base["ts"][None])


def test_map_from_four_views_then_localise_the_fifth(mv):
    """points3d goes, unchanged, into estimate_absolute_pose_matches as points3d_ref for a held-out view matched against the reference view:
    the result is abspose_reference's on the same float32 points, held as tests/test_gpu_abspose.py holds it (winner, iterations, inlier
    count, cost and mask exactly, R and t to 1e-9), and it is the held-out view's pose (0.5 px of noise: within 0.2 degrees and 1 % of |t|)."""
    from accelerated_features_amd import absolute_pose
    rng = np.random.default_rng(21)
    K = 400
    sc = MS.arc_scene(rng, 5, K, noise=0.5)
    MS.plant_outliers(rng, sc, frac=0.2)
    args = (sc["Ks"][None, :4], sc["Rs"][None, :4], sc["ts"][None, :4])
    kp, tr = _cuda(sc["kpts"][None, :4], sc["tracks"][None, :, :4])
    m = mv.triangulate_views_batch(kp, tr, None, *args)
    seen = np.nonzero(sc["tracks"][:, 4] >= 0)[0]
    n = len(seen)
    order = rng.permutation(n)
    idx_ref, idx_q = seen[order].astype(np.int64), sc["tracks"][seen[order], 4].astype(np.int64)
    q, ir, iq, nm = _cuda(sc["kpts"][None, 4], idx_ref[None], idx_q[None], np.array([n], np.int32))
    loc = absolute_pose.estimate_absolute_pose_matches(q, m["points3d"], iq, ir, nm, sc["Ks"][4], 3.0, seed=6)
    torch.cuda.synchronize()
    X = m["points3d"][0].cpu().numpy()
    assert X.dtype == np.float32 and n > 300 and np.isfinite(X[idx_ref]).all(axis=1).sum() > 250
    want = AR.estimate(sc["kpts"][4][idx_q], X[idx_ref], sc["Ks"][4], 3.0, seed=6)
    check_common(loc, want, 0, n)
    R, t = loc["R"][0].cpu().numpy(), loc["t"][0].cpu().numpy()
    assert want["info"][0] == 1 and np.abs(R - want["R"]).max() <= 1e-9 and np.abs(t - want["t"]).max() <= 1e-9 * max(1.0, np.abs(want["t"]).max())
    ang = math.degrees(math.acos(min(1.0, (np.trace(R @ sc["Rs"][4].T) - 1.0) / 2.0)))
    assert ang < 0.2 and np.linalg.norm(t - sc["ts"][4]) < 0.01 * max(1.0, np.linalg.norm(sc["ts"][4]))
