"""xfh_build_tracks_graph (csrc/k_tracks.hip) and xfh_triangulate_tracks (csrc/k_triangulate.hip) on the MI355X against the numpy restatement
tests/tracks_reference.py on the same inputs: every integer output exactly, the points and the reprojection errors as
float32 bits.  Through the restatement every triangulation first asserts that no track of its scene lies within relative 1e-9 of a gate or of
a tie of its two best scores (tracks_reference.gate_margin), as tests/test_gpu_multiview.py does."""
import math

import numpy as np
import pytest
import torch

import abspose_reference as AR
import multiview_reference as MR
import multiview_support as MS
import tracks_reference as TR
import tracks_support as TKS
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
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- build_tracks_graph ---------------------------------------------------------------------------------------------------------------------
def _graph(mv, lists, V, K, **kw):
    """One scene through the device: the four outputs as numpy arrays."""
    out = mv.build_tracks_graph(*_cuda(*(a[None] for a in lists)), V, K, **kw)
    torch.cuda.synchronize()
    return [o[0].cpu().numpy() for o in out]


def _check_graph(got, want):
    tracks, track_of, n_tracks, info = got
    assert tracks.dtype == np.int32 and track_of.dtype == np.int32 and info.dtype == np.int32
    assert list(info) == list(want["info"]), (list(info), list(want["info"]))
    assert int(n_tracks) == want["n_tracks"] and np.array_equal(tracks, want["tracks"]) and np.array_equal(track_of, want["track_of"])
    assert (tracks[int(n_tracks):] == -1).all()


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 300])
def test_three_views_all_pairs(mv, K):
    """The wave and workgroup edges of the thread-per-node and thread-per-match kernels and of the scan's chunks of 256."""
    rng = np.random.default_rng(500 + K)
    lists = TKS.noisy_lists(rng, 3, K, TKS.all_pairs(3))
    if K == 0:
        tracks, track_of, n_tracks, info = _graph(mv, lists, 3, 0)
        assert tracks.shape == (0, 3) and track_of.shape == (3, 0) and n_tracks == 0 and not info.any()
        return
    want = TR.build_tracks_graph(*lists, 3, K)
    _check_graph(_graph(mv, lists, 3, K), want)
    assert want["info"][6] == 0 and (K < 63 or want["info"][2] > K // 2)
    if K == 300:
        assert want["info"][3] > 0
        for kw in (dict(min_length=3), dict(max_tracks=want["n_tracks"] - 7), dict(max_tracks=1)):      # short tracks; fewer rows than tracks
            w = TR.build_tracks_graph(*lists, 3, K, **kw)
            _check_graph(_graph(mv, lists, 3, K, **kw), w)
            assert w["info"][4] > 0 or w["info"][5] > 0


@pytest.mark.parametrize("pairs", ["chain", "all"])
def test_thirty_two_views(mv, pairs):
    """V = 32, K = 65: the chain of 31 pairs and all 496 pairs; the mask's top bit."""
    rng = np.random.default_rng(600)
    lists = TKS.noisy_lists(rng, 32, 65, TKS.chain_pairs(32), 0.03) if pairs == "chain" else TKS.noisy_lists(rng, 32, 65, TKS.all_pairs(32), 0.0005)
    assert len(lists[0]) == (31 if pairs == "chain" else 496) + 3
    want = TR.build_tracks_graph(*lists, 32, 65)
    _check_graph(_graph(mv, lists, 32, 65), want)
    assert want["info"][2] > 20 and want["info"][3] > 0 and (want["tracks"][:, 31] >= 0).any()


def test_zigzag_is_dropped_whole_without_reaching_a_bound(mv):
    K = 300
    lists = TKS.zigzag(K)
    tracks, track_of, n_tracks, info = _graph(mv, lists, 2, K)
    assert list(info) == [2 * K, 1, 0, 1, 0, 0, 0, 0] and n_tracks == 0 and (tracks == -1).all() and (track_of == -1).all()
    _check_graph((tracks, track_of, n_tracks, info), TR.build_tracks_graph(*lists, 2, K))


def test_empty_lists_are_written_without_a_library_call(mv):
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64).cuda()      # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32).cuda()      # noqa: E731
    for S, P, cap in ((2, 0, 4), (2, 3, 0), (0, 3, 4)):
        tracks, track_of, n_tracks, info = mv.build_tracks_graph(i32(S, P, 2), i64(S, P, cap), i64(S, P, cap), i32(S, P), 3, 5)
        assert tracks.shape == (S, 7, 3) and track_of.shape == (S, 3, 5) and n_tracks.shape == (S,) and info.shape == (S, 8)
        assert (tracks == -1).all() and (track_of == -1).all() and not n_tracks.any() and not info.any()
    tracks, _, _, info = mv.build_tracks_graph(i32(3, 2), i64(2, 3, 4), i64(2, 3, 4), i32(2, 3), 3, 5)      # counts of zero: through the library
    assert (tracks == -1).all() and not info.any()


def test_ragged_batch_two_calls_and_a_shuffled_call(mv):
    """Four scenes with different counts, out-of-range indices and views; (P, 2) pairs broadcast; two calls and a call on shuffled lists give
    the same bytes."""
    rng = np.random.default_rng(700)
    V, K, S = 5, 130, 4
    pairs = TKS.all_pairs(V)
    per = [TKS.noisy_lists(rng, V, K, pairs) for _ in range(S)]
    vp = per[0][0]
    ia, ib, n = (np.stack([p[i] for p in per]) for i in (1, 2, 3))
    n[1] //= 2; n[2, ::2] = 0; n[3] = np.minimum(n[3], 1)
    n[0, 0] = K + 50                                       # a count beyond the capacity is clamped
    wants = [TR.build_tracks_graph(vp, ia[s], ib[s], n[s], V, K) for s in range(S)]
    got = mv.build_tracks_graph(*_cuda(vp, ia, ib, n), V, K)
    again = mv.build_tracks_graph(*_cuda(np.broadcast_to(vp, (S,) + vp.shape), ia, ib, n), V, K)
    P = len(vp)
    ja, jb = ia.copy(), ib.copy()
    for s in range(S):
        for p in range(P):
            m = int(min(max(n[s, p], 0), ia.shape[2]))
            o = rng.permutation(m)
            ja[s, p, :m], jb[s, p, :m] = ia[s, p, o], ib[s, p, o]
    o = rng.permutation(P)
    shuffled = mv.build_tracks_graph(*_cuda(vp[o], ja[:, o], jb[:, o], n[:, o]), V, K)
    torch.cuda.synchronize()
    for s in range(S):
        _check_graph([t[s].cpu().numpy() for t in got], wants[s])
    for a, b, c in zip(got, again, shuffled):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert len({int(w["n_tracks"]) for w in wants}) >= 3     # the scenes differ


def test_star_lists_give_build_tracks_rows(mv):
    rng = np.random.default_rng(800)
    for V, K in ((4, 300), (32, 70)):
        sc = MS.arc_scene(rng, V, K)
        a, b, n = MS.match_lists(rng, sc["tracks"])
        star = mv.build_tracks(*_cuda(a[None], b[None], n[None]), K)[0]
        pairs = np.array([(0, v) for v in range(1, V)], np.int32)
        tracks, track_of, n_tracks, info = mv.build_tracks_graph(*_cuda(pairs, a[None], b[None], n[None]), V, K)
        torch.cuda.synchronize()
        want = star[(star[:, 1:] >= 0).any(dim=1)]
        nt = int(n_tracks[0])
        assert nt == len(want) > K // 2 and torch.equal(tracks[0, :nt], want) and list(info[0, 3:].cpu().numpy()) == [0, 0, 0, 0, 0]
        rows = want[:, 0].long()
        assert torch.equal(track_of[0, 0, rows], torch.arange(nt, dtype=torch.int32, device=rows.device))


# ---- anchor='first' -------------------------------------------------------------------------------------------------------------------------
def _scene(seed, V, K, gates=GATES):
    """tests/test_gpu_multiview._scene's kind of scene (0.5 px of noise, planted outliers, holes, a max_depth inside it) with view 0's column
    emptied on a third of the rows, clear of every gate and tie under both anchors."""
    rng = np.random.default_rng(seed)
    for _ in range(50):
        sc = MS.arc_scene(rng, V, K, noise=0.5, cam=seed)
        MS.plant_outliers(rng, sc, frac=0.4)
        off = rng.random(K) < 0.05
        sc["kpts"][0, :K][off] += 3.5
        holes = rng.random(sc["tracks"].shape) < 0.06
        sc["tracks"][holes] = np.where(rng.random(holes.sum()) < 0.5, -1, sc["kpts"].shape[1] + 3)
        sc["tracks"][seed % 3::3, 0] = -1
        args = (sc["kpts"], sc["tracks"], sc["n_views"], sc["Ks"], sc["Rs"], sc["ts"])
        w, ref = TR.triangulate_views(*args, **gates), MR.triangulate_views(*args, **gates)
        if TR.gate_margin(w, gates["max_depth"]) > 1e-9 and MR.gate_margin(ref, gates["max_depth"]) > 1e-9:
            return sc, w, ref
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


def _both(mv, sc, gates):
    args = _cuda(sc["kpts"][None], sc["tracks"][None]) + (None, sc["Ks"][None], sc["Rs"][None], sc["ts"][None])
    first = mv.triangulate_views_batch(*args, **gates, anchor="first")
    ref = mv.triangulate_views_batch(*args, **gates, anchor="reference")
    default = mv.triangulate_views_batch(*args, **gates)
    torch.cuda.synchronize()
    for k in ref:
        assert np.array_equal(ref[k].cpu().numpy().view(np.uint8), default[k].cpu().numpy().view(np.uint8)), k
    return first, ref


@pytest.mark.parametrize("K", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("V", [2, 32])
def test_anchored_triangulation_equals_the_restatement(mv, V, K):
    gates = dict(GATES, min_parallax_deg=1.0) if V == 2 else GATES      # (view 1 is 3 degrees from view 0)
    sc, want, want_ref = _scene(900 + 40 * V + K, V, K, gates)
    first, ref = _both(mv, sc, gates)
    _check(first, 0, want)
    _check(ref, 0, want_ref)                               # anchor='reference': today's results on the same inputs
    if V == 32 and K >= 63:
        high = want["anchor"] > 0
        assert (want["status"][high] == 0).sum() > K // 8 and (want_ref["status"][high] == 1).all()
        zero = want["anchor"] == 0
        assert np.array_equal(first["points3d"][0].cpu().numpy()[zero].view(np.uint32), ref["points3d"][0].cpu().numpy()[zero].view(np.uint32))


def _pose_close(R, t, Rw, tw, deg, rel):
    ang = math.degrees(math.acos(min(1.0, (np.trace(R @ Rw.T) - 1.0) / 2.0)))
    return ang < deg and np.linalg.norm(t - tw) < rel * max(1.0, np.linalg.norm(tw))


def test_chain_scene_end_to_end_and_localisation_against_view_three(mv):
    """triangulate_graph_matches -> bundle_adjust_batch -> the second triangulation on the chain scene (matches of the pairs (v, v + 1) only,
    a third of the tracks without the views 0 and 1); rows >= n_tracks count as unobserved; view_points(view 3) localises a further view that
    is matched against view 3 alone, and the pose is abspose_reference's on the same points, held as tests/test_gpu_multiview.py holds it."""
    from accelerated_features_amd import absolute_pose
    sc = TKS.chain_scene(1, V=7)                           # view 6 is the further image
    K, V = sc["tracks"].shape[0], 6
    keep = sc["lists"][0][:, 1] < V                        # the pairs among the first six views
    lists = tuple(a[keep] for a in sc["lists"])
    kp, = _cuda(sc["kpts"][None, :V])
    cams = (sc["Ks"][None, :V], sc["Rs"][None, :V], sc["ts"][None, :V])
    out = mv.triangulate_graph_matches(kp, *_cuda(lists[0], *(a[None] for a in lists[1:])), None, *cams, max_reproj_error=2.0)
    torch.cuda.synchronize()
    g = TR.build_tracks_graph(*lists, V, K)
    want_table, src = TKS.runs(sc["tracks"][:, :V])
    n = g["n_tracks"]
    assert n == len(want_table) and np.array_equal(g["tracks"][:n], want_table)
    _check_graph([out[k][0].cpu().numpy() for k in ("tracks", "track_of", "n_tracks", "track_info")], g)
    w = TR.triangulate_views(sc["kpts"][:V], g["tracks"], V, sc["Ks"][:V], sc["Rs"][:V], sc["ts"][:V], 2.0, 1.0, np.inf, 2)
    assert TR.gate_margin(w) > 1e-9
    _check(out, 0, w)
    T = g["tracks"].shape[0]
    info = out["info"][0].cpu().numpy()
    assert info[0] == T and info[2] >= T - n and (out["status"][0, n:] == 1).all()      # rows >= n_tracks are unobserved
    removed = sc["removed"][src]
    valid = out["valid"][0, :n].cpu().numpy()
    assert valid[removed].mean() > 0.9 and valid[~removed].mean() > 0.9 and removed.sum() > 80
    # the star path on the same matches maps none of the removed group
    star_lists = [np.zeros((V - 1,) + lists[1].shape[1:], np.int64), np.zeros((V - 1,) + lists[1].shape[1:], np.int64), np.zeros(V - 1, np.int32)]
    star_lists[0][0], star_lists[1][0], star_lists[2][0] = lists[1][0], lists[2][0], lists[3][0]
    star = mv.triangulate_views_matches(kp, *_cuda(*(a[None] for a in star_lists)), None, *cams, max_reproj_error=2.0)
    assert (star["status"][0].cpu().numpy()[sc["removed"]] == 1).all() and star["valid"].any()
    # bundle adjustment consumes the table and the result as they are; then the second triangulation, anchored
    ba = mv.bundle_adjust_batch(kp, out["tracks"], out["inlier_views"], out["points3d"], None, *cams)
    again = mv.refine_views_batch(kp, out["tracks"], None, *cams, max_reproj_error=2.0, anchor="first")
    torch.cuda.synchronize()
    binfo = ba["info"][0].cpu().numpy()
    assert binfo[5] == 0 and binfo[0] == int(valid.sum()) and ba["cost"][0, 1] <= ba["cost"][0, 0]
    assert np.array_equal(again["Rs"].cpu().numpy(), ba["Rs"].cpu().numpy()) and np.array_equal(again["ba_info"].cpu().numpy(), ba["info"].cpu().numpy())
    second = mv.triangulate_views_batch(kp, out["tracks"], None, cams[0], ba["Rs"], ba["ts"], max_reproj_error=2.0, anchor="first")
    for k in second:
        assert np.array_equal(second[k].cpu().numpy().view(np.uint8), again[k].cpu().numpy().view(np.uint8)), k
    v2 = again["valid"][0, :n].cpu().numpy()
    assert v2[removed].mean() > 0.9 and (again["status"][0, n:] == 1).all()
    # a further view matched against view 3 only
    P3 = mv.view_points(out["points3d"], out["track_of"], 3)
    torch.cuda.synchronize()
    X3 = P3[0].cpu().numpy()
    of3 = g["track_of"][3]
    assert P3.shape == (1, K, 3) and P3.dtype == torch.float32
    assert _same_f32(X3[of3 >= 0], w["points3d"][of3[of3 >= 0]]) and np.isnan(X3[of3 < 0]).all()
    rng = np.random.default_rng(31)
    seen = np.nonzero((sc["tracks"][:, 3] >= 0) & (sc["tracks"][:, 6] >= 0))[0]
    seen = seen[rng.permutation(len(seen))]
    idx_ref, idx_q = sc["tracks"][seen, 3].astype(np.int64), sc["tracks"][seen, 6].astype(np.int64)
    m = len(seen)
    q, ir, iq, nm = _cuda(sc["kpts"][None, 6], idx_ref[None], idx_q[None], np.array([m], np.int32))
    loc = absolute_pose.estimate_absolute_pose_matches(q, P3, iq, ir, nm, sc["Ks"][6], 3.0, seed=6)
    torch.cuda.synchronize()
    assert m > 300 and np.isfinite(X3[idx_ref]).all(axis=1).sum() > 250
    assert np.isfinite(X3[idx_ref][sc["removed"][seen]]).all(axis=1).sum() > 60      # points that the star model does not have
    want = AR.estimate(sc["kpts"][6][idx_q], X3[idx_ref], sc["Ks"][6], 3.0, seed=6)
    check_common(loc, want, 0, m)
    R, t = loc["R"][0].cpu().numpy(), loc["t"][0].cpu().numpy()
    assert want["info"][0] == 1 and np.abs(R - want["R"]).max() <= 1e-9 and np.abs(t - want["t"]).max() <= 1e-9 * max(1.0, np.abs(want["t"]).max())
    assert _pose_close(R, t, sc["Rs"][6], sc["ts"][6], 0.2, 0.01)
