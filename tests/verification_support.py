"""Inputs of the match-verification tests (tests/test_verification_*.py, tests/test_gpu_verification.py) and of tools/verify_time.py: what is
not specification (that is tests/verification_reference.py).  The generators consume their numpy generator in a fixed order, which is part
of the tests' inputs."""
import numpy as np

import multiview_support as MS
import pose_reference as PR
import tracks_reference as KR
import tracks_support as TS
import verification_reference as VR

CAPS = (1, 63, 64, 65, 255, 256, 257, 1000)                # around the wave and the workgroup


def wrong_scene(seed, V=6, K=400, wrong=0.2, noise=0.5, pairs=None):
    """MS.arc_scene at V views, K tracks and `noise` pixels, the lists of all pairs (or `pairs`) from its table, and a share `wrong` of the
    list entries with idx_b replaced by a random row of [0, K): what a mutual-nearest-neighbour list holds.  The scene dict with `lists` =
    (view_pairs (P,2) int32, idx_a, idx_b (P,K) int64, n_matches (P,) int32) and `bad` (P,K) bool added."""
    rng = np.random.default_rng(seed)
    sc = MS.arc_scene(rng, V, K, noise=noise)
    vp, ia, ib, n = TS.pair_lists(rng, sc["tracks"], TS.all_pairs(V) if pairs is None else pairs, kcap=K)
    bad = rng.random(ib.shape) < wrong
    ib[bad] = rng.integers(0, K, bad.sum())
    sc["lists"], sc["bad"] = (vp, ia, ib, n), bad
    return sc


def ransac_masks(sc, max_epipolar_error=1.0, max_iterations=1000, min_inliers=15):
    """pose_reference.estimate on every pair of the scene's lists (pair p of the batch, seed 0): mask (P,cap) uint8, keep (P,) uint8 (a pose
    was found with at least min_inliers inliers), the estimates."""
    vp, ia, ib, n = sc["lists"]
    P, cap = ia.shape
    mask, keep, est = np.zeros((P, cap), np.uint8), np.zeros(P, np.uint8), []
    for p, (a, b) in enumerate(vp):
        m = int(n[p])
        r = PR.estimate(sc["kpts"][a][ia[p, :m]], sc["kpts"][b][ib[p, :m]], sc["Ks"][a], sc["Ks"][b], max_epipolar_error=max_epipolar_error,
                        max_iterations=max_iterations, pair=p)
        mask[p, :m] = r["mask"]
        keep[p] = r["info"][0] != 0 and r["info"][3] >= min_inliers
        est.append(r)
    return mask, keep, est


def tracks_kept(sc, lists):
    """tracks_reference.build_tracks_graph on the lists: (tracks kept, its result)."""
    V, K = sc["kpts"].shape[:2]
    r = KR.build_tracks_graph(*lists, V, K)
    return int(r["n_tracks"]), r


def filtered(lists, mask, keep=None, min_keep=0):
    vp, ia, ib, n = lists
    f = VR.filter_matches(ia, ib, n, mask, keep, min_keep)
    return (vp, f["idx_a"], f["idx_b"], f["n"]), f


def filter_case(rng, L, cap, kind="random"):
    """L ragged lists of capacity cap with counts below 0 and above cap among them; mask values 0, 1, 2 and 255."""
    ia, ib = rng.integers(-3, 1 << 40, (L, cap)), rng.integers(-3, 1 << 40, (L, cap))
    n = rng.integers(0, cap + 1, L).astype(np.int32)
    if L >= 3:
        n[0], n[1], n[2] = cap, -2, cap + 5
    if kind == "zeros":
        mask = np.zeros((L, cap), np.uint8)
    elif kind == "ones":
        mask = np.ones((L, cap), np.uint8)
    else:
        mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), (L, cap))
    return ia, ib, n, mask


def verify_case(rng, V, K, pairs, noise=0.5, cap=None, wrong=0.3):
    """An arc scene with its lists over `pairs` (capacity cap, default K + 3, the slots past the count hold junk), a share of wrong entries
    and rows -2 .. K + 1 among them.  Returns kpts (V,K,2), view_pairs, idx_a, idx_b, n_matches, Ks, Rs, ts."""
    sc = MS.arc_scene(rng, V, K, noise=noise)
    cap = K + 3 if cap is None else cap
    vp, ia, ib, n = TS.pair_lists(rng, sc["tracks"], pairs, cap=cap, kcap=K)
    bad = rng.random(ib.shape) < wrong
    ib[bad] = rng.integers(-2, K + 2, bad.sum())
    past = np.arange(cap)[None, :] >= n[:, None]
    ia[past] = rng.integers(-2, K + 2, past.sum())
    return sc["kpts"].copy(), vp, ia, ib, n, sc["Ks"].copy(), sc["Rs"].copy(), sc["ts"].copy()


def assert_clear_of_threshold(r2, thr2, rel=1e-9):
    """No evaluated error within `rel` (relative) of its pair's threshold: a mask compared exactly must not hang on the last bit."""
    r2, thr2 = np.asarray(r2), np.asarray(thr2)
    t = thr2.reshape(thr2.shape + (1,) * (r2.ndim - thr2.ndim))
    with np.errstate(all="ignore"):
        close = np.isfinite(r2) & (np.abs(r2 - t) <= rel * t)
    assert not close.any(), (np.nonzero(close), r2[close])


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def same_bits(got, want):
    """Equal bit for bit, any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def verify_batch(seed, V, K, pairs, cap=None):
    """Four scenes of verify_case over `pairs` plus the pairs (1, 1) and (V, 0): scene 0 as it is, with a count above cap and a negative one;
    scene 1 with the views 0 and 1 at one pose whose rotation is a permutation (a baseline that is zero exactly); scene 2 with a NaN in the rotation of view 1; scene 3 with NaN and
    infinite pixels and n_views = V - 1.  A dict of stacked arrays: kpts (4,V,K,2), view_pairs (4,P,2), idx_a, idx_b (4,P,cap), n_matches
    (4,P), n_views (4,), Ks, Rs (4,V,3,3), ts (4,V,3)."""
    rng = np.random.default_rng(seed)
    keys = ("kpts", "view_pairs", "idx_a", "idx_b", "n_matches", "Ks", "Rs", "ts")
    scenes = []
    for s in range(4):
        c = list(verify_case(rng, V, K, list(pairs), cap=cap))
        c[1] = np.r_[c[1], [[1, 1]], [[V, 0]]].astype(np.int32)
        c[2], c[3], c[4] = np.r_[c[2], c[2][:1], c[2][:1]], np.r_[c[3], c[3][:1], c[3][:1]], np.r_[c[4], c[4][:1], c[4][:1]]
        scenes.append(dict(zip(keys, c)))
    capn = scenes[0]["idx_a"].shape[1]
    scenes[0]["n_matches"][0] = capn + 5
    scenes[0]["n_matches"][-1] = -1
    scenes[1]["Rs"][0] = scenes[1]["Rs"][1] = np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]])      # (R R' is I exactly, so t_rel is 0 exactly)
    scenes[1]["ts"][1] = scenes[1]["ts"][0]
    scenes[2]["Rs"][1, 0, 0] = np.nan
    k = scenes[3]["kpts"]
    k[0, rng.integers(0, K, max(K // 8, 1)), 0] = np.nan
    k[1, rng.integers(0, K, max(K // 8, 1)), 1] = np.inf
    out = {key: np.stack([sc[key] for sc in scenes]) for key in keys}
    out["n_views"] = np.array([V, V, V, V - 1], np.int32)
    return out


def verify_batch_reference(b, max_epipolar_error=1.0, scenes=None):
    """verification_reference.verify_matches on every scene of a verify_batch: stacked mask, err, info, r2, thr2."""
    rs = [VR.verify_matches(b["kpts"][s], b["view_pairs"][s], b["idx_a"][s], b["idx_b"][s], b["n_matches"][s], b["n_views"][s], b["Ks"][s], b["Rs"][s],
                            b["ts"][s], max_epipolar_error) for s in (range(len(b["kpts"])) if scenes is None else scenes)]
    return {k: np.stack([r[k] for r in rs]) for k in rs[0]}


# ---- the chain behind reconstruct_graph_matches(verified=True), and its errors against the scene ------------------------------------------------
def truth(sc):
    """The scene's poses, centres and points in the gauge of view 0 (R_0 = I, c_0 = 0), as posegraph_support.errors wants them."""
    V = sc["Rs"].shape[0]
    c = np.stack([-sc["Rs"][v].T @ sc["ts"][v] for v in range(V)])
    return dict(V=V, Rs=np.stack([sc["Rs"][v] @ sc["Rs"][0].T for v in range(V)]), cs=(c - c[0]) @ sc["Rs"][0].T, X=sc["X"] @ sc["Rs"][0].T + sc["ts"][0])


def chain_errors(sc, Rs, ts, tracks, points3d, valid):
    """(largest rotation error in degrees, largest centre error, median point error over the scene's depth) after the similarity alignment
    of tests/test_gpu_posegraph.py: the gauge of view 0, one least-squares scale from the centres.  The true point of a track is the one that
    owns its key-point in its lowest view."""
    import posegraph_support as PS
    tr = truth(sc)
    V, K = sc["kpts"].shape[:2]
    rot, cen = PS.errors(tr, Rs, ts)
    c = np.stack([-Rs[v].T @ ts[v] for v in range(1, V)])
    s = (c * tr["cs"][1:]).sum() / (c * c).sum()
    owner = np.full((V, K), -1, np.int64)
    for v in range(V):
        seen = sc["tracks"][:, v] >= 0
        owner[v, sc["tracks"][seen, v]] = np.nonzero(seen)[0]
    rows = np.nonzero(np.asarray(valid, bool))[0]
    tracks = np.asarray(tracks)
    first = np.argmax(tracks[rows] >= 0, axis=1)
    own = owner[first, tracks[rows, first]]
    ok = own >= 0
    e = np.linalg.norm(s * np.asarray(points3d, np.float64)[rows][ok] - tr["X"][own[ok]], axis=1) / MS.DEPTH
    return rot, cen, float(np.median(e))


def restatement_chain(sc, max_iterations=1000, min_inliers=15):
    """The restatements chained as reconstruct_graph_matches(verified=True) chains the kernels: pose_reference.estimate per pair ->
    verification_reference.filter_matches -> posegraph_reference.average_poses -> tracks_reference.build_tracks_graph and triangulate_views
    -> bundle_reference.bundle_adjust -> triangulate_views under the refined poses.  Returns (the final triangulation with Rs, ts, tracks
    and n_tracks added, the filter's result)."""
    import bundle_reference as BR
    import posegraph_reference as GR
    vp, ia, ib, n = sc["lists"]
    V, K = sc["kpts"].shape[:2]
    mask, keep, est = ransac_masks(sc, max_iterations=max_iterations, min_inliers=min_inliers)
    lists, f = filtered(sc["lists"], mask, keep)
    Rrel, trel = np.stack([e["R"] for e in est]), np.stack([e["t"] for e in est])
    weight = np.array([float(e["info"][3]) if k else 0.0 for e, k in zip(est, keep)])
    pg = GR.average_poses(vp, Rrel, trel, weight, V, V)
    tab = KR.build_tracks_graph(*lists, V, K)
    first = KR.triangulate_views(sc["kpts"], tab["tracks"], V, sc["Ks"], pg["Rs"], pg["ts"])
    ba = BR.bundle_adjust(sc["kpts"], tab["tracks"], first["inlier_views"], first["points3d"], V, sc["Ks"], pg["Rs"], pg["ts"])
    out = KR.triangulate_views(sc["kpts"], tab["tracks"], V, sc["Ks"], ba["Rs"].reshape(V, 3, 3), ba["ts"].reshape(V, 3))
    out.update(Rs=ba["Rs"].reshape(V, 3, 3), ts=ba["ts"].reshape(V, 3), tracks=tab["tracks"], n_tracks=tab["n_tracks"], Rs_init=pg["Rs"], ts_init=pg["ts"])
    return out, f
