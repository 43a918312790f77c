"""The numpy restatement of the match verification (tests/verification_reference.py) against what it must mean: the filter against boolean
indexing, the verifier's statuses and gates on constructed cases and against the relative-pose restatement's own mask, and the measurement
that DESIGN.md 3.22 rests on: raw lists with 20 % wrong matches leave almost no track, the lists compacted to each pair's RANSAC inliers
bring back more than 95 % of them."""
import numpy as np
import pytest

import pose_reference as PR
import verification_reference as VR
import verification_support as VS

NAN = float("nan")


# ---- the filter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", VS.CAPS)
def test_the_filter_is_boolean_indexing_with_the_order_kept(cap):
    rng = np.random.default_rng(cap)
    ia, ib, n, mask = VS.filter_case(rng, 5, cap)
    f = VR.filter_matches(ia, ib, n, mask)
    for l in range(5):
        m = min(max(int(n[l]), 0), cap)
        sel = np.nonzero(mask[l, :m] != 0)[0]
        c = len(sel)
        assert f["n"][l] == c and list(f["info"][l]) == [m, c, 0, 0]
        assert np.array_equal(f["idx_a"][l, :c], ia[l, :m][mask[l, :m] != 0]) and np.array_equal(f["idx_b"][l, :c], ib[l, :m][mask[l, :m] != 0])
        assert np.array_equal(f["src"][l, :c], sel) and (np.diff(f["src"][l, :c]) > 0).all()
        assert (f["idx_a"][l, c:] == -1).all() and (f["idx_b"][l, c:] == -1).all() and (f["src"][l, c:] == -1).all()
    assert f["src"].dtype == np.int32 and f["idx_a"].dtype == np.int64 and f["n"].dtype == np.int32


def test_mask_values_counts_keep_and_min_keep():
    ia, ib = np.arange(10, 18), np.arange(20, 28)
    mask = np.array([0, 1, 2, 255, 0, 1, 0, 7], np.uint8)
    a, b, src, n, info = VR.filter_list(ia, ib, 8, mask)
    assert n == 5 and list(a[:5]) == [11, 12, 13, 15, 17] and list(b[:5]) == [21, 22, 23, 25, 27] and list(src) == [1, 2, 3, 5, 7, -1, -1, -1]
    assert list(info) == [8, 5, 0, 0]
    assert VR.filter_list(ia, ib, -3, mask)[3] == 0 and list(VR.filter_list(ia, ib, -3, mask)[4]) == [0, 0, 0, 0]          # a negative count
    assert VR.filter_list(ia, ib, 99, mask)[3] == 5 and list(VR.filter_list(ia, ib, 99, mask)[4]) == [8, 5, 0, 0]          # a count above cap
    assert VR.filter_list(ia, ib, 4, mask)[3] == 3
    a, b, src, n, info = VR.filter_list(ia, ib, 8, mask, keep=0)
    assert n == 0 and (a == -1).all() and (b == -1).all() and (src == -1).all() and list(info) == [8, 5, VR.BY_KEEP, 0]
    a, b, src, n, info = VR.filter_list(ia, ib, 8, mask, min_keep=5)            # at the count: kept
    assert n == 5 and list(info) == [8, 5, 0, 0]
    a, b, src, n, info = VR.filter_list(ia, ib, 8, mask, min_keep=6)            # one above: emptied
    assert n == 0 and (a == -1).all() and (src == -1).all() and list(info) == [8, 5, VR.BY_MIN_KEEP, 0]
    assert list(VR.filter_list(ia, ib, 8, mask, keep=0, min_keep=6)[4]) == [8, 5, VR.BY_KEEP, 0]       # keep is tested first
    f = VR.filter_matches(np.stack([ia, ia]).reshape(1, 2, 8), np.stack([ib, ib]).reshape(1, 2, 8), np.array([[8, 8]]), np.stack([mask, mask])[None],
                          keep=np.array([[1, 0]]))
    assert f["idx_a"].shape == (1, 2, 8) and f["n"].tolist() == [[5, 0]] and f["info"].shape == (1, 2, 4)


# ---- the verifier -------------------------------------------------------------------------------------------------------------------------
def _two_views(K=8):
    """Views (I, 0) and (I, (1, 0, 0)) with fx = fy = 512, cx = cy = 256: the epipolar lines are the image rows."""
    Kc = np.array([[512.0, 0, 256], [0, 512, 256], [0, 0, 1]])
    Ks, Rs, ts = np.stack([Kc, Kc, Kc]), np.stack([np.eye(3)] * 3), np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]])
    kpts = np.zeros((3, K, 2), np.float32)
    kpts[0, :, 0], kpts[0, :, 1] = 300 + 10 * np.arange(K), 100 + 20 * np.arange(K)
    kpts[1, :, 0], kpts[1, :, 1] = 280 + 10 * np.arange(K), 100 + 20 * np.arange(K)
    kpts[2] = kpts[0]
    return kpts, Ks, Rs, ts


def test_every_status_by_a_constructed_case():
    kpts, Ks, Rs, ts = _two_views()
    r = np.arange(8)
    pairs = np.array([[0, 1], [1, 1], [0, 3], [-1, 0], [0, 2], [1, 0], [2, 1]], np.int32)
    P = len(pairs)
    ia, ib, n = np.tile(r, (P, 1)), np.tile(r, (P, 1)), np.full(P, 8, np.int32)
    out = VR.verify_matches(kpts, pairs, ia, ib, n, None, Ks, Rs, ts)
    assert out["info"][:, 0].tolist() == [0, 1, 1, 1, 3, 0, 0]                  # (0, 2): equal poses, a zero baseline
    assert out["info"][:, 1].tolist() == [8] * P and out["info"][:, 2].tolist() == [8, 0, 0, 0, 0, 8, 8]
    assert out["mask"][0].all() and not out["mask"][1:5].any() and np.isnan(out["err"][1:5]).all()
    assert (out["err"][0] == 0).all()                                          # exactly on the epipolar line: r2 = 0, kept
    ragged = VR.verify_matches(kpts, pairs, ia, ib, n, 2, Ks, Rs, ts)           # view 2 is outside [0, n_views)
    assert ragged["info"][:, 0].tolist() == [0, 1, 1, 1, 1, 0, 1]
    for bad in ("R", "t", "zero"):
        R2, t2 = Rs.copy(), ts.copy()
        if bad == "R":
            R2[1, 1, 2] = NAN
        elif bad == "t":
            t2[1, 0] = np.inf
        else:
            R2[1] = 0.0
        out = VR.verify_matches(kpts, pairs, ia, ib, n, None, Ks, R2, t2)
        assert out["info"][:, 0].tolist() == [2, 1, 1, 1, 3, 2, 2], bad           # the pair is tested before the poses
        assert not out["mask"].any() and np.isnan(out["err"]).all()


def test_rows_pixels_and_the_strict_threshold():
    kpts, Ks, Rs, ts = _two_views()
    pairs = np.array([[0, 1]], np.int32)
    ia = np.array([[0, -1, 2, 8, 4, 5, 6, 7]])
    ib = np.array([[0, 1, 8, 3, 4, 5, 6, -1]])
    k2 = kpts.copy()
    k2[0, 4, 1] = NAN                                                          # a NaN pixel
    k2[1, 5, 0] = np.inf
    k2[1, 6, 1] += 3.0                                                         # 3 px off its line
    out = VR.verify_matches(k2, pairs, ia, ib, np.array([8]), None, Ks, Rs, ts, 1.0)
    assert out["mask"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and list(out["info"][0]) == [0, 8, 1, 0]
    assert np.isnan(out["err"][0, [1, 2, 3, 4, 5, 7]]).all() and out["err"][0, 0] == 0
    assert abs(out["err"][0, 6] - 3.0 / np.sqrt(2.0)) < 1e-5                    # Sampson: the offset over sqrt(2) for pure translation
    # entries from the count on are not evaluated
    out = VR.verify_matches(k2, pairs, ia, ib, np.array([0]), None, Ks, Rs, ts)
    assert not out["mask"].any() and np.isnan(out["err"]).all() and list(out["info"][0]) == [0, 0, 0, 0]
    # the comparison is strict: an offset d gives r2 = (d / 512)^2 / 2; at max_epipolar_error = d / sqrt(2) the threshold equals it up to rounding
    k3 = kpts.copy()
    k3[1, 0, 1] += 4.0
    e = VR.verify_matches(k3, pairs, ia[:, :1], ib[:, :1], np.array([1]), None, Ks, Rs, ts, 100.0)
    r2 = e["r2"][0, 0]
    px = float(np.sqrt(r2) * 512.0)
    hit = [VR.verify_matches(k3, pairs, ia[:, :1], ib[:, :1], np.array([1]), None, Ks, Rs, ts, m) for m in (np.nextafter(px, 0), px, np.nextafter(px, 9))]
    for h in hit:
        assert bool(h["mask"][0, 0]) == bool(r2 < h["thr2"][0])
    assert not hit[0]["mask"][0, 0] and hit[2]["mask"][0, 0]
    # intrinsics that are not finite: nothing passes, nothing raises
    Kn = Ks.copy()
    Kn[1, 0, 0] = NAN
    out = VR.verify_matches(kpts, pairs, ia, ib, np.array([8]), None, Kn, Rs, ts)
    assert not out["mask"].any() and out["info"][0, 0] == 0


@pytest.mark.parametrize("seed", [1, 2])
def test_the_mask_is_the_relative_pose_restatements_own_under_its_estimate(seed):
    """Views (I, 0) and the estimate's (R, t): R_rel = R and t_rel = t exactly, so E and every Sampson error are the estimator's."""
    sc = VS.wrong_scene(seed, V=2, K=300, wrong=0.3)
    vp, ia, ib, n = sc["lists"]
    m = int(n[0])
    est = PR.estimate(sc["kpts"][0][ia[0, :m]], sc["kpts"][1][ib[0, :m]], sc["Ks"][0], sc["Ks"][1], max_iterations=200)
    assert est["info"][0] == 1 and est["info"][3] > 0.5 * m
    Rs, ts = np.stack([np.eye(3), est["R"]]), np.stack([np.zeros(3), est["t"]])
    out = VR.verify_matches(sc["kpts"], vp, ia, ib, n, None, sc["Ks"], Rs, ts, 1.0)
    assert np.array_equal(out["mask"][0, :m], est["mask"]) and out["info"][0].tolist() == [0, m, int(est["mask"].sum()), 0]
    assert not out["mask"][0, m:].any()
    assert out["thr2"][0] == PR.threshold2(1.0, sc["Ks"][0], sc["Ks"][1])
    # under the true poses the planted wrong matches fail and the true ones pass at 4 sigma
    out = VR.verify_matches(sc["kpts"], vp, ia, ib, n, None, sc["Ks"], sc["Rs"], sc["ts"], 2.0)
    good = ~sc["bad"][0, :m]
    assert out["mask"][0, :m][good].mean() > 0.99 and out["mask"][0, :m][~good].mean() < 0.1


# ---- the measurement of DESIGN.md 3.22 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_raw_lists_lose_the_tracks_and_verified_lists_bring_them_back(seed):
    """V = 6, K = 400, 0.5 px, all 15 pairs, 20 % wrong matches.  Measured: raw 2, 1, 2 tracks; verified 391, 382, 390."""
    sc = VS.wrong_scene(seed)
    raw, _ = VS.tracks_kept(sc, sc["lists"])
    mask, keep, _ = VS.ransac_masks(sc)
    lists, f = VS.filtered(sc["lists"], mask, keep)
    ver, r = VS.tracks_kept(sc, lists)
    print(f"seed {seed}: raw {raw} tracks, verified {ver} tracks, {int(r['info'][3])} components dropped, inliers {int(f['n'].sum())} of {int(sc['lists'][3].sum())}")
    assert keep.all() and (f["info"][:, 2] == 0).all()
    assert raw < 40                                                            # 0.1 K
    assert ver >= 360                                                          # 0.9 K
    # (nearly) every kept track is one point: its key-points belong to one row of the scene's table
    V, K = sc["kpts"].shape[:2]
    owner = np.full((V, K), -1, np.int64)
    for v in range(V):
        seen = sc["tracks"][:, v] >= 0
        owner[v, sc["tracks"][seen, v]] = np.nonzero(seen)[0]
    rows = r["tracks"][:ver]
    pure = sum(len({int(owner[v, row[v]]) for v in range(V) if row[v] >= 0}) == 1 for row in rows)
    assert pure >= 0.97 * ver, (pure, ver)
