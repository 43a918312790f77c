"""The numpy restatement of the retrieval kernels (tests/retrieval_reference.py) against float64 and against its own specification: the error
bounds of DESIGN.md 3.23 hold for the fp32 orders of summation, ties go to the lower index, rows and scores that are not finite never win,
empty clusters keep their centroid, an image without a usable block gives the zero vector, the pair lists are those of a set construction,
and the synthetic places of retrieval_support.place_scene are retrieved exactly with the margins that the GPU tests rely on."""
import numpy as np
import pytest

import retrieval_reference as RR
import retrieval_support as RS
from retrieval_support import bits

F = np.float32


def test_the_bounds_of_assignment_vlad_and_kmeans_hold_for_the_fp32_orders():
    rng = np.random.default_rng(1)
    for K, C in ((33, 32), (257, 256), (2 * RR.CHUNK + 9, 32)):
        desc, counts, cb = RS.tables(rng, 3, K, C)
        got = RR.vlad(desc, counts, cb)
        inside = RR.check_assign(desc, counts, cb, got["assign"])
        frac = RR.check_vlad(desc, counts, cb, got)
        step = RR.kmeans_step(desc, counts, cb)
        assert np.array_equal(step["assign"], got["assign"])
        kfrac = RR.check_kmeans(desc, counts, cb, step)
        print(f"K {K} C {C}: rows inside the assignment window {inside:.2e}, vlad error / bound {frac:.3f}, centroid error / bound {kfrac:.3f}")
        assert inside <= 1e-3
        for g in range(3):                                 # a unit vector, or zero
            n = np.linalg.norm(got["vlad"][g].astype(np.float64))
            assert abs(n - 1) < 1e-6 if got["info"][g, 2] else n == 0


def test_the_score_chain_stays_inside_its_bound_and_the_window_is_below_1e_5():
    rng = np.random.default_rng(2)
    for N, D, k in ((1, 2048, 1), (257, 2048, 8), (300, 16384, 128)):
        q, db = RS.global_vectors(rng, 1, 4, N, D)
        idx, score = RR.retrieve_topk(q, db, None, k, False)
        differ, slots, w = RR.check_topk(q[0], db[0], None, k, False, idx[0], score[0])
        print(f"N {N} D {D} k {k}: slots that differ from the float64 ranking {differ} of {slots}, largest window {w:.2e}")
        assert w < 1e-5 and RR.gamma(RR.DEPTH_SCORE) < 1e-5 and differ * 100 <= slots      # (duplicate rows tie in float64 too: the index decides in both)


def test_ties_go_to_the_lower_index():
    rng = np.random.default_rng(3)
    desc, _, cb = RS.tables(rng, 1, 40, 32, ragged=False, bad_rows=0)
    cb[7], cb[20] = cb[2], cb[2]
    a, _, _ = RR.assign(desc, None, cb)
    assert (a != 7).all() and (a != 20).all() and (a == 2).any()
    q, db = RS.global_vectors(rng, 1, 2, 12, 128, duplicates=False)
    db[0, 9], db[0, 3], db[0, 5] = db[0, 1], db[0, 1], -db[0, 1]
    db[0, 7], db[0, 8] = 0, -0.0                           # scores +0 and -0 compare equal: index order
    idx, score = RR.retrieve_topk(q, db, None, 12, False)
    for j in range(2):
        order = idx[0, j].tolist()
        assert order.index(1) + 1 == order.index(3) and order.index(3) + 1 == order.index(9) and order.index(7) + 1 == order.index(8)
        assert (np.diff(score[0, j]) <= 0).all()


def test_rows_and_scores_that_are_not_finite():
    rng = np.random.default_rng(4)
    desc, _, cb = RS.tables(rng, 2, 20, 32, ragged=False, bad_rows=0)
    counts = np.array([20, 12], np.int32)
    desc[0, 3, 5], desc[0, 4, 0], desc[1, 15, 1] = np.nan, np.inf, np.nan
    cb[0] = np.nan
    got = RR.vlad(desc, counts, cb)
    assert got["assign"][0, 3] == -1 and got["assign"][0, 4] == -1 and (got["assign"][1, 12:] == -1).all()
    assert (got["assign"] != 0).all() and got["info"][0].tolist()[:2] == [18, 2] and got["info"][1].tolist()[:2] == [12, 0]
    assert np.isfinite(got["vlad"]).all() and not got["vlad"][:, :64].any()
    none = RR.vlad(desc, counts, np.full_like(cb, np.nan))      # valid rows without a finite score: no cluster, but counted as valid
    assert (none["assign"] == -1).all() and none["info"].tolist() == [[18, 2, 0, 1], [12, 0, 0, 1]] and not none["vlad"].any()
    step = RR.kmeans_step(desc, counts, np.full_like(cb, np.nan))
    assert step["objective"] == 0 and step["info"].tolist() == [30, 2, 32, 0] and np.isnan(step["codebook"]).all()
    q, db = RS.global_vectors(rng, 1, 3, 6, 64, duplicates=False)
    db[0, 2, 0], db[0, 4, 1] = np.nan, np.inf            # a NaN score and an infinite one
    q[0, 1] *= F(3e38)
    idx, score = RR.retrieve_topk(q, db, np.array([5]), 6, False)
    assert sorted(idx[0, 0].tolist()) == [-1, -1, -1, 0, 1, 3] and np.isnan(score[0, 0, 3:]).all() and np.isfinite(score[0, 0, :3]).all()
    assert (idx[0, 1] == -1).all() or np.isfinite(score[0, 1][idx[0, 1] >= 0]).all()


def test_empty_clusters_keep_their_centroid_and_an_image_without_blocks_is_zero():
    rng = np.random.default_rng(5)
    desc, _, cb = RS.tables(rng, 2, 50, 32, ragged=False, bad_rows=0)
    cb[5] = F(0.5) * cb[4]                                 # half of centroid 4's score: it wins only where every other score is negative
    step = RR.kmeans_step(desc, None, cb)
    assert step["n_assigned"][5] == 0 and np.array_equal(bits(step["codebook"][5]), bits(cb[5])) and step["info"][2] >= 1
    live = step["n_assigned"] > 0
    assert np.allclose(np.linalg.norm(step["codebook"][live].astype(np.float64), axis=1), 1, atol=1e-6)
    again = RR.kmeans_step(desc, None, step["codebook"])
    assert again["objective"] >= step["objective"]          # (a step of spherical k-means never lowers the objective)
    got = RR.vlad(desc, np.array([0, 50], np.int32), cb)
    assert got["info"][0].tolist() == [0, 0, 0, 1] and not got["vlad"][0].any() and got["info"][1, 3] == 0
    same = RR.vlad(np.repeat(cb[None, :4], 2, axis=0), None, cb)      # every row IS its centroid: all residuals zero, m = 0
    assert same["info"][0].tolist() == [4, 0, 0, 1] and not same["vlad"].any() and same["n_assigned"][0, :4].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("V,k", [(2, 1), (5, 2), (32, 4), (32, 128)])
def test_the_pair_lists_are_those_of_a_set_construction(V, k):
    rng = np.random.default_rng(V * 1000 + k)
    idx, n_views = RS.shortlists(rng, 4, V, k)
    for s in range(4):
        for nv in (n_views[s], None):
            vp, n = RR.pairs(idx[s], nv)
            want = RS.pairs_by_sets(idx[s], nv)
            assert n == len(want) and [tuple(p) for p in vp[:n].tolist()] == want and (vp[n:] == -1).all() and len(vp) == RR.pair_capacity(V, k)


def kmeans64(desc, C, iterations):
    """Spherical k-means in float64 from the same start: assignment by the float64 arg-max, the mean direction, empty clusters stay."""
    x = desc.reshape(-1, 64).astype(np.float64)
    cb = RR.initial_codebook(desc, None, C).astype(np.float64)
    for _ in range(iterations):
        a = (x @ cb.T).argmax(axis=1)
        for c in range(C):
            s = x[a == c].sum(axis=0)
            if np.linalg.norm(s) > 0:
                cb[c] = s / np.linalg.norm(s)
    return cb


@pytest.fixture(scope="module", params=[1, 2, 3])
def place(request):
    desc, where = RS.place_scene(request.param)
    cb64 = kmeans64(desc, 64, 10)
    cb32, objective = RR.train_codebook(desc, None, 64, 10)
    return request.param, desc, where, cb64, cb32, objective


def test_place_scene_is_retrieved_exactly_with_margins_far_above_the_windows(place):
    """The figures of DESIGN.md 3.23: every image's top-3 are the other three images of its place, in float64 and in the fp32 restatement."""
    seed, desc, where, cb64, cb32, objective = place
    mates = RS.place_mates(where)
    x = desc.astype(np.float64)
    s = x.reshape(-1, 64) @ cb64.T
    a64 = s.argmax(axis=1).reshape(desc.shape[:2])
    top2 = np.sort(s, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    v64 = np.stack([RR.vlad64(desc[g], a64[g], cb64)[0] for g in range(len(desc))])
    sc = v64 @ v64.T
    np.fill_diagonal(sc, -np.inf)
    order = np.argsort(-sc, axis=1)
    gap_place = min(min(sc[i, list(mates[i])]) - max(sc[i, j] for j in range(len(desc)) if j != i and j not in mates[i]) for i in range(len(desc)))
    top4 = np.take_along_axis(sc, order[:, :4], axis=1)
    gap_rank = float(-np.diff(top4, axis=1).max())
    for i in range(len(desc)):
        assert set(order[i, :3].tolist()) == mates[i], (seed, i)
    # the fp32 restatement: its own codebook, the same answers
    got = RR.vlad(desc, None, cb32)
    inside = RR.check_assign(desc, None, cb32, got["assign"])
    frac = RR.check_vlad(desc, None, cb32, got)
    idx, score = RR.retrieve_topk(got["vlad"][None], got["vlad"][None], None, 3, True)
    differ, slots, w = RR.check_topk(got["vlad"], got["vlad"], None, 3, True, idx[0], score[0])
    dv = max(np.abs(got["vlad"][g].astype(np.float64) - RR.vlad64(desc[g], got["assign"][g], cb32)[0]).max() for g in range(len(desc)))
    print(f"seed {seed}: place gap {gap_place:.4f}, smallest gap in a top-4 {gap_rank:.2e}, smallest assignment margin {margin.min():.2e}, "
          f"rows with margin < 1e-5 {np.mean(margin < 1e-5):.2e}, rows inside the fp32 window {inside:.2e}, |dvlad| {dv:.2e} ({frac:.3f} of the bound), "
          f"top-k window {w:.2e}, slots that differ {differ}")
    for i in range(len(desc)):
        assert set(idx[0, i].tolist()) == mates[i], (seed, i)
    assert gap_place > 100 * 1e-5 and inside <= 1e-3 and w < 1e-5 and differ == 0
    assert (np.diff(objective) >= 0).all()


def test_select_pairs_on_places_with_foreign_images_finds_the_six_pairs_of_the_place(place):
    """Each place plus four foreign images as one scene of V = 8, k = 3: the union of the shortlists holds all six pairs among the place's images."""
    seed, desc, where, cb64, cb32, objective = place
    v = RR.vlad(desc, None, cb32)["vlad"]
    n = len(desc)
    for p in range(int(where.max()) + 1):
        own = np.nonzero(where == p)[0]
        scene = np.concatenate([own, [(own[-1] + 1 + 5 * i) % n for i in range(4)]])
        idx, _ = RR.retrieve_topk(v[scene][None], v[scene][None], None, 3, True)
        vp, cnt = RR.pairs(idx[0], None)
        have = {tuple(r) for r in vp[:cnt].tolist()}
        assert {(a, b) for a in range(4) for b in range(a + 1, 4)} <= have, (seed, p)
