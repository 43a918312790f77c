"""The numpy restatement of the baseline scales (tests/posescale_reference.py) on its own: what the method recovers on chains, strips and two
triangles at a shared view, what the robust factor does with an edge whose tracks are wrong, and the properties of the lower median.  The
figures asserted are those of DESIGN.md 3.20: twice the worst of the seeds 1 - 3 on noisy input (0.5 px, 0.5 degrees), ten times the measured
rounding figure on noise-free input (the pixels are float32: a ratio is exact to about 2e-8)."""
import numpy as np
import pytest

import posegraph_reference as PR
import posegraph_support as PS
import posescale_reference as QR
import posescale_support as QS

NOISY_GATE = dict(max_reproj_error=32.0)      # 0.5 degrees of pose noise move a pixel by about 10: the default of 4 would leave no track
FAMILIES = {"chain3": (3, PS.chain_pairs(3)), "chain8": (8, PS.chain_pairs(8)), "chain32": (32, PS.chain_pairs(32)), "strip8": (8, PS.near_pairs(8)),
            "strip32": (32, PS.near_pairs(32)), "two triangles": (5, PS.TWO_TRIANGLES)}
# measured worst of seeds 1 - 3 (rotation degrees, relative centre error, relative ratio error); asserted at twice that
WORST = {"chain3": (0.832, 0.0216, 0.060), "chain8": (3.446, 0.0339, 0.152), "chain32": (7.669, 0.0794, 0.241), "strip8": (1.422, 0.0457, 0.189),
         "strip32": (1.821, 0.0313, 0.207), "two triangles": (1.490, 0.0700, 0.148)}
# noise-free: the largest of all families and seeds: rotation 3.9e-14 degrees, centres 5.3e-8, ratios 3.2e-8; asserted at ten times that
ROUNDING = (3.9e-14, 5.3e-8, 3.2e-8)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_noise_free_input_gives_the_true_ratios_and_centres_to_rounding(name):
    V, pairs = FAMILIES[name]
    sc = QS.scene(1, V, 400, pairs, 0.0, 0.0, 0.0)
    r = QS.ratios(sc)
    w = QS.run(sc, r)
    wedges = r["shared_view"] >= 0
    assert wedges.sum() > 0 and np.isfinite(r["ratio"][wedges]).all() and np.isnan(r["ratio"][~wedges]).all()
    assert w["info"][6] == PR.ST_OK and w["info"][1] == V
    rot, cen = PS.errors(sc, w["Rs"], w["ts"], w["registered"])
    err, n = QS.ratio_error(sc, r)
    print(name, "rotation %.3g deg, centres %.3g, ratios %.3g (%d)" % (rot, cen, err, n))
    assert rot <= 10 * ROUNDING[0] and cen <= 10 * ROUNDING[1] and err <= 10 * ROUNDING[2]
    if "chain" in name:                                       # without the ratios a chain has no positions
        w0 = QS.run(sc, None)
        assert w0["info"][6] == PR.ST_ROTATIONS_ONLY and np.isnan(w0["ts"][1:]).all()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_noisy_input_gives_the_measured_figures(name):
    V, pairs = FAMILIES[name]
    for seed in (1, 2, 3):
        sc = QS.scene(seed, V, 400, pairs)
        r = QS.ratios(sc, **NOISY_GATE)
        w = QS.run(sc, r)
        assert w["info"][6] == PR.ST_OK and w["info"][1] == V, (name, seed, w["info"])
        rot, cen = PS.errors(sc, w["Rs"], w["ts"], w["registered"])
        err, n = QS.ratio_error(sc, r)
        print(name, seed, "rotation %.3f deg, centres %.4f, ratios %.3f (%d), smallest pivot ratio %.3g" % (rot, cen, err, n, min(w["ratios"])))
        assert rot <= 2 * WORST[name][0] and cen <= 2 * WORST[name][1] and err <= 2 * WORST[name][2], (name, seed, rot, cen, err)
        if name == "two triangles":                           # 3.19's table: 1.1e-3 without the ratios, within 1.3 of a rigid family
            assert min(w["ratios"]) > 1e-2 > 10 * min(QS.run(sc, None)["ratios"])


def test_the_wedges_of_an_edge_with_wrong_tracks_end_below_a_half():
    """Edge 7 = (2, 4) of the strip of 8 views sees a structure of twice the depth: its 8 wedges carry ratios that are wrong by a factor of
    about 2.  All 8 end with a factor < 0.5 and none of the 59 clean wedges does (the cap is 5 %: 2 of them; this scene has no exception)."""
    sc = QS.scene(4, 8, 400, PS.near_pairs(8))
    r, mine = QS.corrupted_ratios(sc, 7, **NOISY_GATE)
    wrong = [abs(r["ratio"][p, q] / QS.true_ratio(sc, p, q) - 1.0) for p, q in np.argwhere(mine)]
    assert min(wrong) > 0.3
    w = QS.run(sc, r)
    took = np.zeros_like(mine)
    took[w["wedges"]] = True
    f = w["ratio_factor"]
    assert w["info"][6] == PR.ST_OK and (mine & took).sum() == 8 and (~mine & took).sum() == 59
    assert (f[mine & took] < 0.5).all()
    assert (f[~mine & took] < 0.5).sum() <= 0.05 * (~mine & took).sum()
    assert (f[~took] == 0.0).all()


def test_a_chain_whose_middle_wedge_has_too_few_common_tracks_stays_without_positions():
    sc = QS.scene(1, 8, 400, PS.chain_pairs(8), 0.0, 0.0, 0.0)
    full = np.nonzero((sc["tracks"][:, 3:6] >= 0).all(axis=1))[0]
    drop = full[5:]                                           # 5 tracks keep the views 3, 4 and 5
    sc["track_of"][4, sc["tracks"][drop, 4]] = -1
    sc["tracks"][drop, 4] = -1
    r = QS.ratios(sc)
    at = [(p, p + 1) for p in range(6)]
    n = np.array([r["count"][a] for a in at])
    assert (n[[0, 1, 5]] >= 8).all() and 0 < n[3] < 8 and np.isnan(r["ratio"][at[3]]) and r["info"][0] == 6 and r["info"][1] == int((n >= 8).sum())
    w = QS.run(sc, r)
    assert w["info"][6] == PR.ST_ROTATIONS_ONLY and np.isnan(w["ts"][1:]).all() and (w["ratio_factor"] == 0.0).all()
    assert QS.run(sc, QS.ratios(sc, min_common=5))["info"][6] == PR.ST_OK


def test_all_pairs_with_ratios_are_no_worse_than_without():
    for seed in (1, 2, 3):
        sc = QS.scene(seed, 8, 400, PS.all_pairs(8))
        w, w0 = QS.run(sc, QS.ratios(sc, **NOISY_GATE)), QS.run(sc, None)
        (rot, cen), (rot0, cen0) = PS.errors(sc, w["Rs"], w["ts"], w["registered"]), PS.errors(sc, w0["Rs"], w0["ts"], w0["registered"])
        print(seed, "with %.3f deg %.4f, without %.3f deg %.4f" % (rot, cen, rot0, cen0))
        assert w["info"][6] == w0["info"][6] == PR.ST_OK and rot == rot0 and cen <= 2 * cen0


def test_without_ratios_the_run_is_posegraph_reference_exactly():
    for sc, kw in ((PS.scene(3, 8, PS.all_pairs(8), 0.5, 0.15), dict(min_pivot_ratio=1e-8)), (PS.scene(7, 8, PS.chain_pairs(8), 0.5), {}),
                   (PS.scene(2, 5, PS.TWO_TRIANGLES), dict(min_pivot_ratio=1e-8))):
        s = dict(PS.DEFAULTS, **kw)
        a = PR.average_poses(sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc["V"], sc["V"], **s)
        b = QR.average_poses(sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc["V"], sc["V"], ratio=None, **s)
        for k in ("Rs", "ts", "edge_factor", "info"):
            assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].tobytes() == b[k].tobytes(), k
        assert a["registered"] == b["registered"] and a["ratios"] == b["ratios"] and (b["ratio_factor"] == 0.0).all()


def test_the_lower_median():
    assert QR.lower_median([3.0, 1.0, 2.0]) == 2.0 and QR.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0 and QR.lower_median([5.0]) == 5.0
    assert QR.lower_median([2.0, 2.0, 2.0, 7.0]) == 2.0 and QR.lower_median([1.0, 2.0, 2.0, 2.0, 9.0, 9.0]) == 2.0
    rng = np.random.default_rng(0)
    for n in (7, 8, 9, 255, 256, 257):
        v = rng.random(n)
        m = QR.lower_median(v)
        assert m in v and (v < m).sum() == (n - 1) // 2 and QR.lower_median(v[rng.permutation(n)]) == m
    # in a wedge: n = min_common - 1 values give a count and no ratio, n = min_common give the element (n - 1) // 2
    sc = QS.scene(2, 3, 400, PS.chain_pairs(3), 0.0, 0.0, 0.0)
    r = QS.ratios(sc)
    vals = r["values"][(0, 1)]
    n = len(vals)
    assert r["count"][0, 1] == n and r["ratio"][0, 1] == np.sort(vals)[(n - 1) // 2]
    assert np.isnan(QS.ratios(sc, min_common=n + 1)["ratio"][0, 1]) and QS.ratios(sc, min_common=n + 1)["count"][0, 1] == n
    assert QS.ratios(sc, min_common=n)["ratio"][0, 1] == r["ratio"][0, 1]


def test_permuted_rows_and_permuted_pairs_give_the_same_ratios():
    sc = QS.scene(5, 6, 200, PS.near_pairs(6))
    r = QS.ratios(sc, **NOISY_GATE)
    rng = np.random.default_rng(1)
    # the key-point rows of every view in another order
    o = dict(sc)
    o["kpts"], o["tracks"], o["track_of"] = sc["kpts"].copy(), sc["tracks"].copy(), sc["track_of"].copy()
    for v in range(6):
        perm = rng.permutation(200)                           # new row of old row i: perm[i]
        o["kpts"][v, perm] = sc["kpts"][v]
        o["track_of"][v, perm] = sc["track_of"][v]
        on = sc["tracks"][:, v] >= 0
        o["tracks"][on, v] = perm[sc["tracks"][on, v]]
    ro = QS.ratios(o, **NOISY_GATE)
    for k in ("ratio", "count", "shared_view", "info"):
        assert r[k].tobytes() == ro[k].tobytes(), k
    # the pairs in another order: wedge (p, q) moves to (min, max) of the new indices; its ratio is inverted when the two swap
    P = sc["pairs"].shape[0]
    perm = rng.permutation(P)                                 # new edge j is old edge perm[j]
    o = dict(sc)
    for k in ("pairs", "Rrel", "trel", "weight"):
        o[k] = sc[k][perm]
    ro = QS.ratios(o, **NOISY_GATE)
    new = np.argsort(perm)
    for p, q in np.argwhere(r["shared_view"] >= 0):
        a, b = new[p], new[q]
        lo, hi = min(a, b), max(a, b)
        assert ro["count"][lo, hi] == r["count"][p, q] and ro["shared_view"][lo, hi] == r["shared_view"][p, q]
        if a < b:
            assert ro["ratio"][lo, hi] == r["ratio"][p, q]
        elif r["count"][p, q] % 2 == 1:                       # the same track's z_p / z_q (at even n the lower median of 1 / x is the upper one of x):
            want = np.sort(1.0 / r["values"][(p, q)])[(r["count"][p, q] - 1) // 2]      # 1 / (z_q / z_p) is that quotient to two roundings
            assert abs(ro["ratio"][lo, hi] / want - 1.0) <= 4.5e-16
    assert list(ro["info"]) == list(r["info"])
