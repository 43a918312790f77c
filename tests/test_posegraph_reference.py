"""The pose-graph restatement (tests/posegraph_reference.py) against the truth of synthetic scenes and against numpy.linalg on the dense
systems (CPU only).  Every bound below is a multiple of the worst figure measured on the restatement itself (DESIGN.md 3.19 records them):
ten times for what holds to rounding, twice the worst seed for what holds to the noise.  Each test prints its figures before it asserts."""
import math

import numpy as np
import pytest

import bundle_reference as BR
import posegraph_reference as PR
import posegraph_support as PS

from accelerated_features_amd.multiview import MIN_PIVOT_RATIO

KW = dict(min_pivot_ratio=MIN_PIVOT_RATIO)
# measured worst: (rotation degrees, relative centre error)
NOISE_FREE = {("all", 2): (0.0, 6.2e-17), ("all", 3): (5.7e-16, 6.0e-16), ("all", 4): (1.1e-14, 8.8e-16), ("all", 8): (1.6e-14, 1.2e-14),
              ("all", 32): (2.5e-14, 3.2e-14), ("near", 8): (1.9e-14, 1.9e-14), ("near", 32): (3.6e-14, 5.3e-13)}
NOISY = {4: (0.765, 3.21e-2), 32: (0.517, 1.78e-2)}                  # sigma 0.5 degrees, all pairs, the worst of seeds 1-3
OUTLIERS = {8: (0.865, 3.63e-2), 32: (0.551, 2.15e-2)}               # the same with 15 % outlier edges
EPS = 2.0 ** -52                                                     # no figure is measured below one rounding: the floor of every bound


def _pairs(kind, V):
    return PS.all_pairs(V) if kind == "all" else PS.near_pairs(V)


@pytest.mark.parametrize("kind,V", sorted(NOISE_FREE))
def test_noise_free_scenes_recover_the_truth_to_rounding(kind, V):
    sc = PS.scene(100 + V, V, _pairs(kind, V))
    r = PS.run(sc, **KW)
    rot, cen = PS.errors(sc, r["Rs"], r["ts"])
    print(f"noise-free {kind} V {V}: rotation {rot:.3e} deg, centres {cen:.3e}, info {list(r['info'])}")
    assert r["info"][6] == PR.ST_OK and r["info"][1] == V and r["registered"] == (1 << V) - 1
    wr, wc = NOISE_FREE[(kind, V)]
    assert rot <= 10.0 * max(wr, math.degrees(EPS)) and cen <= 10.0 * max(wc, EPS)
    assert r["info"][3] == 0 and r["info"][4] == 0 and np.all(r["edge_factor"] > 0.99)


def test_two_views_give_back_the_edge():
    sc = PS.scene(7, 2, PS.all_pairs(2), 0.5)
    sc["trel"] = sc["trel"] * 3.7
    r = PS.run(sc, **KW)
    dR, dt = np.abs(r["Rs"][1] - sc["Rrel"][0]).max(), np.abs(r["ts"][1] - sc["trel"][0] / np.linalg.norm(sc["trel"][0])).max()
    print(f"V 2: |R_1 - R_rel| {dR:.3e}, |t_1 - t_rel / |t_rel|| {dt:.3e}")
    assert r["info"][6] == PR.ST_OK
    assert dR <= 10.0 * EPS and dt <= 10.0 * 2.3e-16                           # measured 0 and 2.3e-16
    assert np.array_equal(r["Rs"][0], np.eye(3)) and np.array_equal(r["ts"][0], np.zeros(3))


def test_one_round_of_each_solve_against_numpy_linalg():
    worst = [0.0, 0.0]
    for V, pairs in ((8, PS.all_pairs(8)), (32, PS.all_pairs(32)), (32, PS.near_pairs(32))):
        sc = PS.scene(40 + V, V, pairs, 0.5)
        d = PS.run(sc, iterations=1, redescend=0, **KW)["dump"]
        L = np.tril(d["lap"]) + np.tril(d["lap"], -1).T
        want = np.linalg.solve(L, d["lap_rhs"])
        worst[0] = max(worst[0], np.abs(d["lap_sol"] - want).max() / np.abs(want).max())
        A = d["pos_A"] + np.tril(d["pos_A"], -1).T
        want = np.linalg.solve(A, d["pos_g"])
        worst[1] = max(worst[1], np.abs(d["pos_sol"] - want).max() / np.abs(want).max())
        assert d["pos_ok"] and d["lap_ok"]
    print(f"one round against numpy.linalg.solve: laplacian {worst[0]:.3e}, positions {worst[1]:.3e} (relative to the largest entry)")
    assert worst[0] <= 10.0 * 4.4e-15 and worst[1] <= 10.0 * 1.2e-12           # measured 4.4e-15 and 1.2e-12


@pytest.mark.parametrize("V", sorted(NOISY))
def test_half_a_degree_of_noise(V):
    got = []
    for seed in (1, 2, 3):
        sc = PS.scene(seed, V, PS.all_pairs(V), 0.5)
        r = PS.run(sc, **KW)
        assert r["info"][6] == PR.ST_OK
        got.append(PS.errors(sc, r["Rs"], r["ts"]))
    print(f"sigma 0.5 deg, V {V}, all pairs, seeds 1-3 (rotation deg, centres): {got}")
    assert max(g[0] for g in got) <= 2.0 * NOISY[V][0] and max(g[1] for g in got) <= 2.0 * NOISY[V][1]


@pytest.mark.parametrize("V", sorted(OUTLIERS))
def test_outlier_edges_are_found_and_do_not_move_the_poses(V):
    """15 % of the edges are outliers, all pairs.  An edge counts as flagged when both final factors are < 0.5.  Measured on seeds 1-3: no
    outlier edge is missed and no clean edge is flagged at either V (share of exceptions 0 %; the cap is 5 % of the edges).  Clean edges
    with ONE factor < 0.5 exist (V = 8: none; V = 32: up to 6 of 496): their direction or rotation alone is in the noise's tail."""
    got = []
    for seed in (1, 2, 3):
        sc = PS.scene(seed, V, PS.all_pairs(V), 0.5, 0.15)
        r = PS.run(sc, **KW)
        f, o = r["edge_factor"], sc["outlier"]
        flagged = (f[:, 0] < 0.5) & (f[:, 1] < 0.5)
        wrong = int((o & ~flagged).sum() + (~o & flagged).sum())
        one = int((~o & ((f[:, 0] < 0.5) | (f[:, 1] < 0.5))).sum())
        got.append(PS.errors(sc, r["Rs"], r["ts"]) + (wrong, one, int(o.sum())))
        assert r["info"][6] == PR.ST_OK
        assert wrong <= 0.05 * o.shape[0], (seed, wrong)
    print(f"15 % outliers, V {V}, seeds 1-3 (rotation deg, centres, exceptions, clean edges with one factor < 0.5, outliers): {got}")
    assert max(g[0] for g in got) <= 2.0 * OUTLIERS[V][0] and max(g[1] for g in got) <= 2.0 * OUTLIERS[V][1]


def test_graphs_that_are_not_rigid_give_rotations_only():
    cases = [("chain 8", 8, PS.chain_pairs(8), 0.0), ("chain 8", 8, PS.chain_pairs(8), 0.5), ("chain 32", 32, PS.chain_pairs(32), 0.5),
             ("two triangles", 5, PS.TWO_TRIANGLES, 0.0)]
    for name, V, pairs, sigma in cases:
        for seed in (1, 2, 3):
            sc = PS.scene(seed, V, pairs, sigma)
            r = PS.run(sc, **KW)
            rot = max(PS.angle_deg(r["Rs"][v], sc["Rs"][v]) for v in range(V))
            print(f"{name} sigma {sigma} seed {seed}: status {r['info'][6]}, pivot ratios {r['ratios']}, rotation {rot:.3e} deg")
            assert r["info"][6] == PR.ST_ROTATIONS_ONLY and r["registered"] == (1 << V) - 1
            # (a chain adds the noise of its edges up: 3 (V - 1) draws of sigma at the far end; four of their standard deviations)
            assert np.all(np.isfinite(r["Rs"])) and rot <= (1e-9 if sigma == 0.0 else 4.0 * sigma * math.sqrt(3.0 * (V - 1)))
            assert np.array_equal(r["ts"][0], np.zeros(3)) and np.all(np.isnan(r["ts"][1:]))
            assert np.all(r["edge_factor"][:, 1] == 0.0) and np.all(r["edge_factor"][:, 0] > 0.0) and r["info"][4] == 0


def test_a_view_without_a_valid_edge_is_unregistered_and_the_rest_is_solved():
    sc = PS.scene(11, 8, PS.all_pairs(8), 0.5)
    touch = (sc["pairs"] == 5).any(axis=1)
    sc["weight"][touch] = 0.0
    r = PS.run(sc, **KW)
    assert r["info"][6] == PR.ST_OK and r["registered"] == 0xFF & ~(1 << 5) and r["info"][1] == 7 and r["info"][0] == 21 and r["info"][5] == 18
    assert np.all(np.isnan(r["Rs"][5])) and np.all(np.isnan(r["ts"][5])) and np.all(r["edge_factor"][touch] == 0.0)
    rot, cen = PS.errors(sc, r["Rs"], r["ts"], r["registered"])
    print(f"view 5 cut off: rotation {rot:.3f} deg, centres {cen:.3e}")
    assert rot <= 2.0 * NOISY[4][0] and cen <= 2.0 * NOISY[4][1]
    # two components: only view 0's is solved, the edges of the other drop out
    sc = PS.scene(12, 6, np.array([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)], np.int32))
    r = PS.run(sc, **KW)
    assert r["registered"] == 0b000111 and r["info"][0] == 6 and np.all(r["edge_factor"][3:] == 0.0) and np.all(r["edge_factor"][:3] > 0.0)
    assert np.all(np.isnan(r["Rs"][3:])) and r["info"][6] == PR.ST_OK


def test_no_valid_edge_at_view_0_is_status_nothing():
    sc = PS.scene(13, 4, PS.all_pairs(4), 0.5)
    sc["weight"][(sc["pairs"] == 0).any(axis=1)] = 0.0
    r = PS.run(sc, **KW)
    assert r["info"][6] == PR.ST_NOTHING and r["registered"] == 1 and r["info"][1] == 1 and r["info"][0] == 3 and r["info"][5] == 0
    assert np.array_equal(r["Rs"][0], np.eye(3)) and np.array_equal(r["ts"][0], np.zeros(3))
    assert np.all(np.isnan(r["Rs"][1:])) and np.all(np.isnan(r["ts"][1:])) and np.all(r["edge_factor"] == 0.0)


def test_a_nan_in_one_relative_rotation_drops_that_edge_alone():
    sc = PS.scene(14, 8, PS.all_pairs(8), 0.5)
    base = PS.run(sc, **KW)
    sc["Rrel"][9, 2, 0] = np.nan
    r = PS.run(sc, **KW)
    assert r["info"][6] == PR.ST_OK and r["info"][0] == 27 and r["registered"] == 0xFF and np.all(r["edge_factor"][9] == 0.0)
    assert np.all(r["edge_factor"][np.arange(28) != 9] > 0.0)
    assert np.abs(r["Rs"] - base["Rs"]).max() < 0.05 and np.all(np.isfinite(r["ts"]))
    # an edge without a direction still takes part in the rotations
    sc = PS.scene(14, 8, PS.all_pairs(8), 0.5)
    sc["trel"][9] = 0.0
    r = PS.run(sc, **KW)
    assert r["info"][6] == PR.ST_OK and r["info"][0] == 28 and r["info"][2] == 27 and r["edge_factor"][9, 0] > 0.0 and r["edge_factor"][9, 1] == 0.0


def test_permuting_the_pairs_leaves_the_registration_and_the_status():
    rng = np.random.default_rng(15)
    for sc in (PS.scene(15, 8, PS.near_pairs(8), 0.5), PS.scene(16, 8, PS.chain_pairs(8), 0.5), PS.scene(17, 8, PS.all_pairs(8), 0.5, 0.15)):
        sc["weight"][(sc["pairs"] == 6).any(axis=1)] = 0.0
        a = PS.run(sc, **KW)
        perm = rng.permutation(sc["pairs"].shape[0])
        for k in ("pairs", "Rrel", "trel", "weight"):
            sc[k] = sc[k][perm]
        b = PS.run(sc, **KW)
        assert a["registered"] == b["registered"] and a["info"][6] == b["info"][6] and list(a["info"][:3]) == list(b["info"][:3])
        assert np.nanmax(np.abs(a["Rs"] - b["Rs"])) < 1e-9


def test_duplicate_and_swapped_pairs_agree():
    """Every edge twice doubles every weight, which moves no minimum: the noisy scene agrees to 1e-9.  An edge given as (b, a) with the
    inverted pose uses R_a' R_rel' in place of R_b' for its direction, which is the same only where R_b = R_rel R_a: the swapped scene is
    noise-free."""
    sc = PS.scene(18, 8, PS.all_pairs(8), 0.5)
    a, b = PS.run(sc, **KW), PS.run(PS.repeat_edges(sc, 56), **KW)
    assert np.abs(a["Rs"] - b["Rs"]).max() < 1e-9 and np.abs(a["ts"] - b["ts"]).max() < 1e-9
    assert np.abs(a["edge_factor"] - b["edge_factor"][:28]).max() < 1e-9 and np.abs(a["edge_factor"] - b["edge_factor"][28:]).max() < 1e-9
    sc = PS.scene(19, 8, PS.all_pairs(8))
    a, b = PS.run(sc, **KW), PS.run(PS.swap_edges(sc, [0, 3, 4, 11, 20, 27]), **KW)
    assert a["info"][6] == b["info"][6] == PR.ST_OK
    assert np.abs(a["Rs"] - b["Rs"]).max() < 1e-9 and np.abs(a["ts"] - b["ts"]).max() < 1e-9


def test_block_sums_order_is_the_library_s():
    """pg_sum's order, restated here by hand for a length that is no multiple of 256, against oracle.twoview_reference.block_sums."""
    x = np.random.default_rng(20).normal(size=600) * 10.0 ** np.random.default_rng(21).integers(-8, 8, 600)
    acc = np.zeros(256)
    for p in range(600):
        acc[p % 256] = acc[p % 256] + x[p]
    q = [np.float64(0.0)] * 8
    for j in range(8):
        for i in range(32):
            q[j] = q[j] + acc[32 * j + i]
    want = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))
    assert PR.edge_sum(x) == want
    assert BR.cholesky_solve(np.eye(2), np.ones(2))[0]
