"""The numpy restatement of the multi-view triangulation (tests/multiview_reference.py) against synthetic ground truth on
the MegaDepth-1500 cameras (tests/multiview_support.arc_scene: views on an arc, the baseline grows with the view index).  Errors are
|X - X_true| / 7, the depth of the scene's centre.  The figures in the docstrings are those of DESIGN.md 3.16."""
import numpy as np

import multiview_reference as MR
import multiview_support as MS


def _run(sc, pixels64=False, **kw):
    return MR.triangulate_views(sc["kpts64"] if pixels64 else sc["kpts"], sc["tracks"], sc["n_views"], sc["Ks"], sc["Rs"], sc["ts"], pixels64=pixels64, **kw)


def test_noise_free_tracks_come_back_to_rounding():
    """float64 pixels: 1.6e-15 measured (bound 1e-12: a few hundred roundings of 1.1e-16 through a 3 degree baseline's 1 / 0.05 gain).
    float32 pixels: 3.4e-7 measured; the bound is the rounding of a pixel, 2^-14 px at 1000 px or more, over focal lengths above 700 px
    and the 0.05 rad of the first baseline: 6.1e-5 / 700 / 0.05 = 1.7e-6, times sqrt(2) for two coordinates."""
    for V in (2, 5, 12):
        sc = MS.arc_scene(np.random.default_rng(V), V, 500)
        r = _run(sc, pixels64=True)
        assert (r["status"] == 0).all() and (r["n_inliers"] == (sc["tracks"] >= 0).sum(axis=1)).all()
        assert MS.world_error(r["X"], sc["X"]).max() < 1e-12
        assert (r["inlier_views"] == ((sc["tracks"] >= 0) << np.arange(V)).sum(axis=1)).all()
        r = _run(sc)
        assert (r["status"] == 0).all() and MS.world_error(r["points3d"], sc["X"]).max() < 2.5e-6


def test_every_status_code_by_a_constructed_case():
    rng = np.random.default_rng(3)
    sc = MS.arc_scene(rng, 3, 40, shuffle=False)
    assert (sc["tracks"] >= 0).all()
    base = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}      # noqa: E731
    # 1: the reference view does not see the track / nothing else does / the reference pose is unusable
    s = base(); s["tracks"][:10, 0] = -1; s["tracks"][10:20, 1:] = -1; s["kpts"][0, 20:30, 0] = np.nan
    r = _run(s)
    assert (r["status"][:30] == MR.UNOBSERVED).all() and (r["status"][30:] == 0).all() and np.isnan(r["reproj_error"][:30]).all()
    s = base(); s["Rs"][0] = 0.0; s["ts"][0] = 0.0
    assert (_run(s)["status"] == MR.UNOBSERVED).all()
    # 2: no pair with a baseline (every view at the reference pose)
    s = base(); s["Rs"][:] = s["Rs"][0]; s["ts"][:] = s["ts"][0]; s["Rs"][0] = np.eye(3); s["Rs"][1:] = np.eye(3); s["ts"][:] = 0.0
    r = _run(s)
    assert (r["status"] == MR.NOT_FINITE).all() and (r["winner"] == -1).all() and np.isnan(r["reproj_error"]).all() and list(r["info"]) == [40, 0, 0, 40, 0, 0, 0, 0]
    # 3: the only other camera turned away from the scene; 4: max_depth inside the scene
    s = MS.arc_scene(np.random.default_rng(3), 2, 40, shuffle=False)
    D = np.diag([-1.0, 1.0, -1.0])
    s["Rs"][1], s["ts"][1] = D @ s["Rs"][1], D @ s["ts"][1]
    MS.reproject(s, s["X"])
    r = _run(s)
    assert (r["status"] == MR.BEHIND).all() and np.isfinite(r["reproj_error"]).all() and np.isnan(r["points3d"]).all()
    r = _run(base(), max_depth=0.3 * MS.DEPTH)
    assert (r["status"] == MR.FAR).all()
    z = (sc["X"] @ sc["Rs"][2].T + sc["ts"][2])[:, 2]
    r = _run(base(), max_depth=float(np.median(z)))        # the hypotheses pass (views 0 and 1 are nearer for some), the final gate looks at every inlier view
    assert set(np.unique(r["status"])) == {MR.VALID, MR.FAR} and (r["status"][z > np.median(z)] == MR.FAR).all()
    # 5: one of three observations 100 px off and three views asked for; the reference observation itself off
    s = base(); s["kpts"][2, :20, 0] += 100.0
    r = _run(s, min_views=3)
    assert (r["status"][:20] == MR.REPROJ).all() and (r["n_inliers"][:20] == 2).all() and (r["inlier_views"][:20] == 3).all() and (r["status"][20:] == 0).all()
    assert (_run(s)["status"] == 0).all()
    s = base(); s["kpts"][0, :20, 1] += 100.0
    assert (_run(s)["status"][:20] == MR.REPROJ).all()
    # 6: points 1e5 times as far: no parallax
    s = base(); c0 = -s["Rs"][0].T @ s["ts"][0]
    MS.reproject(s, c0 + (s["X"] - c0) * 1e5)
    r = _run(s, pixels64=True)
    assert (r["status"] == MR.PARALLAX).all() and np.isnan(r["points3d"]).all() and np.isfinite(r["reproj_error"]).all()
    assert (_run(s, pixels64=True, min_parallax_deg=0.0)["status"] == 0).all()


def test_the_refit_never_raises_the_cost():
    for seed, noise in ((1, 0.5), (2, 2.0), (3, 0.0)):
        sc = MS.arc_scene(np.random.default_rng(seed), 6, 800, noise=noise)
        MS.plant_outliers(np.random.default_rng(seed), sc)
        costs = [_run(sc, gn_iters=it)["cost1"] for it in range(0, 7)]
        r = _run(sc)
        assert (costs[0] == r["cost0"]).all() and (costs[MR.GN_ITERS] == r["cost1"]).all()
        for a, b in zip(costs, costs[1:]):
            assert (b <= a).all()
        if noise:
            assert (r["cost1"][r["refit"]] < r["cost0"][r["refit"]]).mean() > 0.99
            # GN_ITERS = 5: the mean cost stops moving after the third step (relative change below 1e-12 from 3 to 5, below 1e-6 from 1 to 2)
            m = [c[r["refit"]].mean() for c in costs]
            assert abs(m[3] - m[5]) <= 1e-9 * m[5] and m[6] <= m[5]


def test_five_views_beat_the_first_pair_at_half_a_pixel():
    """0.5 px of noise, V = 5 (baselines 3 .. 12 degrees), 2000 tracks, seed 10: median error 1.02e-3 from all views against 4.98e-3 from
    structure_reference.triangulate on the pair (0, 1) (seeds 11, 12: 0.99e-3 / 4.75e-3, 1.03e-3 / 4.69e-3): the ratio of the baselines."""
    sc = MS.arc_scene(np.random.default_rng(10), 5, 2000, noise=0.5)
    r = _run(sc)
    w, Xp, _, both = MS.pair_points(sc)
    ok, okp = r["status"] == 0, (w["status"] == 0) & both
    assert ok.sum() >= 1900 and okp.sum() >= 1900
    mv, pair = np.median(MS.world_error(r["points3d"], sc["X"])[ok]), np.median(MS.world_error(Xp, sc["X"])[okp])
    print(f"median 3D error / depth: 5 views {mv:.3e}, pair (0,1) {pair:.3e}")
    assert mv < pair


def test_planted_outliers_are_rejected():
    """V = 6, 0.5 px of noise, 2000 tracks, 30 % of the tracks with >= 4 views get one observation (of a view >= 1) moved by 50 - 150 px,
    thr = 4.  Every planted view is absent from inlier_views (exact).  Median error, seed 20: contaminated 8.60e-4, clean 7.90e-4 (seeds 21,
    22: 7.53e-4 / 7.36e-4, 8.50e-4 / 7.71e-4): a contaminated track is a clean one with a view fewer.  The margin: at worst the view lost is
    the widest of four, which takes the longest baseline from 3 steps of the arc to 2, and the depth error goes with 1 / baseline: 1.5 x."""
    rng = np.random.default_rng(20)
    sc = MS.arc_scene(rng, 6, 2000, noise=0.5)
    planted = MS.plant_outliers(rng, sc)
    bad = planted >= 0
    assert bad.sum() > 400 and ((sc["tracks"][bad] >= 0).sum(axis=1) >= 4).all()
    r = _run(sc)
    assert (((r["inlier_views"][bad] >> planted[bad]) & 1) == 0).all()
    assert (r["n_inliers"][bad] == (sc["tracks"][bad] >= 0).sum(axis=1) - 1).mean() > 0.95
    ok = r["status"] == 0
    assert ok[bad].mean() > 0.99
    e = MS.world_error(r["points3d"], sc["X"])
    cont, clean = np.median(e[ok & bad]), np.median(e[ok & ~bad])
    print(f"median 3D error / depth: contaminated {cont:.3e}, clean {clean:.3e}")
    assert cont <= 1.5 * clean


V2_LARGEST = 7.05e-4


def test_two_views_agree_with_the_two_view_triangulation():
    """V = 2: the status equals structure_reference.triangulate's on the same pair, and the refit moves Lindstrom's point (optimal in
    calibrated coordinates; the refit minimises pixels under two different focal lengths) by at most, relative to |X|: 9.7e-9 noise-free,
    2.6e-4 / 3.8e-4 / 7.0e-4 at 0.5 / 1 / 2 px (2000 tracks each, seeds 30 - 34).  Asserted at ten times the largest, 7.05e-4."""
    largest = 0.0
    for seed, noise in zip(range(30, 35), (0.0, 0.5, 1.0, 2.0, 0.5)):
        sc = MS.arc_scene(np.random.default_rng(seed), 2, 2000, noise=noise)
        r = _run(sc)
        w, _, Xp, both = MS.pair_points(sc)
        assert (r["status"][both] == w["status"][both]).all() and (r["status"][~both] == MR.UNOBSERVED).all()
        ok = r["status"] == 0
        assert ok.sum() > 1900
        d = np.linalg.norm(r["X"] - Xp, axis=1)[ok] / np.linalg.norm(Xp, axis=1)[ok]
        largest = max(largest, d.max())
    print(f"largest relative difference {largest:.3e}")
    assert largest <= 10 * V2_LARGEST


def test_track_table_is_a_maximum_scatter():
    rng = np.random.default_rng(0)
    sc = MS.arc_scene(rng, 4, 50)
    a, b, n = MS.match_lists(rng, sc["tracks"], dup=10)
    assert np.array_equal(MR.build_tracks(a, b, n, 50), sc["tracks"])
    a[0, 0], b[1, 1] = 50, -1                              # out of range: ignored
    t = MR.build_tracks(a, b, n, 50)
    assert (t[:, 0] == np.arange(50)).all() and (t != sc["tracks"]).sum() <= 2 and (t <= sc["tracks"]).all()
    n[2] = 0
    assert (MR.build_tracks(a, b, n, 50)[:, 3] == -1).all()
