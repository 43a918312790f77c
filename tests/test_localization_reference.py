"""The numpy restatement tests/localization_reference.py of DESIGN.md 3.21 against float64 and against constructed cases: the descriptor of a
track against the float64 normalised mean, every skip reason and their precedence, view 31, rows outside the table, rows that are not finite,
antipodal observations, the capacity, the independence of a row from the other tracks, and the NaN cases of the projection."""
import numpy as np

import localization_reference as LR
import localization_support as LS

U = 2.0 ** -24                                             # unit round-off of fp32


def _scene(V=4, T=6, kcap=8, seed=0):
    """T tracks seen by all V views at rows of their own: everything selected."""
    rng = np.random.default_rng(seed)
    base = LS.unit_rows(rng, T)
    desc = np.stack([LS.unit_rows(rng, kcap).astype(np.float32) for _ in range(V)])
    tracks = np.zeros((T, V), np.int32)
    for v in range(V):
        tracks[:, v] = rng.permutation(kcap)[:T]
        desc[v, tracks[:, v]] = LS.observe(rng, base, 0.05)
    return [desc, tracks, rng.normal(size=(T, 3)).astype(np.float32), np.zeros(T, np.uint8), np.full(T, (1 << V) - 1, np.uint32).view(np.int32)]


def test_the_descriptor_is_the_normalised_mean_to_the_bound_of_its_fp32_sums():
    """Per component the sum of n unit rows takes n - 1 roundings of partial sums of magnitude <= n: |d sum| <= (n - 1) n u.  The squared norm
    takes 8 roundings per path (a product, 3 additions in the lane, 4 in the tree), the root one, the inverse one, the product one: with the
    error of the sum carried through the norm (|d sum|_2 <= 8 |d sum|_inf), |d desc| <= 9 (n - 1) n u / r + 7 u."""
    worst = 0.0
    for V, sigma, seed in ((2, 0.05, 1), (4, 0.05, 2), (8, 0.3, 3), (32, 0.05, 4), (32, 1.0, 5)):
        rng = np.random.default_rng(seed)
        T = 200
        base = LS.unit_rows(rng, T)
        desc = np.stack([LS.observe(rng, base, sigma) for _ in range(V)])
        tracks = np.tile(np.arange(T, dtype=np.int32)[:, None], (1, V))
        m = LR.build_map(desc, tracks, np.ones((T, 3), np.float32), np.zeros(T, np.uint8), np.full(T, -1 if V == 32 else (1 << V) - 1, np.int32))
        assert m["n_points"] == T and (m["n_obs"] == V).all()
        s = desc.astype(np.float64).sum(axis=0)
        r = np.linalg.norm(s, axis=1)
        err = np.abs(m["desc"].astype(np.float64) - s / r[:, None]).max(axis=1)
        bound = 9 * (V - 1) * V * U / r + 7 * U
        assert (err <= bound).all(), (V, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        assert np.abs(m["coherence"] - r / V).max() <= 1e-6 and (m["coherence"] <= 1 + 1e-6).all()
        assert (m["coherence"].mean() > 0.9) == (sigma == 0.05)      # (about 1 / sqrt(1 + 64 sigma^2) for many views: 0.93, 0.38, 0.12)
        assert np.array_equal(m["desc_f16"], (m["desc"] * np.float32(256)).astype(np.float16))
        assert np.abs(np.linalg.norm(m["desc"].astype(np.float64), axis=1) - 1).max() <= 4e-7
    print(f"largest error / bound {worst:.3f}")


def test_every_skip_reason_and_their_precedence():
    a = _scene(T=8)
    desc, tracks, points, status, mask = a
    status[1] = 3                                          # 1: status
    points[2, 1] = np.inf                                  # 2: point
    mask[3] = 1 << 2                                       # 3: one view only
    desc[1, tracks[4, 1]] = -desc[0, tracks[4, 0]]         # 4: two antipodal observations
    mask[4] = 3
    status[5], points[5, 0], mask[5] = 6, np.nan, 0        # status before point before views
    points[6, 2], mask[6] = -np.inf, 0                     # point before views
    desc[1, tracks[7, 1]] = -desc[0, tracks[7, 0]]         # one contributing view (the other masked out): views before norm
    mask[7] = 2
    m = LR.build_map(*a, min_views=2)
    assert list(m["rows"]["flag"]) == [0, 1, 2, 3, 4, 1, 2, 3]
    assert list(m["info"]) == [8, 1, 2, 2, 2, 1, 0, 0] and m["n_points"] == 1 and list(m["track"]) == [0] + [-1] * 7
    assert m["rows"]["n2"][4] == 0.0
    # the rows past the count
    assert np.isnan(m["points"][1:]).all() and not m["desc"][1:].any() and not m["desc_f16"][1:].any() and not m["n_obs"][1:].any()
    assert not m["coherence"][1:].any()
    # with min_views = 1 track 3 and track 7 are selected
    m = LR.build_map(*a, min_views=1)
    assert list(m["track"][:3]) == [0, 3, 7] and list(m["n_obs"][:3]) == [4, 1, 1] and list(m["info"]) == [8, 3, 2, 2, 0, 1, 0, 0]
    assert np.array_equal(m["desc"][1], desc[2, tracks[3, 2]] * (np.float32(1) / np.sqrt(LR.norm2(desc[2, tracks[3, 2]][None])[0])))
    assert m["points"][1].tobytes() == points[3].tobytes()


def test_view_31_is_the_sign_bit():
    a = _scene(V=32, T=4, kcap=4)
    a[4][:] = [np.int32(-2 ** 31), np.int32(-2 ** 31) | 1, 1, -1]
    m = LR.build_map(*a, min_views=1)
    assert list(m["n_obs"]) == [1, 2, 1, 32]
    assert np.array_equal(LR.contributing(a[0], a[1], a[4])[:, 31], [True, True, False, True])
    assert np.abs(m["desc"][0] - a[0][31, a[1][0, 31]]).max() <= 2e-7


def test_rows_outside_the_table_and_rows_that_are_not_finite_do_not_contribute():
    a = _scene(V=4, T=5, kcap=8)
    desc, tracks = a[0], a[1]
    tracks[0, 0], tracks[1, 1], tracks[2, 2] = -1, 8, 2 ** 31 - 1
    desc[3, tracks[3, 3], 17] = np.nan
    desc[0, tracks[4, 0], 63] = np.inf
    m = LR.build_map(*a, min_views=2)
    assert list(m["n_obs"]) == [3, 3, 3, 3, 3] and np.isfinite(m["desc"]).all()
    want = LR.build_map(desc[[1, 2, 3]], tracks[:1, [1, 2, 3]], a[2][:1], a[3][:1], np.array([7], np.int32))
    assert np.array_equal(m["desc"][0], want["desc"][0])
    a[4][:] = 1 | 2                                        # tracks 0 and 1 keep one view
    m = LR.build_map(*a, min_views=2)
    assert list(m["rows"]["flag"]) == [3, 3, 0, 0, 3]


def test_max_points_below_the_selected_count():
    a = _scene(T=6)
    a[3][2] = 1
    full = LR.build_map(*a)
    m = LR.build_map(*a, max_points=3)
    assert list(full["track"]) == [0, 1, 3, 4, 5, -1] and list(m["track"]) == [0, 1, 3]
    assert list(m["info"]) == [6, 3, 1, 0, 0, 0, 2, 0] and m["n_points"] == 3
    for k in ("desc", "points", "coherence", "n_obs", "desc_f16"):
        assert np.array_equal(m[k], full[k][:3]), k
    m = LR.build_map(*a, max_points=9)
    assert m["desc"].shape == (9, 64) and m["n_points"] == 5 and list(m["track"][5:]) == [-1] * 4


def test_a_row_does_not_depend_on_what_the_other_tracks_hold():
    rng = np.random.default_rng(3)
    a = LS.map_inputs(rng, 8, 200, 32)
    full = LR.build_map(*a)
    order = rng.permutation(200)
    b = (a[0],) + tuple(np.ascontiguousarray(x[order]) for x in a[1:])
    perm = LR.build_map(*b)
    n = int(full["n_points"])
    assert n == perm["n_points"] and n > 30 and list(full["info"]) == list(perm["info"])
    back = {int(order[t]): j for j, t in enumerate(perm["track"][:n])}
    for j, t in enumerate(full["track"][:n]):
        for k in ("desc", "desc_f16", "coherence", "points", "n_obs"):
            assert full[k][j].tobytes() == perm[k][back[int(t)]].tobytes(), k


def test_the_nan_cases_of_the_projection():
    K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
    pts = np.array([[0, 0, 2], [0, 0, -2], [0, 0, 0], [np.nan, 0, 2], [0, np.inf, 2], [2, 0, 2], [-1.3125, 0, 2], [0, 0, 2]], np.float32)
    uv = LR.project(pts, 7, np.eye(3), np.zeros(3), K)
    assert np.array_equal(uv[0], [320, 240]) and np.array_equal(uv[5], [820, 240]) and np.array_equal(uv[6], [-8.125, 240])
    assert np.isnan(uv[[1, 2, 3, 4, 7]]).all()
    uv = LR.project(pts, None, np.eye(3), np.zeros(3), K, (640, 480), 8.5)
    assert np.isnan(uv[5]).all() and np.array_equal(uv[6], [-8.125, 240]) and np.array_equal(uv[7], [320, 240])
    uv = LR.project(pts, None, np.eye(3), np.zeros(3), K, (640, 480), 8.0)
    assert np.isnan(uv[6]).all()
    assert np.isnan(LR.project(pts, None, np.zeros((3, 3)), np.zeros(3), K)).all()          # the pose of "nothing found"
    assert np.isnan(LR.project(pts, None, np.full((3, 3), np.nan), np.zeros(3), K)).all()
    # float64 then one rounding: against longdouble
    rng = np.random.default_rng(0)
    X = (rng.normal(size=(500, 3)) + [0, 0, 5]).astype(np.float32)
    R, t = np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(size=3)
    uv = LR.project(X, None, R, t, K)
    Xc = X.astype(np.longdouble) @ R.T.astype(np.longdouble) + t
    ok = Xc[:, 2] > 0
    ref = np.stack([500 * Xc[:, 0] / Xc[:, 2] + 320, 500 * Xc[:, 1] / Xc[:, 2] + 240], axis=1)
    assert np.array_equal(np.isnan(uv[:, 0]), ~ok)
    assert (np.abs(uv[ok].astype(np.longdouble) - ref[ok]) <= np.abs(ref[ok]) * 2.0 ** -24 + 1e-9).all()


def test_the_float64_matcher_and_its_margins():
    rng = np.random.default_rng(1)
    base = LS.unit_rows(rng, 50)
    a, b = LS.observe(rng, base, 0.05), LS.observe(rng, base[::-1], 0.05)
    i0, i1, margin = LR.mnn(a, 40, b, 50, 0.7)
    assert np.array_equal(i0, np.arange(40)) and np.array_equal(i1, 49 - np.arange(40)) and margin > 0.02
    i0, i1, _ = LR.mnn(a, 40, b, 30, 0.8)                  # rows 20 .. 39 lost their partner
    assert np.array_equal(i0, np.arange(20, 40))
    assert len(LR.mnn(a, 0, b, 50)[0]) == 0 and len(LR.mnn(a, 40, b, 0)[0]) == 0
    b2 = b.copy()
    b2[7] = b2[9]                                          # a tie: margin 0
    assert LR.mnn(a, 50, b2, 50)[2] == 0.0
    assert LR.mnn(a, 1, b, 1)[2] == np.inf and abs(LR.mnn(a, 1, b[::-1], 1, 0.5)[2] - (float(a[0].astype(np.float64) @ b[49]) - 0.5)) < 1e-15
