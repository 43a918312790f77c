"""xfh_triangulate / xfh_recover_pose (csrc/k_triangulate.hip) on the MI355X against the numpy restatement tests/structure_reference.py,
given the same R and t (or E) on both sides: status, valid, info, good and inliers exactly, the points and the reprojection error as float32
bits (fp contraction is off and fp64 division and square root are correctly rounded on both sides).  Through the restatement every
comparison first asserts that no correspondence of its scene lies within relative 1e-9 of a gate, so a last-bit difference could not
flip a status."""
import math

import numpy as np
import pytest
import torch

import abspose_reference as AR
import pose_reference as PR
import structure_reference as SR
import structure_support as SS
import twoview_support as TS

pytestmark = pytest.mark.gpu
K = SS.K


@pytest.fixture(scope="module")
def st():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import structure as m
    return m


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_f32(got, want):
    """float32 arrays equal as bits, any NaN equal to any NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _gates(g):
    return dict(max_reproj_error=g["thr"], min_parallax_deg=g["deg"], max_depth=g["max_depth"])


def _check_tri(got, p, n, want, cap):
    status = got["status"][p].cpu().numpy()
    assert np.array_equal(status[:n], want["status"]), np.nonzero(status[:n] != want["status"])[0][:8]
    assert (status[n:] == SR.MASKED).all()
    assert np.array_equal(got["valid"][p].cpu().numpy(), status == 0)
    assert list(got["info"][p].cpu().numpy()) == list(want["info"]), (got["info"][p], want["info"])
    X, err = got["points3d"][p].cpu().numpy(), got["reproj_error"][p].cpu().numpy()
    assert _same_f32(X[:n], want["points3d"]) and _same_f32(err[:n], want["reproj_error"])
    assert np.isnan(X[n:]).all() and np.isnan(err[n:]).all()
    assert np.isfinite(X[status == 0]).all() and np.isnan(X[status != 0]).all()          # no NaN outside rows of status != 0, NaN in all of those
    assert X.shape == (cap, 3)


def _group(seed, n, kind):
    """A scene of test_structure_emulated's kinds with n correspondences whose gates are clear of every correspondence."""
    rng = np.random.default_rng(seed)
    while True:
        g = SS.mixed_group(rng, kind, max(n, 8))
        for k in ("p0", "p1"):
            g[k] = g[k][:n]
        if g["mask"] is not None:
            g["mask"] = g["mask"][:n]
        w = SR.triangulate(g["p0"], g["p1"], K, K, g["R"], g["t"], g["thr"], g["deg"], g["max_depth"], g["mask"])
        if SR.gate_margin(w, g["max_depth"]) > 1e-9:
            return g, w


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300, 1200])
def test_single_pair_equals_the_restatement(st, n):
    """The wave and workgroup edges of a thread-per-correspondence kernel and the ballot counts around them; noisy scene with tight gates
    and a mask (kind 5: every status but 'not finite') and the camera-behind / far / NaN scene (kind 3)."""
    for kind in (5, 3):
        g, want = _group(1000 * kind + n, n, kind)
        cap = max(n, 1)
        p0, c = SS.pack([g["p0"]], cap)
        p1, _ = SS.pack([g["p1"]], cap)
        mask = None if g["mask"] is None else torch.from_numpy(np.pad(g["mask"], (0, cap - n))[None]).cuda()
        a, b = _cuda(p0, p1)
        got = st.triangulate_batch(a, b, torch.from_numpy(c), K, K, g["R"], g["t"], mask=mask, **_gates(g))
        torch.cuda.synchronize()
        _check_tri(got, 0, n, want, cap)
        if n >= 300 and kind == 5:
            assert (np.bincount(want["status"], minlength=7) > 0).sum() >= 4
    if n == 1200:                                          # counts = None: all cap rows
        got = st.triangulate_batch(a, b, None, K, K, g["R"], g["t"], mask=mask, **_gates(g))
        _check_tri(got, 0, n, want, cap)


def _ragged(ns, seed=3):
    rng = np.random.default_rng(seed)
    f = TS.fixture()
    P = len(ns)
    l0, l1, R, t, K0, K1, wants, masks = [], [], np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros((P, 3, 3)), np.zeros((P, 3, 3)), [], []
    for p, n in enumerate(ns):
        K0[p], K1[p], T = f["K0"][p], f["K1"][p], f["T_0to1"][p]
        while True:
            a, b, _ = TS.fixture_pair(f, p, max(n, 1), 1.0, 0.3, rng)
            a, b = a[:n], b[:n]
            R[p], t[p] = T[:3, :3], T[:3, 3] / np.linalg.norm(T[:3, 3])
            m = (rng.random(n) > 0.1).astype(np.uint8)
            w = SR.triangulate(a, b, K0[p], K1[p], R[p], t[p], 2.0, 1.0, 12.0, m)
            if SR.gate_margin(w, 12.0) > 1e-9:
                break
        l0.append(a); l1.append(b); wants.append(w); masks.append(m)
    return l0, l1, R, t, K0, K1, wants, masks


def test_ragged_batch_with_per_pair_intrinsics(st):
    ns = [300, 3, 0, 1200, 57, 2]
    l0, l1, R, t, K0, K1, wants, masks = _ragged(ns)
    p0, c = SS.pack(l0)
    p1, _ = SS.pack(l1)
    cap = p0.shape[1]
    mask = np.zeros((len(ns), cap), np.uint8)
    for p, m in enumerate(masks):
        mask[p, :len(m)] = m
    a, b, mk = _cuda(p0, p1, mask)
    kw = dict(max_reproj_error=2.0, min_parallax_deg=1.0, max_depth=12.0)
    got = st.triangulate_batch(a, b, torch.from_numpy(c), K0, K1, R, t, mask=mk, **kw)
    again = st.triangulate_batch(a, b, torch.from_numpy(c), K0, K1, R, t, mask=mk, **kw)
    torch.cuda.synchronize()
    for p, n in enumerate(ns):
        _check_tri(got, p, n, wants[p], cap)
    for k in ("points3d", "reproj_error"):                 # two calls, the same bits
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(again[k].cpu().numpy()))
    for k in ("status", "info", "valid"):
        assert torch.equal(got[k], again[k])
    unmasked = st.triangulate_batch(a, b, torch.from_numpy(c), K0, K1, R, t, **kw)      # the mask is honoured: only masked rows change
    s0, s1 = got["status"].cpu().numpy(), unmasked["status"].cpu().numpy()
    for p, n in enumerate(ns):
        assert ((s0[p, :n] == SR.MASKED) == (mask[p, :n] == 0)).all() and (s1[p, :n] != SR.MASKED).all()
        keep = mask[p, :n] != 0
        assert np.array_equal(s0[p, :n][keep], s1[p, :n][keep])


def test_index_list_entry_equals_the_batch_entry_and_scatters(st):
    ns = [300, 3, 0, 1200, 57, 2]
    l0, l1, R, t, K0, K1, wants, _ = _ragged(ns, seed=4)
    rng = np.random.default_rng(0)
    P, Kp, cap = len(ns), 1500, max(ns)
    k0, k1 = rng.uniform(0, 640, (P, Kp, 2)).astype(np.float32), rng.uniform(0, 480, (P, Kp, 2)).astype(np.float32)
    idx0, idx1 = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64)
    for p, n in enumerate(ns):
        idx0[p, :n], idx1[p, :n] = rng.permutation(Kp)[:n], rng.permutation(Kp)[:n]      # one to one
        k0[p, idx0[p, :n]], k1[p, idx1[p, :n]] = l0[p], l1[p]
    g0, g1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    for p, n in enumerate(ns):
        g0[p, :n], g1[p, :n] = k0[p, idx0[p, :n]], k1[p, idx1[p, :n]]
    kw = dict(max_reproj_error=2.0, min_parallax_deg=1.0, max_depth=12.0)
    c = torch.tensor(ns, dtype=torch.int32).cuda()
    a, b, i0, i1, ga, gb = _cuda(k0, k1, idx0, idx1, g0, g1)
    got = st.triangulate_matches(a, b, i0, i1, c, K0, K1, R, t, **kw)
    ref = st.triangulate_batch(ga, gb, c, K0, K1, R, t, **kw)
    plain = st.triangulate_matches(a, b, i0, i1, c, K0, K1, R, t, scatter=False, **kw)
    torch.cuda.synchronize()
    assert "points3d_ref" not in plain and "points3d_ref" in got
    for k in ("points3d", "reproj_error"):
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(ref[k].cpu().numpy()))
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(plain[k].cpu().numpy()))
    for k in ("status", "info", "valid"):
        assert torch.equal(got[k], ref[k])
    X, Xref = got["points3d"].cpu().numpy(), got["points3d_ref"].cpu().numpy()
    assert Xref.shape == (P, Kp, 3)
    for p, n in enumerate(ns):
        want = np.full((Kp, 3), np.nan, np.float32)
        want[idx0[p, :n]] = X[p, :n]
        assert _same_f32(Xref[p], want)
        assert np.isfinite(Xref[p]).all(axis=1).sum() == int(got["info"][p, 1])
    # an index out of range is "not finite", and nothing is written for it
    bad = idx0.copy()
    bad[0, 5], bad[3, 7] = Kp, -1
    (ib,) = _cuda(bad)
    r = st.triangulate_matches(a, b, ib, i1, c, K0, K1, R, t, **kw)
    s = r["status"].cpu().numpy()
    assert s[0, 5] == SR.NOT_FINITE and s[3, 7] == SR.NOT_FINITE
    s[0, 5], s[3, 7] = got["status"][0, 5].item(), got["status"][3, 7].item()
    assert np.array_equal(s, got["status"].cpu().numpy())


def test_degenerate_batch(st):
    """collinear / identical / all behind / NaN rows / nothing finite / a zeroed pose: no fault, no NaN outside rows of status != 0, info equal
    to the restatement's."""
    rng = np.random.default_rng(9)
    n = 200
    cases = []
    s = SS.scene(rng, n)
    X = s["X"].copy(); X[:] = X[0] + np.outer(np.linspace(0, 1, n), X[1] - X[0])            # collinear
    cases.append((SS.project_points(X, s["R"], s["t"]), s["R"], s["t"]))
    X = np.repeat(s["X"][:1], n, axis=0)                                                     # identical
    cases.append((SS.project_points(X, s["R"], s["t"]), s["R"], s["t"]))
    tb = np.array([0.1, 0.0, -10.0])                                                         # all behind camera 1
    cases.append((SS.project_points(s["X"], s["R"], tb), s["R"], tb))
    p0, p1 = (v.copy() for v in SS.project_points(s["X"], s["R"], s["t"]))
    p0[::3, 0] = np.nan; p1[1::7] = np.inf                                                   # NaN rows
    cases.append(((p0, p1), s["R"], s["t"]))
    cases.append(((np.full((n, 2), np.nan), np.full((n, 2), np.nan)), s["R"], s["t"]))      # nothing finite
    cases.append((SS.project_points(s["X"], s["R"], s["t"]), np.zeros((3, 3)), np.zeros(3)))   # a zeroed pose
    p0, c = SS.pack([v[0][0] for v in cases])
    p1, _ = SS.pack([v[0][1] for v in cases])
    R, t = np.stack([v[1] for v in cases]), np.stack([v[2] for v in cases])
    a, b = _cuda(p0, p1)
    got = st.triangulate_batch(a, b, torch.from_numpy(c), K, K, R, t)
    torch.cuda.synchronize()
    for p in range(len(cases)):
        want = SR.triangulate(p0[p], p1[p], K, K, R[p], t[p])
        assert list(got["info"][p].cpu().numpy()) == list(want["info"]), p
        status, X = got["status"][p].cpu().numpy(), got["points3d"][p].cpu().numpy()
        assert np.isfinite(X[status == 0]).all() and np.isnan(X[status != 0]).all()
        assert _same_f32(X, want["points3d"]) and np.array_equal(status, want["status"])
    info = got["info"].cpu().numpy()
    assert info[2, 4] == n and info[4, 3] == n and info[5, 3] == n and info[3, 3] >= n // 3
    # recover pose on the same rows: an E of a real pose, then a zero E
    E = np.stack([TS.essential_from_pose(s["R"], s["t"])] * 5 + [np.zeros((3, 3))])
    r = st.recover_pose_batch(E, a, b, torch.from_numpy(c), K, K)
    torch.cuda.synchronize()
    for p in range(len(cases)):
        want = SR.recover_pose(E[p], p0[p], p1[p], K, K)
        assert list(r["good"][p].cpu().numpy()) == list(want["good"]) and list(r["info"][p].cpu().numpy()) == list(want["info"]), p
        assert np.array_equal(r["inliers"][p].cpu().numpy(), want["mask"])
    assert not r["info"][5, 0] and not r["R"][5].any() and not r["info"][4, 0]


@pytest.mark.parametrize("scale", SS.SCALES)
def test_recover_pose_batch_on_scaled_E(st, scale):
    rng = np.random.default_rng(5)
    ns = [60, 300, 5, 1, 700, 0]
    scenes = [SS.scene_in_front(rng, max(n, 1), noise=0.5 if p % 2 else 0.0, min_t=0.5) for p, n in enumerate(ns)]
    l0, l1 = [s["p0"][:n].astype(np.float32) for s, n in zip(scenes, ns)], [s["p1"][:n].astype(np.float32) for s, n in zip(scenes, ns)]
    tu = [s["t"] / np.linalg.norm(s["t"]) for s in scenes]
    E = np.stack([scale * TS.essential_from_pose(s["R"], u) for s, u in zip(scenes, tu)])
    p0, c = SS.pack(l0)
    p1, _ = SS.pack(l1)
    mask = (rng.random(p0.shape[:2]) > 0.1).astype(np.uint8)
    a, b, mk = _cuda(p0, p1, mask)
    got = st.recover_pose_batch(E, a, b, torch.from_numpy(c), K, K, 50.0, mask=mk)
    torch.cuda.synchronize()
    for p, n in enumerate(ns):
        want = SR.recover_pose(E[p], l0[p], l1[p], K, K, 50.0, mask=mask[p, :n])
        live = mask[p, :n] != 0
        assert np.abs(np.minimum(want["l0"], want["l1"])[:, live]).min(initial=1.0) > 1e-9      # no depth at the gate
        assert list(got["good"][p].cpu().numpy()) == list(want["good"]), p
        assert list(got["info"][p].cpu().numpy()) == list(want["info"]), p
        assert np.array_equal(got["inliers"][p, :n].cpu().numpy(), want["mask"]) and not got["inliers"][p, n:].any()
        assert _same_f32(got["points3d"][p, :n].cpu().numpy(), want["points3d"]) and np.isnan(got["points3d"][p, n:].cpu().numpy()).all()
        R, t = got["R"][p].cpu().numpy(), got["t"][p].cpu().numpy()
        assert np.array_equal(R, want["R"]) and np.array_equal(t, want["t"])
        if live.sum() > 0:
            assert want["found"] and np.abs(R - scenes[p]["R"]).max() <= 1e-9 and np.abs(t - tu[p]).max() <= 1e-9
            assert want["good"][want["pose"]] == live.sum()
        else:
            assert not want["found"] and not R.any() and not t.any()


def test_recover_pose_matches_and_the_cv2_shaped_wrapper(st):
    from accelerated_features_amd import _lib
    rng = np.random.default_rng(12)
    n, Kp = 300, 400
    s = SS.scene_in_front(rng, n, noise=0.5, min_t=0.5)
    tu = s["t"] / np.linalg.norm(s["t"])
    E = -2.5 * TS.essential_from_pose(s["R"], tu)
    p0, p1 = s["p0"].astype(np.float32), s["p1"].astype(np.float32)
    a, b = _cuda(p0[None], p1[None])
    batch = st.recover_pose_batch(E, a, b, None, K, K, 50.0)
    # the index-list entry on a permuted key-point list
    k0, k1 = np.zeros((1, Kp, 2), np.float32), np.zeros((1, Kp, 2), np.float32)
    i0, i1 = rng.permutation(Kp)[:n], rng.permutation(Kp)[:n]
    k0[0, i0], k1[0, i1] = p0, p1
    ka, kb, ia, ib = _cuda(k0, k1, i0[None].astype(np.int64), i1[None].astype(np.int64))
    lists = st.recover_pose_matches(E, ka, kb, ia, ib, torch.tensor([n], dtype=torch.int32).cuda(), K, K, 50.0)
    for k in batch:
        assert np.array_equal(batch[k].cpu().numpy().view(np.uint8), lists[k].cpu().numpy().view(np.uint8)), k
    # cv2.recoverPose's shape
    cnt, R, t, mask = st.recover_pose(E, p0, p1, K)
    assert t.shape == (3, 1) and R.shape == (3, 3) and mask.shape == (n, 1) and mask.dtype == np.uint8
    assert cnt == int(batch["info"][0, 3]) == n and set(np.unique(mask)) <= {0, 255}
    assert np.array_equal(R, batch["R"][0].cpu().numpy()) and np.array_equal(t[:, 0], batch["t"][0].cpu().numpy())
    assert np.array_equal(mask[:, 0] != 0, batch["inliers"][0].cpu().numpy() != 0)
    out = st.recover_pose(E, p0.reshape(n, 1, 2), p1.reshape(n, 1, 2), cameraMatrix=K, distanceThresh=50.0, mask=np.r_[np.zeros(10), np.ones(n - 10)])
    assert len(out) == 5 and out[4].shape == (4, n) and out[0] == n - 10
    X = out[4]
    assert np.isnan(X[:, :10]).all() and (X[3, 10:] == 1.0).all()
    assert np.abs(X[:3, 10:].T * np.linalg.norm(s["t"]) - s["X"][10:]).max() < 0.2        # 0.5 px of noise at depth 2 - 6
    # calibrated points and the default camera matrix
    x0, x1 = (p0 - K[:2, 2]) / SS.F, (p1 - K[:2, 2]) / SS.F
    cnt2, R2, _, _ = st.recover_pose(E, x0, x1)
    assert cnt2 == n and np.abs(R2 - R).max() < 1e-6
    # the argument errors raise
    for kw in (dict(distance_thresh=0.0), dict(distance_thresh=-1.0), dict(distance_thresh=float("nan"))):
        with pytest.raises(_lib.XFeatHipError):
            st.recover_pose_batch(E, a, b, None, K, K, **kw)
    for kw in (dict(max_reproj_error=0.0), dict(max_reproj_error=math.inf), dict(max_depth=0.0), dict(max_depth=float("nan")), dict(min_parallax_deg=-1.0),
               dict(min_parallax_deg=200.0)):
        with pytest.raises(_lib.XFeatHipError):
            st.triangulate_batch(a, b, None, K, K, s["R"], tu, **kw)
    with pytest.raises(RuntimeError):
        st.triangulate_batch(a, b, None, K, K, np.zeros((2, 3, 3)), tu)
    with pytest.raises(RuntimeError):
        st.recover_pose(E, p0, p1[:-1], K)
    with pytest.raises(RuntimeError):
        st.triangulate_batch(a, b, None, K, K, s["R"], tu, mask=np.ones((1, n + 1)))
    # nothing to do: fully written outputs without a library call
    e = st.triangulate_batch(torch.zeros((0, 4, 2)).cuda(), torch.zeros((0, 4, 2)).cuda(), None, K, K, np.zeros((0, 3, 3)), np.zeros((0, 3)))
    assert e["points3d"].shape == (0, 4, 3) and e["info"].shape == (0, 8)
    e = st.triangulate_batch(torch.zeros((2, 0, 2)).cuda(), torch.zeros((2, 0, 2)).cuda(), None, K, K, s["R"], tu)
    assert e["status"].shape == (2, 0) and not e["info"].any()
    e = st.recover_pose_batch(E, torch.zeros((2, 0, 2)).cuda(), torch.zeros((2, 0, 2)).cuda(), None, K, K)
    assert list(e["info"][0].cpu().numpy()) == [0, -1, 0, 0, 0, 0, 0, 0] and not e["R"].any()


def _pose_errors(T, R, t):
    from accelerated_features_amd.pose import relative_pose_error
    return relative_pose_error(T, R, t)


def test_map_then_localise(st):
    """detect -> match -> relative pose -> points -> absolute pose of image 1 from the points, all on the device: the absolute pose returns to
    the relative one.  The same chain through the three restatements on the CPU gives the reference errors; the device chain's rotation and
    translation-angle errors against ground truth must be at most 10 x those (floor 1e-6 degrees; discrete RANSAC choices may differ by one
    hypothesis).  Measured, restatement chain on the host: pair 3 translation angle 0.0189 deg, rotation 0.0047 deg (relative pose alone
    0.0184 / 0.0042), 176 valid points of 300; pair 40 0.1165 / 0.0514 deg (0.1158 / 0.0513), 193 valid points; the localised pose is
    within 0.002 deg of the relative one and |t| = 1 to 2e-4.  The device chain's values are printed by the test."""
    from accelerated_features_amd import absolute_pose, pose
    pairs, n = (3, 40), 300
    sc = [TS.scene(i, n, 0.5, 0.3, 100 + i) for i in pairs]
    p0, p1 = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
    K0, K1, T = np.stack([s[3] for s in sc]), np.stack([s[4] for s in sc]), [s[5] for s in sc]
    a, b = _cuda(p0, p1)
    rel = pose.estimate_relative_pose_batch(a, b, None, K0, K1, 1.0, max_iterations=300, seed=3)
    tri = st.triangulate_batch(a, b, None, K0, K1, rel["R"], rel["t"], mask=rel["inliers"])
    loc = absolute_pose.estimate_absolute_pose_batch(b, tri["points3d"], None, K1, 2.0, max_iterations=300, seed=3)
    torch.cuda.synchronize()
    for k, i in enumerate(pairs):
        w_rel = PR.estimate(p0[k], p1[k], K0[k], K1[k], 1.0, max_iterations=300, seed=3, pair=k)
        w_tri = SR.triangulate(p0[k], p1[k], K0[k], K1[k], w_rel["R"], w_rel["t"], mask=w_rel["mask"])
        w_loc = AR.estimate(p1[k], w_tri["points3d"], K1[k], 2.0, max_iterations=300, seed=3, pair=k)
        assert w_rel["info"][0] == 1 and w_loc["info"][0] == 1 and int(loc["info"][k, 0]) == 1
        assert w_tri["info"][1] >= 0.5 * n and int(tri["info"][k, 1]) >= 0.5 * n
        t_ref, R_ref = _pose_errors(T[k], w_loc["R"], w_loc["t"])
        t_gpu, R_gpu = _pose_errors(T[k], loc["R"][k].cpu().numpy(), loc["t"][k].cpu().numpy())
        t_rel, R_rel = _pose_errors(T[k], rel["R"][k].cpu().numpy(), rel["t"][k].cpu().numpy())
        print(f"pair {i}: relative pose t {t_rel:.4f} R {R_rel:.4f} deg; localised t {t_gpu:.4f} R {R_gpu:.4f} deg; restatement chain t {t_ref:.4f} R {R_ref:.4f} deg; "
              f"valid points {int(tri['info'][k, 1])} / {w_tri['info'][1]}")
        assert R_gpu <= max(10.0 * R_ref, 1e-6) and t_gpu <= max(10.0 * t_ref, 1e-6)
        # the absolute pose returns to the relative one: the points are in camera 0's frame, in the unit of the relative t
        Rl, tl = loc["R"][k].cpu().numpy(), loc["t"][k].cpu().numpy()
        assert _pose_errors(np.c_[rel["R"][k].cpu().numpy(), rel["t"][k].cpu().numpy()], Rl, tl)[1] < 0.5
        assert abs(np.linalg.norm(tl) - 1.0) < 0.05
