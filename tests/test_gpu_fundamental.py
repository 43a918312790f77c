"""xfh_find_fundamental (csrc/k_fundamental.hip) on the MI355X against the numpy restatement tests/fundamental_reference.py: the winner,
the iteration count, the inlier count, the integer quality and the mask exactly; F to 1e-9.  The restatement is given the tables the
device computed (xfh_homography_tables), so the quality sums are the same integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import fundamental_reference as FR
import pose_reference as PR
from twoview_support import check_common, fixture as _fixture, holdout, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import fundamental as m
    return m


_TABLES = {}


def _tab(thr):
    """The device's tables of threshold thr, in the restatement's form."""
    if thr not in _TABLES:
        from accelerated_features_amd import _lib as L
        st = torch.zeros(FR.NBINS, dtype=torch.int32, device="cuda")
        wt = torch.zeros(FR.NBINS, dtype=torch.float64, device="cuda")
        L.check(L.load().xfh_homography_tables(float(thr), C.c_void_p(st.data_ptr()), C.c_void_p(wt.data_ptr()), None), "tables")
        torch.cuda.synchronize()
        _TABLES[thr] = (FR.bin_scale_of(thr), st.cpu().numpy().astype(np.uint32), wt.cpu().numpy())
    return _TABLES[thr]


def _check(got, want, p, n, method=FR.USAC_MAGSAC):
    check_common(got, want, p, n)
    g = got["F"][p].cpu().numpy().reshape(-1, 9)
    w = want["F"] if method == FR.FM_7POINT else want["F"][:1]
    assert np.isfinite(g).all()
    assert np.abs(g - w).max() <= 1e-9, (g, w)


def _batch(fm, p0, p1, thr, iters, seed, counts=None, method=38, conf=0.99):
    return fm.find_fundamental_batch(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), counts, thr, iters, conf, seed, method)


@pytest.mark.parametrize("n,outliers,thr,iters", [(7, 0.0, 1.0, 1000), (8, 0.0, 3.0, 1000), (300, 0.3, 1.0, 1000), (300, 0.7, 3.0, 10000),
                                                  (2000, 0.5, 1.0, 1000), (4096, 0.6, 2.0, 4000), (2000, 0.0, 1.0, 16384)])
def test_single_pair_equals_the_restatement(fm, n, outliers, thr, iters):
    p0, p1 = scene(7, n, 0.7, outliers, seed=n)[:2]
    got = _batch(fm, p0[None], p1[None], thr, iters, 11)
    torch.cuda.synchronize()
    want = FR.estimate(p0, p1, thr, iters, 0.99, seed=11, tab=_tab(thr))
    _check(got, want, 0, n)
    if n >= 300:
        assert want["info"][0] == 1


def test_ragged_batch_equals_the_restatement_pair_by_pair(fm):
    ns = [300, 7, 0, 1200, 57, 6, 2500]
    P, cap = len(ns), max(ns)
    pts0, pts1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    for p, n in enumerate(ns):
        a, b = scene(100 + p, max(n, 1), 0.5, 0.4, seed=p)[:2]
        pts0[p, :n], pts1[p, :n] = a[:n], b[:n]
    pts0[:, cap - 1] = np.nan                          # rows past the counts are never read
    got = _batch(fm, pts0, pts1, 1.5, 1000, 5, torch.tensor(ns, dtype=torch.int32))
    torch.cuda.synchronize()
    for p, n in enumerate(ns):
        want = FR.estimate(pts0[p, :n], pts1[p, :n], 1.5, 1000, 0.99, seed=5, pair=p, tab=_tab(1.5))
        _check(got, want, p, n)


def test_chunked_batch_equals_one_call(fm, monkeypatch):
    """Pairs split into chunks (the workspace limit) draw as in one call: the seed is advanced per chunk."""
    P, n = 5, 400
    pts0, pts1 = np.zeros((P, n, 2), np.float32), np.zeros((P, n, 2), np.float32)
    for p in range(P):
        pts0[p], pts1[p] = scene(200 + p, n, 0.6, 0.5, seed=p)[:2]
    one = _batch(fm, pts0, pts1, 2.0, 1000, 3)
    monkeypatch.setattr(fm, "WORKSPACE_LIMIT", 2 * fm._lib.load().xfh_fundamental_workspace_bytes(1, 1000))
    many = _batch(fm, pts0, pts1, 2.0, 1000, 3)
    torch.cuda.synchronize()
    for k in one:
        assert torch.equal(one[k], many[k]), k


def test_index_list_entry_equals_gathered_points(fm):
    P, K, cap = 3, 700, 500
    rng = np.random.default_rng(3)
    kp0, kp1 = np.zeros((P, K, 2), np.float32), np.zeros((P, K, 2), np.float32)
    idx0, idx1 = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64)
    nm = np.array([500, 333, 20], np.int32)
    for p in range(P):
        a, b = scene(p, K, 0.5, 0.3, seed=p)[:2]
        kp0[p], kp1[p] = a, b[rng.permutation(K)]
        idx0[p] = rng.choice(K, cap, replace=False)
        idx1[p] = rng.choice(K, cap, replace=False)
    for method in (38, 2):
        r1 = fm.find_fundamental_matches(torch.from_numpy(kp0).cuda(), torch.from_numpy(kp1).cuda(), torch.from_numpy(idx0).cuda(),
                                         torch.from_numpy(idx1).cuda(), torch.from_numpy(nm).cuda(), 2.5, 1000, 0.99, 9, method)
        pts0 = np.take_along_axis(kp0, idx0[:, :, None], 1)
        pts1 = np.take_along_axis(kp1, idx1[:, :, None], 1)
        r2 = _batch(fm, pts0, pts1, 2.5, 1000, 9, torch.from_numpy(nm), method)
        torch.cuda.synchronize()
        for k in r1:
            assert torch.equal(r1[k], r2[k]), (method, k)


def test_same_seed_same_bits(fm):
    p0, p1 = scene(3, 1500, 1.0, 0.5, seed=1)[:2]
    a = _batch(fm, p0[None], p1[None], 1.0, 1000, 4)
    b = _batch(fm, p0[None], p1[None], 1.0, 1000, 4)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_degenerate_inputs_do_not_fault_or_nan(fm):
    """Too few points, all points identical, collinear points, NaN rows, a planar scene; zero counts; counts at and past the capacity."""
    cap = 64
    rng = np.random.default_rng(0)
    pts0 = rng.uniform(0, 500, (6, cap, 2)).astype(np.float32)
    pts1 = pts0 + rng.normal(size=(6, cap, 2)).astype(np.float32)
    pts0[1], pts1[1] = pts0[1, :1], pts1[1, :1]              # all identical
    t = rng.uniform(0, 400, cap).astype(np.float32)
    pts0[2] = np.c_[t, 0.5 * t + 10]                           # collinear in both images
    pts1[2] = np.c_[t + 3, 0.5 * t + 20]
    pts0[3, ::3] = np.nan                                      # NaN rows
    Hm = np.array([[1.1, 0.05, 12], [-0.03, 0.95, 7], [1e-4, 2e-5, 1.0]])   # a planar scene: F is not determined
    x = np.c_[pts0[4].astype(np.float64), np.ones(cap)] @ Hm.T
    pts1[4] = (x[:, :2] / x[:, 2:]).astype(np.float32)
    counts = np.array([6, cap, cap, cap, cap, cap + 10], np.int32)
    for method in (38, 2, 1):
        r = _batch(fm, pts0, pts1, 1.0, 500, 1, torch.from_numpy(counts), method)
        z = _batch(fm, pts0, pts1, 1.0, 500, 1, torch.zeros(6, dtype=torch.int32), method)
        torch.cuda.synchronize()
        assert torch.isfinite(r["F"]).all() and torch.isfinite(z["F"]).all()
        assert (z["info"][:, 0] == 0).all() and not z["inliers"].any() and not z["F"].any()
        info = r["info"].cpu().numpy()
        assert info[0, 0] == 0 and info[1, 0] == 0
        for p in range(6):
            n = min(int(counts[p]), cap)
            want = FR.estimate(pts0[p, :n], pts1[p, :n], 1.0, 500, 0.99, seed=1, pair=p, method=method, tab=_tab(1.0))
            assert list(info[p]) == list(want["info"]), (method, p)


def test_seven_and_eight_point_modes_equal_the_restatement(fm):
    P = 6
    rng = np.random.default_rng(8)
    pts0, pts1 = np.zeros((P, 40, 2), np.float32), np.zeros((P, 40, 2), np.float32)
    for p in range(P):
        pts0[p], pts1[p] = scene(300 + p, 40, 0.3 * (p % 2), 0.0, seed=p)[:2]
    ns = np.array([7, 7, 7, 40, 8, 6], np.int32)
    r7 = _batch(fm, pts0, pts1, 1.0, 1, 0, torch.from_numpy(ns), 1)
    r8 = _batch(fm, pts0, pts1, 1.0, 1, 0, torch.from_numpy(ns), 2)
    torch.cuda.synchronize()
    assert r7["F"].shape == (P, 3, 3, 3) and r8["F"].shape == (P, 3, 3)
    for p in range(P):
        n = int(ns[p])
        _check(r7, FR.estimate(pts0[p, :n], pts1[p, :n], method=1), p, n, method=1)
        _check(r8, FR.estimate(pts0[p, :n], pts1[p, :n], method=2), p, n, method=2)
    assert (r7["info"][:3, 2] >= 1).all() and r8["info"][3, 0] == 1


def test_megadepth1500_holdout_error(fm):
    """1500 synthetic MegaDepth pairs (200-1024 matches, 0.5-1 px noise, 40 % outliers) in one call at 1000 iterations: the Sampson error
    of held-out true correspondences under the estimated F clears the floors derived from the restatement on the CPU."""
    f = _fixture()
    P = 1500
    pts0, pts1, counts = PR.megadepth_synthetic(f)
    r = _batch(fm, pts0, pts1, 1.5, 1000, 0, torch.from_numpy(counts))
    info, F = r["info"].cpu().numpy(), r["F"].cpu().numpy()
    med = np.full(P, np.inf)
    for p in range(P):
        if info[p, 0]:
            h0, h1 = holdout(f, p, 200)
            med[p] = np.median(FR.sampson_px(F[p], h0, h1))
    found = info[:, 0].mean()
    print("synthetic MegaDepth-1500: found", found, "median", np.median(med), "p90", np.percentile(med, 90))
    assert found >= FR.HOLDOUT_FLOORS["found"]
    assert np.median(med) <= FR.HOLDOUT_FLOORS["median"] and np.percentile(med, 90) <= FR.HOLDOUT_FLOORS["p90"]
    for p in range(0, P, 100):                   # 15 pairs exactly against the restatement
        want = FR.estimate(pts0[p, :counts[p]], pts1[p, :counts[p]], 1.5, 1000, 0.99, seed=0, pair=p, tab=_tab(1.5))
        assert list(info[p]) == list(want["info"]), p
        assert np.abs(F[p].reshape(9) - want["F"][0]).max() <= 1e-9


def test_cv2_shaped_wrapper_equals_the_batch_entry(fm):
    p0, p1 = scene(11, 800, 0.5, 0.3, seed=2)[:2]
    F, mask = fm.find_fundamental_mat(p0, p1, fm.USAC_MAGSAC, 1.5, 0.999, 2000)
    r = _batch(fm, p0[None], p1[None], 1.5, 2000, 0, conf=0.999)
    assert np.array_equal(F, r["F"][0].cpu().numpy()) and F.shape == (3, 3) and F[2, 2] == 1.0
    assert mask.shape == (800, 1) and mask.dtype == np.uint8 and np.array_equal(mask[:, 0], r["inliers"][0].cpu().numpy())
    F7, m7 = fm.find_fundamental_mat(p0[:7], p1[:7], fm.FM_7POINT)
    r7 = _batch(fm, p0[None, :7], p1[None, :7], 3.0, 1, 0, method=1)
    k = int(r7["info"][0, 2])
    assert k >= 1 and F7.shape == (3 * k, 3) and np.array_equal(F7, r7["F"][0, :k].cpu().numpy().reshape(-1, 3))
    assert m7.shape == (7, 1) and m7.all()
    F8, m8 = fm.find_fundamental_mat(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), fm.FM_8POINT)
    assert np.array_equal(F8, _batch(fm, p0[None], p1[None], 3.0, 1, 0, method=2)["F"][0].cpu().numpy())
    assert fm.find_fundamental_mat(p0[:6], p1[:6]) == (None, None)
    for bad in (4, 8, 16, 32, 35):                # FM_RANSAC, FM_LMEDS, USAC_DEFAULT, USAC_PARALLEL, USAC_ACCURATE
        with pytest.raises(fm._lib.XFeatHipError):
            fm.find_fundamental_mat(p0, p1, bad)


def test_match_pairs_device_then_index_list_entry(fm):
    """XFeat.match_pairs_device on the golden fixture's images -> find_fundamental_matches equals the point-list entry on the gathered
    matches."""
    import fixtures
    from accelerated_features_amd import XFeat
    xf = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=4096)
    a, b = fixtures.shifted_pair(1, 480, 640, seed=7)
    kp, sc, de, nv, nc, cap, hw = xf._detect_device(xf.parse_input(torch.cat([a, b])), 4096)
    i0, i1, nm = xf.match_pairs_device(de, nv, -1)
    kp0, kp1 = kp[0::2].contiguous(), kp[1::2].contiguous()
    r = fm.find_fundamental_matches(kp0, kp1, i0, i1, nm, 2.0, 1000, 0.99, 0)
    live = torch.arange(i0.shape[1], device="cuda")[None, :] < nm[:, None]          # rows past n_matches hold no valid index
    g0, g1 = torch.where(live, i0, 0), torch.where(live, i1, 0)
    pts0 = torch.gather(kp0, 1, g0[:, :, None].expand(-1, -1, 2)).contiguous()
    pts1 = torch.gather(kp1, 1, g1[:, :, None].expand(-1, -1, 2)).contiguous()
    g = fm.find_fundamental_batch(pts0, pts1, nm, 2.0, 1000, 0.99, 0)
    torch.cuda.synchronize()
    assert int(nm[0]) >= 7
    for k in r:
        assert torch.equal(r[k], g[k]), k
    n = int(nm[0])
    want = FR.estimate(pts0[0, :n].cpu().numpy(), pts1[0, :n].cpu().numpy(), 2.0, 1000, 0.99, seed=0, tab=_tab(2.0))
    _check(r, want, 0, n)
