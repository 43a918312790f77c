"""The fundamental-matrix restatement (tests/fundamental_reference.py) against ground truth, and the public surface of
accelerated_features_amd.fundamental without a GPU.  CPU only: the restatement is what the GPU tests hold the kernels to, so it is checked
here on its own."""
import numpy as np
import pytest

import fundamental_reference as FR
import pose_reference as PR
from twoview_support import fixture as _fixture, fixture_pair, holdout, true_samples

IDENT = (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)


def _samples(rng, H):
    return true_samples(rng, H, 7)[0]


def test_every_candidate_is_a_rank_two_matrix_through_the_sample():
    rng = np.random.default_rng(0)
    x = _samples(rng, 1000)
    x[:, 500:] = rng.uniform(-1, 1, (4, 500, 7))               # half of them random (no true motion)
    for oriented in (True, False):
        cand, nc = FR.solve(*x, IDENT, oriented=oriented)
        # (a random motion can put sample points behind camera 1: the oriented check then rightly drops the true F)
        assert (nc[:500] > 0).mean() >= (0.9 if oriented else 1.0) and (nc[500:] > 0).mean() >= (0.05 if oriented else 1.0)
        res = []
        for h in range(1000):
            x0 = np.c_[x[0, h], x[1, h], np.ones(7)]
            x1 = np.c_[x[2, h], x[3, h], np.ones(7)]
            for c in range(nc[h]):
                F = cand[h, c].reshape(3, 3)
                s = np.linalg.norm(F)
                epi = np.abs(np.einsum("ij,jk,ik->i", x1, F, x0)) / (s * np.linalg.norm(x0, axis=1) * np.linalg.norm(x1, axis=1))
                res.append(max(epi.max(), abs(np.linalg.det(F)) / s ** 3))
        res = np.array(res)
        assert (res <= 1e-10).mean() >= 0.99, np.sort(res)[-10:]
        assert res.max() <= 1e-6


def test_true_F_is_among_the_candidates_on_the_megadepth_cameras():
    """Noise-free 7-point samples of the MegaDepth-1500 cameras (fp32 pixels), conditioned as the prep kernel does: the true F is among the
    candidates, after the oriented check, for >= 99 % of the samples -- the candidate's median Sampson error on 100 held-out true
    correspondences is below 0.01 px (measured: median 4e-5 px, 99th percentile 3e-3 px; the entries themselves are ill-conditioned
    against the fp32 rounding of the sample on short baselines, so they are not compared)."""
    f = _fixture()
    rng = np.random.default_rng(1)
    hits, dmin = 0, []
    P = 1500
    for p in range(0, P, 3):
        p0, p1, _ = fixture_pair(f, p, 7, 0.0, 0.0, rng)
        P0, P1 = p0.astype(np.float64), p1.astype(np.float64)
        nt = FR.conditioning(P0, P1)
        cand, nc = FR.solve(*FR.normalised(P0[None], P1[None], nt), nt)
        h0, h1 = holdout(f, p, 100)
        d = min([np.median(FR.sampson_px(cand[0, c], h0, h1)) for c in range(nc[0])] or [np.inf])
        dmin.append(d)
        hits += d <= 1e-2
    assert hits >= 0.99 * len(dmin), np.sort(dmin)[-20:]


def test_cubic_roots_find_every_real_root():
    rng = np.random.default_rng(2)
    H = 4000
    r = rng.uniform(-5, 5, (H, 3))
    near = np.arange(H) % 2 == 1
    r[near, 1] = r[near, 0] + rng.uniform(1e-5, 1e-3, near.sum()) * rng.choice([-1, 1], near.sum())        # near-double roots
    one = np.arange(H) % 5 == 0                                                                             # one real root, two complex
    a = np.zeros((3, H))
    for h in range(H):
        if one[h]:
            c = np.poly([r[h, 0], complex(r[h, 1], 0.5 + abs(r[h, 2])), complex(r[h, 1], -0.5 - abs(r[h, 2]))]).real
        else:
            c = np.poly(r[h])
        a[:, h] = c[3], c[2], c[1]
    roots, nr = FR.cubic_roots(a)
    for h in range(H):
        want = np.roots([1.0, a[2, h], a[1, h], a[0, h]])
        real = np.sort(want[np.abs(want.imag) <= 1e-9 * (1 + np.abs(want.real))].real)
        expect = 1 if one[h] else 3
        assert nr[h] == expect, (h, nr[h], want)
        got = roots[h, :nr[h]]
        assert np.all(np.diff(got) > 0)
        if len(real) == nr[h]:
            sep = 1e-5 if near[h] else 1.0
            assert np.abs(got - real).max() <= 1e-8 * (1 + np.abs(real).max()) / min(sep, 1.0) * 1e-2 + 1e-9, (h, got, real)
        p = np.polyval([1.0, a[2, h], a[1, h], a[0, h]], got)
        assert np.all(np.abs(p) <= 1e-10 * (1 + np.abs(got) ** 3))


@pytest.mark.parametrize("outliers,iters", [(0.0, 1000), (0.3, 1000), (0.6, 10000), (0.7, 16384)])
def test_estimator_recovers_the_true_F_and_the_inliers(outliers, iters):
    """Synthetic scenes, 0.3 px noise: F explains held-out true correspondences to well below the noise, and the mask is the inlier set up to
    the points near the threshold.  (At 80 % outliers one clean 7-point sample takes 1 / 0.2^7 = 78000 draws on average: beyond the
    16384 iterations the kernel allows.)"""
    f = _fixture()
    i = 17
    rng = np.random.default_rng(int(outliers * 10))
    n = 400
    p0, p1, out = fixture_pair(f, i, n, 0.3, outliers, rng)
    r = FR.estimate(p0, p1, 1.0, iters, 0.999, seed=3)
    assert r["info"][0] == 1
    h0, h1, _ = fixture_pair(f, i, 200, 0.0, 0.0, np.random.default_rng(5))
    e = FR.sampson_px(r["F"][0], h0, h1)
    assert np.median(e) <= 0.15 and np.percentile(e, 95) <= 0.5, (np.median(e), e.max())
    m = r["mask"].astype(bool)
    assert (m & out).sum() <= 0.02 * n + 2                 # an outlier that happens to lie near its epipolar line counts as an inlier
    assert (~m & ~out).sum() <= 0.02 * (~out).sum() + 2
    assert r["F"][0, 8] == 1.0 and not r["F"][1:].any()


def test_eight_point_equals_the_textbook_svd_fit():
    f = _fixture()
    for i in (3, 99, 1234):
        rng = np.random.default_rng(i)
        p0, p1, _ = fixture_pair(f, i, 60, 0.0, 0.0, rng)
        r = FR.estimate(p0, p1, method=FR.FM_8POINT)
        assert list(r["info"]) == [1, -1, 1, 60, 0, 60, 0, 0] and r["mask"].all()
        P0, P1 = p0.astype(np.float64), p1.astype(np.float64)

        def T(P):
            c = P.mean(0)
            s = np.sqrt(2) / np.linalg.norm(P - c, axis=1).mean()
            return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
        T0, T1 = T(P0), T(P1)
        x0 = np.c_[P0, np.ones(60)] @ T0.T
        x1 = np.c_[P1, np.ones(60)] @ T1.T
        A = np.stack([x1[:, 0] * x0[:, 0], x1[:, 0] * x0[:, 1], x1[:, 0], x1[:, 1] * x0[:, 0], x1[:, 1] * x0[:, 1], x1[:, 1], x0[:, 0], x0[:, 1],
                      np.ones(60)], 1)
        Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
        U, S, Vt = np.linalg.svd(Fn)
        F = T1.T @ (U @ np.diag([S[0], S[1], 0.0]) @ Vt) @ T0
        assert FR.f_distance(r["F"][0], F) <= 1e-9
        assert FR.f_distance(r["F"][0], FR.true_F(f["K0"][i], f["K1"][i], f["T_0to1"][i])) <= 1e-5


def test_degenerate_inputs_find_nothing_and_give_no_nan():
    rng = np.random.default_rng(4)
    p = rng.uniform(0, 600, (50, 2)).astype(np.float32)
    q = p + 5
    cases = [(p[:6], q[:6]),                                                # fewer than 7 points
             (np.repeat(p[:1], 50, 0), np.repeat(q[:1], 50, 0)),            # one repeated point
             (np.c_[p[:, 0], 0.5 * p[:, 0] + 3], np.c_[q[:, 0], 0.5 * q[:, 0] - 7])]   # collinear in both images
    for a, b in cases:
        for method in (FR.USAC_MAGSAC, FR.FM_8POINT, FR.FM_7POINT):
            r = FR.estimate(a.astype(np.float32), b.astype(np.float32), 1.0, 300, method=method)
            assert r["info"][0] == 0, (len(a), method, r["info"])
            assert np.isfinite(r["F"]).all() and not r["F"].any() and not r["mask"].any()


def test_megadepth_synthetic_holdout_error_on_every_25th_pair():
    """The floors of fundamental_reference.HOLDOUT_FLOORS: the restatement's held-out Sampson error on every 25th synthetic MegaDepth pair."""
    f = _fixture()
    pts0, pts1, counts = PR.megadepth_synthetic(f)
    med, found = [], []
    for p in range(0, 1500, 25):
        r = FR.estimate(pts0[p, :counts[p]], pts1[p, :counts[p]], 1.5, 1000, 0.99, seed=0, pair=p)
        found.append(r["info"][0])
        if r["info"][0]:
            h0, h1 = holdout(f, p, 200)
            med.append(np.median(FR.sampson_px(r["F"][0].reshape(3, 3), h0, h1)))
        else:
            med.append(np.inf)
    med = np.array(med)
    print("restatement: found", np.mean(found), "median", np.median(med), "p90", np.percentile(med, 90))
    assert np.mean(found) == 1.0
    assert np.median(med) <= 0.1 and np.percentile(med, 90) <= 0.2


def test_find_fundamental_mat_has_cv2s_signature_and_no_cpu_path():
    """cv2.findFundamentalMat(points1, points2[, method[, ransacReprojThreshold[, confidence[, maxIters[, mask]]]]]) binds positionally /
    by these keywords; the constants are cv2's; without a GPU every entry raises (there is no host estimator in the product)."""
    import inspect

    import torch
    from accelerated_features_amd import _lib, fundamental
    sig = inspect.signature(fundamental.find_fundamental_mat)
    assert list(sig.parameters)[:7] == ["points1", "points2", "method", "ransacReprojThreshold", "confidence", "maxIters", "mask"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["method"] == 38 and d["ransacReprojThreshold"] == 3.0 and d["confidence"] == 0.99 and d["maxIters"] == 1000 and d["mask"] is None
    assert (fundamental.USAC_MAGSAC, fundamental.FM_7POINT, fundamental.FM_8POINT) == (38, 1, 2)
    b = inspect.signature(fundamental.find_fundamental_batch)
    assert list(b.parameters) == ["pts0", "pts1", "counts", "ransac_thr", "max_iters", "confidence", "seed", "method"]
    assert fundamental.MAX_ITERATIONS == 16384 and fundamental.WORKSPACE_LIMIT == 512 << 20
    sig.bind(np.zeros((8, 2)), np.zeros((8, 2)), 38, 1.0, 0.999, 5000)
    with pytest.raises(_lib.XFeatHipError):
        fundamental.find_fundamental_mat(np.zeros((8, 2)), np.zeros((8, 2)), 8)          # FM_RANSAC: not implemented
    if not torch.cuda.is_available():
        with pytest.raises(_lib.XFeatHipError):
            fundamental.find_fundamental_mat(np.zeros((8, 2)), np.zeros((8, 2)))
        with pytest.raises(_lib.XFeatHipError):
            fundamental.find_fundamental_batch(torch.zeros(1, 8, 2), torch.zeros(1, 8, 2))
