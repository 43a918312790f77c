"""The numpy restatement of the 3D-3D alignment estimator (tests/alignment_reference.py, the specification of csrc/k_align.hip) against
ground truth and against an SVD fit: the minimal solver on noise-free samples, the closed-form fit against numpy.linalg.svd's Umeyama fit,
degenerate samples, a mirrored cloud, and recovery on scenes with noise, gross outliers and NaN rows.

Measured (the restatement on this file's seeds; DESIGN.md 3.15 quotes the same figures):
  * al_solve on 2000 noise-free samples, s in [0.05, 20]: worst error 1.8e-14 in R, relative s and t / max(1, |t|);
  * al_fit against the SVD fit on 400 clouds x with_scale on / off: 4.2e-12 in R, 8.9e-16 in relative s, 4.8e-12 in t / max(1, |t|);
  * recovery: MEASURED below, per case the worst rotation error (degrees), relative scale error and RMS of s R A + t - B_true over the true
    inliers relative to thr over seeds 0..11 at 256 iterations; the bounds are twice these; every run found a model; the mask differs from
    the true labels in at most 1 row of 300 (an outlier that fell within the threshold of its true place)."""
import numpy as np
import pytest

import alignment_reference as AL
import alignment_support as AS

SEEDS = range(12)
# (n, sigma, outlier share, NaN share, with_scale) -> measured worst (rotation degrees, relative scale, RMS / thr)
MEASURED = {(300, 0.01, 0.4, 0.0, True): (0.1581, 1.059e-3, 0.0700),
            (300, 0.01, 0.7, 0.0, True): (0.2937, 1.491e-3, 0.1041),
            (60, 0.01, 0.3, 0.2, True): (0.3510, 2.643e-3, 0.1686),
            (300, 0.02, 0.5, 0.3, True): (0.3759, 2.555e-3, 0.0842),
            (300, 0.01, 0.4, 0.0, False): (0.1258, 0.0, 0.0618)}


def _model_errors(m, s, R, t):
    return max(np.abs(m[:9].reshape(3, 3) - R).max(), abs(m[12] / s - 1.0), np.abs(m[9:12] - t).max() / max(1.0, np.abs(t).max()))


def test_solver_recovers_noise_free_similarities():
    rng = np.random.default_rng(1)
    A, B, gt = AS.true_samples(rng, 2000)
    m, ok = AL.solve(A, B)
    assert ok.all()
    s_true = np.array([g[0] for g in gt])
    assert s_true.min() < 0.06 and s_true.max() > 18.0
    worst = max(_model_errors(m[h], *gt[h]) for h in range(2000))
    print("al_solve worst error", worst)
    assert worst <= 1e-9
    A, B, gt = AS.true_samples(rng, 200, with_scale=False)
    m, ok = AL.solve(A, B, with_scale=False)
    assert ok.all() and (m[:, 12] == 1.0).all() and max(_model_errors(m[h], *gt[h]) for h in range(200)) <= 1e-9


def test_fit_equals_the_svd_fit():
    rng = np.random.default_rng(2)
    worst = np.zeros(3)
    kinds = (0, 1, 1, 3, 4)                  # noise-free, noisy (twice), planar, 1e3 away from the origin
    for i in range(400):
        A, B = AS.shaped_cloud(rng, int(rng.integers(3, 201)), kinds[i % 5])
        for with_scale in (True, False):
            m, ok = AL.fit_points(A, B, with_scale)
            assert ok
            s, R, t = AS.umeyama(A, B, with_scale)
            assert np.linalg.det(m[:9].reshape(3, 3)) > 0.999999
            worst = np.maximum(worst, (np.abs(m[:9].reshape(3, 3) - R).max(), abs(m[12] / s - 1.0), np.abs(m[9:12] - t).max() / max(1.0, np.abs(t).max())))
    print("al_fit against the SVD fit: worst R, relative s, t / max(1, |t|)", worst)
    assert (worst <= 1e-9).all()


def test_degenerate_samples_give_no_model():
    rng = np.random.default_rng(3)
    A, B, _ = AS.true_samples(rng, 8)
    A[0, 2] = A[0, 0] + 0.3 * (A[0, 1] - A[0, 0])            # collinear in A
    B[1, 2] = B[1, 0] + 1.7 * (B[1, 1] - B[1, 0])            # collinear in B
    A[2] = A[2, :1]                                          # coincident: va = 0
    B[3] = B[3, :1]                                          # vb = 0
    A[4, 1] = A[4, 0]                                        # a zero first side
    A[5, 0, 1] = np.nan
    B[6, 2, 2] = np.inf
    for with_scale in (True, False):
        m, ok = AL.solve(A, B, with_scale)
        assert list(ok) == [False] * 7 + [True]
        assert not m[:7].any() and np.isfinite(m).all()
    # the estimator never samples a NaN row into a model: all rows NaN but two -> nothing found
    sc = AS.scene(40, 0.01, 0.0, 0.0, 0)
    a, b = sc["A"].copy(), sc["B"].copy()
    a[2:] = np.nan
    r = AL.estimate(a, b, sc["thr"], max_iterations=64)
    assert r["info"][0] == 0 and r["info"][1] == -1 and not r["mask"].any() and r["s"] == 0.0


def test_mirrored_cloud_gets_a_proper_rotation_and_no_consensus():
    sc = AS.scene(300, 0.01, 0.0, 0.0, 5)
    Bm = sc["B"].copy()
    Bm[:, 0] = -Bm[:, 0]
    m, ok = AL.fit_points(sc["A"], Bm)
    assert ok and abs(np.linalg.det(m[:9].reshape(3, 3)) - 1.0) < 1e-12
    idx = np.random.default_rng(0).integers(0, 300, (500, 3))
    ms, oks = AL.solve(sc["A"][idx].astype(np.float64), Bm[idx].astype(np.float64))
    assert oks.mean() > 0.9 and np.abs(np.linalg.det(ms[oks, :9].reshape(-1, 3, 3)) - 1.0).max() < 1e-12
    r = AL.estimate(sc["A"], Bm, sc["thr"], max_iterations=256)
    assert r["info"][3] <= 30                                 # a triangle fits its mirror image, the cloud does not: no consensus
    if r["info"][0]:
        assert abs(np.linalg.det(r["R"]) - 1.0) < 1e-12
    good = AL.estimate(sc["A"], sc["B"], sc["thr"], max_iterations=256)
    assert good["info"][3] >= 295


@pytest.mark.parametrize("case", list(MEASURED), ids=lambda c: "n%d-sigma%g-out%g-nan%g-%s" % (c[:4] + ("similarity" if c[4] else "rigid",)))
def test_recovery_against_ground_truth(case):
    n, sigma, outliers, nan_share, with_scale = case
    worst, worst_mask = np.zeros(3), 0.0
    for seed in SEEDS:
        sc = AS.scene(n, sigma, outliers, nan_share, seed, with_scale)
        r = AL.estimate(sc["A"], sc["B"], sc["thr"], with_scale, max_iterations=256, seed=seed)
        assert r["info"][0] == 1, seed
        worst = np.maximum(worst, AS.errors(sc, r["s"], r["R"], r["t"]))
        truth = ~sc["outlier"] & ~sc["nan"]
        worst_mask = max(worst_mask, float((r["mask"].astype(bool) != truth).mean()))
        assert not r["mask"][sc["nan"]].any()
        if not with_scale:
            assert r["s"] == 1.0
    print(case, "worst rotation (deg), relative scale, RMS / thr:", worst, "mask difference", worst_mask)
    assert (worst <= 2.0 * np.array(MEASURED[case])).all(), (worst, MEASURED[case])
    assert worst_mask <= 0.02
