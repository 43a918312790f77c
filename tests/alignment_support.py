"""Test data of the 3D-3D alignment estimator (csrc/k_align.hip, tests/alignment_reference.py) that is not specification: random samples
and clouds of the solver and the fit, scenes with ground truth, an SVD fit to compare against, ground-truth errors.

The generators consume their ``numpy`` generator in a fixed order, which is part of the tests' inputs."""
import numpy as np

import twoview_support as TS

S_MIN, S_MAX = 0.05, 20.0


def similarity(rng, with_scale=True):
    """A random (s, R, t): s log-uniform in [0.05, 20] (1 when rigid), a rotation of any angle, t of the order of the scaled cloud."""
    s = float(np.exp(rng.uniform(np.log(S_MIN), np.log(S_MAX)))) if with_scale else 1.0
    R = TS.rotation(rng.normal(size=3) * 1.5)
    return s, R, rng.normal(size=3) * 2.0 * s


def cloud(rng, n):
    """n points in a box in front of a camera (TS.motion's box)."""
    return np.c_[rng.uniform(-1, 1, (n, 2)), rng.uniform(2, 6, n)]


def transform(A, s, R, t):
    return s * (A @ R.T) + t


# ---- random inputs of the solver and of the fit ---------------------------------------------------------------------------------------------
def true_samples(rng, H, with_scale=True):
    """H noise-free samples A, B (H, 3, 3) and their transforms [(s, R, t)]."""
    A, B, gt = np.zeros((H, 3, 3)), np.zeros((H, 3, 3)), []
    for h in range(H):
        s, R, t = similarity(rng, with_scale)
        A[h] = cloud(rng, 3)
        B[h] = transform(A[h], s, R, t)
        gt.append((s, R, t))
    return A, B, gt


KINDS = ("noise-free", "noisy", "near-collinear", "planar", "far from the origin")


def shaped_cloud(rng, n, kind):
    """A cloud of n points of one of KINDS (by index) and its image under a random similarity, noisy for kind 1 (and for every other odd
    draw of the later kinds): (A, B)."""
    A = cloud(rng, n)
    if kind == 2:                                     # on a line, up to a perturbation around the solver's sine threshold (1e-4)
        A = A[0] + rng.uniform(-1, 1, (n, 1)) * (A[1] - A[0]) + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-6, -2)
    elif kind == 3:                                   # in a plane
        u, v = rng.normal(size=3), rng.normal(size=3)
        A = A[0] + rng.uniform(-1, 1, (n, 1)) * u + rng.uniform(-1, 1, (n, 1)) * v
    elif kind == 4:                                   # 1e3 away from the origin
        A = A + rng.normal(size=3) * 1e3
    s, R, t = similarity(rng)
    B = transform(A, s, R, t)
    if kind == 1 or (kind > 1 and rng.random() < 0.5):
        B = B + rng.normal(size=B.shape) * 1e-3 * s
    return A, B


def centred_sums(A, B):
    """(S (10,), ca, cb) of a cloud: the inputs of the fit, in plain numpy (the test's data; any order of summation will do)."""
    ca, cb = A.mean(axis=0), B.mean(axis=0)
    x, y = A - ca, B - cb
    return np.r_[(x.T @ y).reshape(-1), (x * x).sum()], ca, cb


def mixed_inputs(rng, H):
    """H inputs of the host-compiled solver slice, the five KINDS in turn: samples A, B (H, 3, 3), and for the fit the centred sums S
    (H, 10) and centroids ca, cb (H, 3) of a cloud of 3..40 points of the same kind."""
    A, B = np.zeros((H, 3, 3)), np.zeros((H, 3, 3))
    S, ca, cb = np.zeros((H, 10)), np.zeros((H, 3)), np.zeros((H, 3))
    for h in range(H):
        kind = h % len(KINDS)
        A[h], B[h] = shaped_cloud(rng, 3, 0 if kind == 3 else kind)      # (three points are always in a plane)
        S[h], ca[h], cb[h] = centred_sums(*shaped_cloud(rng, int(rng.integers(3, 41)), kind))
    return A, B, S, ca, cb


# ---- the SVD fit the closed form is compared with ----------------------------------------------------------------------------------------------
def umeyama(A, B, with_scale=True):
    """The least-squares (s, R, t) of B ~= s R A + t by numpy.linalg.svd with the determinant correction (Umeyama, PAMI 1991)."""
    ca, cb = A.mean(axis=0), B.mean(axis=0)
    x, y = A - ca, B - cb
    U, D, Vt = np.linalg.svd(y.T @ x)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    s = float((D * d).sum() / (x * x).sum()) if with_scale else 1.0
    return s, R, cb - s * R @ ca


# ---- scenes and ground truth ----------------------------------------------------------------------------------------------------------------
def scene(n, sigma, outliers, nan_share, seed, with_scale=True, scale=None):
    """n 3D-3D correspondences from a generator of its own: a cloud A in a box in front of a camera, a true (s, R, t), B = s R A + t with
    Gaussian noise of sigma per coordinate in A's unit (sigma s in B's, which is what makes thr = 3 sqrt(3) sigma s three times the RMS
    length of the noise), a share of gross outliers (B uniform in the box of the true B grown to at least 10 thresholds per side), a share
    of NaN rows (all of A's row, all of B's row, or both).  Returns dict A, B (n, 3) float32, B_true (n, 3) = s R A + t of the fp32 A,
    outlier and nan flags, s, R, t, thr.  `scale`: the true s, in place of the drawn one."""
    rng = np.random.default_rng(seed)
    s, R, t = similarity(rng, with_scale)
    if scale is not None:
        s, t = float(scale), t / s * float(scale)
    A = cloud(rng, n).astype(np.float32)
    B_true = transform(A.astype(np.float64), s, R, t)
    thr = 3.0 * np.sqrt(3.0) * sigma * s
    B = B_true + rng.normal(size=(n, 3)) * sigma * s
    out = rng.random(n) < outliers
    lo, hi = B_true.min(axis=0), B_true.max(axis=0)
    grow = np.maximum(0.0, 10.0 * thr - (hi - lo)) / 2.0
    B[out] = rng.uniform(lo - grow, hi + grow, (int(out.sum()), 3))
    nan = rng.random(n) < nan_share
    side = rng.integers(0, 3, n)
    A, B = A.copy(), B.astype(np.float32)
    A[nan & (side != 1)] = np.nan
    B[nan & (side != 0)] = np.nan
    return dict(A=A, B=B, B_true=B_true, outlier=out, nan=nan, s=s, R=R, t=t, thr=float(thr))


def errors(sc, s, R, t):
    """(rotation error in degrees, relative scale error, RMS of s R A + t - B_true over the true inliers relative to thr) of an estimate
    against the scene's truth."""
    c = np.clip((np.trace(sc["R"].T @ np.asarray(R, np.float64)) - 1.0) / 2.0, -1.0, 1.0)
    good = ~sc["outlier"] & ~sc["nan"]
    d = transform(sc["A"][good].astype(np.float64), s, np.asarray(R, np.float64), np.asarray(t, np.float64)) - sc["B_true"][good]
    return float(np.rad2deg(np.arccos(c))), float(abs(s / sc["s"] - 1.0)), float(np.sqrt((d * d).sum(axis=1).mean()) / sc["thr"])


def ragged(ns, sigma=0.01, outliers=0.4, nan_share=0.1, with_scale=True, seed0=100):
    """A batch of scenes with ns[p] correspondences in (P, max(ns), 3) float32 tables (zeros past the count), all of one true scale
    (2.5, or 1 when rigid) and so of one threshold: A, B, thr."""
    P, cap = len(ns), max(max(ns), 1)
    A, B, thr = np.zeros((P, cap, 3), np.float32), np.zeros((P, cap, 3), np.float32), 0.0
    for p, n in enumerate(ns):
        sc = scene(max(n, 1), sigma, outliers, nan_share, seed0 + p, with_scale, scale=2.5 if with_scale else 1.0)
        A[p, :n], B[p, :n], thr = sc["A"][:n], sc["B"][:n], sc["thr"]
    return A, B, thr


def alignment_batch(P=1500, cap=1024, seed=1500, nlo=200):
    """The time tool's set: P scenes of nlo..cap correspondences, sigma 0.01, 40 % outliers, 5 % NaN rows, true scale 2.5.  Returns A, B
    (P, cap, 3) float32, counts (P,) int32, the scenes' truths [(s, R, t)] and thr."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(nlo, cap + 1, P).astype(np.int32)
    A, B, gt, thr = np.zeros((P, cap, 3), np.float32), np.zeros((P, cap, 3), np.float32), [], 0.0
    for p in range(P):
        sc = scene(int(counts[p]), 0.01, 0.4, 0.05, seed + p, scale=2.5)
        A[p, :counts[p]], B[p, :counts[p]], thr = sc["A"], sc["B"], sc["thr"]
        gt.append((sc["s"], sc["R"], sc["t"]))
    return A, B, counts, gt, thr
