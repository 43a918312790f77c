"""Test data of the absolute-pose estimator (csrc/k_abspose.hip, tests/abspose_reference.py) that is not specification: random P3P
samples, 2D-3D scenes on the MegaDepth-1500 cameras and poses (tests/golden/megadepth1500_poses.npz), ground-truth errors.

The generators consume their ``numpy`` generator in a fixed order, which is part of the tests' inputs."""
import numpy as np

import twoview_support as TS


# ---- random samples of the solver ---------------------------------------------------------------------------------------------------------
def true_samples(rng, H):
    """H noise-free samples: x, y (H, 3) normalised coordinates in the camera, X (H, 3, 3) world points, and the poses [(R, t)] with
    X_cam = R X_world + t (TS.motion: points in front of the world frame's origin, a random motion; redrawn until the camera sees them)."""
    x, y, X = np.zeros((H, 3)), np.zeros((H, 3)), np.zeros((H, 3, 3))
    gt = []
    for h in range(H):
        while True:                                  # until the camera sees the three points: in front of it, inside a 90 degree field of view
            R, t, Xw = TS.motion(rng, 3)
            _, _, x[h], y[h] = TS.project(Xw, R, t)
            if ((Xw @ R.T + t)[:, 2] > 0).all() and max(np.abs(x[h]).max(), np.abs(y[h]).max()) <= 1.0:
                break
        X[h] = Xw
        gt.append((R, t))
    return x, y, X, gt


def degenerate(X, sub):
    """TS.mixed_samples' near-degenerate kinds for three 3D points, in place: collinear / a repeated point / nearly collinear."""
    if sub == 0:
        X[2] = X[0] + 0.7 * (X[1] - X[0])           # collinear
    elif sub == 1:
        X[2] = X[1] * (1 + 1e-9)                    # a repeated point
    else:
        X[2] = X[0] + 0.4 * (X[1] - X[0]) + 1e-5    # nearly collinear (around the solver's sine threshold)


def mixed_samples(rng, H):
    """TS.mixed_samples adapted to 3 points with 3D coordinates: H samples x, y (H, 3), X (H, 3, 3) of four kinds in turn -- uniform noise
    (image coordinates in [-0.8, 0.8], points in a box), noise-free scenes, noisy scenes, near-degenerate scenes."""
    x, y = rng.uniform(-0.8, 0.8, (H, 3)), rng.uniform(-0.8, 0.8, (H, 3))
    X = np.stack([rng.uniform(-1, 1, (H, 3)), rng.uniform(-1, 1, (H, 3)), rng.uniform(2, 6, (H, 3))], axis=-1)
    kind = np.arange(H) % 4
    for h in np.nonzero(kind > 0)[0]:
        R, t, Xw = TS.motion(rng, 3)
        if kind[h] == 3:
            degenerate(Xw, h % 3)
        _, _, x[h], y[h] = TS.project(Xw, R, t)
        X[h] = Xw
        if kind[h] == 2:
            x[h] += rng.normal(size=3) * 1e-3
            y[h] += rng.normal(size=3) * 1e-3
    return x, y, X


# ---- scenes and ground truth ----------------------------------------------------------------------------------------------------------------
def scene3d(i, n, noise, outliers, seed, f=None):
    """n 2D-3D correspondences on pair i of the fixture, from a generator of its own: the construction of TS.synthetic_pair -- points drawn
    in camera 0 through uniform pixels of image 0, depths uniform in [0.5, 2] max(1, 4 |t|), kept if in front of camera 1 and inside image 1
    (after 20 rounds: in front of it only).  Camera 0's frame is the world.  Returns X (n, 3) float32, the pixels in image 1 (n, 2) float32
    (Gaussian noise, then a fraction of outliers uniform in the image), the outlier flags, K1 and T_0to1 (3, 4) = the true pose."""
    f = TS.fixture() if f is None else f
    rng = np.random.default_rng(seed)
    K0, K1, T = (np.asarray(f[k][i], np.float64) for k in ("K0", "K1", "T_0to1"))
    R, t = T[:3, :3], T[:3, 3]
    h0, w0 = (int(v) for v in f["size0_hw"][i])
    h1, w1 = (int(v) for v in f["size1_hw"][i])
    depth = max(1.0, 4.0 * np.linalg.norm(t))
    Xs, ps = [], []
    for rnd in range(1000):
        if sum(len(v) for v in Xs) >= n:
            break
        m = 4 * max(n, 1)
        uv = np.c_[rng.uniform(0, w0, m), rng.uniform(0, h0, m)]
        z = rng.uniform(0.5 * depth, 2.0 * depth, m)
        X = np.c_[(uv[:, 0] - K0[0, 2]) / K0[0, 0] * z, (uv[:, 1] - K0[1, 2]) / K0[1, 1] * z, z].astype(np.float32).astype(np.float64)
        X1 = X @ R.T + t
        ok = X1[:, 2] > 1e-3
        u1 = K1[0, 0] * X1[:, 0] / np.where(ok, X1[:, 2], 1.0) + K1[0, 2]
        v1 = K1[1, 1] * X1[:, 1] / np.where(ok, X1[:, 2], 1.0) + K1[1, 2]
        if rnd < 20:
            ok &= (u1 >= 0) & (u1 < w1) & (v1 >= 0) & (v1 < h1)
        Xs.append(X[ok])
        ps.append(np.c_[u1, v1][ok])
    X = np.concatenate(Xs)[:n]
    p = np.concatenate(ps)[:n] + rng.normal(size=(n, 2)) * noise
    out = rng.random(n) < outliers
    p[out] = np.c_[rng.uniform(0, w1, out.sum()), rng.uniform(0, h1, out.sum())]
    return X.astype(np.float32), p.astype(np.float32), out, K1, T[:3, :4]


def pose_errors(T_true, R, t):
    """(rotation error in degrees, |t - t_true| / max(1, 4 |t_true|)) of an estimated pose against the true (3, 4) one."""
    T = np.asarray(T_true, np.float64)
    c = np.clip((np.trace(T[:3, :3].T @ np.asarray(R, np.float64)) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.rad2deg(np.arccos(c))), float(np.linalg.norm(np.asarray(t, np.float64) - T[:3, 3]) / max(1.0, 4.0 * np.linalg.norm(T[:3, 3])))


def abspose_batch(P=1500, cap=1024, seed=1500, nlo=200):
    """The time tool's set: pair p of the fixture, nlo..cap correspondences, 0.5-1 px noise, 40 % outliers.  Returns pts2d (P, cap, 2),
    pts3d (P, cap, 3) float32, counts (P,) int32, K (P, 3, 3), T (P, 3, 4)."""
    rng = np.random.default_rng(seed)
    pts2d, pts3d = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 3), np.float32)
    counts = rng.integers(nlo, cap + 1, P).astype(np.int32)
    K, T = np.zeros((P, 3, 3)), np.zeros((P, 3, 4))
    f = TS.fixture()
    for p in range(P):
        X, px, _, K[p], T[p] = scene3d(p, int(counts[p]), float(rng.uniform(0.5, 1.0)), 0.4, seed + p, f)
        pts3d[p, :counts[p]], pts2d[p, :counts[p]] = X, px
    return pts2d, pts3d, counts, K, T
