"""What the tests and the time tools of the three two-view estimators share that is not specification (that is oracle/twoview_reference.py
and the three restatements): building a solver for the host, random samples, synthetic scenes on the MegaDepth-1500 cameras
(tests/golden/megadepth1500_poses.npz), ground truth, the common half of the GPU comparisons, the tools' timed loop.

The generators consume their ``numpy`` generator in a fixed order, which is part of the tests' inputs: a motion is w, t, then the points."""
import os
import subprocess
import tempfile

import numpy as np

from oracle.twoview_reference import sampson

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated_features_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
POSES = os.path.join(ROOT, "tests", "golden", "megadepth1500_poses.npz")


# ---- a solver of the product source, built for the host ------------------------------------------------------------------------------------
def _between(name, begin, end):
    """(whole text, text between the two markers) of a product source file."""
    t = open(os.path.join(CSRC, name)).read()
    a = t.index(begin)
    return t, t[a:t.index(end, a)]


def slice_solver(hip_file, begin, end):
    """The shared geometry (twoview_math.hpp, which must be host-compilable as a whole file) in front of the solver's own slice."""
    header, shared = _between("twoview_math.hpp", "// ---- twoview math begin", "// ---- twoview math end")
    _, solver = _between(hip_file, begin, end)
    for s in (header, solver):
        assert "__shared__" not in s and "asm" not in s and "__builtin_amdgcn" not in s
    assert "gauss_jordan" in shared and "gauss_jordan(S s" not in solver
    return (shared + solver).replace("__device__ ", "")


def build_emu(slice_name, driver, src):
    """Compile tests/emu/<driver>.cpp (fp contraction off) against the slice `src`, written as <slice_name>; returns the program's path."""
    import pytest
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, slice_name), "w").write(src)
    out = os.path.join(td, driver)
    subprocess.run([CLANG, "-O2", "-w", "-std=c++20", "-ffp-contract=off", "-I", td, "-I", EMU, os.path.join(EMU, driver + ".cpp"), "-o", out],
                   check=True)
    return out


# ---- random samples of a solver ---------------------------------------------------------------------------------------------------------------
def rotation(w):
    """Rodrigues: the rotation by |w| about w."""
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def motion(rng, m):
    """A random motion and m points in front of camera 0: R, t, X (m, 3)."""
    R, t = rotation(rng.normal(size=3) * 0.3), rng.normal(size=3)
    return R, t, np.c_[rng.uniform(-1, 1, (m, 2)), rng.uniform(2, 6, m)]


def project(X, R, t):
    """Normalised coordinates (x0, y0, x1, y1) of the points X in camera 0 and in camera 1 = R X + t."""
    X2 = X @ R.T + t
    return X[:, 0] / X[:, 2], X[:, 1] / X[:, 2], X2[:, 0] / X2[:, 2], X2[:, 1] / X2[:, 2]


def true_samples(rng, H, m, unit_t=False):
    """H noise-free samples of m points, x (4, H, m), and their motions [(R, t)]."""
    x = np.zeros((4, H, m))
    gt = []
    for h in range(H):
        R, t, X = motion(rng, m)
        if unit_t:
            t /= np.linalg.norm(t)
        x[:, h] = project(X, R, t)
        gt.append((R, t))
    return x, gt


def mixed_samples(rng, H, m, spread, degenerate):
    """H samples of m points, x (4, H, m), of four kinds in turn: uniform noise in [-spread, spread], noise-free scenes, noisy scenes,
    near-degenerate scenes (degenerate(X, h % 3) edits the points in place: coplanar / collinear / repeated)."""
    x = rng.uniform(-spread, spread, (4, H, m))
    kind = np.arange(H) % 4
    for h in np.nonzero(kind > 0)[0]:
        R, t, X = motion(rng, m)
        if kind[h] == 3:
            degenerate(X, h % 3)
        x[:, h] = project(X, R, t)
        if kind[h] == 2:
            x[:, h] += rng.normal(size=(4, m)) * 1e-3
    return x


# ---- synthetic scenes and ground truth ----------------------------------------------------------------------------------------------------------
def essential_from_pose(R, t):
    """[t]x R (the definition of accelerated_features_amd.pose, restated)."""
    t = np.asarray(t, np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ np.asarray(R, np.float64)


def true_F(K0, K1, T_0to1):
    """F = K1^-T [t]x R K0^-1 of X1 = R X0 + t (unit Frobenius norm)."""
    T = np.asarray(T_0to1, np.float64)
    F = np.linalg.inv(np.asarray(K1, np.float64)).T @ essential_from_pose(T[:3, :3], T[:3, 3]) @ np.linalg.inv(np.asarray(K0, np.float64))
    return F / np.linalg.norm(F)


def f_distance(F, G):
    """Distance of two F up to scale and sign: min over the sign of |F/|F| -+ G/|G||_F."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    G = np.asarray(G, np.float64).reshape(3, 3)
    F, G = F / np.linalg.norm(F), G / np.linalg.norm(G)
    return min(np.linalg.norm(F - G), np.linalg.norm(F + G))


def sampson_px(F, p0, p1):
    """Sampson errors (pixels, not squared) of correspondences p0, p1 (n, 2) under F (3, 3)."""
    F = np.asarray(F, np.float64).reshape(-1)
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    return np.sqrt(sampson(F, p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]))


def synthetic_pair(K0, K1, T_0to1, n, noise=0.5, outliers=0.0, size0=(480, 640), size1=(480, 640), rng=None):
    """n correspondences (fp32 pixels) of 3D points in front of both cameras, seen in both images, with Gaussian pixel noise in image 1
    and a fraction of outliers (uniform in image 1).  Returns pts0, pts1 (n, 2) float32 and the outlier flags."""
    rng = np.random.default_rng(0) if rng is None else rng
    K0, K1, T = (np.asarray(v, np.float64) for v in (K0, K1, T_0to1))
    R, t = T[:3, :3], T[:3, 3]
    h0, w0 = size0
    h1, w1 = size1
    depth = max(1.0, 4.0 * np.linalg.norm(t))
    p0s, p1s = [], []
    for rnd in range(1000):
        if sum(len(p) for p in p0s) >= n:
            break
        m = 4 * n
        uv = np.c_[rng.uniform(0, w0, m), rng.uniform(0, h0, m)]
        z = rng.uniform(0.5 * depth, 2.0 * depth, m)
        X = np.c_[(uv[:, 0] - K0[0, 2]) / K0[0, 0] * z, (uv[:, 1] - K0[1, 2]) / K0[1, 1] * z, z]
        X1 = X @ R.T + t
        ok = X1[:, 2] > 1e-3
        u1 = K1[0, 0] * X1[:, 0] / np.where(ok, X1[:, 2], 1.0) + K1[0, 2]
        v1 = K1[1, 1] * X1[:, 1] / np.where(ok, X1[:, 2], 1.0) + K1[1, 2]
        if rnd < 20:                              # in image 1 as well; after 20 rounds (poses whose views barely overlap) in front of it only
            ok &= (u1 >= 0) & (u1 < w1) & (v1 >= 0) & (v1 < h1)
        p0s.append(uv[ok])
        p1s.append(np.c_[u1, v1][ok])
    p0 = np.concatenate(p0s)[:n]
    p1 = np.concatenate(p1s)[:n] + rng.normal(size=(n, 2)) * noise
    out = rng.random(n) < outliers
    p1[out] = np.c_[rng.uniform(0, w1, out.sum()), rng.uniform(0, h1, out.sum())]
    return p0.astype(np.float32), p1.astype(np.float32), out


def fixture():
    """The MegaDepth-1500 cameras, poses and image sizes."""
    return dict(np.load(POSES))


def fixture_pair(f, i, n, noise, outliers, rng):
    """synthetic_pair on pair i of the fixture."""
    return synthetic_pair(f["K0"][i], f["K1"][i], f["T_0to1"][i], n, noise, outliers, tuple(f["size0_hw"][i]), tuple(f["size1_hw"][i]), rng)


def scene(i, n, noise, outliers, seed):
    """n correspondences on pair i of the fixture from a generator of its own: pts0, pts1, outlier flags, K0, K1, T_0to1."""
    f = fixture()
    return fixture_pair(f, i, n, noise, outliers, np.random.default_rng(seed)) + (f["K0"][i], f["K1"][i], f["T_0to1"][i])


def holdout(f, p, n):
    """n noise-free true correspondences of pair p that no estimator saw (generator seeded with p)."""
    return fixture_pair(f, p, n, 0.0, 0.0, np.random.default_rng(p))[:2]


def megadepth_synthetic(f, P=1500, cap=1024, seed=1500, nlo=200):
    """The synthetic MegaDepth-1500 set of the AUC / held-out-error tests and of the time tools: pair p on the fixture's K0 / K1 / T_0to1 /
    sizes, nlo..cap correspondences, 0.5-1 px noise, 40 % outliers.  Returns pts0, pts1 (P, cap, 2) float32 and counts (P,) int32."""
    rng = np.random.default_rng(seed)
    pts0, pts1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    counts = rng.integers(nlo, cap + 1, P).astype(np.int32)
    for p in range(P):
        a, b, _ = fixture_pair(f, p, int(counts[p]), rng.uniform(0.5, 1.0), 0.4, rng)
        pts0[p, :counts[p]], pts1[p, :counts[p]] = a, b
    return pts0, pts1, counts


def homography_pair(n, outlier_frac, noise, seed, size=(640.0, 480.0)):
    """n correspondences under a random plausible homography: (p0, p1, H_true, inlier flags)."""
    g = np.random.default_rng(seed)
    w, h = size
    a = g.uniform(-0.35, 0.35)
    s = g.uniform(0.8, 1.25)
    H = np.array([[s * np.cos(a), -s * np.sin(a), g.uniform(-60, 60)],
                  [s * np.sin(a), s * np.cos(a), g.uniform(-40, 40)],
                  [g.uniform(-2e-4, 2e-4), g.uniform(-2e-4, 2e-4), 1.0]])
    p0 = np.stack([g.uniform(0, w, n), g.uniform(0, h, n)], axis=1)
    q = np.concatenate([p0, np.ones((n, 1))], axis=1) @ H.T
    p1 = q[:, :2] / q[:, 2:] + g.normal(0, noise, (n, 2))
    out = g.random(n) < outlier_frac
    p1[out] = np.stack([g.uniform(0, w, out.sum()), g.uniform(0, h, out.sum())], axis=1)
    return p0.astype(np.float32), p1.astype(np.float32), H, ~out


# ---- the GPU comparisons and the time tools ---------------------------------------------------------------------------------------------------
def check_common(got, want, p, n):
    """Pair p of a batch result against the restatement's: the info words and the mask exactly, nothing past the pair's count."""
    info = got["info"][p].cpu().numpy()
    assert list(info) == list(want["info"]), (list(info), list(want["info"]))
    assert np.array_equal(got["inliers"][p, :n].cpu().numpy(), want["mask"])
    assert not got["inliers"][p, n:].any()


def timed(call, warm, reps):
    """(the last result, milliseconds per call) of `reps` event-timed calls after `warm` untimed ones."""
    import torch
    for _ in range(warm):
        r = call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        r = call()
    e1.record()
    torch.cuda.synchronize()
    return r, e0.elapsed_time(e1) / reps


def time_megadepth(call, label, tail):
    """The relative-pose and fundamental tools' cases: one pair with 2000 matches at 1000 iterations, the 1500 pairs (200-1024 matches) at
    1000 and at 10000.  call(pts0, pts1, counts, f, P, iters) -> result dict; tail(f, P, result, info) -> the end of the report line."""
    import torch
    f = fixture()
    for P, nlo, nhi, iters, reps in ((1, 2000, 2000, 1000, 20), (1500, 200, 1024, 1000, 3), (1500, 200, 1024, 10000, 2)):
        a, b, c = (torch.from_numpy(v).cuda() for v in megadepth_synthetic(f, P, nhi, 1500, nlo))
        r, ms = timed(lambda: call(a, b, c, f, P, iters), 1, reps)
        info = r["info"].cpu().numpy()
        print(f"P {P:4d} n {nlo}-{nhi} {label} {iters:5d}: {ms:9.3f} ms per call, found {int(info[:, 0].sum())}/{P}, "
              f"loop iterations mean {info[:, 2].mean():.0f} max {info[:, 2].max()}, refinement steps {info[:, 4].mean():.1f}, "
              f"{tail(f, P, r, info)}", flush=True)
