"""Scenes of the two-view structure tests (tests/test_structure_*.py, tests/test_gpu_structure.py) and of tools/structure_time.py: what is
not specification (that is tests/structure_reference.py).  Built on twoview_support.motion / project; the generators consume their numpy
generator in a fixed order, which is part of the tests' inputs."""
import math

import numpy as np

import twoview_support as TS

F = 800.0
K = np.array([[F, 0.0, 640.0], [0.0, F, 480.0], [0.0, 0.0, 1.0]])
SCALES = (1.0, -1.0, 3.7, -1e-3)


def pixels(x, y, Km=K):
    return np.c_[Km[0, 0] * x + Km[0, 2], Km[1, 1] * y + Km[1, 2]]


def scene(rng, n, noise=0.0, Km=K):
    """n points of a random motion seen by two cameras with intrinsics Km: dict p0, p1 (n,2) float64 pixels, R, t, X (n,3)."""
    R, t, X = TS.motion(rng, n)
    x0, y0, x1, y1 = TS.project(X, R, t)
    p0, p1 = pixels(x0, y0, Km), pixels(x1, y1, Km)
    if noise:
        p0, p1 = p0 + rng.normal(size=p0.shape) * noise, p1 + rng.normal(size=p1.shape) * noise
    return dict(p0=p0, p1=p1, R=R, t=t, X=X)


def scene_in_front(rng, n, noise=0.0, Km=K, min_t=0.0):
    """scene() redrawn until every point is at least 0.5 in front of camera 1 as well (motion() only puts them in front of camera 0) and
    the baseline is at least min_t (depths in the unit of t stay below 6 / min_t)."""
    while True:
        s = scene(rng, n, noise, Km)
        if (s["X"] @ s["R"].T + s["t"])[:, 2].min() > 0.5 and np.linalg.norm(s["t"]) >= min_t:
            return s


def project_points(X, R, t, Km=K):
    x0, y0, x1, y1 = TS.project(X, R, t)
    return pixels(x0, y0, Km), pixels(x1, y1, Km)


def mixed_group(rng, g, m):
    """m correspondences under one pose, of six kinds in turn: noise-free; noisy (0.5 - 10 px); uniform random pixels; camera 1 far behind
    camera 0's scene + far points + rows that are not finite; an unusable pose (zeroed / a NaN entry); tight gates (max_depth inside the
    scene, 0.5 px reprojection, 8 degrees of parallax) with a random mask."""
    kind = g % 6
    s = scene(rng, m, noise=(0.0, (0.5, 1.0, 3.0, 10.0)[(g // 6) % 4], 0.0, 0.0, 0.5, 0.5)[kind])
    out = dict(p0=s["p0"], p1=s["p1"], K0=K, K1=K, R=s["R"], t=s["t"], thr=4.0, deg=1.0, max_depth=math.inf, mask=None)
    if kind == 2:
        out["p0"], out["p1"] = np.c_[rng.uniform(0, 1280, m), rng.uniform(0, 960, m)], np.c_[rng.uniform(0, 1280, m), rng.uniform(0, 960, m)]
        out["thr"] = 400.0
    elif kind == 3:
        t = np.array([0.1, 0.0, -10.0])
        X = s["X"].copy()
        X[m // 2:, :2] *= 1e5
        X[m // 2:, 2] *= 1e5                              # the second half far away, in front of both cameras: no parallax
        X[m // 4:m // 2] = (-s["R"].T @ t)[None, :] * rng.uniform(1.5, 3.0, (m // 2 - m // 4, 1))      # on the baseline
        out["t"] = t
        out["p0"], out["p1"] = project_points(X, s["R"], t)
        out["p0"][3, 0] = np.nan; out["p1"][5, 1] = np.inf; out["p0"][m - 2] = np.nan
    elif kind == 4:
        out["R"] = np.zeros((3, 3)) if (g // 6) % 2 == 0 else np.where(np.arange(9).reshape(3, 3) == 4, np.nan, s["R"])
        out["t"] = np.zeros(3) if (g // 6) % 2 == 0 else s["t"]
    elif kind == 5:
        out.update(thr=0.5, deg=8.0, max_depth=4.0, mask=(rng.random(m) > 0.2).astype(np.uint8))
    out["p0"], out["p1"] = out["p0"].astype(np.float32), out["p1"].astype(np.float32)
    return out


def records(g):
    """The host driver's records (m, 28) of a group."""
    m = g["p0"].shape[0]
    import structure_reference as SR
    head = np.concatenate([np.asarray(g["R"], np.float64).reshape(9), np.asarray(g["t"], np.float64).reshape(3), SR.calibration(g["K0"], g["K1"])])
    masked = np.zeros(m) if g["mask"] is None else (np.asarray(g["mask"]) == 0).astype(np.float64)
    tail = np.array([g["thr"] * g["thr"], math.cos(math.radians(g["deg"])), g["max_depth"]])
    return np.c_[np.tile(head, (m, 1)), g["p0"].astype(np.float64), g["p1"].astype(np.float64), masked, np.tile(tail, (m, 1))]


def recover_case(rng, h, m):
    """An E and m correspondences: s [t]x R of a scene at the scales SCALES (noise-free, 1 px, 3 px), a random 3x3 matrix, an E that cannot
    be decomposed (zero / a NaN entry / rank one).  truth = (R, unit t) or None."""
    kind = h % 5
    s = scene(rng, m, noise=(0.0, 1.0, 3.0, 1.0, 0.0)[kind])
    tu = s["t"] / np.linalg.norm(s["t"])
    E = SCALES[(h // 5) % 4] * TS.essential_from_pose(s["R"], tu)
    truth = (s["R"], tu)
    if kind == 3:
        E, truth = rng.normal(size=(3, 3)), None
    elif kind == 4:
        sub = (h // 5) % 3
        E = np.zeros((3, 3)) if sub == 0 else (np.where(np.arange(9).reshape(3, 3) == 2, np.nan, E) if sub == 1 else np.outer(rng.normal(size=3), rng.normal(size=3)))
        truth = None
    return dict(E=E, p0=s["p0"].astype(np.float32), p1=s["p1"].astype(np.float32), K0=K, K1=K, thr=50.0 if h % 2 else math.inf, truth=truth)


def pack(lists, cap=None):
    """[(n_p, 2) arrays] -> (P, cap, 2) float32 (zeros beyond the counts) and counts (P,) int32."""
    cap = max([len(v) for v in lists] + [1]) if cap is None else cap
    out = np.zeros((len(lists), cap, 2), np.float32)
    for p, v in enumerate(lists):
        out[p, :len(v)] = v
    return out, np.array([len(v) for v in lists], np.int32)
