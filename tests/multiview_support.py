"""Scenes of the multi-view triangulation tests (tests/test_multiview_*.py, tests/test_gpu_multiview.py) and of tools/multiview_time.py: what
is not specification (that is tests/multiview_reference.py).  Cameras are the MegaDepth-1500 intrinsics of tests/golden/megadepth1500_poses.npz
on an arc around the scene, so the baseline to the reference view grows with the view index; the generators consume their numpy generator in
a fixed order, which is part of the tests' inputs."""
import numpy as np

import twoview_support as TS

DEPTH = 7.0                                  # of the scene's centre in the reference camera
STEP_DEG = 3.0                               # of arc per view, up to ARC_DEG in all
ARC_DEG = 45.0


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def arc_poses(rng, V, ref_identity=False):
    """World -> camera poses of V views: view 0 at a random pose (ref_identity: at (I, 0)), view v on an arc about the scene's centre,
    looking at it."""
    R0, t0 = TS.rotation(rng.normal(size=3) * 0.3), rng.normal(size=3)
    if ref_identity:
        R0, t0 = np.eye(3), np.zeros(3)
    step = np.radians(min(STEP_DEG, ARC_DEG / max(V - 1, 1)))
    P = np.array([0.0, 0.0, DEPTH])
    Rs, ts = np.zeros((V, 3, 3)), np.zeros((V, 3))
    for v in range(V):
        A = _ry(step * v)                                  # the camera's axes in the reference camera's frame
        c = P - A @ P                                      # its centre there
        Rrel, trel = A.T, -A.T @ c
        Rs[v], ts[v] = Rrel @ R0, Rrel @ t0 + trel
    return Rs, ts


def arc_scene(rng, V, K, noise=0.0, cam=0, kcap=None, shuffle=True, ref_identity=False):
    """K tracks seen from V views: dict kpts (V,kcap,2) float32, kpts64 (the same before rounding), tracks (K,V) int32 (-1 where the point
    is outside the image or behind the camera), Ks, Rs (V,3,3), ts (V,3), X (K,3) world points, n_views.  Row k of view 0 is track k; the
    rows of the other views are shuffled."""
    f = TS.fixture()
    kcap = K if kcap is None else kcap
    Ks = np.stack([f["K0" if v % 2 == 0 else "K1"][(cam + v // 2) % len(f["K0"])] for v in range(V)]).astype(np.float64)
    sizes = [tuple(f["size0_hw" if v % 2 == 0 else "size1_hw"][(cam + v // 2) % len(f["K0"])]) for v in range(V)]
    Rs, ts = arc_poses(rng, V, ref_identity)
    h0, w0 = sizes[0]
    uv = np.c_[rng.uniform(0.1 * w0, 0.9 * w0, K), rng.uniform(0.1 * h0, 0.9 * h0, K)]
    z = rng.uniform(0.6 * DEPTH, 1.4 * DEPTH, K)
    X0 = np.c_[(uv[:, 0] - Ks[0][0, 2]) / Ks[0][0, 0] * z, (uv[:, 1] - Ks[0][1, 2]) / Ks[0][1, 1] * z, z]
    X = (X0 - ts[0]) @ Rs[0]                               # R0' (X0 - t0)
    kpts = np.zeros((V, kcap, 2))
    tracks = np.full((K, V), -1, np.int32)
    for v in range(V):
        Xc = X @ Rs[v].T + ts[v]
        front = Xc[:, 2] > 0.1
        zc = np.where(front, Xc[:, 2], 1.0)
        p = np.c_[Ks[v][0, 0] * Xc[:, 0] / zc + Ks[v][0, 2], Ks[v][1, 1] * Xc[:, 1] / zc + Ks[v][1, 2]]
        h, w = sizes[v]
        seen = front & (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)
        if v == 0:
            seen[:] = True
        p = p + rng.normal(size=p.shape) * noise
        rows = rng.permutation(kcap)[:K] if (shuffle and v > 0) else np.arange(K)
        kpts[v, rows] = p
        tracks[:, v] = np.where(seen, rows, -1)
    return dict(kpts=kpts.astype(np.float32), kpts64=kpts, tracks=tracks, Ks=Ks, Rs=Rs, ts=ts, X=X, n_views=V, sizes=sizes)


def plant_outliers(rng, sc, frac=0.3, lo=50.0, hi=150.0):
    """Moves the observation of one view v >= 1 of a fraction of the tracks with at least 4 observing views by lo .. hi pixels in a random
    direction (in place, kpts and kpts64).  Returns planted (K,) int: the view, or -1."""
    tracks = sc["tracks"]
    K, V = tracks.shape
    planted = np.full(K, -1)
    for k in np.nonzero((tracks >= 0).sum(axis=1) >= 4)[0]:
        if rng.random() >= frac:
            continue
        v = rng.choice(np.nonzero(tracks[k, 1:] >= 0)[0]) + 1
        a, d = rng.uniform(0, 2 * np.pi), rng.uniform(lo, hi)
        sc["kpts64"][v, tracks[k, v]] += d * np.array([np.cos(a), np.sin(a)])
        planted[k] = v
    sc["kpts"] = sc["kpts64"].astype(np.float32)
    return planted


def reproject(sc, X):
    """Replaces the scene's world points by X (K,3) and every observed pixel by its noise-free projection (in place; a point behind a
    camera keeps its table entry and projects through the centre)."""
    t = sc["tracks"]
    for v in range(t.shape[1]):
        Xc = X @ sc["Rs"][v].T + sc["ts"][v]
        p = np.c_[sc["Ks"][v][0, 0] * Xc[:, 0] / Xc[:, 2] + sc["Ks"][v][0, 2], sc["Ks"][v][1, 1] * Xc[:, 1] / Xc[:, 2] + sc["Ks"][v][1, 2]]
        k = np.nonzero(t[:, v] >= 0)[0]
        sc["kpts64"][v, t[k, v]] = p[k]
    sc["X"] = X
    sc["kpts"] = sc["kpts64"].astype(np.float32)


def pair_points(sc, v=1, **kw):
    """structure_reference.triangulate on the pair (0, v) of a scene, its points moved to the world frame: (result, X world (K,3) float64
    from the float32 points, X world from the float64 depths, both-observed flags)."""
    import multiview_reference as MR
    import structure_reference as SR
    b = MR.stage_view(sc["Rs"][v], sc["ts"][v], sc["Ks"][v], sc["Rs"][0], sc["ts"][0])
    t = sc["tracks"]
    both = (t[:, 0] >= 0) & (t[:, v] >= 0)
    p0, p1 = sc["kpts"][0][np.where(both, t[:, 0], 0)], sc["kpts"][v][np.where(both, t[:, v], 0)]
    w = SR.triangulate(p0, p1, sc["Ks"][0], sc["Ks"][v], np.array(b["Rrel"]).reshape(3, 3), np.array(b["trel"]), **kw)
    Xc = np.stack([w["l0"] * w["y0"][0], w["l0"] * w["y0"][1], w["l0"]], axis=1)
    to_world = lambda P: (P - sc["ts"][0]) @ sc["Rs"][0]      # noqa: E731
    return w, to_world(w["points3d"].astype(np.float64)), to_world(Xc), both


MIXED_V = (2, 3, 8, 32)


def mixed_scene(rng, g, m):
    """Scene g of the bit-for-bit comparisons: m tracks seen from MIXED_V[g % 4] views, of eight kinds in turn (g // 4 % 8): noise-free;
    noisy (0.5 - 3 px); planted outliers; a view with a pose that is not finite (every fourth such scene: view 0) and NaN pixels; a
    zero-baseline view (reference pose (I, 0) and a copy of it; at V = 2 nothing else); far points and points behind a turned camera under
    a max_depth inside the scene; uniform random pixels at a 400 px threshold; tight gates (0.5 px, 8 degrees, min_views 3).  All of them
    with holes in the table (-1, and rows past the table).  Returns the scene with thr, deg, max_depth, min_views."""
    V, kind = MIXED_V[g % 4], (g // 4) % 8
    noise = (0.0, (0.5, 1.0, 3.0)[(g // 32) % 3], 0.5, 0.5, 0.5, 0.2, 0.0, 0.5)[kind]
    sc = arc_scene(rng, V, m, noise=noise, cam=g, ref_identity=kind == 4)
    sc.update(thr=4.0, deg=1.0, max_depth=np.inf, min_views=2)
    k64, tracks = sc["kpts64"], sc["tracks"]
    if kind == 2:
        plant_outliers(rng, sc, frac=0.5)
    elif kind == 3:
        v = 0 if (g // 32) % 4 == 3 else 1 + (g // 32) % (V - 1)
        if (g // 32) % 2:
            sc["Rs"][v, 1, 1] = np.nan
        else:
            sc["ts"][v, 2] = np.inf
        k64[rng.integers(0, V, m // 5), rng.integers(0, m, m // 5), rng.integers(0, 2, m // 5)] = np.nan
    elif kind == 4:
        sc["Rs"][V - 1], sc["ts"][V - 1] = np.eye(3), np.zeros(3)
        sc["Ks"][V - 1] = sc["Ks"][0]
        k64[V - 1, np.where(tracks[:, V - 1] >= 0, tracks[:, V - 1], 0)] = np.where((tracks[:, V - 1] >= 0)[:, None], k64[0, :m], k64[V - 1, np.where(tracks[:, V - 1] >= 0, tracks[:, V - 1], 0)])
    elif kind == 5:
        X = sc["X"].copy()
        c0 = -sc["Rs"][0].T @ sc["ts"][0]
        X[: m // 3] = c0 + (X[: m // 3] - c0) * 1e5        # far: no parallax
        sc["max_depth"] = DEPTH if (g // 32) % 2 == 0 else np.inf
        if V > 2:
            sc["Rs"][V - 1] = np.diag([-1.0, 1.0, -1.0]) @ sc["Rs"][V - 1]      # the last camera turned away: every point behind it
            sc["ts"][V - 1] = np.diag([-1.0, 1.0, -1.0]) @ sc["ts"][V - 1]
        for v in range(V):
            Xc = X @ sc["Rs"][v].T + sc["ts"][v]
            p = np.c_[sc["Ks"][v][0, 0] * Xc[:, 0] / Xc[:, 2] + sc["Ks"][v][0, 2], sc["Ks"][v][1, 1] * Xc[:, 1] / Xc[:, 2] + sc["Ks"][v][1, 2]]
            rows = np.where(tracks[:, v] >= 0, tracks[:, v], 0)
            k64[v, rows] = np.where((tracks[:, v] >= 0)[:, None], p + rng.normal(size=p.shape) * noise, k64[v, rows])
    elif kind == 6:
        k64[:] = np.stack([rng.uniform(0, 1600, k64.shape[:2]), rng.uniform(0, 1200, k64.shape[:2])], axis=-1)
        sc["thr"] = 400.0
    elif kind == 7:
        sc.update(thr=0.5, deg=8.0, max_depth=1.2 * DEPTH, min_views=min(3, V))
    holes = rng.random(tracks.shape) < 0.08
    holes[:, 0] &= rng.random(m) < 0.3
    tracks[holes] = np.where(rng.random(holes.sum()) < 0.5, -1, k64.shape[1] + rng.integers(0, 5, holes.sum()))
    sc["kpts"] = k64.astype(np.float32)
    return sc


def match_lists(rng, tracks, cap=None, dup=0):
    """The matcher's lists of the pairs (view 0, view v) that give the table `tracks` (K,V): idx_ref, idx_view (V-1,cap) int64 in a random
    order, n_matches (V-1,) int32; `dup` further matches per pair repeat a reference row with a smaller view row (which loses)."""
    K, V = tracks.shape
    cap = K + dup if cap is None else cap
    idx_ref, idx_view, n = np.zeros((V - 1, cap), np.int64), np.zeros((V - 1, cap), np.int64), np.zeros(V - 1, np.int32)
    for v in range(1, V):
        k = np.nonzero(tracks[:, v] >= 0)[0]
        a, b = k, tracks[k, v].astype(np.int64)
        if dup and len(k):
            e = rng.choice(len(k), dup)
            a, b = np.r_[a, a[e]], np.r_[b, np.maximum(b[e] - 1 - rng.integers(0, 3, dup), -1)]
        o = rng.permutation(len(a))
        n[v - 1] = len(a)
        idx_ref[v - 1, :len(a)], idx_view[v - 1, :len(a)] = a[o], b[o]
    return idx_ref, idx_view, n


def world_error(got, X):
    """|got - X| / depth-scale per track (NaN rows stay NaN)."""
    return np.linalg.norm(np.asarray(got, np.float64) - X, axis=1) / DEPTH
