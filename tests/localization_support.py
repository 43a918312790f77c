"""Scenes of the localisation tests (tests/test_localization_*.py, tests/test_gpu_localization.py) and of tools/localize_time.py: what is not
specification (that is tests/localization_reference.py).  The generators consume their numpy generator in a fixed order, which is part of the
tests' inputs."""
import numpy as np

import localization_reference as LR
import multiview_support as MS
import twoview_support as TS


def unit_rows(rng, n):
    """n random unit 64-vectors, float64."""
    d = rng.normal(size=(n, 64))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def observe(rng, base, sigma):
    """normalise(base + sigma * noise), rounded to fp32."""
    d = base + sigma * rng.normal(size=base.shape)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def descriptor_scene(rng, V, K, noise=0.5, sigma=0.05, **kw):
    """multiview_support.arc_scene with descriptors: every 3D point a random unit 64-vector ('base' (K,64) float64), every observation
    normalise(vector + sigma * noise) in fp32 at its key-point's row ('desc' (V,kcap,64) float32); rows that belong to no point hold vectors of
    their own."""
    sc = MS.arc_scene(rng, V, K, noise=noise, **kw)
    kcap = sc["kpts"].shape[1]
    base = unit_rows(rng, K)
    desc = np.zeros((V, kcap, 64), np.float32)
    for v in range(V):
        desc[v] = unit_rows(rng, kcap).astype(np.float32)
        seen = np.nonzero(sc["tracks"][:, v] >= 0)[0]
        desc[v, sc["tracks"][seen, v]] = observe(rng, base[seen], sigma)
    sc["base"], sc["desc"] = base, desc
    return sc


def map_inputs(rng, V, T, kcap, view31=False):
    """Random inputs of xfh_build_map for one scene with holes and every skip reason (for T >= 64): rows -1 and >= Kcap, masks with bits of
    views that observe nothing, non-finite descriptor rows, non-finite points, every status, and tracks whose two observations are antipodal
    (row 0 of view 1 is minus row 0 of view 0).  view31: a third of the masks have bit 31 (the sign bit) set.  Returns desc (V,kcap,64) fp32,
    tracks (T,V) int32, points3d (T,3) fp32, status (T,) uint8, inlier_views (T,) int32."""
    desc = unit_rows(rng, V * kcap).reshape(V, kcap, 64).astype(np.float32)
    if V >= 2:
        desc[1, 0] = -desc[0, 0]
    if kcap >= 8:                                          # a few rows with one component that is not finite
        for v in range(V):
            r = rng.integers(1, kcap, 2)
            desc[v, r[0], rng.integers(0, 64)] = np.nan
            desc[v, r[1], rng.integers(0, 64)] = np.inf if v % 2 else -np.inf
    tracks = rng.integers(-1, kcap + 1, (T, V)).astype(np.int32)          # -1 and Kcap included
    far = rng.random((T, V)) < 0.02
    tracks[far] = np.where(rng.random(int(far.sum())) < 0.5, -7, kcap + 1000)
    points = rng.normal(size=(T, 3)).astype(np.float32) * 5
    status = np.where(rng.random(T) < 0.2, rng.integers(1, 7, T), 0).astype(np.uint8)
    bits = rng.random((T, V)) < (0.6 if V > 3 else 0.85)
    if view31 and V == 32:
        bits[::3, 31] = True
    mask = (bits.astype(np.uint64) << np.arange(V, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    for k in range(T):
        kind = k % 16
        if kind == 3:
            points[k, k % 3] = [np.nan, np.inf, -np.inf][(k // 16) % 3]
        elif kind == 5 and V >= 2:                          # two antipodal observations, nothing else
            tracks[k, :2], mask[k], status[k], points[k] = 0, 3, 0, 1.0
        elif kind == 7:                                    # no contributing view at all
            mask[k], status[k] = 0, 0
        elif kind == 9:                                    # a status and a bad point: the status counts
            status[k], points[k, 0] = 1 + (k // 16) % 6, np.nan
        elif kind == 11 and V >= 2:                        # antipodal and a bad point: the point counts
            tracks[k, :2], mask[k], status[k], points[k, 2] = 0, 3, 0, np.inf
    return desc, tracks, points, status, mask.view(np.int32)


def truth_pose_errors(R, t, R_true, t_true):
    """(rotation error in degrees, distance of the camera centres) of a pose against the truth."""
    R, t, R_true, t_true = (np.asarray(v, np.float64) for v in (R, t, R_true, t_true))
    c = np.clip((np.trace(R @ R_true.T) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(-R.T @ t + R_true.T @ t_true))


def project_case(rng, Q, M):
    """Inputs of xfh_map_project: points in front of, behind and on the plane of the camera, rows that are not finite, the all-zero pose of
    "nothing found" for query 1, ragged counts."""
    pts = (rng.normal(size=(Q, M, 3)) * 3 + [0, 0, 4]).astype(np.float32)          # a good part behind the camera or close to its plane
    pts[:, ::7, 2] = 0.0
    if M > 4:
        pts[:, 3] = [np.nan, 1.0, 5.0]
        pts[:, 4] = [1.0, np.inf, 5.0]
    R = np.stack([TS.rotation(rng.normal(size=3) * 0.2) for _ in range(Q)])
    t = rng.normal(size=(Q, 3)) * 0.3
    K = np.tile(np.array([[600.0, 0.0, 320.0], [0.0, 610.0, 240.0], [0.0, 0.0, 1.0]]), (Q, 1, 1))
    if Q > 1:
        R[1], t[1] = 0.0, 0.0                               # the pose of "nothing found"
    n = rng.integers(0, M + 1, Q).astype(np.int32)
    n[0] = M
    return pts, n, R, t, K


# ---- comparisons shared by the emulated and the GPU tests --------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def check_build(got, s, want):
    """Scene s of a batch result (numpy arrays) against the restatement's: integers exactly, floats as bits (NaN points: any NaN)."""
    n = int(want["n_points"])
    assert int(got["n_points"][s]) == n and list(got["info"][s]) == list(want["info"]), (list(got["info"][s]), list(want["info"]))
    for k in ("track", "n_obs"):
        assert np.array_equal(got[k][s], want[k]), k
    for k in ("desc", "desc_f16", "coherence"):
        assert np.array_equal(bits(got[k][s]), bits(want[k])), (k, np.nonzero(bits(got[k][s]) != bits(want[k])))
    assert np.array_equal(bits(got["points"][s, :n]), bits(want["points"][:n])) and np.isnan(got["points"][s, n:]).all()


def check_project(got, pts, n, R, t, K, size):
    hit = 0
    for q in range(pts.shape[0]):
        want = LR.project(pts[q], None if n is None else n[q], R[q], t[q], K[q], None if size[0] == 0 else size[:2], size[2])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[q]), nan) and np.array_equal(bits(got[q])[~nan], bits(want)[~nan]), q
        hit += int((~nan).sum())
    return hit
