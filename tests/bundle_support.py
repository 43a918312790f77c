"""Scenes of the bundle adjustment tests (tests/test_bundle_*.py, tests/test_gpu_bundle.py) and of tools/bundle_time.py: what is not
specification (that is tests/bundle_reference.py).  A scene is multiview_support.arc_scene with the poses of the free views perturbed and the
tracks triangulated under the perturbed poses by multiview_reference.triangulate_views at max_reproj_error = 30 px, so that every view keeps
its observations (at a gate of 8 px a view perturbed by 0.2 degrees loses all of them and stays wrong): the per-view counts are asserted
here.  The generators consume their numpy generator in a fixed order, which is part of the tests' inputs."""
import numpy as np

import multiview_reference as MR
import multiview_support as MS
import twoview_support as TS

GATE = 30.0
KEEP = 0.9                                   # of a view's table entries that the triangulation must keep as inliers


def perturb(rng, Rs, ts, deg, tr, fixed):
    """Every view outside the mask `fixed`: R <- R rot(deg about a random axis), t <- t + tr along a random direction."""
    Rs, ts = Rs.copy(), ts.copy()
    for v in range(len(Rs)):
        w, d = rng.normal(size=3), rng.normal(size=3)
        if (fixed >> v) & 1:
            continue
        Rs[v] = Rs[v] @ TS.rotation(w / np.linalg.norm(w) * np.radians(deg))
        ts[v] = ts[v] + d / np.linalg.norm(d) * tr
    return Rs, ts


def triangulated(sc, Rs0, ts0, check=True):
    """Adds the start of an adjustment to a scene: Rs0, ts0 (the perturbed poses), inlier_views, points3d (the triangulation under them)."""
    V = sc["Rs"].shape[0]
    tri = MR.triangulate_views(sc["kpts"], sc["tracks"], sc["n_views"], sc["Ks"], Rs0, ts0, max_reproj_error=GATE)
    kept = [int(((tri["inlier_views"] >> v) & 1).sum()) for v in range(V)]
    t = sc["tracks"]
    nv = sc["n_views"]
    seen = [int(((t[:, v] >= 0) & (t[:, 0] >= 0) & ((t[:, :nv] >= 0).sum(axis=1) >= 2)).sum()) if v < nv else 0 for v in range(V)]
    if check:
        assert all(k >= KEEP * s for k, s in zip(kept, seen)), (kept, seen)
    sc.update(Rs0=Rs0, ts0=ts0, inlier_views=tri["inlier_views"], points3d=tri["points3d"], kept=kept, tri=tri)
    return sc


def scene(seed, V, K, noise=0.5, deg=0.2, tr=0.02, fixed=3, holes=0.0, cam=0, n_views=None):
    """An arc scene of K tracks in V views at `noise` pixels, the views outside `fixed` perturbed, triangulated; `holes`: the fraction of
    the table entries of the views v >= 1 that is removed first; n_views: the scene uses its first n_views views."""
    rng = np.random.default_rng(seed)
    sc = MS.arc_scene(rng, V, K, noise=noise, cam=cam)
    if holes:
        gone = rng.random(sc["tracks"].shape) < holes
        gone[:, 0] = False
        sc["tracks"][gone] = -1
    if n_views is not None:
        sc["n_views"] = n_views
    Rs0, ts0 = perturb(rng, sc["Rs"], sc["ts"], deg, tr, fixed)
    return triangulated(sc, Rs0, ts0)


def starve_view(sc, v, keep=5):
    """Leaves view v `keep` table entries (fewer than MIN_VIEW_OBS: it is held) and triangulates again."""
    rows = np.nonzero(sc["tracks"][:, v] >= 0)[0]
    sc["tracks"][rows[keep:], v] = -1
    return triangulated(sc, sc["Rs0"], sc["ts0"], check=False)


def axis_scene(seed, K, noise=0.5):
    """Three views with view 0 at (I, 0), view 1 at (I, (0, 0, -1)), noisy pixels and a perturbed view 2; track 0 lies on the common optical
    axis of views 0 and 1 and is observed by them alone: its point block is diag(a, b, 0), exactly singular under any damping."""
    rng = np.random.default_rng(seed)
    sc = MS.arc_scene(rng, 3, K, noise=0.0, cam=1, ref_identity=True)
    sc["Rs"][1], sc["ts"][1] = np.eye(3), np.array([0.0, 0.0, -1.0])
    X = sc["X"].copy()
    X[0] = [0.0, 0.0, MS.DEPTH]
    sc["tracks"][:, 1] = np.arange(K)                      # (every point is in front of view 1 and inside its image or near it)
    MS.reproject(sc, X)
    sc["kpts64"] += rng.normal(size=sc["kpts64"].shape) * noise
    for v in (0, 1):
        sc["kpts64"][v, sc["tracks"][0, v]] = [sc["Ks"][v][0, 2], sc["Ks"][v][1, 2]]      # the principal points: exact in float32? rounded alike
    sc["kpts"] = sc["kpts64"].astype(np.float32)
    sc["tracks"][0, 2] = -1
    Rs0, ts0 = perturb(rng, sc["Rs"], sc["ts"], 0.2, 0.02, 3)
    triangulated(sc, Rs0, ts0, check=False)
    sc["inlier_views"] = sc["inlier_views"].copy()
    sc["points3d"] = sc["points3d"].copy()
    sc["inlier_views"][0] = 3                              # (a zero-parallax track: the triangulation refuses it; the adjustment is handed it)
    sc["points3d"][0] = [0.0, 0.0, MS.DEPTH]
    return sc


def far_view_scene(seed, V, K, noise=0.5):
    """A scene whose last view stands 1e200 units away along its own axis (and sees every track there): its Jacobians underflow, the
    diagonal block of the reduced system is exactly zero and the first pivot of its rows fails in every round."""
    sc = scene(seed, V, K, noise=noise, fixed=3)
    v = V - 1
    t = np.array([1e199, 1e199, 1e200])
    sc["Rs"][v], sc["ts"][v] = np.eye(3), t
    Xc = sc["X"] + t
    p = np.c_[sc["Ks"][v][0, 0] * Xc[:, 0] / Xc[:, 2] + sc["Ks"][v][0, 2], sc["Ks"][v][1, 1] * Xc[:, 1] / Xc[:, 2] + sc["Ks"][v][1, 2]]
    sc["tracks"][:, v] = np.arange(K)
    sc["kpts64"][v, :K] = p
    sc["kpts"] = sc["kpts64"].astype(np.float32)
    Rs0, ts0 = sc["Rs0"].copy(), sc["ts0"].copy()
    Rs0[v], ts0[v] = sc["Rs"][v], sc["ts"][v]
    return triangulated(sc, Rs0, ts0, check=False)


def pose_errors(sc, Rs, ts):
    """(worst rotation error in degrees, worst camera-centre error) of poses against the scene's."""
    rot = max(np.degrees(np.arccos(np.clip((np.trace(Rs[v] @ sc["Rs"][v].T) - 1.0) / 2.0, -1.0, 1.0))) for v in range(len(Rs)))
    cen = max(np.linalg.norm(-Rs[v].T @ ts[v] + sc["Rs"][v].T @ sc["ts"][v]) for v in range(len(Rs)))
    return float(rot), float(cen)


def point_error(sc, X, rows):
    """Median |X - truth| / depth over the tracks `rows`."""
    return float(np.median(np.linalg.norm(np.asarray(X, np.float64)[rows] - sc["X"][rows], axis=1)) / MS.DEPTH)


def run_reference(sc, **kw):
    import bundle_reference as BR
    return BR.bundle_adjust(sc["kpts"], sc["tracks"], sc["inlier_views"], sc["points3d"], sc["n_views"], sc["Ks"], sc["Rs0"], sc["ts0"], **kw)
