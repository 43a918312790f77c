"""What the baseline-scale tests share that is not specification (that is tests/posescale_reference.py): the scenes, the true ratios,
an edge with wrong tracks.  The generators consume their numpy generator in a fixed order, which is part of the tests' inputs."""
import math

import numpy as np

import multiview_support as MS
import posegraph_support as PS
import posescale_reference as QR
import twoview_support as TS

SETTINGS = dict(PS.DEFAULTS, min_pivot_ratio=6.5e-9)        # multiview.MIN_PIVOT_RATIO
SCALE = dict(scale_weight=1.0, scale_tol=0.1)


def tables(tracks, V, K):
    """(tracks (T,V), track_of (V,K)) of a ground-truth table (K,V): track k is row k."""
    tracks = np.asarray(tracks, np.int32)
    track_of = np.full((V, K), -1, np.int32)
    for v in range(V):
        k = np.nonzero(tracks[:, v] >= 0)[0]
        track_of[v, tracks[k, v]] = k
    return tracks.copy(), track_of


STEP_DEG = 10.0                              # of arc per view: 0.5 degrees of pose noise against 3 degrees of parallax leave no depth to compare


def scene(seed, V, K, pairs, noise=0.5, sigma_deg=0.5, wrong=0.05, step_deg=STEP_DEG):
    """MS.arc_scene (view 0 at (I, 0): the gauge of the pose graph) with `noise` pixels, a share `wrong` of the tracks with one observation
    moved by 50 .. 150 pixels, its ground-truth track tables, and the relative poses of `pairs` from the truth, R_rel and the direction
    rotated by N(0, sigma_deg) per axis (PS.scene's noise).  The arc advances by step_deg per view (MS's own 3 degrees suit its
    triangulation tests; here the depths of two noisy relative poses are compared).  Weights: integers in [50, 500)."""
    rng = np.random.default_rng(seed)
    keep = MS.STEP_DEG, MS.ARC_DEG
    MS.STEP_DEG, MS.ARC_DEG = step_deg, step_deg * max(V - 1, 1)           # (arc_scene reads them when called)
    try:
        sc = MS.arc_scene(rng, V, K, noise=noise, ref_identity=True)
    finally:
        MS.STEP_DEG, MS.ARC_DEG = keep
    if wrong > 0.0:
        MS.plant_outliers(rng, sc, frac=wrong)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    Rs, ts = sc["Rs"], sc["ts"]
    cs = -np.einsum("vji,vj->vi", Rs, ts)
    Rrel, trel = np.zeros((P, 3, 3)), np.zeros((P, 3))
    sig = math.radians(sigma_deg)
    for p, (a, b) in enumerate(pairs):
        R = Rs[b] @ Rs[a].T
        t = Rs[b] @ (cs[a] - cs[b])
        t = t / np.linalg.norm(t)
        nr, nt = rng.normal(size=3), rng.normal(size=3)
        if sig > 0.0:
            R, t = TS.rotation(nr * sig) @ R, TS.rotation(nt * sig) @ t
        Rrel[p], trel[p] = R, t
    weight = rng.integers(50, 500, P).astype(np.float64)
    sc["tracks"], sc["track_of"] = tables(sc["tracks"], V, K)
    sc.update(V=V, K=K, pairs=pairs, Rrel=Rrel, trel=trel, weight=weight, cs=cs)
    return sc


def ratios(sc, **kw):
    return QR.baseline_ratios(sc["kpts"], sc["tracks"], sc["track_of"], sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc["Ks"],
                              sc.get("n_views", sc["V"]), sc["V"], **kw)


def run(sc, r=None, **kw):
    s = dict(SETTINGS)
    s.update(SCALE)
    s.update(kw)
    return QR.average_poses(sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc.get("n_views", sc["V"]), sc["V"],
                            ratio=None if r is None else r["ratio"], ratio_count=None if r is None else r["count"], **s)


def true_ratio(sc, p, q):
    c, pr = sc["cs"], sc["pairs"]
    return float(np.linalg.norm(c[pr[p, 0]] - c[pr[p, 1]]) / np.linalg.norm(c[pr[q, 0]] - c[pr[q, 1]]))


def ratio_error(sc, r):
    """The largest relative error of a ratio against the true baseline ratio, and how many ratios there are."""
    at = np.argwhere(np.isfinite(r["ratio"]))
    err = [abs(r["ratio"][p, q] / true_ratio(sc, p, q) - 1.0) for p, q in at]
    return (max(err) if err else 0.0), len(err)


def corrupted_ratios(sc, p, factor=2.0, **gates):
    """The ratios of the scene with the matches of edge p = (a, b) alone corrupted: for its wedges every track's key-point in b is where a
    point at `factor` times its depth along the ray of a would be seen (a consistent, wrong structure: no gate catches it), every other
    wedge sees the scene as it is.  Returns (the result, the wedges of p as a (P,P) mask)."""
    clean = ratios(sc, **gates)
    a, b = (int(v) for v in sc["pairs"][p])
    bad = dict(sc)
    ca = sc["cs"][a]
    X = ca + factor * (sc["X"] - ca)
    Xc = X @ sc["Rs"][b].T + sc["ts"][b]
    px = np.c_[sc["Ks"][b][0, 0] * Xc[:, 0] / Xc[:, 2] + sc["Ks"][b][0, 2], sc["Ks"][b][1, 1] * Xc[:, 1] / Xc[:, 2] + sc["Ks"][b][1, 2]]
    kp = sc["kpts"].copy()
    k = np.nonzero(sc["tracks"][:, b] >= 0)[0]
    kp[b, sc["tracks"][k, b]] = px[k].astype(np.float32)
    bad["kpts"] = kp
    wrong = ratios(bad, **gates)
    P = sc["pairs"].shape[0]
    mine = np.zeros((P, P), bool)
    mine[p, :] = mine[:, p] = True
    mine &= clean["shared_view"] >= 0
    out = {key: np.where(mine, wrong[key], clean[key]) for key in ("ratio", "count", "shared_view")}
    return out, mine


def similarity_errors(sc, Rs, ts, views):
    """(largest rotation error in degrees, largest centre error relative to the rms distance of the true centres from their mean) over
    `views` after the least-squares similarity that maps the estimated centres on the true ones."""
    c = np.stack([-Rs[v].T @ ts[v] for v in views])
    ct = sc["cs"][views]
    mc, mt = c.mean(0), ct.mean(0)
    U, S, Vt = np.linalg.svd((ct - mt).T @ (c - mc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    s = (S * np.diag(D)).sum() / ((c - mc) ** 2).sum()
    fit = s * (c - mc) @ Q.T + mt
    cen = float(np.max(np.linalg.norm(fit - ct, axis=1)) / math.sqrt(((ct - mt) ** 2).sum(axis=1).mean()))
    rot = max(PS.angle_deg(Rs[v] @ Q.T, sc["Rs"][v]) for v in views)
    return rot, cen
