"""What the pose-graph tests share that is not specification (that is tests/posegraph_reference.py): the synthetic scenes, the pair graphs,
the error measures.  The generators consume their numpy generator in a fixed order, which is part of the tests' inputs."""
import math

import numpy as np

import posegraph_reference as PR
import twoview_support as TS

DEFAULTS = dict(iterations=30, redescend=10, rot_scale_rad=math.radians(2.0), pos_scale_sin=math.sin(math.radians(2.0)))


def all_pairs(V):
    return np.array([(a, b) for a in range(V) for b in range(a + 1, V)], np.int32)


def near_pairs(V, dist=3):
    return np.array([(a, b) for a in range(V) for b in range(a + 1, min(V, a + dist + 1))], np.int32)


def chain_pairs(V):
    return np.array([(a, a + 1) for a in range(V - 1)], np.int32)


TWO_TRIANGLES = np.array([(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (2, 4)], np.int32)       # V = 5, the triangles share view 2


def scene(seed, V, pairs, sigma_deg=0.0, outliers=0.0):
    """Random views (rotations of about 0.5 rad, centres of about 2 units; view 0 = (I, 0): the gauge) and the relative poses of `pairs`:
    R_rel = R_b R_a', t_rel = the unit vector along R_b (c_a - c_b); noise rotates R_rel and t_rel by N(0, sigma) per axis; an outlier edge
    (round(outliers P) of them, chosen at random) gets a random rotation of about 1 rad and a random direction.  Weights: integers in [50, 500)."""
    rng = np.random.default_rng(seed)
    Rs = np.stack([np.eye(3)] + [TS.rotation(rng.normal(size=3) * 0.3) for _ in range(V - 1)])
    cs = np.concatenate([np.zeros((1, 3)), rng.normal(size=(V - 1, 3)) * 1.2])
    pairs = np.asarray(pairs, np.int32)
    P = pairs.shape[0]
    Rrel, trel = np.zeros((P, 3, 3)), np.zeros((P, 3))
    out = np.zeros(P, bool)
    out[rng.permutation(P)[:int(round(outliers * P))]] = True
    sig = math.radians(sigma_deg)
    for p, (a, b) in enumerate(pairs):
        R = Rs[b] @ Rs[a].T
        t = Rs[b] @ (cs[a] - cs[b])
        t = t / np.linalg.norm(t)
        nr, nt = rng.normal(size=3), rng.normal(size=3)
        wr, wt = rng.normal(size=3), rng.normal(size=3)
        if sig > 0.0:
            R, t = TS.rotation(nr * sig) @ R, TS.rotation(nt * sig) @ t
        if out[p]:
            R, t = TS.rotation(wr * 0.6), wt / np.linalg.norm(wt)
        Rrel[p], trel[p] = R, t
    weight = rng.integers(50, 500, P).astype(np.float64)
    ts = -np.einsum("vij,vj->vi", Rs, cs)
    return dict(V=V, pairs=pairs, Rrel=Rrel, trel=trel, weight=weight, Rs=Rs, cs=cs, ts=ts, outlier=out)


def run(sc, **kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return PR.average_poses(sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc.get("n_views", sc["V"]), sc["V"], **s)


def swap_edges(sc, which):
    """The scene with the edges `which` given as (b, a) and the pose inverted: R' and -R' t."""
    o = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    for p in which:
        o["pairs"][p] = sc["pairs"][p][::-1]
        o["Rrel"][p] = sc["Rrel"][p].T
        o["trel"][p] = -sc["Rrel"][p].T @ sc["trel"][p]
    return o


def repeat_edges(sc, P):
    """The scene with its edge list repeated up to P edges (duplicates are edges of their own)."""
    o = dict(sc)
    sel = np.arange(P) % sc["pairs"].shape[0]
    for k in ("pairs", "Rrel", "trel", "weight", "outlier"):
        o[k] = sc[k][sel].copy()
    return o


def angle_deg(Ra, Rb):
    """The angle between two rotations from the chord |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2) (exact near 0, where the trace is not)."""
    return math.degrees(2.0 * math.asin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * math.sqrt(2.0)))))


def errors(sc, Rs, ts, registered=None):
    """(the largest rotation error in degrees, the largest centre error after one least-squares scale, relative to the rms of the true
    centres' norms) over the registered views but 0 (both gauges hold view 0 at (I, 0))."""
    V = sc["V"]
    vs = [v for v in range(1, V) if registered is None or (registered >> v) & 1]
    rot = max(angle_deg(Rs[v], sc["Rs"][v]) for v in vs)
    c = np.stack([-Rs[v].T @ ts[v] for v in vs])
    ct = sc["cs"][vs]
    s = (c * ct).sum() / (c * c).sum()
    return rot, float(np.max(np.linalg.norm(s * c - ct, axis=1)) / math.sqrt((ct * ct).sum(axis=1).mean()))


def batch(scenes, V=None, P=None):
    """Scenes padded to one (S, P, ...) batch: padding edges have weight 0 (not valid)."""
    V = max(sc["V"] for sc in scenes) if V is None else V
    P = max(sc["pairs"].shape[0] for sc in scenes) if P is None else P
    S = len(scenes)
    pairs, Rrel, trel, weight = np.zeros((S, P, 2), np.int32), np.zeros((S, P, 3, 3)), np.zeros((S, P, 3)), np.zeros((S, P))
    nv = np.zeros(S, np.int32)
    for i, sc in enumerate(scenes):
        m = sc["pairs"].shape[0]
        pairs[i, :m], Rrel[i, :m], trel[i, :m], weight[i, :m] = sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"]
        nv[i] = sc.get("n_views", sc["V"])
    return pairs, Rrel, trel, weight, nv, V
