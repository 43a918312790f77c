"""Synthetic inputs of the match refinement tests.  Every generator consumes its numpy Generator in a fixed order, so a seed names one scene on every machine."""
import numpy as np

GRID = 1600                       # key-points lie on the pixel grid [0, GRID]^2
SCALES = (1.0 / 0.6, 1.0 / 1.3)   # what the dual-scale extraction hands out (detectAndComputeDense: s1 = 0.6, s2 = 1.3)


def descriptors(rng, P, N, norm=1.0):
    """(P, N, 64) float32 of the given norm (unit norm: what the extraction hands out)."""
    d = rng.standard_normal((P, N, 64))
    d *= norm / np.linalg.norm(d, axis=-1, keepdims=True)
    return d.astype(np.float32)


def keypoints(rng, P, N):
    """(P, N, 2) float32 (x, y): N DISTINCT grid points per pair, so that a row names the key-point it came from."""
    out = np.empty((P, N, 2), np.float32)
    for p in range(P):
        cell = rng.choice((GRID + 1) * (GRID + 1), size=N, replace=False)
        out[p, :, 0], out[p, :, 1] = cell % (GRID + 1), cell // (GRID + 1)
    return out


def scales(rng, P, N):
    return np.asarray(SCALES, np.float32)[rng.integers(0, 2, size=(P, N))]


def index_lists(rng, P, N, table=None):
    """(P, N) int64 below `table` (N when None): per pair a random permutation of the table, cut to N entries -- or, for a table shorter than N, followed by uniform draws."""
    table = N if table is None else table
    out = np.empty((P, N), np.int64)
    for p in range(P):
        perm = rng.permutation(table)[:N]
        out[p] = np.concatenate([perm, rng.integers(0, table, size=N - len(perm))])
    return out


def repeated_index_lists(rng, P, N, table=None):
    """(P, N) int64 below `table`: uniform draws, so indices repeat and others are missing."""
    return rng.integers(0, N if table is None else table, size=(P, N)).astype(np.int64)


def scene(seed, P, N, N1=None, table_draw=index_lists, norm=1.0):
    """One (P, N) batch: dict of desc0, desc1, kp0, kp1, scale0, idx0, idx1.  N1: rows of the second set when it is smaller than N; norm: of every descriptor."""
    rng = np.random.default_rng(seed)
    N1 = N if N1 is None else N1
    s = {"desc0": descriptors(rng, P, N, norm), "desc1": descriptors(rng, P, N1, norm), "kp0": keypoints(rng, P, N), "kp1": keypoints(rng, P, N1), "scale0": scales(rng, P, N)}
    s["idx0"] = table_draw(rng, P, N)
    s["idx1"] = table_draw(rng, P, N, N1)
    return s


def pick_fine_conf(conf, lo=0.2, hi=0.3):
    """-> (fine_conf, gap): the midpoint of the widest gap between neighbouring confidences inside [lo, hi] (the two ends count as neighbours, so a case without any
    confidence in the interval still has its gap) and the gap's width.  Every confidence is then at least gap / 2 away from fine_conf."""
    c = np.asarray(conf, np.float64).ravel()
    c = np.sort(np.concatenate([[lo], c[(c > lo) & (c < hi)], [hi]]))
    g = np.diff(c)
    i = int(np.argmax(g))
    return float(0.5 * (c[i] + c[i + 1])), float(g[i])
