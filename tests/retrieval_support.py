"""What the retrieval tests share that is not specification (that is retrieval_reference.py): the synthetic places, random tables with ragged
counts and rows that are not finite, and the bit patterns that the comparisons look at."""
import numpy as np

F = np.float32


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[x.dtype.itemsize])


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def place_scene(seed, G=8, n_img=4, L=400, K=256, outliers=0.2, sigma=0.05):
    """G places of L random unit 64-vectors (landmarks).  An image of a place holds K (1 - outliers) of its landmarks (a random choice) as
    normalise(v + sigma noise) and K outliers random unit rows, shuffled, in fp32.
    -> desc (G n_img, K, 64) float32, place (G n_img,) the place of every image (image g n_img + i shows place g)."""
    rng = np.random.default_rng(seed)
    n_out = int(round(K * outliers))
    n_in = K - n_out
    marks = unit(rng.standard_normal((G, L, 64)))
    desc, place = np.zeros((G * n_img, K, 64), F), np.repeat(np.arange(G), n_img)
    for g in range(G):
        for i in range(n_img):
            seen = marks[g, rng.choice(L, n_in, replace=False)]
            rows = np.concatenate([unit(seen + sigma * rng.standard_normal(seen.shape)), unit(rng.standard_normal((n_out, 64)))])
            desc[g * n_img + i] = rows[rng.permutation(K)].astype(F)
    return desc, place


def place_mates(place):
    """For every image the set of the other images of its place."""
    return [set(np.nonzero((place == p) & (np.arange(len(place)) != i))[0].tolist()) for i, p in enumerate(place)]


def tables(rng, G, K, C, ragged=True, bad_rows=3):
    """Random unit descriptors (G,K,64), counts (G,) (ragged: 0, K and values between) and a random unit codebook; a few rows below the counts
    hold a NaN or an infinity."""
    desc = unit(rng.standard_normal((G, K, 64))).astype(F)
    counts = np.full(G, K, np.int32)
    if ragged:
        counts = rng.integers(0, K + 1, G).astype(np.int32)
        counts[0] = K
        if G > 1:
            counts[-1] = 0
    for _ in range(bad_rows):
        g = int(rng.integers(0, G))
        if counts[g] > 0:
            desc[g, int(rng.integers(0, counts[g])), int(rng.integers(0, 64))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
    return desc, counts, unit(rng.standard_normal((C, 64))).astype(F)


def global_vectors(rng, G, Q, N, D, duplicates=True):
    """Random unit queries (G,Q,D) and database rows (G,N,D); with duplicates some database rows repeat an earlier one bit for bit and one
    holds a NaN."""
    q, db = unit(rng.standard_normal((G, Q, D))).astype(F), unit(rng.standard_normal((G, N, D))).astype(F)
    if duplicates and N >= 4:
        for g in range(G):
            for _ in range(max(N // 8, 2)):
                a, b = rng.integers(0, N, 2)
                db[g, b] = db[g, a]
            db[g, int(rng.integers(0, N)), int(rng.integers(0, D))] = np.nan
    return q, db


def shortlists(rng, S, V, k):
    """Random shortlists (S,V,k) with -1, out-of-range and self entries among them, and n_views (S,) with one scene below V."""
    idx = rng.integers(-2, V + 2, (S, V, k)).astype(np.int32)
    n_views = np.full(S, V, np.int32)
    n_views[S - 1] = max(V - 3, 1)
    return idx, n_views


def pairs_by_sets(idx, n_views):
    """The pair list of one scene as a sorted list built from a set of frozensets."""
    V = idx.shape[0]
    nv = V if n_views is None else min(max(int(n_views), 0), V)
    edges = {frozenset((v, int(w))) for v in range(nv) for w in idx[v] if 0 <= w < nv and w != v}
    return sorted(tuple(sorted(e)) for e in edges)
