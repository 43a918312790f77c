"""Inputs of the track-graph tests (tests/test_tracks_*.py, tests/test_gpu_tracks.py) and of tools/tracks_time.py: what is not
specification (that is tests/tracks_reference.py).  The generators consume their numpy generator in a fixed order, which is part of the
tests' inputs."""
import numpy as np

import multiview_support as MS


def chain_pairs(V):
    return [(v, v + 1) for v in range(V - 1)]


def all_pairs(V):
    return [(a, b) for a in range(V) for b in range(a + 1, V)]


def pair_lists(rng, tracks, pairs, cap=None, kcap=None):
    """The matcher's lists of the given pairs of views that a table `tracks` (K,V) gives: view_pairs (P,2) int32, idx_a, idx_b (P,cap) int64
    in a random order, n_matches (P,) int32.  Entries of the table outside [0, kcap) match nothing."""
    tracks = np.asarray(tracks)
    kcap = (int(tracks.max()) + 1 if tracks.size else 0) if kcap is None else kcap
    seen = (tracks >= 0) & (tracks < kcap)
    cap = max(tracks.shape[0], 1) if cap is None else cap
    P = len(pairs)
    idx_a, idx_b, n = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64), np.zeros(P, np.int32)
    for p, (a, b) in enumerate(pairs):
        k = np.nonzero(seen[:, a] & seen[:, b])[0]
        k = k[rng.permutation(len(k))][:cap]
        n[p] = len(k)
        idx_a[p, :len(k)], idx_b[p, :len(k)] = tracks[k, a], tracks[k, b]
    return np.array(pairs, np.int32).reshape(P, 2), idx_a, idx_b, n


def noisy_lists(rng, V, K, pairs, wrong=0.03):
    """A scene's own matches over the given pairs (MS.arc_scene at V views and max(K, 1) tracks, tables of K rows) with a fraction of wrong
    matches (merged tracks: inconsistent components; rows -2 .. K + 1: indices out of range), a repeated pair, a pair with a view out of
    range and a pair (1, 1)."""
    sc = MS.arc_scene(rng, V, max(K, 1))
    vp, ia, ib, n = pair_lists(rng, sc["tracks"], pairs, cap=K + 3, kcap=K)
    bad = rng.random(ia.shape) < wrong
    ib[bad] = rng.integers(-2, K + 2, bad.sum())
    return (np.r_[vp, vp[:1], [[V, 0]], [[1, 1]]].astype(np.int32), np.r_[ia, ia[:1], ia[:1], ia[:1]], np.r_[ib, ib[:1], ib[:1], ib[:1]],
            np.r_[n, n[:1], n[:1], n[:1]])


def runs(tracks, min_length=2):
    """What the chain of pairs (v, v + 1) makes of a table: one row per maximal run of consecutive observing views of a track of at least
    min_length views, in ascending (first view, its row).  Returns (table (n,V) int32, the source row of each)."""
    tracks = np.asarray(tracks)
    rows, src = [], []
    for k in range(tracks.shape[0]):
        v = 0
        while v < tracks.shape[1]:
            if tracks[k, v] < 0:
                v += 1
                continue
            e = v
            while e + 1 < tracks.shape[1] and tracks[k, e + 1] >= 0:
                e += 1
            if e - v + 1 >= min_length:
                r = np.full(tracks.shape[1], -1, np.int32)
                r[v:e + 1] = tracks[k, v:e + 1]
                rows.append(r); src.append(k)
            v = e + 1
    order = sorted(range(len(rows)), key=lambda i: next((v, int(r)) for v, r in enumerate(rows[i]) if r >= 0))
    table = np.stack([rows[i] for i in order]) if rows else np.zeros((0, tracks.shape[1]), np.int32)
    return table, np.array([src[i] for i in order], np.int64)


def zigzag(K):
    """(0, r) - (1, r), (1, r) - (0, r + 1) for all r: one component of 2 K nodes with K key-points of either view, whose parent chain is the
    deepest that two views can produce.  view_pairs (2,2), idx_a, idx_b (2,K), n_matches (2,)."""
    r = np.arange(K, dtype=np.int64)
    idx_a, idx_b = np.stack([r, r]), np.stack([r, r + 1])
    return np.array([[0, 1], [1, 0]], np.int32), idx_a, idx_b, np.array([K, max(K - 1, 0)], np.int32)


def chain_scene(seed, K=400, V=6, noise=0.5, removed_frac=0.3):
    """MS.arc_scene at V views and `noise` pixels; a fraction of the tracks loses its observations in the views 0 and 1; the matches are
    those of the pairs (v, v + 1) alone.  Returns the scene with `removed` (K,) bool and `lists` = (view_pairs, idx_a, idx_b, n_matches)."""
    rng = np.random.default_rng(seed)
    sc = MS.arc_scene(rng, V, K, noise=noise)
    removed = rng.random(K) < removed_frac
    sc["tracks"][removed, :2] = -1
    sc["removed"] = removed
    sc["lists"] = pair_lists(rng, sc["tracks"], chain_pairs(V), kcap=K)
    return sc
