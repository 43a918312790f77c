"""numpy restatement of the tracks over a graph of view pairs (csrc/k_tracks.hip) and of the anchored triangulation (mv_track<true> of
csrc/k_triangulate.hip), DESIGN.md 3.18.

``build_tracks_graph`` is a sequential union-find with minimum labels: the label of a component is its smallest node id v K + row, the
view mask and the inconsistency flag live at the root, the track ids are the ranks of the surviving roots in ascending node id.  Nothing in
it depends on the order of the matches, so it is comparable with the device's tables exactly.

``triangulate_views(..., anchor='first')`` is built on multiview_reference's functions: the tracks whose lowest observing view is a are
handed to ``multiview_reference.triangulate_views`` with the views a .. n_views - 1 (view a becomes its view 0; the views below a do not
observe these tracks and would add an exact + 0.0 to every sum), so the results are comparable bit for bit like that restatement's.

TEST INFRASTRUCTURE ONLY: nothing under ``accelerated_features_amd/`` imports it.
"""
import math

import numpy as np

import multiview_reference as MR
from oracle.twoview_reference import finite

INFO_FIELDS = ("nodes", "components", "tracks", "inconsistent", "short", "over_capacity", "status", "spare")
_ERR = dict(all="ignore")


def edges(view_pairs, idx_a, idx_b, n_matches, V, K):
    """The node pairs (u, v) (two int64 arrays) of the matches that count: pair p = (a, b) with a != b, both in [0, V), its first
    min(n_matches[p], cap) matches, both rows in [0, K); node (view, row) = view K + row."""
    view_pairs, idx_a, idx_b = np.asarray(view_pairs, np.int64).reshape(-1, 2), np.asarray(idx_a, np.int64), np.asarray(idx_b, np.int64)
    P, cap = idx_a.shape
    us, vs = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for p in range(P):
        a, b = int(view_pairs[p, 0]), int(view_pairs[p, 1])
        if a == b or not (0 <= a < V and 0 <= b < V):
            continue
        n = min(max(int(n_matches[p]), 0), cap)
        ia, ib = idx_a[p, :n], idx_b[p, :n]
        ok = (ia >= 0) & (ia < K) & (ib >= 0) & (ib < K)
        us.append(a * K + ia[ok]); vs.append(b * K + ib[ok])
    return np.concatenate(us), np.concatenate(vs)


def components(u, v, N):
    """Union-find over the edges in their order, the larger root hooked under the smaller: label (N,) int64 = the smallest node id of a
    matched node's component, -1 for a node without a match."""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.full(N, -1, np.int64)
    for x in np.unique(np.concatenate([u, v])).tolist():
        label[x] = find(x)
    return label


def build_tracks_graph(view_pairs, idx_a, idx_b, n_matches, V, K, min_length=2, max_tracks=None):
    """One scene: view_pairs (P,2), idx_a, idx_b (P,cap) integers, n_matches (P,).  Returns a dict: tracks (T,V) int32, track_of (V,K) int32,
    n_tracks, info (8,) int32 (INFO_FIELDS), label (N,) (the root of a matched node, -1 otherwise), mask (N,) uint32 and bad (N,) bool (at
    the roots)."""
    N = V * K
    T = N // 2 if max_tracks is None else int(max_tracks)
    u, v = edges(view_pairs, idx_a, idx_b, n_matches, V, K)
    label = components(u, v, N)
    nodes = np.nonzero(label >= 0)[0]
    mask, bad = np.zeros(N, np.uint32), np.zeros(N, bool)
    count = np.zeros((N, V), np.int64)
    np.add.at(count, (label[nodes], nodes // max(K, 1)), 1)
    roots = nodes[label[nodes] == nodes]
    for b in range(V):
        mask[roots] |= ((count[roots, b] > 0).astype(np.uint32) << np.uint32(b))
    bad[roots] = (count[roots] > 1).any(axis=1)
    length = (count[roots] > 0).sum(axis=1)
    keep = ~bad[roots] & (length >= min_length)
    rank = np.full(N, -1, np.int64)
    ids = np.cumsum(keep) - keep                           # the exclusive scan in ascending node id
    rank[roots] = np.where(keep & (ids < T), ids, -1)
    total = int(keep.sum())
    kept = min(total, T)
    tracks, track_of = np.full((T, V), -1, np.int32), np.full(N, -1, np.int32)
    t = rank[label[nodes]]
    track_of[nodes] = t
    on = t >= 0
    tracks[t[on], nodes[on] // max(K, 1)] = nodes[on] % max(K, 1)
    info = np.array([len(nodes), len(roots), kept, int(bad[roots].sum()), int((~bad[roots] & (length < min_length)).sum()), total - kept, 0, 0], np.int32)
    return dict(tracks=tracks, track_of=track_of.reshape(V, K), n_tracks=kept, info=info, label=label, mask=mask, bad=bad)


def observed(kpts, tracks, n_views, Rs, ts, Ks, pixels64=False):
    """The observed sets of mv_track<false> / mv_track<true>: (nv, K) bool, view w observes track k (an entry in range, a finite pixel, a usable pose)."""
    kpts = np.asarray(kpts, np.float64 if pixels64 else np.float32).astype(np.float64)
    tracks = np.asarray(tracks, np.int64)
    V, kcap = kpts.shape[0], kpts.shape[1]
    nv = min(max(int(n_views), 0), V)
    O = np.zeros((nv, tracks.shape[0]), bool)
    with np.errstate(**_ERR):
        for w in range(nv):
            r = tracks[:, w]
            inr = (r >= 0) & (r < kcap)
            q = kpts[w][np.where(inr, r, 0)] if kcap else np.zeros((tracks.shape[0], 2))
            ok = MR.stage_view(Rs[w], ts[w], Ks[w], Rs[w], ts[w])["ok"]
            O[w] = inr & finite(q[:, 0]) & finite(q[:, 1]) & ok
    return O


def triangulate_views(kpts, tracks, n_views, Ks, Rs, ts, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=math.inf, min_views=2,
                      pixels64=False, anchor="first"):
    """One scene, the arguments of multiview_reference.triangulate_views.  anchor='reference' is that function; anchor='first' restates
    mv_track<true>.  Returns a dict: points3d (K,3) float32, status, n_inliers (K,) uint8, inlier_views (K,) int32, reproj_error (K,)
    float32, valid, info (8,), winner (K,) (the view of the winning hypothesis, -1: none), score, cost0, cost1 (K,) float64, anchor (K,)
    (-1: nothing observes the track) and groups: [(anchor, the track indices, multiview_reference's result for them)]."""
    gates = dict(max_reproj_error=max_reproj_error, min_parallax_deg=min_parallax_deg, max_depth=max_depth, min_views=min_views, pixels64=pixels64)
    if anchor == "reference":
        return MR.triangulate_views(kpts, tracks, n_views, Ks, Rs, ts, **gates)
    assert anchor == "first", anchor
    kpts, tracks = np.asarray(kpts), np.asarray(tracks, np.int64)
    Ks, Rs, ts = np.asarray(Ks, np.float64), np.asarray(Rs, np.float64), np.asarray(ts, np.float64)
    K, V = tracks.shape[0], kpts.shape[0]
    nv = min(max(int(n_views), 0), V)
    O = observed(kpts, tracks, nv, Rs, ts, Ks, pixels64)
    nobs = O.sum(axis=0) if nv else np.zeros(K, int)
    first = np.where(nobs > 0, np.argmax(O, axis=0), -1) if nv else np.full(K, -1)
    out = dict(points3d=np.full((K, 3), np.nan, np.float32), status=np.full(K, MR.UNOBSERVED, np.uint8), n_inliers=np.zeros(K, np.uint8),
               inlier_views=np.zeros(K, np.int32), reproj_error=np.full(K, np.nan, np.float32), winner=np.full(K, -1), score=np.zeros(K),
               cost0=np.zeros(K), cost1=np.zeros(K), anchor=first, groups=[])
    for a in range(max(nv - 1, 0)):
        g = np.nonzero((first == a) & (nobs >= 2))[0]
        if not len(g):
            continue
        r = MR.triangulate_views(kpts[a:nv], tracks[g][:, a:nv], nv - a, Ks[a:nv], Rs[a:nv], ts[a:nv], **gates)
        for k in ("points3d", "status", "n_inliers", "reproj_error", "score", "cost0", "cost1"):
            out[k][g] = r[k]
        out["inlier_views"][g] = (r["inlier_views"].view(np.uint32).astype(np.uint64) << np.uint64(a)).astype(np.uint32).view(np.int32)
        out["winner"][g] = np.where(r["winner"] >= 0, r["winner"] + a, -1)
        out["groups"].append((a, g, r))
    out["valid"] = out["status"] == MR.VALID
    out["info"] = np.array([K] + [int((out["status"] == s).sum()) for s in range(7)], np.int32)
    return out


def gate_margin(r, max_depth=math.inf):
    """multiview_reference.gate_margin of a triangulate_views(anchor='first') result: the least over its groups."""
    return min([MR.gate_margin(sub, max_depth) for _, _, sub in r["groups"]], default=math.inf)
