"""numpy restatement of DESIGN.md 3.21 (csrc/k_map.hip): the map rows of one scene in the kernel's fp32 operation order, the projection of the
rows in float64 rounded once, and a brute-force float64 mutual-nearest-neighbour matcher that reports the margin of every decision it takes.
Specification only: scenes are in tests/localization_support.py."""
import numpy as np

SELECTED, SKIP_STATUS, SKIP_POINT, SKIP_VIEWS, SKIP_NORM = 0, 1, 2, 3, 4
FLT_MIN = np.float32(1.17549435e-38)
F32 = np.float32


def contributing(desc, tracks, inlier_views):
    """(T, V) bool: view v contributes to track t (bit v of the mask read as unsigned, a row in range, a finite row)."""
    V, kcap = desc.shape[:2]
    T = tracks.shape[0]
    bits = (np.asarray(inlier_views).astype(np.int64) & 0xffffffff)[:, None] >> np.arange(V)[None, :] & 1
    rows = np.asarray(tracks).astype(np.int64)
    inside = (rows >= 0) & (rows < kcap)
    fin = np.isfinite(desc).all(axis=2)                    # (V, kcap)
    ok = np.zeros((T, V), bool)
    for v in range(V):
        r = np.where(inside[:, v], rows[:, v], 0)
        ok[:, v] = (bits[:, v] != 0) & inside[:, v] & (fin[v, r] if kcap else False)
    return ok


def norm2(acc):
    """The squared norm of (T, 64) fp32 sums in the kernel's order: four components per lane in sequence, a balanced tree over the 16 lanes."""
    s = acc.reshape(-1, 16, 4)
    with np.errstate(all="ignore"):
        p = ((s[:, :, 0] * s[:, :, 0] + s[:, :, 1] * s[:, :, 1]) + s[:, :, 2] * s[:, :, 2]) + s[:, :, 3] * s[:, :, 3]
        while p.shape[1] > 1:
            p = p[:, 0::2] + p[:, 1::2]
    assert p.dtype == np.float32
    return p[:, 0]


def track_rows(desc, tracks, points3d, status, inlier_views, min_views=2):
    """Per track: flag (T,), n_obs (T,), sum (T,64), n2 (T,), desc (T,64), coherence (T,) -- before the selected ones are compacted."""
    desc = np.ascontiguousarray(desc, np.float32)
    T, V = tracks.shape
    ok = contributing(desc, tracks, inlier_views)
    status = np.asarray(status)
    flag = np.where(status != 0, SKIP_STATUS, np.where(~np.isfinite(np.asarray(points3d, np.float32)).all(axis=1), SKIP_POINT, SELECTED))
    live = flag == SELECTED
    acc = np.zeros((T, 64), np.float32)
    n = np.zeros(T, np.int64)
    with np.errstate(all="ignore"):
        for v in range(V):                                 # views ascending, one fp32 addition per component
            use = live & ok[:, v]
            k = np.nonzero(use)[0]
            acc[k] = acc[k] + desc[v, tracks[k, v]]
            n[k] += 1
        n2 = norm2(acc)
        flag = np.where((flag == SELECTED) & (n < min_views), SKIP_VIEWS, flag)
        flag = np.where((flag == SELECTED) & (~np.isfinite(n2) | (n2 < FLT_MIN)), SKIP_NORM, flag)
        r = np.sqrt(n2)
        inv = F32(1.0) / r
        d = acc * inv[:, None]
        coh = r / n.astype(np.float32)
    assert r.dtype == np.float32 and d.dtype == np.float32 and coh.dtype == np.float32
    return dict(flag=flag, n_obs=n, sum=acc, n2=n2, desc=d, coherence=coh)


def build_map(desc, tracks, points3d, status, inlier_views, min_views=2, max_points=None):
    """One scene: desc (V,Kcap,64) fp32, tracks (T,V), points3d (T,3) fp32, status (T,), inlier_views (T,) int32 -> the outputs of
    xfh_build_map (M = max_points or T rows)."""
    tracks = np.asarray(tracks)
    T = tracks.shape[0]
    M = T if max_points is None else int(max_points)
    tr = track_rows(desc, tracks, points3d, status, inlier_views, min_views)
    sel = np.nonzero(tr["flag"] == SELECTED)[0]
    kept = sel[:M]
    k = len(kept)
    out = dict(points=np.full((M, 3), np.nan, np.float32), desc=np.zeros((M, 64), np.float32), desc_f16=np.zeros((M, 64), np.float16),
               track=np.full(M, -1, np.int32), n_obs=np.zeros(M, np.uint8), coherence=np.zeros(M, np.float32), n_points=np.int32(k))
    out["points"][:k] = np.asarray(points3d, np.float32)[kept]
    out["desc"][:k] = tr["desc"][kept]
    out["desc_f16"][:k] = (tr["desc"][kept] * F32(256.0)).astype(np.float16)      # (numpy rounds to nearest even)
    out["track"][:k] = kept
    out["n_obs"][:k] = tr["n_obs"][kept]
    out["coherence"][:k] = tr["coherence"][kept]
    out["info"] = np.array([T, k] + [int((tr["flag"] == f).sum()) for f in (SKIP_STATUS, SKIP_POINT, SKIP_VIEWS, SKIP_NORM)] + [len(sel) - k, 0], np.int32)
    out["rows"] = tr
    return out


def project(points, n_points, R, t, K, image_size=None, margin=0.0):
    """One query: points (M,3) fp32 -> uv (M,2) fp32, float64 arithmetic in the kernel's order rounded once."""
    X = np.asarray(points, np.float32).astype(np.float64)
    R, t, K = np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), np.asarray(K, np.float64).reshape(9)
    M = X.shape[0]
    n = M if n_points is None else int(n_points)
    with np.errstate(all="ignore"):
        x = ((R[0] * X[:, 0] + R[1] * X[:, 1]) + R[2] * X[:, 2]) + t[0]
        y = ((R[3] * X[:, 0] + R[4] * X[:, 1]) + R[5] * X[:, 2]) + t[1]
        z = ((R[6] * X[:, 0] + R[7] * X[:, 1]) + R[8] * X[:, 2]) + t[2]
        a = (K[0] * x + K[1] * y) + K[2] * z
        b = (K[3] * x + K[4] * y) + K[5] * z
        w = (K[6] * x + K[7] * y) + K[8] * z
        u, v = a / w, b / w
        ok = (np.arange(M) < n) & np.isfinite(z) & (z > 0.0) & np.isfinite(u) & np.isfinite(v)
        if image_size is not None:
            W, H = float(image_size[0]), float(image_size[1])
            ok &= ~(u < -margin) & ~(u > W + margin) & ~(v < -margin) & ~(v > H + margin)
        uv = np.stack([u, v], axis=1).astype(np.float32)
    uv[~ok] = np.nan
    return uv


def mnn(d1, n1, d2, n2, min_cossim=-1.0):
    """Brute-force float64 mutual nearest neighbours of the first n1 rows of d1 and the first n2 of d2 (ties to the lowest index, the
    similarity test `> min_cossim` when min_cossim > 0).  Returns idx0 (ascending), idx1 and margin.  Element (i, j) is a match iff its
    similarity exceeds every other one of row i, every other one of column j and min_cossim; its slack is the largest of (best other of the
    row) - s, (best other of the column) - s and min_cossim - s: negative for a match, positive for everything else.  margin is the smallest
    |slack| of all n1 n2 elements: no perturbation of the similarities below it changes the lists."""
    a, b = np.asarray(d1, np.float64)[:n1], np.asarray(d2, np.float64)[:n2]
    if n1 == 0 or n2 == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.inf
    s = a @ b.T
    j, i = s.argmax(axis=1), s.argmax(axis=0)
    rows, cols = np.arange(n1), np.arange(n2)
    slack = np.full(s.shape, -np.inf)
    if n2 > 1:
        top = np.partition(s, n2 - 2, axis=1)[:, n2 - 2:]  # (second best, best) of every row
        other = np.repeat(top[:, 1:2], n2, axis=1)
        other[rows, j] = top[:, 0]
        slack = np.maximum(slack, other - s)
    if n1 > 1:
        top = np.partition(s, n1 - 2, axis=0)[n1 - 2:, :]
        other = np.repeat(top[1:2, :], n1, axis=0)
        other[i, cols] = top[0]
        slack = np.maximum(slack, other - s)
    if min_cossim > 0:
        slack = np.maximum(slack, min_cossim - s)
    mutual = i[j] == rows
    if min_cossim > 0:
        mutual &= s[rows, j] > min_cossim
    return rows[mutual].astype(np.int64), j[mutual].astype(np.int64), float(np.abs(slack).min())
