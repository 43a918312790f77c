"""numpy restatement of csrc/k_retrieval.hip, operation by operation in fp32 with the kernels' orders of summation, the same
stages in float64, and the checkers that hold the device (or the host build of the kernels) to float64.

Orders (fp32, every product and sum rounded on its own):
  dot64(x, c)  = (((0 + x0 c0) + x1 c1) + ...) + x63 c63                                                        depth 64
  cluster sum  = chunks of CHUNK = 1024 rows: ((0 + t_i0) + t_i1) + ... over the chunk's rows of the cluster ascending, then the chunk
                 sums ascending onto 0; t = row (k-means) or row - centroid (VLAD)
  n2 of a block: lane l of 16 holds components 4 l .. 4 l + 3: p_l = ((v0 v0 + v1 v1) + v2 v2) + v3 v3, then the balanced tree over the lanes
  score        = dot64 per 64-block, ((0 + b_0) + b_1) + ... over the 16 blocks of a segment, the segments likewise        depth 96
  objective    = fp64: per chunk, lane t of 256 adds the scores of rows 4 t .. 4 t + 3 onto 0, p[t] += p[t + h] for h = 128 .. 1; chunks onto 0
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
CHUNK, SEG = 1024, 16
DEPTH_ASSIGN, DEPTH_SCORE = 64, 96
FLT_MIN = np.float32(1.17549435e-38)


def gamma(n):
    """The factor of an n-deep chain of rounded operations (Higham): n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def dot64(x, cb):
    """x (n,64), cb (C,64) fp32 -> (n,C) fp32, the chain over the 64 components."""
    x, cb = np.asarray(x, F), np.asarray(cb, F)
    s = np.zeros((x.shape[0], cb.shape[0]), F)
    with np.errstate(all="ignore"):
        for j in range(64):
            s = s + x[:, j, None] * cb[None, :, j]
    return s


def row_state(desc, counts):
    """(G,K) uint8: 0 beyond the count, 1 valid, 2 below the count but not finite."""
    G, K = desc.shape[:2]
    n = np.full(G, K) if counts is None else np.clip(np.asarray(counts, np.int64), 0, K)
    below = np.arange(K)[None, :] < n[:, None]
    fin = np.isfinite(desc).all(axis=2)
    return np.where(below, np.where(fin, 1, 2), 0).astype(np.uint8)


def pick(scores, valid):
    """The lowest index of the largest finite score per row, -1 where there is none or the row is not valid; and that score (NaN: none)."""
    fin = np.isfinite(scores)
    masked = np.where(fin, scores, -np.inf)
    best = masked.argmax(axis=1)
    none = ~fin.any(axis=1) | ~valid
    win = np.where(none, np.nan, masked[np.arange(len(best)), best]).astype(scores.dtype)
    return np.where(none, -1, best).astype(np.int32), win


def assign(desc, counts, cb):
    """-> assign (G,K) int32, winning score (G,K) fp32, state (G,K) uint8."""
    desc = np.asarray(desc, F)
    G, K = desc.shape[:2]
    state = row_state(desc, counts)
    valid = (state == 1).reshape(-1)
    a, w = pick(dot64(np.where(valid[:, None], desc.reshape(-1, 64), 0), cb), valid)
    return a.reshape(G, K), w.reshape(G, K), state


def chunk_sums(rows, a, cb, residual):
    """rows (R,64) fp32, a (R,) int32, cb (C,64) -> the sum per cluster (C,64) fp32 and the counts (C,), in the kernels' order."""
    R, C = rows.shape[0], cb.shape[0]
    nch = max((R + CHUNK - 1) // CHUNK, 1)
    X = np.zeros((nch * CHUNK, 64), F)
    A = np.full(nch * CHUNK, -1, np.int64)
    X[:R], A[:R] = rows, a
    X, A = X.reshape(nch, CHUNK, 64), A.reshape(nch, CHUNK)
    part, cnt = np.zeros((nch, C, 64), F), np.zeros((nch, C), np.int64)
    with np.errstate(all="ignore"):
        for r in range(min(CHUNK, R)):
            ch = np.nonzero(A[:, r] >= 0)[0]
            if len(ch) == 0:
                continue
            c = A[ch, r]
            t = X[ch, r] - cb[c] if residual else X[ch, r]
            part[ch, c] = part[ch, c] + t
            cnt[ch, c] += 1
        total = np.zeros((C, 64), F)
        for ch in range(nch):
            total = total + part[ch]
    return total, cnt.sum(axis=0).astype(np.int32)


def norm2(v):
    """v (..., 64) fp32 -> the squared norm by the 16-lane tree."""
    with np.errstate(all="ignore"):
        q = np.asarray(v, F).reshape(v.shape[:-1] + (16, 4))
        p = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
        while p.shape[-1] > 1:
            p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def unit_blocks(total):
    """(C,64) sums -> ok (C,) and the blocks times 1 / sqrt(n2) (zero where not ok)."""
    n2 = norm2(total)
    with np.errstate(all="ignore"):
        ok = np.isfinite(n2) & (n2 >= FLT_MIN)
        inv = np.where(ok, F(1) / np.sqrt(np.where(ok, n2, F(1))), F(0)).astype(F)
        return ok, np.where(ok[:, None], total * inv[:, None], F(0)).astype(F)


def vlad(desc, counts, cb):
    desc, cb = np.asarray(desc, F), np.asarray(cb, F)
    G, K = desc.shape[:2]
    C = cb.shape[0]
    a, _, state = assign(desc, counts, cb)
    out = {"vlad": np.zeros((G, C * 64), F), "assign": a, "n_assigned": np.zeros((G, C), np.int32), "info": np.zeros((G, 4), np.int32)}
    for g in range(G):
        total, cnt = chunk_sums(desc[g], a[g], cb, True)
        ok, blocks = unit_blocks(total)
        m = int(ok.sum())
        if m:
            blocks = blocks * (F(1) / np.sqrt(F(m)))
        out["vlad"][g], out["n_assigned"][g] = blocks.reshape(-1), cnt
        out["info"][g] = [(state[g] == 1).sum(), (state[g] == 2).sum(), m, m == 0]
    return out


def objective(win, a):
    """The fp64 sum of the winning scores (win fp32 (R,), a (R,)) in the kernels' order."""
    R = len(a)
    nch = max((R + CHUNK - 1) // CHUNK, 1)
    w = np.zeros(nch * CHUNK, np.float64)
    w[:R] = np.where(a >= 0, np.nan_to_num(win.astype(np.float64)), 0.0)
    w = w.reshape(nch, 256, 4)
    p = np.zeros((nch, 256))
    for u in range(4):
        p = p + w[:, :, u]
    h = 128
    while h >= 1:
        p = p[:, :h] + p[:, h:2 * h]
        h //= 2
    o = 0.0
    for ch in range(nch):
        o = o + p[ch, 0]
    return np.float64(o)


def kmeans_step(desc, counts, cb):
    desc, cb = np.asarray(desc, F), np.asarray(cb, F)
    a, win, state = assign(desc, counts, cb)
    total, cnt = chunk_sums(desc.reshape(-1, 64), a.reshape(-1), cb, False)
    ok, blocks = unit_blocks(total)
    return {"codebook": np.where(ok[:, None], blocks, cb).astype(F), "assign": a, "n_assigned": cnt, "objective": objective(win.reshape(-1), a.reshape(-1)),
            "info": np.array([(state == 1).sum(), (state == 2).sum(), (~ok).sum(), 0], np.int32)}


def initial_codebook(desc, counts, C):
    """retrieval.initial_codebook: the finite rows below their counts numbered in (group, row) order, centroid c = row floor(c R / C)."""
    flat = np.asarray(desc, F).reshape(-1, 64)
    ok = (row_state(np.asarray(desc, F), counts) == 1).reshape(-1)
    order = np.cumsum(ok)
    want = (np.arange(C, dtype=np.int64) * order[-1]) // C
    return flat[np.minimum(np.searchsorted(order, want + 1), len(flat) - 1)].copy()


def train_codebook(desc, counts, C, iterations, step=kmeans_step):
    cb, objs = initial_codebook(desc, counts, C), []
    for _ in range(iterations):
        r = step(desc, counts, cb)
        cb = r["codebook"]
        objs.append(r["objective"])
    return cb, np.array(objs)


def scores(q, db):
    """q (Q,D), db (N,D) fp32 -> (Q,N) fp32 in the kernel's order."""
    q, db = np.asarray(q, F), np.asarray(db, F)
    nblk = q.shape[1] // 64
    tot = np.zeros((q.shape[0], db.shape[0]), F)
    with np.errstate(all="ignore"):
        for b0 in range(0, nblk, SEG):
            seg = np.zeros_like(tot)
            for b in range(b0, min(b0 + SEG, nblk)):
                seg = seg + dot64(q[:, 64 * b:64 * b + 64], db[:, 64 * b:64 * b + 64])
            tot = tot + seg
    return tot


def topk(s, n_db, k, exclude_self):
    """s (Q,N) scores -> idx (Q,k) int32, score (Q,k) of s's dtype: finite scores of rows < n_db by (score descending, index ascending)."""
    Q, N = s.shape
    n = N if n_db is None else int(np.clip(n_db, 0, N))
    idx, out = np.full((Q, k), -1, np.int32), np.full((Q, k), np.nan, s.dtype)
    for j in range(Q):
        cand = np.nonzero(np.isfinite(s[j, :n]) & ~((np.arange(n) == j) & bool(exclude_self)))[0]
        key = np.where(s[j, cand] == 0, 0, s[j, cand])
        order = cand[np.lexsort((cand, -key))][:k]
        idx[j, :len(order)], out[j, :len(order)] = order, s[j, order]
    return idx, out


def retrieve_topk(q, db, n_db, k, exclude_self):
    """(G,Q,D), (G,N,D), n_db (G,) or None -> idx (G,Q,k), score (G,Q,k)."""
    r = [topk(scores(q[g], db[g]), None if n_db is None else n_db[g], k, exclude_self) for g in range(len(q))]
    return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])


def pair_capacity(V, k):
    return min(V * k, V * (V - 1) // 2)


def pairs(idx, n_views):
    """idx (V,k) of one scene -> view_pairs (Pcap,2) int32, n_pairs."""
    V, k = idx.shape
    nv = V if n_views is None else int(np.clip(n_views, 0, V))
    adj = np.zeros((V, V), bool)
    for v in range(nv):
        for w in idx[v]:
            if 0 <= w < nv and w != v:
                adj[min(v, w), max(v, w)] = True
    got = np.argwhere(adj)                                  # (row-major: ascending (a, b))
    out = np.full((pair_capacity(V, k), 2), -1, np.int32)
    out[:len(got)] = got
    return out, len(got)


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
def scores64(x, cb):
    """-> the exact-ish inner products (n,C) and the sums of the magnitudes of their terms."""
    x, cb = np.asarray(x, np.float64), np.asarray(cb, np.float64)
    with np.errstate(all="ignore"):
        return x @ cb.T, np.abs(x) @ np.abs(cb).T


def vlad64(desc_g, a_g, cb):
    """One group in float64 from a given assignment -> the vector (C*64), m, and per block (norm of the sum, sum of |residuals| per component)."""
    x, cb = np.asarray(desc_g, np.float64), np.asarray(cb, np.float64)
    C = cb.shape[0]
    tot, mag = np.zeros((C, 64)), np.zeros((C, 64))
    for c in range(C):
        r = x[a_g == c] - cb[c]
        tot[c], mag[c] = r.sum(axis=0), np.abs(r).sum(axis=0)
    nrm = np.linalg.norm(tot, axis=1)
    ok = nrm * nrm >= float(FLT_MIN)
    m = int(ok.sum())
    v = np.where(ok[:, None], tot / np.where(ok, nrm, 1.0)[:, None], 0.0) / np.sqrt(max(m, 1))
    return v.reshape(-1), m, nrm, mag


# ---- checkers ---------------------------------------------------------------------------------------------------------------------------
def check_assign(desc, counts, cb, got):
    """The device's assignment against float64 (module docstring of the tests): a choice is right when its float64 score is within
    2 gamma(64) max(sum |x_j c_j|) of the float64 maximum; outside that window it is the float64 arg-max.  Returns the share of valid rows
    whose float64 runner-up is inside the window (a property of the data: the tests bound it by 0.1 %)."""
    desc = np.asarray(desc, F)
    state = row_state(desc, counts).reshape(-1)
    got = np.asarray(got).reshape(-1)
    assert (got[state != 1] == -1).all()
    v = state == 1
    s, mag = scores64(desc.reshape(-1, 64)[v], cb)
    fin = np.isfinite(s)
    g = got[v]
    has = fin.any(axis=1)
    assert ((g >= 0) == has).all() and (g < len(cb)).all()
    s, mag, g = s[has], mag[has], g[has]
    s = np.where(np.isfinite(s), s, -np.inf)
    best = s.argmax(axis=1)
    r = np.arange(len(g))
    window = 2 * gamma(DEPTH_ASSIGN) * np.maximum(mag[r, g], mag[r, best])
    assert (s[r, g] >= s[r, best] - window).all(), "a choice outside the window is not the float64 arg-max"
    second = np.partition(s, -2, axis=1)[:, -2] if s.shape[1] > 1 else np.full(len(g), -np.inf)
    close = second >= s[r, best] - 2 * gamma(DEPTH_ASSIGN) * mag.max(axis=1)
    return float(close.mean()) if len(g) else 0.0


def sum_depth(K):
    """The deepest chain behind a component of a cluster sum of K rows: the subtraction, a chunk's rows, the chunks."""
    return 1 + min(K, CHUNK) + (K + CHUNK - 1) // CHUNK


def check_vlad(desc, counts, cb, got):
    """'vlad', 'n_assigned', 'info' of the device against float64 computed from the device's own 'assign'.
    Bound per block, with e_j = gamma(sum_depth) sum_i |r_ij| the error of component j of the block's sum s: the unit block s / |s| moves by at
    most 2 |e| / |s|, the norm (a tree of depth 9), the square root, the reciprocal and the two products add 10 u; all over sqrt(m).
    Returns the largest error as a fraction of the bound."""
    desc = np.asarray(desc, F)
    G, K = desc.shape[:2]
    C = len(cb)
    state = row_state(desc, counts)
    worst = 0.0
    for g in range(G):
        a = np.asarray(got["assign"][g])
        v, m, nrm, mag = vlad64(desc[g], a, cb)
        assert list(got["info"][g]) == [(state[g] == 1).sum(), (state[g] == 2).sum(), m, int(m == 0)], (g, got["info"][g], m)
        assert np.array_equal(got["n_assigned"][g], np.bincount(a[a >= 0], minlength=C))
        d = np.abs(np.asarray(got["vlad"][g], np.float64) - v).reshape(C, 64).max(axis=1)
        e = gamma(sum_depth(K)) * np.linalg.norm(mag, axis=1)
        bound = (2 * e / np.where(nrm > 0, nrm, 1.0) + 10 * U) / np.sqrt(max(m, 1))
        assert (d[nrm == 0] == 0).all()
        live = nrm > 0
        if live.any():
            worst = max(worst, float((d[live] / bound[live]).max()))
    assert worst <= 1.0, worst
    return worst


def check_kmeans(desc, counts, cb, got):
    """One k-means step of the device against float64 from the device's own 'assign': the centroids within 2 |e| / |s| + 8 u of s / |s| (e as
    in check_vlad without the subtraction), the objective within sum_i gamma(64) sum_j |x_ij c_j| + gamma(14) sum_i |score_i| of the float64
    sum, kept clusters unchanged.  Returns the largest centroid error as a fraction of its bound."""
    desc, cb = np.asarray(desc, F), np.asarray(cb, F)
    C = len(cb)
    x = desc.reshape(-1, 64).astype(np.float64)
    a = np.asarray(got["assign"]).reshape(-1)
    state = row_state(desc, counts)
    worst, kept = 0.0, 0
    for c in range(C):
        rows = x[a == c]
        s, mag = rows.sum(axis=0), np.abs(rows).sum(axis=0)
        n = np.linalg.norm(s)
        assert got["n_assigned"][c] == len(rows)
        if n * n < float(FLT_MIN):
            assert np.array_equal(got["codebook"][c].view(np.uint32), cb[c].view(np.uint32)), c
            kept += 1
            continue
        bound = 2 * gamma(sum_depth(len(x))) * np.linalg.norm(mag) / n + 8 * U
        worst = max(worst, float(np.abs(got["codebook"][c].astype(np.float64) - s / n).max() / bound))
    assert worst <= 1.0, worst
    assert list(got["info"]) == [(state == 1).sum(), (state == 2).sum(), kept, 0]
    s64, mag = scores64(x[a >= 0], cb)
    r = np.arange(len(s64))
    want, slack = s64[r, a[a >= 0]].sum(), gamma(DEPTH_ASSIGN) * mag[r, a[a >= 0]].sum() + gamma(14) * np.abs(s64[r, a[a >= 0]]).sum()
    assert abs(float(got["objective"]) - want) <= slack, (got["objective"], want, slack)
    return worst


def check_topk(q, db, n_db, k, exclude_self, idx, score):
    """One group's shortlists against float64.  W(j, i) = gamma(96) sum |q_j d_i| bounds the error of one score; two scores are told apart
    outside W_a + W_b.  The returned float64 scores are non-increasing up to that window, no row left out beats the k-th by more than it, a
    returned score is within W of float64, the number returned is the number of candidates (up to k), and equal device scores come out lower
    index first.  Returns (slots whose index differs from the float64 ranking, slots, the largest W)."""
    q64, d64 = np.asarray(q, np.float64), np.asarray(db, np.float64)
    Q, N = len(q64), len(d64)
    n = N if n_db is None else int(np.clip(n_db, 0, N))
    with np.errstate(all="ignore"):
        s, W = q64 @ d64.T, gamma(DEPTH_SCORE) * (np.abs(q64) @ np.abs(d64).T)
    want, _ = topk(s, n, k, exclude_self)
    differ = 0
    for j in range(Q):
        cand = np.isfinite(s[j, :n]) & ~((np.arange(n) == j) & bool(exclude_self))
        found = min(k, int(cand.sum()))
        got = idx[j, :found]
        assert (idx[j, found:] == -1).all() and np.isnan(score[j, found:]).all(), j
        assert len(set(got.tolist())) == found and cand[got].all(), j
        assert (np.abs(score[j, :found].astype(np.float64) - s[j, got]) <= W[j, got]).all(), j
        for a, b in zip(got[:-1], got[1:]):
            assert s[j, a] >= s[j, b] - (W[j, a] + W[j, b]), (j, a, b)
        dev = score[j, :found]
        same = dev[:-1] == dev[1:]
        assert (got[:-1][same] < got[1:][same]).all(), j
        if found:
            out = cand.copy()
            out[got] = False
            last = got[-1]
            assert (s[j, :n][out] <= s[j, last] + W[j, :n][out] + W[j, last]).all(), j
        differ += int((got != want[j, :found]).sum())
    return differ, Q * k, float(np.nanmax(W[:, :n])) if n else 0.0
