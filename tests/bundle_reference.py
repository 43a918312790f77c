"""float64 numpy restatement of the bundle adjustment of csrc/k_triangulate.hip: the observation set, the Huber loss, the
Jacobians of an observation (ba_term), the point blocks (ba_point), the blocks of the reduced camera system (ba_pair_add, summed in
rs::block_sums' order by oracle.twoview_reference.block_sums), the packed Cholesky solve (ba_cholesky_solve), the pose and point updates
(ba_pose_update, ba_point_step), the decision (ba_decide) and the Levenberg-Marquardt loop of the launches.

It performs the kernels' operations in the kernels' order, vectorised over the tracks of one scene (numpy never fuses a multiply and an add; a
view that a track skips contributes an exact + 0.0 or - 0.0 to a sum that started at + 0.0), so its results are comparable bit for bit.  The
Cholesky factorisation is written right-looking (column j is subtracted from the whole trailing triangle at once): every element still
receives its subtractions in ascending column order, which is all that the result depends on.

TEST INFRASTRUCTURE ONLY: nothing under ``accelerated_features_amd/`` imports it.
"""
import math

import numpy as np

import multiview_reference as MR
from oracle.twoview_reference import block_sums, finite

MIN_VIEW_OBS = 6
FTOL = 1e-8
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-10, 1e10
ST_OK, ST_NOTHING, ST_NOT_FINITE = 0, 1, 2
_ERR = dict(all="ignore")


def stage_view(Rv, tv, Kv):
    """mv_stage_pose, which stages the bundle kernels' views: the first 20 doubles of multiview_reference.stage_view's block (of them the
    bundle solver reads what mv_reproj reads, and the pose flag; the centre is written and not read)."""
    return MR.stage_view(Rv, tv, Kv, Rv, tv)


def rho(e2, c):
    """ba_rho: (Huber's rho of e^2 at c pixels, the weight, the Huber switch's distance from a tie)."""
    with np.errstate(**_ERR):
        e = np.sqrt(e2)
        far = e > c
        wt = np.where(far, c / e, 1.0)
        r = np.where(far, (2.0 * c) * e - c * c, e2)
        tie = np.abs(e - c) / c if math.isfinite(c) else np.full(np.shape(e), np.inf)
    return r, wt, tie


def pixels(kpts, tracks, nv):
    """The pixels of the tracks through the table: [(u, v, in range)] per view (NaN outside)."""
    kcap, K = kpts.shape[1], tracks.shape[0]
    px = []
    for w in range(nv):
        r = tracks[:, w]
        inr = (r >= 0) & (r < kcap)
        q = kpts[w][np.where(inr, r, 0)] if kcap else np.zeros((K, 2))
        px.append((np.where(inr, q[:, 0], np.nan), np.where(inr, q[:, 1], np.nan), inr))
    return px


def observation_set(views, nv, px, inl, X):
    """ba_mask: M[w] (K,) bool per view; a track with fewer than 2 observations has none.  Also the depths' distance from 0."""
    K = X[0].shape[0]
    xfin = finite(X[0]) & finite(X[1]) & finite(X[2])
    M, tie = [], np.inf
    with np.errstate(**_ERR):
        for w in range(nv):
            u, v, inr = px[w]
            pre = (((inl >> w) & 1) != 0) & inr & finite(u) & finite(v) & views[w]["ok"] & xfin
            e2, z = MR.reproj(views[w], X, u, v)
            M.append(pre & (z > 0.0) & finite(e2))
            tie = min(tie, np.min(np.abs(z[pre & finite(z)]) / np.maximum(1.0, np.abs(z[pre & finite(z)])), initial=np.inf))
    n = np.sum(M, axis=0) if nv else np.zeros(K, int)
    return [m & (n >= 2) for m in M], float(tie)


def cost(views, nv, px, M, X, c):
    """ba_cost: (cost (K,), bad (K,), the Huber switch's least distance from a tie)."""
    K = X[0].shape[0]
    tot, bad, tie = np.zeros(K), np.zeros(K, bool), np.inf
    with np.errstate(**_ERR):
        for w in range(nv):
            if not M[w].any():
                continue
            e2, z = MR.reproj(views[w], X, px[w][0], px[w][1])
            bad = bad | (M[w] & (~(z > 0.0) | ~finite(e2)))
            r, _, t = rho(e2, c)
            tot = tot + np.where(M[w], r, 0.0)
            tie = min(tie, np.min(t[M[w] & finite(t)], initial=np.inf))
    return tot, bad, float(tie)


def term(p, X, u, v, c):
    """ba_term: dict du, dv, wt, jp (6: u row, v row), jc (12: u row, v row) of arrays over the tracks."""
    R, t, cal = p["R"], p["t"], p["cal"]
    with np.errstate(**_ERR):
        e2, z = MR.reproj(p, X, u, v)
        _, wt, _ = rho(e2, c)
        x = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0]
        y = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1]
        a, b = x / z, y / z
        du, dv = (cal[0] * a + cal[2]) - u, (cal[1] * b + cal[3]) - v
        jp = [cal[0] * ((R[j] - a * R[6 + j]) / z) for j in range(3)] + [cal[1] * ((R[3 + j] - b * R[6 + j]) / z) for j in range(3)]
        gu0, gu2, gv1, gv2 = cal[0] / z, -((cal[0] * a) / z), cal[1] / z, -((cal[1] * b) / z)
        d = [[R[3 * i + 2] * X[1] - R[3 * i + 1] * X[2], R[3 * i] * X[2] - R[3 * i + 2] * X[0], R[3 * i + 1] * X[0] - R[3 * i] * X[1]] for i in range(3)]
        zero = np.zeros_like(z)
        jc = [gu0 * d[0][j] + gu2 * d[2][j] for j in range(3)] + [gu0, zero, gu2] + [gv1 * d[1][j] + gv2 * d[2][j] for j in range(3)] + [zero, gv1, gv2]
    return dict(du=du, dv=dv, wt=wt, jp=jp, jc=jc)


def point_block(views, nv, px, M, X, c, opl):
    """ba_point: (Vi (6 arrays: 00 01 02 11 12 22), g (3 arrays), ok (K,), det / (A00 A11 A22) for the margin)."""
    K = X[0].shape[0]
    A, s = [np.zeros(K) for _ in range(6)], [np.zeros(K) for _ in range(3)]
    with np.errstate(**_ERR):
        for w in range(nv):
            if not M[w].any():
                continue
            t = term(views[w], X, px[w][0], px[w][1], c)
            jp, wt = t["jp"], t["wt"]
            add = lambda acc, val: acc + np.where(M[w], val, 0.0)      # noqa: E731
            for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                A[k] = add(A[k], wt * (jp[i] * jp[j] + jp[3 + i] * jp[3 + j]))
            for i in range(3):
                s[i] = add(s[i], wt * (jp[i] * t["du"] + jp[3 + i] * t["dv"]))
        g = [-s[i] for i in range(3)]
        A[0], A[3], A[5] = A[0] * opl, A[3] * opl, A[5] * opl
        c00, c01, c02 = A[3] * A[5] - A[4] * A[4], A[2] * A[4] - A[1] * A[5], A[1] * A[4] - A[2] * A[3]
        det = (A[0] * c00 + A[1] * c01) + A[2] * c02
        one, zero = np.full(K, -1.0), np.zeros(K)
        q0, q1, q2 = MR.step(A, [one, zero, zero]), MR.step(A, [zero, one, zero]), MR.step(A, [zero, zero, one])
        Vi = [q0[0], q0[1], q0[2], q1[1], q1[2], q2[2]]
        ok = finite(det) & (det > 0.0)
        rel = det / ((A[0] * A[3]) * A[5])
    return Vi, g, ok, rel


def W_of(t):
    """ba_W: 18 arrays, row a (6) x column c (3)."""
    return [t["wt"] * (t["jc"][a] * t["jp"][c] + t["jc"][6 + a] * t["jp"][3 + c]) for a in range(6) for c in range(3)]


def Y_of(W, Vi):
    """ba_Y: W V^-1."""
    Y = []
    for a in range(6):
        w0, w1, w2 = W[3 * a], W[3 * a + 1], W[3 * a + 2]
        Y += [(w0 * Vi[0] + w1 * Vi[1]) + w2 * Vi[2], (w0 * Vi[1] + w1 * Vi[3]) + w2 * Vi[4], (w0 * Vi[2] + w1 * Vi[4]) + w2 * Vi[5]]
    return Y


def pair_terms(tr, tc, Vi, g, held, opl, diag, both):
    """ba_pair_add: the per-track terms (K, 36 or 42) of block (row view, column view); tracks outside `both` give 0."""
    with np.errstate(**_ERR):
        Wr, Wc = W_of(tr), W_of(tc)
        Y = Y_of(Wr, Vi)
        cols = []
        for a in range(6):
            for b in range(6):
                s = np.where(held, 0.0, (Y[3 * a] * Wc[3 * b] + Y[3 * a + 1] * Wc[3 * b + 1]) + Y[3 * a + 2] * Wc[3 * b + 2])
                if diag:
                    u = tr["wt"] * (tr["jc"][a] * tr["jc"][b] + tr["jc"][6 + a] * tr["jc"][6 + b])
                    cols.append((u * opl if a == b else u) - s)
                else:
                    cols.append(-s)                    # (acc - s is acc + (-s), bit for bit)
        if diag:
            for a in range(6):
                r = -(tr["wt"] * (tr["jc"][a] * tr["du"] + tr["jc"][6 + a] * tr["dv"]))
                yg = np.where(held, 0.0, (Y[3 * a] * g[0] + Y[3 * a + 1] * g[1]) + Y[3 * a + 2] * g[2])
                cols.append(r - yg)
        return np.where(both[:, None], np.stack(cols, axis=1), 0.0)


def reduced_system(views, nv, V, px, M, X, c, opl, Vi, g, held, free):
    """The launches of ba_schur_kernel: the lower triangle of the reduced camera system (n, n), n = 6 V, dense with zeros above, and rhs (n,)."""
    n, K = 6 * V, X[0].shape[0]
    S, rhs = np.zeros((n, n)), np.zeros(n)
    terms = {}
    for w in range(V):
        for v in range(w + 1):
            if not ((free >> v) & 1 and (free >> w) & 1):
                if v == w:
                    S[6 * w:6 * w + 6, 6 * w:6 * w + 6] = np.eye(6)
                continue
            for x in (v, w):
                if x not in terms:
                    terms[x] = term(views[x], X, px[x][0], px[x][1], c)
            both = M[v] & M[w]
            T = pair_terms(terms[w], terms[v], Vi, g, held, opl, v == w, both) if K else np.zeros((0, 42 if v == w else 36))
            tot = block_sums(T) if K else np.zeros(T.shape[1])
            blk = tot[:36].reshape(6, 6)
            if v == w:
                S[6 * w:6 * w + 6, 6 * w:6 * w + 6] = np.tril(blk)
                rhs[6 * w:6 * w + 6] = tot[36:]
            else:
                S[6 * w:6 * w + 6, 6 * v:6 * v + 6] = blk
    return S, rhs


def cholesky_solve(S, rhs):
    """ba_cholesky_solve on the lower triangle S (n, n) and rhs (n,): (ok, the solution, L, the pivots' squares relative to the diagonal)."""
    L, r = np.tril(S).astype(np.float64), rhs.astype(np.float64).copy()
    n = L.shape[0]
    piv, rel = np.zeros(n), np.zeros(n)
    diag0 = np.diag(S).copy()
    with np.errstate(**_ERR):
        for j in range(n):
            d = L[j, j]
            rel[j] = d / diag0[j]
            if not (d > 0.0) or not math.isfinite(d):
                return False, None, L, rel[:j + 1]
            piv[j] = np.sqrt(d)
            L[j + 1:, j] = L[j + 1:, j] / piv[j]
            col = L[j + 1:, j]
            L[j + 1:, j + 1:] = L[j + 1:, j + 1:] - np.tril(col[:, None] * col[None, :])
        for q in range(n):
            r[q] = r[q] / piv[q]
            r[q + 1:] = r[q + 1:] - L[q + 1:, q] * r[q]
        for q in range(n - 1, -1, -1):
            r[q] = r[q] / piv[q]
            r[:q] = r[:q] - L[q, :q] * r[q]
    return True, r, L, rel


def pose_update(R, t, d6):
    """ba_pose_update: R cay(w), t + d of d6 = (w, d); R (9,), t (3,) float64."""
    with np.errstate(**_ERR):
        w = [np.float64(x) for x in d6[:3]]
        n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        f = 1.0 / (1.0 + 0.25 * n2)
        W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
        Cm = [(1.0 if i == j else 0.0) + f * (W[3 * i + j] + 0.5 * (w[i] * w[j] - (n2 if i == j else 0.0))) for i in range(3) for j in range(3)]
        Rn = [(R[3 * i] * Cm[j] + R[3 * i + 1] * Cm[3 + j]) + R[3 * i + 2] * Cm[6 + j] for i in range(3) for j in range(3)]
        tn = [t[i] + d6[3 + i] for i in range(3)]
    return np.array(Rn, np.float64), np.array(tn, np.float64)


def point_step(views, nv, px, M, free, X, c, Vi, g, held, dcam):
    """ba_point_step: the candidate points (3 arrays)."""
    q = [g[0].copy(), g[1].copy(), g[2].copy()]
    with np.errstate(**_ERR):
        for w in range(nv):
            if not (free >> w) & 1 or not M[w].any():
                continue
            W = W_of(term(views[w], X, px[w][0], px[w][1], c))
            d = dcam[6 * w:6 * w + 6]
            for i in range(3):
                s = ((((W[i] * d[0] + W[3 + i] * d[1]) + W[6 + i] * d[2]) + W[9 + i] * d[3]) + W[12 + i] * d[4]) + W[15 + i] * d[5]
                q[i] = q[i] - np.where(M[w], s, 0.0)
        dx = [(Vi[0] * q[0] + Vi[1] * q[1]) + Vi[2] * q[2], (Vi[1] * q[0] + Vi[3] * q[1]) + Vi[4] * q[2], (Vi[2] * q[0] + Vi[4] * q[1]) + Vi[5] * q[2]]
        return [np.where(held, X[i], X[i] + dx[i]) for i in range(3)]


def decide(failed, cand, lam, cst, ftol=FTOL):
    """ba_decide: (accepted, lambda, cost, done)."""
    accept = (not failed) and math.isfinite(cand) and cand < cst
    if accept:
        done = cst - cand < ftol * cst
        return True, max(lam / 10.0, LAMBDA_MIN), cand, done
    return False, min(10.0 * lam, LAMBDA_MAX), cst, lam >= LAMBDA_MAX


def chunk_sum(per_track):
    """The cost of a scene from the per-track costs: block_sums per chunk of 256 tracks, the chunks added in ascending order."""
    tot = np.float64(0.0)
    for a in range(0, per_track.shape[0], 256):
        tot = tot + block_sums(per_track[a:a + 256, None])[0]
    return float(tot)


def bundle_adjust(kpts, tracks, inlier_views, points3d, n_views, Ks, Rs, ts, fixed_views=1, max_iterations=10, huber_px=1.0, ftol=None):
    """One scene: kpts (V, kcap, 2) float32, tracks (K, V), inlier_views (K,) int32, points3d (K, 3) float32, n_views an integer or None,
    Ks, Rs (V,3,3), ts (V,3).  Returns a dict: Rs, ts float64, points3d float32, refined (K,) bool, free_views int, cost (2,), info (8,)
    int32, X (K,3) float64 (the state), costs (the accepted sequence, from the initial cost on), dump (the first round's intermediate
    results) and the quantities behind decision_margin."""
    kpts = np.asarray(kpts, np.float32).astype(np.float64)
    tracks = np.asarray(tracks, np.int64)
    P0 = np.asarray(points3d, np.float32)
    V, K = kpts.shape[0], tracks.shape[0]
    nv = V if n_views is None else min(max(int(n_views), 0), V)
    c = float(huber_px)
    inl = np.asarray(inlier_views).astype(np.int64) & 0xFFFFFFFF
    Rs, ts = np.array(Rs, np.float64).reshape(V, 9), np.array(ts, np.float64).reshape(V, 3)
    Ks = np.asarray(Ks, np.float64)
    stage = lambda R, t: [stage_view(R[v], t[v], Ks[v]) for v in range(V)]      # noqa: E731
    views = stage(Rs, ts)
    px = pixels(kpts, tracks, nv)
    X = [P0[:, i].astype(np.float64) for i in range(3)]
    margins = []
    M, tie = observation_set(views, nv, px, inl, X)
    margins.append(("depth", tie))
    refined = np.any(M, axis=0) if nv else np.zeros(K, bool)
    counts = [int(M[w].sum()) if w < nv else 0 for w in range(V)]
    free = 0
    for v in range(V):
        if not (fixed_views >> v) & 1 and counts[v] >= MIN_VIEW_OBS:
            free |= 1 << v
    ct, _, tie = cost(views, nv, px, M, X, c)
    margins.append(("huber", tie))
    cst = chunk_sum(ct)
    cost0 = cst
    status = ST_NOTHING if (free == 0 or not refined.any()) else (ST_OK if math.isfinite(cst) else ST_NOT_FINITE)
    lam, done, iters, accepted = LAMBDA0, status != ST_OK, 0, 0
    costs, lambdas, dump = [cst], [], None
    ftol = FTOL if ftol is None else ftol
    if True:
        for _ in range(int(max_iterations)):
            if done:
                break
            opl = 1.0 + lam
            lambdas.append(lam)
            Vi, g, okp, rel = point_block(views, nv, px, M, X, c, opl)
            held = ~okp
            margins.append(("det", float(np.min(np.abs(rel[refined & finite(rel)]), initial=np.inf))))
            S, rhs = reduced_system(views, nv, V, px, M, X, c, opl, Vi, g, held, free)
            ok, dcam, _, rel = cholesky_solve(S, rhs)
            margins.append(("pivot", float(np.min(np.abs(rel[np.isfinite(rel)]), initial=np.inf))))
            failed, cand = not ok, 0.0
            if ok:
                Rn, tn = Rs.copy(), ts.copy()
                for v in range(V):
                    if (free >> v) & 1:
                        Rn[v], tn[v] = pose_update(Rs[v], ts[v], dcam[6 * v:6 * v + 6])
                Xn = point_step(views, nv, px, M, free, X, c, Vi, g, held, dcam)
                Xn = [np.where(refined, Xn[i], X[i]) for i in range(3)]
                vn = stage(Rn, tn)
                ct, bad, tie = cost(vn, nv, px, M, Xn, c)
                failed = bool(bad.any())
                if not failed:
                    cand = chunk_sum(ct)
                    margins.append(("huber", tie))
                    if math.isfinite(cand) and cst > 0.0:
                        margins.append(("accept", abs(cand - cst) / cst))
                        if cand < cst:
                            margins.append(("ftol", abs((cst - cand) - ftol * cst) / (ftol * cst) if ftol > 0.0 else np.inf))
            if dump is None:
                dump = dict(Vi=Vi, g=g, held=held, S=S, rhs=rhs, ok=ok, dcam=dcam, Rn=Rn if ok else None, tn=tn if ok else None,
                            Xn=Xn if ok else None, cand=cand, failed=failed,
                            terms=[term(views[w], X, px[w][0], px[w][1], c) for w in range(nv)])
            acc, lam, cst, done = decide(failed, cand, lam, cst, ftol)
            iters += 1
            if acc:
                accepted += 1
                Rs, ts, X, views = Rn, tn, Xn, vn
                costs.append(cst)
    ran = status == ST_OK
    ref = refined & ran
    with np.errstate(**_ERR):
        pts = np.where(ref[:, None], np.stack(X, axis=1).astype(np.float32), P0) if K else np.zeros((0, 3), np.float32)
    info = np.array([int(ref.sum()), int(sum(counts)), bin(free).count("1"), iters, accepted, status, 0, 0], np.int32)
    return dict(Rs=Rs.reshape(V, 3, 3), ts=ts, points3d=pts, refined=ref, free_views=free, cost=np.array([cost0, cst]), info=info,
                X=np.stack(X, axis=1) if K else np.zeros((0, 3)), costs=costs, lambdas=lambdas, margins=margins, mask=M, counts=counts, dump=dump)


def decision_margin(r):
    """The least relative distance of any decision of a bundle_adjust() result from a tie that a last-bit difference could flip: the depth
    tests of the observation set, the Huber switch of every evaluated observation, the determinant test of the point blocks (relative to
    the product of the diagonal), the pivots (relative to the diagonal entry they started from), the accept / reject comparisons and the
    FTOL test.  Above 1e-9 or so the discrete results of two bit-faithful implementations cannot differ."""
    return float(min([m for _, m in r["margins"]], default=np.inf))
