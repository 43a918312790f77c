"""Pose-graph initialisation restated in numpy float64, operation for operation (the specification is the comment at the head of the pose-graph
slice of csrc/k_triangulate.hip): the spanning tree, the rotation rounds, the position rounds, the rigidity test.  numpy's
elementwise + - * / sqrt round once each, as the device code does with fp contraction off, so tests/test_posegraph_emulated.py can ask for
equal bits.  Sums over edges go through block_sums (oracle/twoview_reference.py); the entries of a system add their edges in ascending
pair index (numpy.add.at works through its index list in order)."""
import math

import numpy as np

import bundle_reference as BR
from oracle.twoview_reference import block_sums

ST_OK, ST_NOTHING, ST_ROTATIONS_ONLY, ST_NOT_FINITE = 0, 1, 2, 3
HUBER, CAUCHY = 0, 1
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")


def finite(x):
    return (x - x) == 0.0


def mul(A, B, ta=False):
    """pg_mul on lists of 9: A B, or A' B."""
    if ta:
        return [(A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j] for i in range(3) for j in range(3)]
    return [(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def factor(x, c, kind):
    """pg_factor."""
    with np.errstate(**_ERR):
        if kind == CAUCHY:
            return (c * c) / (c * c + x * x)
        return np.where(x > c, c / x, 1.0)


def kind_of(k, iterations, redescend):
    return HUBER if k < iterations - redescend else CAUCHY


def keys(pairs, Rrel, trel, weight, nv):
    """pg_keys: (valid, has a direction) per edge."""
    a, b = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    with np.errstate(**_ERR):
        ok = (a != b) & (a >= 0) & (a < nv) & (b >= 0) & (b < nv) & finite(weight) & (weight > 0.0) & np.all(finite(Rrel.reshape(-1, 9)), axis=1)
        n2 = (trel[:, 0] * trel[:, 0] + trel[:, 1] * trel[:, 1]) + trel[:, 2] * trel[:, 2]
        has = np.all(finite(trel), axis=1) & finite(n2) & (n2 > 0.0)
    return ok, ok & has


def tree(pairs, Rrel, weight, valid, nv):
    """pg_tree: the rotations (32, 9) of the reached views, the mask, the tree's edges in the order they were taken."""
    rot = np.tile(np.eye(3).reshape(9), (32, 1))
    reg, taken = 1, []
    a, b = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    for _ in range(max(nv - 1, 0)):
        ra, rb = (reg >> np.where(valid, a, 0)) & 1, (reg >> np.where(valid, b, 0)) & 1
        cand = np.nonzero(valid & (ra != rb))[0]
        if cand.size == 0:
            break
        p = int(cand[np.argmax(weight[cand])])               # (argmax: the first of equal weights, the lowest pair index)
        Rr = list(Rrel[p].reshape(9))
        if (reg >> int(a[p])) & 1:
            rot[b[p]] = mul(Rr, list(rot[a[p]]))
            reg |= 1 << int(b[p])
        else:
            rot[a[p]] = mul(Rr, list(rot[b[p]]), ta=True)
            reg |= 1 << int(a[p])
        taken.append(p)
    return rot, reg, taken


def rot_residuals(Rrel, rot, a, b):
    """pg_rot_residual of E = R_b' (R_rel R_a) for edge arrays: r (3 arrays), |r|, the scalar part over the norm (its sign is a decision)."""
    with np.errstate(**_ERR):
        Rr = [Rrel[:, i, j] for i in range(3) for j in range(3)]
        Ra, Rb = [rot[a, k] for k in range(9)], [rot[b, k] for k in range(9)]
        E = mul(Rb, mul(Rr, Ra), ta=True)
        tr = (E[0] + E[4]) + E[8]
        c1 = tr > 0.0
        c2 = ~c1 & (E[0] > E[4]) & (E[0] > E[8])
        c3 = ~c1 & ~c2 & (E[4] > E[8])
        h1 = np.sqrt(tr + 1.0) * 2.0
        h2 = np.sqrt(((1.0 + E[0]) - E[4]) - E[8]) * 2.0
        h3 = np.sqrt(((1.0 + E[4]) - E[0]) - E[8]) * 2.0
        h4 = np.sqrt(((1.0 + E[8]) - E[0]) - E[4]) * 2.0
        sel = lambda x1, x2, x3, x4: np.where(c1, x1, np.where(c2, x2, np.where(c3, x3, x4)))      # noqa: E731
        qw = sel(0.25 * h1, (E[7] - E[5]) / h2, (E[2] - E[6]) / h3, (E[3] - E[1]) / h4)
        qx = sel((E[7] - E[5]) / h1, 0.25 * h2, (E[1] + E[3]) / h3, (E[2] + E[6]) / h4)
        qy = sel((E[2] - E[6]) / h1, (E[1] + E[3]) / h2, 0.25 * h3, (E[5] + E[7]) / h4)
        qz = sel((E[3] - E[1]) / h1, (E[2] + E[6]) / h2, (E[5] + E[7]) / h3, 0.25 * h4)
        nq = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        sg = np.where(qw < 0.0, -2.0, 2.0)
        r = [sg * (qx / nq), sg * (qy / nq), sg * (qz / nq)]
        return r, np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]), qw / nq


def laplacian(nr, ia, ib, w, r):
    """The packed triangle (dense lower, (nr, nr)) and the three right-hand sides (nr, 3) of a rotation round; ia, ib: compact indices (-1: view 0)."""
    L, rhs = np.zeros((nr, nr)), np.zeros((nr, 3))
    rows = np.stack([ia, ib, np.maximum(ia, ib)], axis=1).ravel()
    cols = np.stack([ia, ib, np.minimum(ia, ib)], axis=1).ravel()
    vals = np.stack([w, w, -w], axis=1).ravel()
    keep = np.stack([ia >= 0, ib >= 0, (ia >= 0) & (ib >= 0)], axis=1).ravel()
    np.add.at(L, (rows[keep], cols[keep]), vals[keep])
    wr = np.stack([w * r[0], w * r[1], w * r[2]], axis=1)
    rr = np.stack([ia, ib], axis=1).ravel()
    vv = np.stack([-wr, wr], axis=1).reshape(-1, 3)
    kk = rr >= 0
    np.add.at(rhs, rr[kk], vv[kk])
    return L, rhs


def directions(trel, rot, b):
    """pg_directions: d = R_b' (t_rel / |t_rel|) for edge arrays, (n, 3)."""
    with np.errstate(**_ERR):
        n = np.sqrt((trel[:, 0] * trel[:, 0] + trel[:, 1] * trel[:, 1]) + trel[:, 2] * trel[:, 2])
        u = [trel[:, 0] / n, trel[:, 1] / n, trel[:, 2] / n]
        return np.stack([(rot[b, x] * u[0] + rot[b, 3 + x] * u[1]) + rot[b, 6 + x] * u[2] for x in range(3)], axis=1)


def pos_residuals(cen, a, b, d):
    """rho of the position edges at the centres cen (32, 3)."""
    with np.errstate(**_ERR):
        e = [cen[a, x] - cen[b, x] for x in range(3)]
        pr = (d[:, 0] * e[0] + d[:, 1] * e[1]) + d[:, 2] * e[2]
        q = [e[x] - pr * d[:, x] for x in range(3)]
        return np.where(pr > 0.0, np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]), 1.0)


def pos_system(nr, ia, ib, w, d):
    """M (dense lower, (3 nr, 3 nr)) and g (3 nr,) of a position round."""
    n = 3 * nr
    M, g = np.zeros((n, n)), np.zeros(n)
    eye = np.eye(3)
    pm = w[:, None, None] * (eye[None] - d[:, :, None] * d[:, None, :])                 # (m, 3, 3)
    hi, lo = np.maximum(ia, ib), np.minimum(ia, ib)
    x, y = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    rows = np.stack([3 * ia[:, None, None] + x, 3 * ib[:, None, None] + x, 3 * hi[:, None, None] + x], axis=1)       # (m, 3 kinds, 3, 3)
    cols = np.stack([3 * ia[:, None, None] + y, 3 * ib[:, None, None] + y, 3 * lo[:, None, None] + y], axis=1)
    vals = np.stack([pm, pm, -pm], axis=1)
    low = np.broadcast_to(y <= x, pm.shape)
    keep = np.stack([(ia >= 0)[:, None, None] & low, (ib >= 0)[:, None, None] & low, np.broadcast_to(((ia >= 0) & (ib >= 0))[:, None, None], pm.shape)], axis=1)
    np.add.at(M, (rows[keep], cols[keep]), vals[keep])
    wd = w[:, None] * d
    rr = np.stack([3 * ia[:, None] + np.arange(3), 3 * ib[:, None] + np.arange(3)], axis=1)                           # (m, 2, 3)
    vv = np.stack([wd, -wd], axis=1)
    kk = np.stack([np.broadcast_to((ia >= 0)[:, None], wd.shape), np.broadcast_to((ib >= 0)[:, None], wd.shape)], axis=1)
    np.add.at(g, rr[kk], vv[kk])
    return M, g


def regularised(M, g):
    """mu and A = M + (mu g_i) g_j (dense lower)."""
    n = g.shape[0]
    trm, gg = np.float64(0.0), np.float64(0.0)
    with np.errstate(**_ERR):
        for i in range(n):
            trm = trm + M[i, i]
            gg = gg + g[i] * g[i]
        mu = trm / gg
        return mu, np.tril(M + (mu * g)[:, None] * g[None, :])


def edge_sum(x):
    return block_sums(np.ascontiguousarray(x, np.float64)[:, None])[0] if x.shape[0] else np.float64(0.0)


def average_poses(pairs, Rrel, trel, weight, n_views, V, iterations=30, redescend=10, rot_scale_rad=math.radians(2.0),
                  pos_scale_sin=math.sin(math.radians(2.0)), min_pivot_ratio=0.0):
    """One scene.  Returns a dict: Rs (V,3,3), ts (V,3), registered, edge_factor (P,2), info (8), and what the tests look at: tree (the
    edges in order), rot_tree (the rotations after the tree), dump (the first round of each solve), ratios (the smallest pivot ratio of every
    position round), margin (how close the run's decisions came to a tie, relative)."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    Rrel, trel, weight = np.asarray(Rrel, np.float64).reshape(P, 3, 3), np.asarray(trel, np.float64).reshape(P, 3), np.asarray(weight, np.float64).reshape(P)
    nv = min(max(int(n_views), 0), V)
    crot, cpos = np.float64(rot_scale_rad), np.float64(pos_scale_sin)
    valid, hasdir = keys(pairs, Rrel, trel, weight, nv)
    rot, reg, taken = tree(pairs, Rrel, weight, valid, nv)
    a, b = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    inreg = lambda v: ((reg >> np.where(valid, v, 0)) & 1).astype(bool)                 # noqa: E731
    active = valid & inreg(a) & inreg(b)
    views = [v for v in range(1, 32) if (reg >> v) & 1]
    nr = len(views)
    idx = np.full(32, -1, np.int64)
    idx[views] = np.arange(nr)
    ea = np.nonzero(active)[0]
    ia, ib = idx[a[ea]], idx[b[ea]]
    fac = np.zeros((P, 2))
    dump = dict(rot_tree=rot.copy())
    margin = dict(quat=np.inf, pivot=np.inf, half=np.inf)
    ratios = []
    last = kind_of(iterations - 1, iterations, redescend)
    pos = False
    cen = np.zeros((32, 3))
    with np.errstate(**_ERR):
        if nr > 0:
            for k in range(iterations):
                r, nrm, qs = rot_residuals(Rrel[ea], rot, a[ea], b[ea])
                margin["quat"] = min(margin["quat"], float(np.min(np.abs(qs))))
                f = factor(nrm, crot, kind_of(k, iterations, redescend))
                w = weight[ea] * f
                L, rhs = laplacian(nr, ia, ib, w, r)
                sol, ok = np.zeros((nr, 3)), True
                for x in range(3):
                    okx, sx, _, _ = BR.cholesky_solve(L, rhs[:, x])
                    ok = ok and okx
                    if okx:
                        sol[:, x] = sx
                if k == 0:
                    dump.update(rot_res=np.stack(r, axis=1), rot_factor=f.copy(), lap=L.copy(), lap_rhs=rhs.copy(), lap_ok=ok, lap_sol=sol.copy())
                if ok:
                    for i, v in enumerate(views):
                        rot[v] = BR.pose_update(rot[v], np.zeros(3), np.concatenate([sol[i], np.zeros(3)]))[0]
            r, nrm, qs = rot_residuals(Rrel[ea], rot, a[ea], b[ea])
            margin["quat"] = min(margin["quat"], float(np.min(np.abs(qs))))
            fac[ea, 0] = factor(nrm, crot, last)
            ep = np.nonzero(active & hasdir)[0]
            pa, pb = idx[a[ep]], idx[b[ep]]
            d = directions(trel[ep], rot, b[ep])
            pos = True
            f = np.ones(ep.shape[0])
            for k in range(iterations):
                if k > 0:
                    f = factor(pos_residuals(cen, a[ep], b[ep], d), cpos, kind_of(k, iterations, redescend))
                w = weight[ep] * f
                M, g = pos_system(nr, pa, pb, w, d)
                mu, A = regularised(M, g)
                if k == 0:
                    dump.update(pos_dir=d.copy(), pos_M=np.tril(M).copy(), pos_g=g.copy(), pos_mu=float(mu), pos_A=A.copy())
                if not (finite(mu) and mu > 0.0):
                    pos = False
                    break
                ok, c, _, rel = BR.cholesky_solve(A, g)
                if k == 0:
                    dump.update(pos_ok=ok, pos_sol=None if not ok else c.copy())
                if not ok:
                    ratios.append(0.0)
                    pos = False
                    break
                lo = float(np.min(rel))
                ratios.append(lo)
                if min_pivot_ratio > 0.0:
                    margin["pivot"] = min(margin["pivot"], abs(lo - min_pivot_ratio) / min_pivot_ratio)
                if not lo >= min_pivot_ratio:
                    pos = False
                    break
                cen[:] = 0.0
                cen[views] = c.reshape(nr, 3)
                e = cen[a[ep]] - cen[b[ep]]
                proj = (d[:, 0] * e[:, 0] + d[:, 1] * e[:, 1]) + d[:, 2] * e[:, 2]
                ta, tb = np.zeros(P), np.zeros(P)
                ta[ep], tb[ep] = w * proj, w
                scale = edge_sum(ta) / edge_sum(tb)
                if not (finite(scale) and scale > 0.0):
                    pos = False
                    break
                cen[views] = cen[views] / scale
                if k == 0:
                    dump.update(pos_cen=cen.copy())
            if pos:
                fac[ep, 1] = factor(pos_residuals(cen, a[ep], b[ep], d), cpos, last)
        Rs, ts = np.full((V, 3, 3), np.nan), np.full((V, 3), np.nan)
        bad = False
        for v in range(V):
            if not (reg >> v) & 1:
                continue
            R = rot[v]
            Rs[v] = R.reshape(3, 3)
            t = np.array([-((R[3 * x] * cen[v, 0] + R[3 * x + 1] * cen[v, 1]) + R[3 * x + 2] * cen[v, 2]) for x in range(3)])
            has = pos or v == 0
            if has:
                ts[v] = 0.0 if v == 0 else t
            bad = bad or not np.all(np.isfinite(R)) or (has and not np.all(np.isfinite(t)))
    part = active[:, None] & np.stack([np.ones(P, bool), hasdir], axis=1)
    n_rot = int((active & (fac[:, 0] < 0.5)).sum())
    n_pos = int((active & hasdir & (fac[:, 1] < 0.5)).sum()) if pos else 0
    if part.any():
        sel = part.copy()
        if not pos:
            sel[:, 1] = False
        if sel.any():
            margin["half"] = float(np.min(np.abs(fac[sel] - 0.5))) / 0.5
    status = ST_NOTHING if nr == 0 else (ST_NOT_FINITE if bad else (ST_OK if pos else ST_ROTATIONS_ONLY))
    info = np.array([int(valid.sum()), bin(reg).count("1"), int(hasdir.sum()), n_rot, n_pos, 3 * nr, status, 0], np.int32)
    return dict(Rs=Rs, ts=ts, registered=reg, edge_factor=fac, info=info, tree=taken, dump=dump, ratios=ratios, margin=margin, views=views,
                active=active, hasdir=hasdir, centres=cen[:V].copy())


def average_poses_batch(pairs, Rrel, trel, weight, n_views, **kw):
    """The scenes of a batch one by one: pairs (S,P,2) or (P,2), Rrel (S,P,3,3), trel (S,P,3), weight (S,P), n_views (S,)."""
    S, V = Rrel.shape[0], int(kw.pop("V"))
    out = []
    for s in range(S):
        out.append(average_poses(pairs[s] if pairs.ndim == 3 else pairs, Rrel[s], trel[s], weight[s], n_views[s], V, **kw))
    return out
