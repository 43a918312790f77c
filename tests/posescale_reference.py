"""Baseline scales from shared tracks restated in numpy float64, operation for operation (the specification is the comments of
csrc/posescale_body.hpp): the baseline ratios of the edge pairs that share a view (``baseline_ratios``) and the pose graph with
their terms in its position rounds (``average_poses``).  It stands on structure_reference's tg_* functions and on posegraph_reference's
pieces; numpy's elementwise + - * / sqrt round once each, as the device code does with fp contraction off, so
tests/test_posescale_emulated.py can ask for equal bits.  An entry of the position system adds its edges first, then its wedges in ascending
(p, q) (numpy.add.at works through its index list in order).

TEST INFRASTRUCTURE ONLY: nothing under ``accelerated_features_amd/`` imports it."""
import math

import numpy as np

import bundle_reference as BR
import posegraph_reference as PR
import structure_reference as SR

_ERR = dict(all="ignore")
ST_OK = 0


def lower_median(values):
    """Element (n - 1) // 2 of the ascending order: a selection, no average."""
    v = np.sort(np.asarray(values, np.float64))
    return v[(v.shape[0] - 1) // 2]


def shared_view(a0, b0, a1, b1):
    """ps_shared_view: the one view that two edges share, else -1."""
    n = int(a0 == a1) + int(a0 == b1) + int(b0 == a1) + int(b0 == b1)
    if n != 1 or a0 == b0 or a1 == b1:
        return -1
    return a0 if (a0 == a1 or a0 == b1) else b0


def unit_t(t):
    with np.errstate(**_ERR):
        n = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        return np.array([t[0] / n, t[1] / n, t[2] / n])


def edge_depths(kpts, pairs, Rrel, trel, Ks, p, v, rows_v, rows_o, gates):
    """ps_depth for arrays of rows: (valid, the depth in v) of the tracks with row rows_v in the shared view v and rows_o in the other view of
    edge p, triangulated under edge p in the edge's own (a, b) order."""
    a, b = int(pairs[p, 0]), int(pairs[p, 1])
    first = a == v
    o = b if first else a
    xv, xo = kpts[v][rows_v], kpts[o][rows_o]
    r = SR.triangulate(xv if first else xo, xo if first else xv, Ks[a], Ks[b], Rrel[p], unit_t(trel[p]), **gates)
    return r["valid"], (r["l0"] if first else r["l1"]), r


def baseline_ratios(kpts, tracks, track_of, pairs, Rrel, trel, weight, Ks, n_views, V, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=math.inf,
                    min_common=8):
    """One scene.  Returns a dict: ratio (P,P), count (P,P), shared_view (P,P), info (8,), and what the tests look at: values (the values of
    every wedge, in row order), margin (how close a gate of a track that was examined came to a tie, relative)."""
    kpts = np.asarray(kpts, np.float32)
    tracks, track_of = np.asarray(tracks, np.int64), np.asarray(track_of, np.int64)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P, K, T = pairs.shape[0], kpts.shape[1], tracks.shape[0]
    Rrel, trel, weight = np.asarray(Rrel, np.float64).reshape(P, 3, 3), np.asarray(trel, np.float64).reshape(P, 3), np.asarray(weight, np.float64).reshape(P)
    Ks = np.asarray(Ks, np.float64)
    nv = min(max(int(n_views), 0), V)
    valid, hasdir = PR.keys(pairs, Rrel, trel, weight, nv)
    gates = dict(max_reproj_error=max_reproj_error, min_parallax_deg=min_parallax_deg, max_depth=max_depth)
    ratio, count, shared = np.full((P, P), np.nan), np.zeros((P, P), np.int32), np.full((P, P), -1, np.int32)
    info = np.zeros(8, np.int32)
    values, margin = {}, np.inf
    for p in range(P):
        for q in range(p + 1, P):
            if not (hasdir[p] and hasdir[q]):
                continue
            v = shared_view(*[int(x) for x in pairs[p]], *[int(x) for x in pairs[q]])
            if v < 0:
                continue
            op = int(pairs[p, 1] if pairs[p, 0] == v else pairs[p, 0])
            oq = int(pairs[q, 1] if pairs[q, 0] == v else pairs[q, 0])
            t = track_of[v]
            k = np.nonzero((t >= 0) & (t < T))[0]
            rp, rq = tracks[t[k], op], tracks[t[k], oq]
            on = (rp >= 0) & (rp < K) & (rq >= 0) & (rq < K)
            k, rp, rq = k[on], rp[on], rq[on]
            okp, zp, wp = edge_depths(kpts, pairs, Rrel, trel, Ks, p, v, k, rp, gates)
            okq, zq, wq = edge_depths(kpts, pairs, Rrel, trel, Ks, q, v, k, rq, gates)
            both = okp & okq
            with np.errstate(**_ERR):
                vals = (zq / zp)[both]
            n = int(both.sum())
            if k.size:
                margin = min(margin, SR.gate_margin(wp, max_depth), SR.gate_margin(wq, max_depth))
            count[p, q], shared[p, q] = n, v
            if n >= min_common and n > 0:
                ratio[p, q] = lower_median(vals)
                info[1] += 1
            info[0] += 1
            info[2] += k.size
            info[3] += n
            values[(p, q)] = vals
    return dict(ratio=ratio, count=count, shared_view=shared, info=info, values=values, margin=margin)


def wedge_list(pairs, part, ratio, count):
    """PgRatioTerms::prepare: the wedges (p, q) that take part, ascending; part: the edge is active and has a direction."""
    a, b = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    n = ((a[:, None] == a[None]).astype(int) + (a[:, None] == b[None]) + (b[:, None] == a[None]) + (b[:, None] == b[None]))
    with np.errstate(**_ERR):
        ok = np.triu(np.ones_like(n, bool), 1) & (n == 1) & part[:, None] & part[None] & PR.finite(ratio) & (ratio > 0.0) & (count > 0)
    wp, wq = np.nonzero(ok)
    return wp, wq


def ratio_residuals(cen, a, b, d, wp, wq, r):
    """rho of the wedges at the centres cen (32, 3); d (P, 3) the directions of all edges (0 where there is none).  Also u_p, u_q."""
    with np.errstate(**_ERR):
        u = []
        for e in (wp, wq):
            ee = [cen[a[e], x] - cen[b[e], x] for x in range(3)]
            u.append((d[e, 0] * ee[0] + d[e, 1] * ee[1]) + d[e, 2] * ee[2])
        ru = r * u[1]
        dd = u[0] - ru
        rho = np.where((u[0] > 0.0) & (u[1] > 0.0), np.where(dd < 0.0, -dd, dd) / (u[0] + ru), 1.0)
    return rho, u[0], u[1]


def add_ratio_terms(M, idx, a, b, d, wp, wq, w, sr):
    """PgRatioTerms::assemble on the dense lower M (in place): every wedge adds (w h_vi[x]) h_vj[y] to the blocks of its three views."""
    m = wp.shape[0]
    if m == 0:
        return
    with np.errstate(**_ERR):
        gp, gq = d[wp] / sr[:, None], sr[:, None] * d[wq]                                     # (m, 3)
        views = np.stack([a[wp], b[wp], a[wq], b[wq]], axis=1)                               # (m, 4): the shared view twice
        cp = (views == a[wp][:, None]).astype(np.float64) - (views == b[wp][:, None]).astype(np.float64)
        cq = (views == a[wq][:, None]).astype(np.float64) - (views == b[wq][:, None]).astype(np.float64)
        h = cp[:, :, None] * gp[:, None, :] - cq[:, :, None] * gq[:, None, :]                # (m, 4, 3)
        first = np.ones((m, 4), bool)                                                        # every view once: drop its second occurrence
        for j in range(1, 4):
            for i in range(j):
                first[:, j] &= views[:, j] != views[:, i]
        ii = np.where(first, idx[views], -1)                                                 # (m, 4) compact indices, -1: none
        vals = (w[:, None, None, None, None] * h[:, :, None, :, None]) * h[:, None, :, None, :]     # (m, vi, vj, x, y)
        x, y = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
        I, J = ii[:, :, None, None, None], ii[:, None, :, None, None]
        rows, cols = np.broadcast_to(3 * I + x, vals.shape), np.broadcast_to(3 * J + y, vals.shape)
        keep = np.broadcast_to((I >= 0) & (J >= 0) & ((I > J) | ((I == J) & (y <= x))), vals.shape)
        np.add.at(M, (rows[keep], cols[keep]), vals[keep])


def average_poses(pairs, Rrel, trel, weight, n_views, V, ratio=None, ratio_count=None, scale_weight=1.0, scale_tol=0.1, iterations=30, redescend=10,
                  rot_scale_rad=math.radians(2.0), pos_scale_sin=math.sin(math.radians(2.0)), min_pivot_ratio=0.0):
    """One scene: posegraph_reference.average_poses with the ratio terms (pg_run_with<PgRatioTerms>); ratio None: no wedge takes part.
    Returns its dict with ratio_factor (P,P), wedges (the list) and the margins ratio_half and ratio_u added."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    Rrel, trel, weight = np.asarray(Rrel, np.float64).reshape(P, 3, 3), np.asarray(trel, np.float64).reshape(P, 3), np.asarray(weight, np.float64).reshape(P)
    nv = min(max(int(n_views), 0), V)
    crot, cpos, ctol = np.float64(rot_scale_rad), np.float64(pos_scale_sin), np.float64(scale_tol)
    valid, hasdir = PR.keys(pairs, Rrel, trel, weight, nv)
    rot, reg, taken = PR.tree(pairs, Rrel, weight, valid, nv)
    a, b = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    inreg = lambda v: ((reg >> np.where(valid, v, 0)) & 1).astype(bool)                 # noqa: E731
    active = valid & inreg(a) & inreg(b)
    views = [v for v in range(1, 32) if (reg >> v) & 1]
    nr = len(views)
    idx = np.full(32, -1, np.int64)
    idx[views] = np.arange(nr)
    ea = np.nonzero(active)[0]
    ia, ib = idx[a[ea]], idx[b[ea]]
    fac, rfac = np.zeros((P, 2)), np.zeros((P, P))
    if ratio is None:
        wp = wq = np.zeros(0, np.int64)
        wr = wsr = wbase = np.zeros(0)
    else:
        ratio, ratio_count = np.asarray(ratio, np.float64).reshape(P, P), np.asarray(ratio_count, np.int32).reshape(P, P)
        wp, wq = wedge_list(pairs, active & hasdir, ratio, ratio_count)
        wr = ratio[wp, wq]
        wsr = np.sqrt(wr)
        wbase = np.float64(scale_weight) * ratio_count[wp, wq].astype(np.float64)
    dump = dict(rot_tree=rot.copy())
    margin = dict(quat=np.inf, pivot=np.inf, half=np.inf, ratio_half=np.inf, ratio_u=np.inf)
    ratios = []
    last = PR.kind_of(iterations - 1, iterations, redescend)
    pos = False
    cen = np.zeros((32, 3))
    dall = np.zeros((P, 3))

    def wedge_factor(kind):
        rho, up, uq = ratio_residuals(cen, a, b, dall, wp, wq, wr)
        if wp.size:
            margin["ratio_u"] = min(margin["ratio_u"], float(np.min(np.abs(np.r_[up, uq]))))
        return PR.factor(rho, ctol, kind)

    with np.errstate(**_ERR):
        if nr > 0:
            for k in range(iterations):
                r, nrm, qs = PR.rot_residuals(Rrel[ea], rot, a[ea], b[ea])
                margin["quat"] = min(margin["quat"], float(np.min(np.abs(qs))))
                f = PR.factor(nrm, crot, PR.kind_of(k, iterations, redescend))
                L, rhs = PR.laplacian(nr, ia, ib, weight[ea] * f, r)
                sol, ok = np.zeros((nr, 3)), True
                for x in range(3):
                    okx, sx, _, _ = BR.cholesky_solve(L, rhs[:, x])
                    ok = ok and okx
                    if okx:
                        sol[:, x] = sx
                if ok:
                    for i, v in enumerate(views):
                        rot[v] = BR.pose_update(rot[v], np.zeros(3), np.concatenate([sol[i], np.zeros(3)]))[0]
            r, nrm, qs = PR.rot_residuals(Rrel[ea], rot, a[ea], b[ea])
            margin["quat"] = min(margin["quat"], float(np.min(np.abs(qs))))
            fac[ea, 0] = PR.factor(nrm, crot, last)
            ep = np.nonzero(active & hasdir)[0]
            pa, pb = idx[a[ep]], idx[b[ep]]
            d = PR.directions(trel[ep], rot, b[ep])
            dall[ep] = d
            pos = True
            f, fw = np.ones(ep.shape[0]), np.ones(wp.shape[0])
            for k in range(iterations):
                if k > 0:
                    kind = PR.kind_of(k, iterations, redescend)
                    f = PR.factor(PR.pos_residuals(cen, a[ep], b[ep], d), cpos, kind)
                    fw = wedge_factor(kind)
                w, ww = weight[ep] * f, wbase * fw
                M, g = PR.pos_system(nr, pa, pb, w, d)
                add_ratio_terms(M, idx, a, b, dall, wp, wq, ww, wsr)
                mu, A = PR.regularised(M, g)
                if k == 0:
                    dump.update(pos_dir=d.copy(), pos_M=np.tril(M).copy(), pos_g=g.copy(), pos_mu=float(mu), pos_A=A.copy())
                if not (PR.finite(mu) and mu > 0.0):
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
                scale = PR.edge_sum(ta) / PR.edge_sum(tb)
                if not (PR.finite(scale) and scale > 0.0):
                    pos = False
                    break
                cen[views] = cen[views] / scale
                if k == 0:
                    dump.update(pos_cen=cen.copy())
            if pos:
                fac[ep, 1] = PR.factor(PR.pos_residuals(cen, a[ep], b[ep], d), cpos, last)
                rfac[wp, wq] = wedge_factor(last)
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
    n_rot = int((active & (fac[:, 0] < 0.5)).sum())
    n_pos = int((active & hasdir & (fac[:, 1] < 0.5)).sum()) if pos else 0
    sel = np.stack([active, active & hasdir & pos], axis=1)
    if sel.any():
        margin["half"] = float(np.min(np.abs(fac[sel] - 0.5))) / 0.5
    if pos and wp.size:
        margin["ratio_half"] = float(np.min(np.abs(rfac[wp, wq] - 0.5))) / 0.5
    status = PR.ST_NOTHING if nr == 0 else (PR.ST_NOT_FINITE if bad else (PR.ST_OK if pos else PR.ST_ROTATIONS_ONLY))
    info = np.array([int(valid.sum()), bin(reg).count("1"), int(hasdir.sum()), n_rot, n_pos, 3 * nr, status, 0], np.int32)
    return dict(Rs=Rs, ts=ts, registered=reg, edge_factor=fac, ratio_factor=rfac, info=info, tree=taken, dump=dump, ratios=ratios, margin=margin,
                views=views, active=active, hasdir=hasdir, centres=cen[:V].copy(), wedges=(wp, wq))
