"""numpy restatement of the match verification: xfh_filter_matches (csrc/k_matchfilter.hip) and xfh_verify_matches (the
match-verify slice of csrc/k_triangulate.hip), operation for operation.  The filter is integers only; the verifier is float64 with every
product and sum rounded once, in the kernel's order: the pair by multiview_reference.stage_view (mv_stage_pose, mv_pair), the threshold and
the coordinates as pose_reference.threshold2 and pose_reference.calibrate have them (RpPair::thr2_of, RpPair::get), the error by
oracle.twoview_reference.sampson (tv::sampson)."""
import numpy as np

import multiview_reference as MR
from oracle.twoview_reference import finite, sampson

FILTER_INFO_FIELDS = ("read", "set", "emptied", "spare")
NONE, BY_KEEP, BY_MIN_KEEP = 0, 1, 2
VERIFY_INFO_FIELDS = ("status", "read", "kept", "spare")
ST_OK, ST_PAIR, ST_POSE, ST_BASELINE = 0, 1, 2, 3
_ERR = dict(all="ignore")


def filter_list(idx_a, idx_b, n, mask, keep=1, min_keep=0):
    """One list: idx_a, idx_b, mask (cap,), the count n, the list's keep flag.  Returns out_a, out_b (cap,) int64, src (cap,) int32, n_out,
    info (4,) int32."""
    idx_a, idx_b, mask = np.asarray(idx_a, np.int64), np.asarray(idx_b, np.int64), np.asarray(mask)
    cap = idx_a.shape[0]
    n = min(max(int(n), 0), cap)
    out_a, out_b, src = np.full(cap, -1, np.int64), np.full(cap, -1, np.int64), np.full(cap, -1, np.int32)
    at = 0
    for i in range(n):                                      # ascending: the order is kept
        if mask[i] != 0:
            if keep != 0:
                out_a[at], out_b[at], src[at] = idx_a[i], idx_b[i], i
            at += 1
    reason = BY_KEEP if keep == 0 else (BY_MIN_KEEP if at < min_keep else NONE)
    count = at if reason == NONE else 0
    out_a[count:], out_b[count:], src[count:] = -1, -1, -1
    return out_a, out_b, src, count, np.array([n, at, reason, 0], np.int32)


def filter_matches(idx_a, idx_b, n_matches, mask, keep=None, min_keep=0):
    """Lists of any leading shape: idx_a, idx_b, mask (..., cap), n_matches, keep (...).  Returns a dict idx_a, idx_b, src, n, info."""
    idx_a = np.asarray(idx_a, np.int64)
    lead, cap = idx_a.shape[:-1], idx_a.shape[-1]
    L = int(np.prod(lead, dtype=np.int64))
    ia, ib, mk = idx_a.reshape(L, cap), np.asarray(idx_b, np.int64).reshape(L, cap), np.asarray(mask).reshape(L, cap)
    nm = np.asarray(n_matches).reshape(L)
    kp = np.ones(L, np.uint8) if keep is None else np.asarray(keep).reshape(L)
    oa, ob, sr = np.zeros((L, cap), np.int64), np.zeros((L, cap), np.int64), np.zeros((L, cap), np.int32)
    no, info = np.zeros(L, np.int32), np.zeros((L, 4), np.int32)
    for l in range(L):
        oa[l], ob[l], sr[l], no[l], info[l] = filter_list(ia[l], ib[l], nm[l], mk[l], int(kp[l]), min_keep)
    return dict(idx_a=oa.reshape(lead + (cap,)), idx_b=ob.reshape(lead + (cap,)), src=sr.reshape(lead + (cap,)), n=no.reshape(lead),
                info=info.reshape(lead + (4,)))


def stage_pair(a, b, nv, Ks, Rs, ts, max_err):
    """vm_stage_pair: (status, E (9 scalars), cal_a, cal_b, thr2, f) of the pair (a, b) of a scene with nv views."""
    a, b = int(a), int(b)
    if a == b or not (0 <= a < nv and 0 <= b < nv):
        return ST_PAIR, None
    pb = MR.stage_view(Rs[b], ts[b], Ks[b], Rs[a], ts[a])    # mv_stage_pose of b and mv_pair(R_a, t_a, R_b, t_b)
    pa = MR.stage_view(Rs[a], ts[a], Ks[a], Rs[a], ts[a])
    if not (pa["ok"] and pb["ok"]):
        return ST_POSE, None
    if all(bool(x == 0.0) for x in pb["trel"]):
        return ST_BASELINE, None
    ca, cb = pa["cal"], pb["cal"]                            # (fx, fy, cx, cy)
    with np.errstate(**_ERR):
        f = 0.5 * ((ca[0] + ca[1]) * 0.5 + (cb[0] + cb[1]) * 0.5)
        thr = np.float64(max_err) / f
        thr2 = thr * thr
    return ST_OK, dict(E=pb["E"], ca=ca, cb=cb, thr2=thr2, f=f)


def verify_pair(kpts_a, kpts_b, idx_a, idx_b, n, st, pr):
    """One pair: the (K,2) float32 tables of its views, its lists (cap,), its count, stage_pair's result.  Returns mask (cap,) uint8,
    err (cap,) float32, info (4,) int32, r2 (cap,) float64 (NaN where not evaluated), thr2."""
    idx_a, idx_b = np.asarray(idx_a, np.int64), np.asarray(idx_b, np.int64)
    cap, K = idx_a.shape[0], kpts_a.shape[0]
    n = min(max(int(n), 0), cap)
    mask, err, r2 = np.zeros(cap, np.uint8), np.full(cap, np.nan, np.float32), np.full(cap, np.nan)
    if st != ST_OK or n == 0 or K == 0:
        return mask, err, np.array([st, n, 0, 0], np.int32), r2, np.nan
    ia, ib = idx_a[:n], idx_b[:n]
    inr = (ia >= 0) & (ia < K) & (ib >= 0) & (ib < K)
    qa = np.asarray(kpts_a, np.float32)[np.where(inr, ia, 0)].astype(np.float64)
    qb = np.asarray(kpts_b, np.float32)[np.where(inr, ib, 0)].astype(np.float64)
    ev = inr & np.isfinite(qa).all(axis=1) & np.isfinite(qb).all(axis=1)
    ca, cb = pr["ca"], pr["cb"]
    with np.errstate(**_ERR):
        x1, y1 = (qa[:, 0] - ca[2]) / ca[0], (qa[:, 1] - ca[3]) / ca[1]
        x2, y2 = (qb[:, 0] - cb[2]) / cb[0], (qb[:, 1] - cb[3]) / cb[1]
        r = sampson(pr["E"], x1, y1, x2, y2)
        m = ev & finite(r) & (r < pr["thr2"])
        e = (np.sqrt(r) * pr["f"]).astype(np.float32)
    mask[:n] = m
    err[:n] = np.where(ev, e, np.float32(np.nan))
    r2[:n] = np.where(ev, r, np.nan)
    return mask, err, np.array([st, n, int(m.sum()), 0], np.int32), r2, pr["thr2"]


def verify_matches(kpts, view_pairs, idx_a, idx_b, n_matches, n_views, Ks, Rs, ts, max_epipolar_error=1.0):
    """One scene: kpts (V,K,2) float32, view_pairs (P,2), idx_a, idx_b (P,cap), n_matches (P,), n_views or None, Ks, Rs (V,3,3), ts (V,3).
    Returns a dict mask (P,cap) uint8, err (P,cap) float32, info (P,4) int32, r2 (P,cap) float64, thr2 (P,)."""
    kpts = np.asarray(kpts, np.float32)
    V = kpts.shape[0]
    nv = V if n_views is None else min(max(int(n_views), 0), V)
    view_pairs, idx_a = np.asarray(view_pairs, np.int64).reshape(-1, 2), np.asarray(idx_a, np.int64)
    P, cap = idx_a.shape
    out = dict(mask=np.zeros((P, cap), np.uint8), err=np.zeros((P, cap), np.float32), info=np.zeros((P, 4), np.int32), r2=np.zeros((P, cap)),
               thr2=np.zeros(P))
    for p in range(P):
        a, b = view_pairs[p]
        st, pr = stage_pair(a, b, nv, Ks, Rs, ts, max_epipolar_error)
        ka, kb = (kpts[a], kpts[b]) if st == ST_OK else (kpts[0], kpts[0])
        out["mask"][p], out["err"][p], out["info"][p], out["r2"][p], out["thr2"][p] = verify_pair(ka, kb, idx_a[p], np.asarray(idx_b)[p], n_matches[p], st, pr)
    return out
