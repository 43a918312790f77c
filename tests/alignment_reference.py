"""float64 numpy restatement of the 3D-3D alignment estimator of csrc/k_align.hip: RANSAC over a 3-point similarity (or
rigid) solver, B ~= s R A + t, with an MSAC score on the point distance, the sequential loop's stopping rule and a closed-form refit of the
consensus set (Horn's quaternion method, the symmetric 4x4 matrix diagonalised by a fixed number of cyclic Jacobi sweeps).

It performs the kernel's operations in the kernel's order (numpy never fuses a multiply and an add, and every product and sum here is
rounded once, as in the kernel's file with fp contraction off), vectorised over hypotheses, so its results are comparable bit for bit:
the model of a sample (``solve``), the fit of a set of centred sums (``fit``), the integer costs, the winner, the iteration count, the
mask and -- because the refit's sums are formed in the select kernel's fixed block order -- the refitted model.  The one function outside
+ - * / sqrt is the bound's log, as in the kernel.

Here is what only this estimator has: the solver, the residual, the refit.  The draws, the stopping rule, the fixed-order sums and the
shared geometry are oracle/twoview_reference.py's, the triangle frame is the absolute pose's (tests/abspose_reference.py::frame, which
restates tv::triangle_frame); the synthetic scenes are tests/alignment_support.py's.
"""
import math

import numpy as np

from oracle import twoview_reference as TR
from oracle.twoview_reference import block_sums, dot, finite

import abspose_reference as AR
from abspose_reference import frame

SAMPLE, LO_ITERS, MAX_ITERS, MODEL_DOUBLES, JACOBI_SWEEPS = 3, 10, 16384, 13, 8
COLLINEAR_EPS2 = 1e-8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
assert AR.COLLINEAR_EPS2 == COLLINEAR_EPS2          # frame() applies the absolute pose's constant: the two solvers share the test


def cost(r2, thr2):
    m = np.where(r2 < thr2, r2, thr2)
    return np.floor(m / thr2 * 1048576.0).astype(np.int64)


def residual2(sR, t, a0, a1, a2, b0, b1, b2):
    """|b - ((sR) a + t)|^2 (sR a list of 9, t a list of 3; arrays broadcast)."""
    d0 = b0 - (((sR[0] * a0 + sR[1] * a1) + sR[2] * a2) + t[0])
    d1 = b1 - (((sR[3] * a0 + sR[4] * a1) + sR[5] * a2) + t[1])
    d2 = b2 - (((sR[6] * a0 + sR[7] * a1) + sR[8] * a2) + t[2])
    return (d0 * d0 + d1 * d1) + d2 * d2


def scaled_rotation(model):
    """sR (list of 9) of a model (..., 13) = R, t, s."""
    return [model[..., 12] * model[..., k] for k in range(9)]


def finish(R, s, ca, cb):
    """t = cb - s (R ca) and whether everything in the model is finite: (t list of 3, ok)."""
    t = [cb[i] - s * ((R[3 * i] * ca[0] + R[3 * i + 1] * ca[1]) + R[3 * i + 2] * ca[2]) for i in range(3)]
    ok = finite(s)
    for v in t + list(R):
        ok = ok & finite(v)
    return t, ok


# ---- the minimal solver -------------------------------------------------------------------------------------------------------------------
def solve(A, B, with_scale=True):
    """Models of H samples: A, B (H, 3, 3) point-major.  Returns (model (H, 13) = R row-major, t, s; zeros where there is none, ok (H,))."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    H = A.shape[0]
    with np.errstate(all="ignore"):
        ok = finite(A).all(axis=(1, 2)) & finite(B).all(axis=(1, 2))
        PA = [[A[:, i, k] for k in range(3)] for i in range(3)]
        PB = [[B[:, i, k] for k in range(3)] for i in range(3)]
        ea1, ea2, ea3, oka = frame(PA[0], PA[1], PA[2])
        eb1, eb2, eb3, okb = frame(PB[0], PB[1], PB[2])
        ok &= oka & okb
        ea, eb = [ea1, ea2, ea3], [eb1, eb2, eb3]
        R = [(eb[0][i] * ea[0][j] + eb[1][i] * ea[1][j]) + eb[2][i] * ea[2][j] for i in range(3) for j in range(3)]
        ca = [((PA[0][k] + PA[1][k]) + PA[2][k]) / 3.0 for k in range(3)]
        cb = [((PB[0][k] + PB[1][k]) + PB[2][k]) / 3.0 for k in range(3)]
        na, nb = [], []
        for i in range(3):
            da = [PA[i][k] - ca[k] for k in range(3)]
            db = [PB[i][k] - cb[k] for k in range(3)]
            na.append(dot(da, da))
            nb.append(dot(db, db))
        va, vb = (na[0] + na[1]) + na[2], (nb[0] + nb[1]) + nb[2]
        ok &= (va > 0.0) & (vb > 0.0)
        s = np.sqrt(vb / va) if with_scale else np.ones(H)
        t, fin = finish(R, s, ca, cb)
        ok &= fin
        model = np.stack(R + t + [s], axis=-1)
    return np.where(ok[:, None], model, 0.0), ok


# ---- the closed-form fit ------------------------------------------------------------------------------------------------------------------
def fit(S, ca, cb, with_scale=True):
    """The least-squares model of consensus sets from their centred sums: S (H, 10) = sum x_i y_j (row-major), then sum |x|^2, with
    x = A - ca, y = B - cb; ca, cb (H, 3).  Returns (model (H, 13), ok (H,))."""
    S, ca, cb = (np.asarray(v, np.float64) for v in (S, ca, cb))
    H = S.shape[0]
    S = [S[:, k] for k in range(10)]
    with np.errstate(all="ignore"):
        N = [[None] * 4 for _ in range(4)]
        N[0][0] = (S[0] + S[4]) + S[8]
        N[1][1] = (S[0] - S[4]) - S[8]
        N[2][2] = (S[4] - S[0]) - S[8]
        N[3][3] = (S[8] - S[0]) - S[4]
        N[0][1], N[0][2], N[0][3] = S[5] - S[7], S[6] - S[2], S[1] - S[3]
        N[1][2], N[1][3], N[2][3] = S[1] + S[3], S[6] + S[2], S[5] + S[7]
        for i in range(4):
            for j in range(i):
                N[i][j] = N[j][i]
        V = [[np.full(H, 1.0 if i == j else 0.0) for j in range(4)] for i in range(4)]
        for _ in range(JACOBI_SWEEPS):
            for p, q in PAIRS:
                apq = N[p][q]
                go = apq != 0.0
                theta = (N[q][q] - N[p][p]) / (2.0 * apq)
                at = np.abs(theta) + np.sqrt(theta * theta + 1.0)
                t = np.where(theta >= 0.0, 1.0, -1.0) / at
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                npp, nqq = N[p][p] - t * apq, N[q][q] + t * apq
                N[p][p], N[q][q] = np.where(go, npp, N[p][p]), np.where(go, nqq, N[q][q])
                N[p][q] = N[q][p] = np.where(go, 0.0, apq)
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = N[k][p], N[k][q]
                        N[k][p] = N[p][k] = np.where(go, c * akp - s * akq, akp)
                        N[k][q] = N[q][k] = np.where(go, s * akp + c * akq, akq)
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = np.where(go, c * vkp - s * vkq, vkp)
                    V[k][q] = np.where(go, s * vkp + c * vkq, vkq)
        lam, qv = N[0][0], [V[i][0] for i in range(4)]
        for k in range(1, 4):
            up = N[k][k] > lam
            lam = np.where(up, N[k][k], lam)
            qv = [np.where(up, V[i][k], qv[i]) for i in range(4)]
        ww, xx, yy, zz = qv[0] * qv[0], qv[1] * qv[1], qv[2] * qv[2], qv[3] * qv[3]
        nq = ((ww + xx) + yy) + zz
        wx, wy, wz, xy, xz, yz = qv[0] * qv[1], qv[0] * qv[2], qv[0] * qv[3], qv[1] * qv[2], qv[1] * qv[3], qv[2] * qv[3]
        R = [(((ww + xx) - yy) - zz) / nq, (2.0 * (xy - wz)) / nq, (2.0 * (xz + wy)) / nq,
             (2.0 * (xy + wz)) / nq, (((ww - xx) + yy) - zz) / nq, (2.0 * (yz - wx)) / nq,
             (2.0 * (xz - wy)) / nq, (2.0 * (yz + wx)) / nq, (((ww - xx) - yy) + zz) / nq]
        if with_scale:
            r = [(R[3 * i] * S[i] + R[3 * i + 1] * S[3 + i]) + R[3 * i + 2] * S[6 + i] for i in range(3)]
            sc = ((r[0] + r[1]) + r[2]) / S[9]
        else:
            sc = np.ones(H)
        ok = sc > 0.0
        t, fin = finish(R, sc, [ca[:, k] for k in range(3)], [cb[:, k] for k in range(3)])
        ok = ok & fin
        model = np.stack(R + t + [sc], axis=-1)
    return np.where(ok[:, None], model, 0.0), ok


def centred_terms(C, inl, ca, cb):
    """The 10 per-correspondence terms of the refit's second pass (zeros off the consensus set `inl`)."""
    with np.errstate(all="ignore"):
        x = [C[k] - ca[k] for k in range(3)]
        y = [C[3 + k] - cb[k] for k in range(3)]
        T = np.zeros((len(inl), 10))
        for i in range(3):
            for j in range(3):
                T[:, 3 * i + j] = np.where(inl, x[i] * y[j], 0.0)
        T[:, 9] = np.where(inl, dot(x, x), 0.0)
    return T


def fit_points(A, B, with_scale=True):
    """al_fit of one cloud A -> B (n, 3), all points in the consensus set, with the sums in the select kernel's order: (model (13,), ok)."""
    C = correspondences(A, B, fp32=False)
    n = C[0].shape[0]
    inl = np.ones(n, bool)
    s1 = block_sums(np.stack(C, axis=-1))
    ca, cb = [float(s1[k]) / float(n) for k in range(3)], [float(s1[3 + k]) / float(n) for k in range(3)]
    s2 = block_sums(centred_terms(C, inl, ca, cb))
    m, ok = fit(s2[None], np.array(ca)[None], np.array(cb)[None], with_scale)
    return m[0], bool(ok[0])


# ---- sampling, the estimator ----------------------------------------------------------------------------------------------------------------
def correspondences(pts_a, pts_b, fp32=True):
    """(a0, a1, a2, b0, b1, b2), each (n,) fp64, of two (n, 3) point lists (through fp32, as the kernel reads them)."""
    a, b = np.asarray(pts_a), np.asarray(pts_b)
    if fp32:
        a, b = a.astype(np.float32), b.astype(np.float32)
    a, b = a.astype(np.float64).reshape(-1, 3), b.astype(np.float64).reshape(-1, 3)
    return (a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2])


def hypotheses(C, seed, pair, its, thr2, with_scale):
    """Costs (H, 1) int64, inlier counts (H, 1), models (H, 1, 13), ncand (H,) in {0, 1}."""
    n = C[0].shape[0]
    idx, ok = TR.sample_distinct(seed, pair, its, n, SAMPLE)
    ii = np.where(ok[:, None], idx, 0)
    model, okm = solve(np.stack([C[0][ii], C[1][ii], C[2][ii]], axis=-1), np.stack([C[3][ii], C[4][ii], C[5][ii]], axis=-1), with_scale)
    nc = (ok & okm).astype(np.int64)
    H = len(its)
    costs, cnts = np.full((H, 1), -1, np.int64), np.zeros((H, 1), np.int64)
    sel = np.nonzero(nc)[0]
    if len(sel):
        with np.errstate(all="ignore"):
            sR = [v[:, None] for v in scaled_rotation(model[sel])]
            t = [model[sel, 9 + k][:, None] for k in range(3)]
            r2 = residual2(sR, t, *(c[None] for c in C))
            costs[sel, 0] = cost(r2, thr2).sum(axis=1)
            cnts[sel, 0] = (r2 < thr2).sum(axis=1)
    return costs, cnts, model[:, None], nc


def estimate(pts_a, pts_b, max_error, with_scale=True, success_prob=0.9999, min_iterations=20, max_iterations=1000, seed=0, pair=0):
    """One pair.  Returns dict R (3,3), t (3,), s, mask (n,) uint8, info (8,) int (found, best_it, iters, n_inliers, lo_accepted, n,
    cost_lo, cost_hi) -- the kernel's outputs for this pair (`pair` = its index in the batch, which enters the draws)."""
    C = correspondences(pts_a, pts_b)
    n = C[0].shape[0]
    thr2 = float(max_error) * float(max_error)
    log1mp = math.log(1.0 - success_prob)
    zero = dict(R=np.zeros((3, 3)), t=np.zeros(3), s=0.0, mask=np.zeros(n, np.uint8))
    if n < SAMPLE:
        return dict(zero, info=np.array([0, -1, 0, 0, 0, n, 0, 0]))
    best, _, best_model, it = TR.stopping_rule(lambda its: hypotheses(C, seed, pair, its, thr2, with_scale), n, log1mp, max_iterations, SAMPLE,
                                               lower=True, min_iters=min_iterations)
    if best < 0:
        return dict(zero, info=np.array([0, -1, it, 0, 0, n, 0, 0]))
    cur = np.array(best_model, np.float64)
    bst, c_best, lo = cur, None, 0
    with np.errstate(all="ignore"):
        for step in range(LO_ITERS + 1):
            sR, t = [float(v) for v in scaled_rotation(cur)], [float(v) for v in cur[9:12]]
            r2 = residual2(sR, t, *C)
            inl = r2 < thr2
            c_now, n_cur = int(cost(r2, thr2).sum()), int(inl.sum())
            s1 = block_sums(np.where(inl[:, None], np.stack(C, axis=-1), 0.0))
            if step > 0 and not c_now < c_best:
                break
            bst = cur
            if step > 0:
                lo += 1
            c_best = c_now
            if step == LO_ITERS or n_cur < 3:
                break
            ca, cb = [float(s1[k]) / float(n_cur) for k in range(3)], [float(s1[3 + k]) / float(n_cur) for k in range(3)]
            s2 = block_sums(centred_terms(C, inl, ca, cb))
            m, ok = fit(s2[None], np.array(ca)[None], np.array(cb)[None], with_scale)
            if not ok[0]:
                break
            cur = m[0]
        sR, t = [float(v) for v in scaled_rotation(bst)], [float(v) for v in bst[9:12]]
        m = residual2(sR, t, *C) < thr2
    n_in = int(m.sum())
    found = n_in >= SAMPLE
    info = np.array([int(found), best, it, n_in, lo, n, *TR.info_words(c_best)])
    if not found:
        return dict(zero, info=info)
    return dict(R=bst[:9].reshape(3, 3).copy(), t=bst[9:12].copy(), s=float(bst[12]), mask=m.astype(np.uint8), info=info)
