"""float64 numpy restatement of the absolute-pose estimator of csrc/k_abspose.hip: P3P RANSAC (the classical quartic in
a depth ratio) with an MSAC score on the reprojection error, the sequential loop's stopping rule, Gauss-Newton refinement of the winner.

It performs the kernel's operations in the kernel's order (numpy never fuses a multiply and an add, and every product and sum here is
rounded once, as in the kernel's file with fp contraction off), vectorised over hypotheses, so its results are comparable bit for bit:
the candidate poses of a sample (``solve``), the integer costs, the winner, the iteration count, the mask and -- because the
refinement's sums are formed in the select kernel's fixed block order -- the refined pose.  The one function outside + - * / sqrt is
the bound's log, as in the kernel.

Here is what only this estimator has: the P3P solver, the reprojection residual, the 6-parameter refinement.  The draws, the stopping
rule, the fixed-order sums and the shared geometry are oracle/twoview_reference.py's; the synthetic scenes are tests/abspose_support.py's.
"""
import math

import numpy as np

from oracle import twoview_reference as TR
from oracle.twoview_reference import block_sums, cross, dot, finite, pmul

SAMPLE, LO_ITERS, MAX_ITERS, MAX_CAND, NSUM = 3, 10, 16384, 4, 27
STURM_STEPS, SIGN_STEPS, NEWTON_STEPS, POLISH_STEPS = 48, 48, 4, 3
LEAD_EPS, DEN_EPS, COLLINEAR_EPS2, SQFREE_EPS, RES_EPS = 1e-12, 1e-12, 1e-8, 1e-9, 1e-10
BEHIND = 1e300               # the squared residual of a point that is not in front of the camera


def cost(r2, thr2):
    m = np.where(r2 < thr2, r2, thr2)
    return np.floor(m / thr2 * 1048576.0).astype(np.int64)


def horner(a, x):
    """a: list of coefficient arrays (ascending powers)."""
    v = a[-1]
    for c in a[-2::-1]:
        v = v * x + c
    return v


def residual2(R, t, x, y, X0, X1, X2):
    """Squared reprojection error (R a list of 9, t a list of 3; arrays broadcast); BEHIND where Y_z > 0 does not hold."""
    Y0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0]
    Y1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1]
    Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2]
    iz = 1.0 / Y2
    dx, dy = x - Y0 * iz, y - Y1 * iz
    return np.where(Y2 > 0.0, dx * dx + dy * dy, BEHIND)


def frame(A, B, Cc):
    """(e1, e2, e3, ok) of the triangle (A, B, Cc), each a list of 3 arrays."""
    d1 = [B[k] - A[k] for k in range(3)]
    d2 = [Cc[k] - A[k] for k in range(3)]
    n1 = dot(d1, d1)
    r1 = np.sqrt(n1)
    e1 = [d1[k] / r1 for k in range(3)]
    c = cross(e1, d2)
    n3, n2 = dot(c, c), dot(d2, d2)
    r3 = np.sqrt(n3)
    e3 = [c[k] / r3 for k in range(3)]
    e2 = cross(e3, e1)
    return e1, e2, e3, (n1 > 0.0) & (n3 > COLLINEAR_EPS2 * n2)


def sturm(p):
    """(the Sturm sequence [s0 .. s4] of the monic form of the quartic p (5 arrays, ascending), Cauchy bound, ok) -- the kernel's ApSturm."""
    lead = p[4]
    ok = (np.abs(lead) >= LEAD_EPS) & finite(lead)
    s0 = [p[k] / lead for k in range(4)] + [np.ones_like(lead)]
    bound = np.zeros_like(lead)
    for k in range(4):
        av = np.abs(s0[k])
        bound = np.where(av > bound, av, bound)
    bound = 1.0 + bound
    seq = [s0, [float(k + 1) * s0[k + 1] for k in range(4)]]
    for d in range(3, 0, -1):
        a, b = seq[-2], seq[-1]
        q1 = a[d + 1] / b[d]
        q0 = (a[d] - q1 * b[d - 1]) / b[d]
        seq.append([-((a[0] if i == 0 else a[i] - q1 * b[i - 1]) - q0 * b[i]) for i in range(d)])
    s2, s3 = seq[2], seq[3]                      # a last term that is all cancellation: its sign is noise (quartic_roots picks it)
    q1 = s2[2] / s3[1]
    q0 = (s2[1] - q1 * s3[0]) / s3[1]
    noise = np.abs(seq[4][0]) <= SQFREE_EPS * (np.abs(s2[0]) + np.abs(q0 * s3[0]))
    fin = finite(bound)
    for s in seq:
        for c in s:
            fin = fin & finite(c)
    return seq, bound, ok & fin, noise


def quartic_roots(p):
    """Real roots of the quartics p (5 arrays (H,), ascending powers) as the kernel isolates them: (roots (H, 4) ascending, their number
    (H,), ok (H,))."""
    with np.errstate(all="ignore"):
        p = [np.asarray(c, np.float64) for c in p]
        H = p[0].shape[0]
        seq, bound, ok, noise = sturm(p)

        def changes(x):           # x (H, 4)
            n = np.zeros(x.shape, np.int64)
            have = np.zeros(x.shape, bool)
            prev = np.zeros(x.shape, bool)
            for s in seq:
                v = horner([c[:, None] for c in s], x) if len(s) > 1 else np.broadcast_to(s[0][:, None], x.shape)
                nz = v != 0.0
                g = v > 0.0
                n += (have & nz & (g != prev)).astype(np.int64)
                prev = np.where(nz, g, prev)
                have = have | nz
            return n

        bb = np.repeat(bound[:, None], 4, axis=1)
        s4 = seq[4][0]                               # a last term that is noise takes the sign that counts more real roots (the positive one on ties)
        seq[4] = [np.abs(s4)]
        n_pos = (changes(-bb) - changes(bb))[:, 0]
        seq[4] = [-np.abs(s4)]
        n_neg = (changes(-bb) - changes(bb))[:, 0]
        seq[4] = [np.where(noise, np.where(n_neg > n_pos, -np.abs(s4), np.abs(s4)), s4)]
        v_lo, v_hi = changes(-bb), changes(bb)
        nroots = np.clip(v_lo - v_hi, 0, 4)[:, 0]
        kk = np.arange(4)[None, :]
        lo, hi = -bb, bb.copy()
        for _ in range(STURM_STEPS):
            mid = 0.5 * (lo + hi)
            cnd = (v_lo - changes(mid)) > kk
            hi = np.where(cnd, mid, hi)
            lo = np.where(cnd, lo, mid)
        s0c = [c[:, None] for c in seq[0]]
        flo, fhi = horner(s0c, lo), horner(s0c, hi)
        doit = (flo > 0.0) != (fhi > 0.0)
        slo = flo > 0.0
        for _ in range(SIGN_STEPS):
            mid = 0.5 * (lo + hi)
            cnd = (horner(s0c, mid) > 0.0) == slo
            lo = np.where(doit & cnd, mid, lo)
            hi = np.where(doit & ~cnd, mid, hi)
        z = 0.5 * (lo + hi)
        s1c = [c[:, None] for c in seq[1]]
        for _ in range(NEWTON_STEPS):
            f, df = horner(s0c, z), horner(s1c, z)
            zn = z - f / df
            z = np.where(np.abs(horner(s0c, zn)) < np.abs(f), zn, z)
    return z, np.where(ok, nroots, 0), ok


def polish(u, v, ra, rc, ca, cg, q1):
    """POLISH_STEPS Newton steps on the two cosine-law equations F1 = u^2 + v^2 - 2 ca u v - ra q(v), F2 = 1 + u^2 - 2 cg u - rc q(v) in
    (u, v), each kept only if it lowers |F1| + |F2|; the third result: |F1| + |F2| <= RES_EPS at the end."""
    def F(u, v):
        qv = (v + q1) * v + 1.0
        return ((u * u + v * v) - (2.0 * ca) * (u * v)) - ra * qv, ((1.0 + u * u) - (2.0 * cg) * u) - rc * qv
    for _ in range(POLISH_STEPS):
        F1, F2 = F(u, v)
        dq = 2.0 * v + q1
        a11, a12 = 2.0 * u - (2.0 * ca) * v, (2.0 * v - (2.0 * ca) * u) - ra * dq
        a21, a22 = 2.0 * u - 2.0 * cg, -(rc * dq)
        det = a11 * a22 - a12 * a21
        un = u - (F1 * a22 - F2 * a12) / det
        vn = v - (a11 * F2 - a21 * F1) / det
        G1, G2 = F(un, vn)
        take = (np.abs(G1) + np.abs(G2)) < (np.abs(F1) + np.abs(F2))
        u, v = np.where(take, un, u), np.where(take, vn, v)
    F1, F2 = F(u, v)
    return u, v, (np.abs(F1) + np.abs(F2)) <= RES_EPS


# ---- the minimal solver -------------------------------------------------------------------------------------------------------------------
def solve(x, y, X):
    """Candidate poses of H samples: x, y (H, 3) normalised image coordinates, X (H, 3, 3) the 3D points (point-major).  Returns
    (cand (H, 4, 12) = R row-major + t, ncand (H,))."""
    x, y, X = (np.asarray(v, np.float64) for v in (x, y, X))
    H = x.shape[0]
    with np.errstate(all="ignore"):
        ok = finite(x).all(axis=1) & finite(y).all(axis=1) & finite(X).all(axis=(1, 2))
        f = []
        for i in range(3):
            nn = np.sqrt((x[:, i] * x[:, i] + y[:, i] * y[:, i]) + 1.0)
            f.append([x[:, i] / nn, y[:, i] / nn, 1.0 / nn])
        P = [[X[:, i, k] for k in range(3)] for i in range(3)]
        sub = lambda a, b: [a[k] - b[k] for k in range(3)]      # noqa: E731
        d23, d13, d12 = sub(P[1], P[2]), sub(P[0], P[2]), sub(P[0], P[1])
        a2, b2, c2 = dot(d23, d23), dot(d13, d13), dot(d12, d12)
        ok &= b2 > 0.0
        ra, rc = a2 / b2, c2 / b2
        ca, cb, cg = dot(f[1], f[2]), dot(f[0], f[2]), dot(f[0], f[1])
        ep1, ep2, ep3, okp = frame(P[0], P[1], P[2])
        ok &= okp
        q1 = -2.0 * cb
        kq = rc - ra
        N = [kq - 1.0, kq * q1, 1.0 + kq]
        D = [-(2.0 * cg), 2.0 * ca]
        g = [1.0 - rc, -(rc * q1), -rc]
        m = 2.0 * cg
        NN, ND, DD = pmul(N, N), pmul(N, D), pmul(D, D)
        gDD = pmul(g, DD)
        p = [(NN[k] - m * ND[k]) + gDD[k] for k in range(4)] + [NN[4] + gDD[4]]
        z, nroots, okr = quartic_roots(p)
        ok &= okr
        kk = np.arange(4)[None, :]
        valid = ok[:, None] & (kk < nroots[:, None])
        col = lambda a: a[:, None]      # noqa: E731
        v = z
        Dv = col(D[1]) * v + col(D[0])
        Nv = (col(N[2]) * v + col(N[1])) * v + col(N[0])
        valid &= np.abs(Dv) >= DEN_EPS
        u = Nv / Dv
        u, v, solved = polish(u, v, col(ra), col(rc), col(ca), col(cg), col(q1))
        valid &= solved
        qv = (v + col(q1)) * v + 1.0
        valid &= (v > 0.0) & (u > 0.0) & (qv > 0.0)
        s1 = np.sqrt(col(b2) / qv)
        sd = [s1, u * s1, v * s1]
        Cp = [[sd[i] * col(f[i][j]) for j in range(3)] for i in range(3)]
        ec1, ec2, ec3, okc = frame(Cp[0], Cp[1], Cp[2])
        valid &= okc
        ec, ep = [ec1, ec2, ec3], [[col(c) for c in e] for e in (ep1, ep2, ep3)]
        R = [(ec[0][i] * ep[0][j] + ec[1][i] * ep[1][j]) + ec[2][i] * ep[2][j] for i in range(3) for j in range(3)]
        t = [Cp[0][i] - ((R[3 * i] * col(P[0][0]) + R[3 * i + 1] * col(P[0][1])) + R[3 * i + 2] * col(P[0][2])) for i in range(3)]
        for c in R + t:
            valid &= finite(c)
        poses = np.stack(R + t, axis=-1)                # (H, 4, 12)
    ncand = valid.sum(axis=1)
    slot = np.cumsum(valid, axis=1) - 1
    cand = np.zeros((H, MAX_CAND, 12))
    hi_, ki_ = np.nonzero(valid)
    cand[hi_, slot[hi_, ki_]] = poses[hi_, ki_]
    return cand, ncand


# ---- sampling, calibration, the estimator -----------------------------------------------------------------------------------------------
def draws(seed, pair, its, n):
    """Sample indices (H, 3) and ok (H,) of hypotheses `its` of pair `pair` with n correspondences."""
    return TR.sample_distinct(seed, pair, its, n, SAMPLE)


def calibrate(pts2d, pts3d, K):
    """fp32 pixels and fp32 3D points -> fp64 (x, y, X0, X1, X2), each (n,)."""
    p = np.asarray(pts2d, np.float32).astype(np.float64).reshape(-1, 2)
    X = np.asarray(pts3d, np.float32).astype(np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    return ((p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1], X[:, 0], X[:, 1], X[:, 2])


def threshold2(max_err, K):
    thr = max_err / ((float(K[0][0]) + float(K[1][1])) * 0.5)
    return thr * thr


def hypotheses(C, seed, pair, its, thr2):
    """Costs (H, 4) int64 (-1 where no candidate), inlier counts (H, 4), candidates (H, 4, 12), ncand (H,)."""
    x, y, X0, X1, X2 = C
    n = x.shape[0]
    idx, ok = draws(seed, pair, its, n)
    ii = np.where(ok[:, None], idx, 0)
    cand, nc = solve(x[ii], y[ii], np.stack([X0[ii], X1[ii], X2[ii]], axis=-1))
    nc = np.where(ok, nc, 0)
    H = len(its)
    costs = np.full((H, MAX_CAND), -1, np.int64)
    cnts = np.zeros((H, MAX_CAND), np.int64)
    with np.errstate(all="ignore"):
        for c in range(MAX_CAND):
            sel = np.nonzero(nc > c)[0]
            if not len(sel):
                continue
            R = [cand[sel, c, k][:, None] for k in range(9)]
            t = [cand[sel, c, 9 + k][:, None] for k in range(3)]
            r2 = residual2(R, t, x[None], y[None], X0[None], X1[None], X2[None])
            costs[sel, c] = cost(r2, thr2).sum(axis=1)
            cnts[sel, c] = (r2 < thr2).sum(axis=1)
    return costs, cnts, cand, nc


def gn_update(sm, R, t):
    sm = [float(v) for v in sm]
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = sm[k]
            k += 1
    g = sm[21:27]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        dj = H[j][j]
        for q in range(j):
            dj = dj - L[j][q] * L[j][q]
        if not dj > 0.0:
            return None
        L[j][j] = math.sqrt(dj)
        for i in range(j + 1, 6):
            v = H[i][j]
            for q in range(j):
                v = v - L[i][q] * L[j][q]
            L[i][j] = v / L[j][j]
    y, d = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = -g[i]
        for q in range(i):
            v = v - L[i][q] * y[q]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for q in range(i + 1, 6):
            v = v - L[q][i] * d[q]
        d[i] = v / L[i][i]
    w = d[:3]
    n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    f = 1.0 / (1.0 + 0.25 * n2)
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    Cm = [0.0] * 9
    for i in range(3):
        for j in range(3):
            w2 = w[i] * w[j] - (n2 if i == j else 0.0)
            Cm[3 * i + j] = (1.0 if i == j else 0.0) + f * (W[3 * i + j] + 0.5 * w2)
    Rn = [(R[3 * i] * Cm[j] + R[3 * i + 1] * Cm[3 + j]) + R[3 * i + 2] * Cm[6 + j] for i in range(3) for j in range(3)]
    tn = [t[i] + d[3 + i] for i in range(3)]
    if not all(math.isfinite(v) for v in Rn + tn):
        return None
    return Rn, tn


def refine_terms(C, R, t, thr2):
    """Cost (int) and the 27 per-correspondence terms of one refinement pass."""
    x, y, X0, X1, X2 = C
    with np.errstate(all="ignore"):
        Y0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0]
        Y1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1]
        Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2]
        iz = 1.0 / Y2
        px, py = Y0 * iz, Y1 * iz
        dx, dy = x - px, y - py
        r2 = np.where(Y2 > 0.0, dx * dx + dy * dy, BEHIND)
        inl = r2 < thr2
        e0, e1 = px - x, py - y
        G = [[R[2] * X1 - R[1] * X2, R[5] * X1 - R[4] * X2, R[8] * X1 - R[7] * X2],
             [R[0] * X2 - R[2] * X0, R[3] * X2 - R[5] * X0, R[6] * X2 - R[8] * X0],
             [R[1] * X0 - R[0] * X1, R[4] * X0 - R[3] * X1, R[7] * X0 - R[6] * X1]]
        ax, ay = -(px * iz), -(py * iz)
        zero = np.zeros_like(iz)
        J0 = [iz * G[0][0] + ax * G[0][2], iz * G[1][0] + ax * G[1][2], iz * G[2][0] + ax * G[2][2], iz, zero, ax]
        J1 = [iz * G[0][1] + ay * G[0][2], iz * G[1][1] + ay * G[1][2], iz * G[2][1] + ay * G[2][2], zero, iz, ay]
        T = np.zeros((len(x), NSUM))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                T[:, k] = np.where(inl, J0[i] * J0[j] + J1[i] * J1[j], 0.0)
                k += 1
            T[:, 21 + i] = np.where(inl, J0[i] * e0 + J1[i] * e1, 0.0)
    return int(cost(r2, thr2).sum()), T


def estimate(pts2d, pts3d, K, max_reproj_error=12.0, success_prob=0.9999, min_iterations=20, max_iterations=1000, seed=0, pair=0):
    """One pair.  Returns dict R (3,3), t (3,), mask (n,) uint8, info (8,) int (found, best_it, iters, n_inliers, lo_accepted, n, cost_lo,
    cost_hi) -- the kernel's outputs for this pair (`pair` = its index in the batch, which enters the draws)."""
    C = calibrate(pts2d, pts3d, K)
    n = C[0].shape[0]
    thr2 = threshold2(max_reproj_error, K)
    log1mp = math.log(1.0 - success_prob)
    zero = dict(R=np.zeros((3, 3)), t=np.zeros(3), mask=np.zeros(n, np.uint8))
    if n < SAMPLE:
        return dict(zero, info=np.array([0, -1, 0, 0, 0, n, 0, 0]))
    best, _, best_pose, it = TR.stopping_rule(lambda its: hypotheses(C, seed, pair, its, thr2), n, log1mp, max_iterations, SAMPLE, lower=True,
                                              min_iters=min_iterations)
    if best < 0:
        return dict(zero, info=np.array([0, -1, it, 0, 0, n, 0, 0]))
    Rc, tc = [float(v) for v in best_pose[:9]], [float(v) for v in best_pose[9:]]
    Rb, tb, c_best, lo = Rc, tc, None, 0
    for step in range(LO_ITERS + 1):
        c_now, T = refine_terms(C, Rc, tc, thr2)
        sm = block_sums(T)
        if step > 0 and not c_now < c_best:
            break
        Rb, tb = Rc, tc
        if step > 0:
            lo += 1
        c_best = c_now
        if step == LO_ITERS:
            break
        up = gn_update(sm, Rc, tc)
        if up is None:
            break
        Rc, tc = up
    with np.errstate(all="ignore"):
        m = residual2(Rb, tb, *C) < thr2
    n_in = int(m.sum())
    found = n_in >= SAMPLE
    info = np.array([int(found), best, it, n_in, lo, n, *TR.info_words(c_best)])
    if not found:
        return dict(zero, info=info)
    return dict(R=np.array(Rb).reshape(3, 3), t=np.array(tb), mask=m.astype(np.uint8), info=info)
