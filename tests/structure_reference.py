"""float64 numpy restatement of the two-view structure kernels of csrc/k_triangulate.hip: the per-correspondence
function (calibration, Lindstrom's niter2 correction, the depths of the corrected rays, the status gates), the decomposition of an
essential matrix into its four poses and the vote among them.

It performs the kernel's operations in the kernel's order (numpy never fuses a multiply and an add, and every product and sum here is
rounded once, as in the kernel's file with fp contraction off), vectorised over correspondences, so its results are comparable bit for
bit: the points as float32, the status, the reprojection error, the four poses, the counts, the winner.  ``dot`` / ``cross`` / ``finite``
are oracle/twoview_reference.py's (the host side of csrc/twoview_math.hpp).

TEST INFRASTRUCTURE ONLY: nothing under ``accelerated_features_amd/`` imports it.
"""
import math

import numpy as np

from oracle.twoview_reference import cross, dot, finite

VALID, MASKED, NOT_FINITE, BEHIND, FAR, REPROJ, PARALLAX = range(7)
_ERR = dict(all="ignore")


def pose_E(R, t):
    """[t]x R; R a list of 9 (row-major), t a list of 3 (tg_pose_E)."""
    E = [None] * 9
    for j in range(3):
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j]
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j]
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j]
    return E


def pose_ok(R, t):
    R, t = np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)
    return bool(np.isfinite(R).all() and np.isfinite(t).all() and (R != 0).any() and (t != 0).any())


def calibration(K0, K1):
    """cal = fx0 fy0 cx0 cy0 fx1 fy1 cx1 cy1."""
    K0, K1 = np.asarray(K0, np.float64), np.asarray(K1, np.float64)
    return [K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2]]


def correct(E, cal, u0, v0, u1, v1):
    """tg_correct on arrays of pixels: a dict with the calibrated points x0, x1, the corrected y0, y1, e2 = max(e0^2, e1^2) and fin."""
    with np.errstate(**_ERR):
        fin = finite(u0) & finite(v0) & finite(u1) & finite(v1)
        x0x, x0y = (u0 - cal[2]) / cal[0], (v0 - cal[3]) / cal[1]
        x1x, x1y = (u1 - cal[6]) / cal[4], (v1 - cal[7]) / cal[5]
        n0, n1 = (E[0] * x0x + E[1] * x0y) + E[2], (E[3] * x0x + E[4] * x0y) + E[5]
        m0, m1 = (E[0] * x1x + E[3] * x1y) + E[6], (E[1] * x1x + E[4] * x1y) + E[7]
        a = n0 * (E[0] * m0 + E[1] * m1) + n1 * (E[3] * m0 + E[4] * m1)
        b = 0.5 * ((n0 * n0 + n1 * n1) + (m0 * m0 + m1 * m1))
        c = (x1x * n0 + x1y * n1) + ((E[6] * x0x + E[7] * x0y) + E[8])
        d = np.sqrt(b * b - a * c)
        lam = c / (b + d)
        d1x, d1y, d0x, d0y = lam * n0, lam * n1, lam * m0, lam * m1
        p0, p1, q0, q1 = n0, n1, m0, m1                       # the gradients at the measured pair
        n0, n1 = n0 - (E[0] * d0x + E[1] * d0y), n1 - (E[3] * d0x + E[4] * d0y)
        m0, m1 = m0 - (E[0] * d1x + E[3] * d1y), m1 - (E[1] * d1x + E[4] * d1y)
        a = n0 * (E[0] * m0 + E[1] * m1) + n1 * (E[3] * m0 + E[4] * m1)
        b = 0.5 * ((n0 * p0 + n1 * p1) + (m0 * q0 + m1 * q1))
        lam = c / (b + np.sqrt(b * b - a * c))
        y1x, y1y = x1x - lam * n0, x1y - lam * n1
        y0x, y0y = x0x - lam * m0, x0y - lam * m1
        ax, ay = (y0x - x0x) * cal[0], (y0y - x0y) * cal[1]
        bx, by = (y1x - x1x) * cal[4], (y1y - x1y) * cal[5]
        e0, e1 = ax * ax + ay * ay, bx * bx + by * by
        e2 = np.where(e0 > e1, e0, e1)
    return dict(x0=(x0x, x0y), x1=(x1x, x1y), y0=(y0x, y0y), y1=(y1x, y1y), e2=e2, fin=fin)


def depths(R, t, q):
    """tg_depths: l0, l1, zz, r."""
    with np.errstate(**_ERR):
        one = np.ones_like(q["y1"][0])
        y1 = [q["y1"][0], q["y1"][1], one]
        r = [(R[3 * i] * q["y0"][0] + R[3 * i + 1] * q["y0"][1]) + R[3 * i + 2] for i in range(3)]
        z, a, b = cross(y1, r), cross(y1, t), cross(t, r)
        zz = dot(z, z)
        l0 = -dot(z, a) / zz
        l1 = dot(z, b) / zz
    return l0, l1, zz, r


def depth_status(usable, q, l0, l1, zz, max_depth):
    """tg_depth_status: (status of gates 2-4, X (3 arrays))."""
    with np.errstate(**_ERR):
        X = [l0 * q["y0"][0], l0 * q["y0"][1], l0]
        fin = usable & q["fin"] & (zz > 0.0) & finite(X[0]) & finite(X[1]) & finite(X[2]) & finite(l1)
        st = np.full(np.shape(l0), VALID, np.int64)
        st = np.where((l0 > max_depth) | (l1 > max_depth), FAR, st)
        st = np.where(~(l0 > 0.0) | ~(l1 > 0.0), BEHIND, st)
        st = np.where(~fin, NOT_FINITE, st)
    return st, X


def _f32(v, keep):
    with np.errstate(**_ERR):
        return np.where(keep, v, np.nan).astype(np.float32)


def _pixels(pts, pixels64):
    p = np.asarray(pts, np.float64 if pixels64 else np.float32).astype(np.float64).reshape(-1, 2)
    return p


def triangulate(pts0, pts1, K0, K1, R, t, max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=math.inf, mask=None, in_range=None,
                pixels64=False):
    """One pair: pts0, pts1 (n, 2) float32 pixels (already gathered), K0, K1 (3,3), R (3,3), t (3,).  in_range: (n,) bool, False where an
    index of the list form was out of range (the kernel then reads nothing and sees NaN coordinates).  pixels64: the pixels are taken as
    float64 (the per-correspondence function itself, without the rounding of the kernels' float32 inputs).  Returns a dict: points3d (n,3)
    float32, status (n,) uint8, reproj_error (n,) float32, valid, info (8,), and the gate quantities l0, l1, e2, cos (float64)."""
    p0, p1 = _pixels(pts0, pixels64), _pixels(pts1, pixels64)
    n = p0.shape[0]
    if in_range is not None:
        p0, p1 = np.where(in_range[:, None], p0, np.nan), np.where(in_range[:, None], p1, np.nan)
    Rl, tl = [float(v) for v in np.asarray(R, np.float64).reshape(9)], [float(v) for v in np.asarray(t, np.float64).reshape(3)]
    cal = calibration(K0, K1)
    with np.errstate(**_ERR):
        E = [np.float64(v) for v in pose_E([np.float64(v) for v in Rl], [np.float64(v) for v in tl])]
        usable = pose_ok(Rl, tl)
        q = correct(E, cal, p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1])
        l0, l1, zz, r = depths(Rl, tl, q)
        st, X = depth_status(usable, q, l0, l1, zz, max_depth)
        y1 = [q["y1"][0], q["y1"][1], np.ones(n)]
        cosv = dot(r, y1) / np.sqrt(dot(r, r) * dot(y1, y1))
        thr2 = float(max_reproj_error) * float(max_reproj_error)
        cos_min = math.cos(math.radians(float(min_parallax_deg)))
        st = np.where((st == VALID) & (q["e2"] > thr2), REPROJ, st)
        st = np.where((st == VALID) & (cosv > cos_min), PARALLAX, st)
        if mask is not None:
            st = np.where(np.asarray(mask).reshape(-1) == 0, MASKED, st)
        ok = st == VALID
        pts = np.stack([_f32(X[k], ok) for k in range(3)], axis=1) if n else np.zeros((0, 3), np.float32)
        err = _f32(np.sqrt(q["e2"]), (st != MASKED) & (st != NOT_FINITE))
    info = np.array([n] + [int((st == s).sum()) for s in range(7)], np.int32)
    return dict(points3d=pts, status=st.astype(np.uint8), reproj_error=err, valid=ok, info=info, l0=l0, l1=l1, e2=q["e2"], cos=cosv,
                thr2=thr2, cos_min=cos_min, y0=q["y0"], y1=q["y1"], x0=q["x0"], x1=q["x1"])


def gate_margin(r, max_depth=math.inf):
    """The least relative distance of a decided correspondence of a triangulate() result from the gate that decided it or that it passed:
    a last-bit difference cannot flip a status while this is above 1e-9 or so."""
    st = r["status"]
    m = np.inf
    with np.errstate(**_ERR):
        live = st >= BEHIND                                   # reached the depth gates
        live |= st == VALID
        for v in (r["l0"], r["l1"]):
            m = min(m, np.min(np.abs(v[live]) / np.maximum(1.0, np.abs(v[live])), initial=np.inf))      # against 0: depths are O(1) or more
            if math.isfinite(max_depth):
                m = min(m, np.min(np.abs(v[live] - max_depth) / max_depth, initial=np.inf))
        past = (st == VALID) | (st >= REPROJ)
        m = min(m, np.min(np.abs(r["e2"][past] - r["thr2"]) / r["thr2"], initial=np.inf))
        past = (st == VALID) | (st == PARALLAX)
        m = min(m, np.min(np.abs(r["cos"][past] - r["cos_min"]), initial=np.inf))
    return float(m)


POLAR_STEPS = 3


def orthonormalise(R):
    """tg_orthonormalise: Newton-Schulz steps R <- R (3 I - R'R) / 2 towards the nearest rotation; R a list of 9."""
    for _ in range(POLAR_STEPS):
        M = [(1.5 if i == j else 0.0) - 0.5 * ((R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j]) for i in range(3) for j in range(3)]
        R = [(R[3 * r] * M[j] + R[3 * r + 1] * M[3 + j]) + R[3 * r + 2] * M[6 + j] for r in range(3) for j in range(3)]
    return R


def decompose(E):
    """tg_decompose: (usable, Ra, Rb, t, En) as lists of float64."""
    E = [np.float64(v) for v in np.asarray(E, np.float64).reshape(9)]
    with np.errstate(**_ERR):
        ok = all(bool(finite(v)) for v in E)
        s2 = np.float64(0.0)
        for m in range(9):
            s2 = s2 + E[m] * E[m]
        s2 = s2 * 0.5
        k0, k1, k2 = [E[0], E[3], E[6]], [E[1], E[4], E[7]], [E[2], E[5], E[8]]
        c01, c02, c12 = cross(k0, k1), cross(k0, k2), cross(k1, k2)
        n01, n02, n12 = dot(c01, c01), dot(c02, c02), dot(c12, c12)
        tp = 2 if n12 > (n02 if n02 > n01 else n01) else (1 if n02 > n01 else 0)
        nt = (n01, n02, n12)[tp]
        tc = (c01, c02, c12)[tp]
        ok = ok and bool(nt > 0.0) and bool(s2 > 0.0)
        tn, sc = np.sqrt(nt), np.sqrt(s2)
        t = [tc[m] / tn for m in range(3)]
        cof = cross(E[3:6], E[6:9]) + cross(E[6:9], E[0:3]) + cross(E[0:3], E[3:6])
        te = pose_E(E, t)
        Ra, Rb, En = [None] * 9, [None] * 9, [None] * 9
        for m in range(9):
            a, b = cof[m] / s2, te[m] / sc
            Ra[m], Rb[m], En[m] = a - b, a + b, E[m] / sc
        Ra, Rb = orthonormalise(Ra), orthonormalise(Rb)
        for m in range(9):
            ok = ok and bool(finite(Ra[m])) and bool(finite(Rb[m])) and bool(finite(En[m]))
        ok = ok and all(bool(finite(v)) for v in t)
    return ok, Ra, Rb, t, En


def winner(counts):
    w, best = 0, counts[0]
    for q in (1, 2, 3):
        if counts[q] > best:
            w, best = q, counts[q]
    return w


def recover_pose(E, pts0, pts1, K0, K1, distance_thresh=50.0, mask=None, in_range=None, pixels64=False):
    """One pair.  Returns a dict: found, pose (index or -1), R (3,3), t (3,), good (4,), mask (n,) uint8, points3d (n,3) float32, info (8,),
    poses = (Ra, Rb, t) as float64 arrays, usable, and the depths l0 / l1 (4, n) under the four poses."""
    p0, p1 = _pixels(pts0, pixels64), _pixels(pts1, pixels64)
    n = p0.shape[0]
    if in_range is not None:
        p0, p1 = np.where(in_range[:, None], p0, np.nan), np.where(in_range[:, None], p1, np.nan)
    usable, Ra, Rb, t, En = decompose(E)
    cal = calibration(K0, K1)
    live = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    q = correct(En, cal, p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1])
    good, passes, Xs, L0, L1 = [], [], [], [], []
    for k in range(4):
        sg = -1.0 if k & 1 else 1.0
        with np.errstate(**_ERR):
            tq = [sg * t[0], sg * t[1], sg * t[2]]
        l0, l1, zz, _ = depths(Ra if k < 2 else Rb, tq, q)
        st, X = depth_status(usable, q, l0, l1, zz, distance_thresh)
        ok = (st == VALID) & live
        good.append(int(ok.sum())); passes.append(ok); Xs.append(X); L0.append(l0); L1.append(l1)
    w = winner(good)
    found = bool(usable and good[w] > 0)
    if found:
        R = np.array(Ra if w < 2 else Rb, np.float64).reshape(3, 3)
        with np.errstate(**_ERR):
            tt = np.array([(-1.0 if w & 1 else 1.0) * v for v in t], np.float64)
        m = passes[w]
        pts = np.stack([_f32(Xs[w][k], m) for k in range(3)], axis=1)
    else:
        R, tt, m, pts = np.zeros((3, 3)), np.zeros(3), np.zeros(n, bool), np.full((n, 3), np.nan, np.float32)
    info = np.array([int(found), w if found else -1, 0, good[w] if found else 0, 0, n, 0, 0], np.int32)
    return dict(found=found, pose=w if found else -1, R=R, t=tt, good=np.array(good if usable else [0] * 4, np.int32), mask=m.astype(np.uint8),
                points3d=pts, info=info, poses=(np.array(Ra, np.float64), np.array(Rb, np.float64), np.array(t, np.float64)), usable=usable,
                l0=np.array(L0), l1=np.array(L1))
