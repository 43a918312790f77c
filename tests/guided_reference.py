"""Float64 restatement of xfh_match_mnn_guided (include/xfeat_hip.h, csrc/k_match_guided.hip) and the checker its tests share.

The gate, as the header states it.  kind 'fundamental' (x1' M x0 = 0): with l = M (x0_i, 1), rho_i = l0^2 + l1^2, m = M' (x1_j, 1),
gamma_j = m0^2 + m1^2, e = (l0 x1_j.x + l1 x1_j.y) + l2, element (i, j) passes iff e^2 <= thr^2 (rho_i + gamma_j).  kind 'homography':
(U, V) = dehom(H (x0_i, 1)), element (i, j) passes iff (U - x1_j.x)^2 + (V - x1_j.y)^2 <= thr^2; a row whose w is non-finite or
|w| <= DBL_EPSILON |row 3 of H| passes nothing.  An all-zero model and a model with a non-finite entry pass nothing.

The error window.  The kernel evaluates the per-row and per-column constants in float64 and rounds them to fp32 once; e, the squares, the
sum and the compare run in fp32 (u = 2^-24, first order):

  fundamental: l0, l1, l2 carry one rounding each; l0 x and l1 y one more each, the two additions one each: a term that goes through both
  additions has seen four roundings, l2 two, so |delta e| <= 4u (|l0 x| + |l1 y| + |l2|).  e e: 2 |e| |delta e| + u e^2.  The right side
  fl(thr^2 rho) + fl(thr^2 gamma): one rounding each and one for the sum, 2u thr^2 (rho + gamma).  An element is DECIDED when
      |e^2 - thr^2 (rho + gamma)| > 2 |e| 4u (|l0 x| + |l1 y| + |l2|) + 4u (e^2 + thr^2 (rho + gamma)).
  (A fused multiply-add in place of a product and a sum only removes roundings.)

  homography: U carries one rounding, du = fl(U' - x) one more: |delta du| <= u |U| + u |U' - x| ~ u (|U| + |U - x|), the same for dv.
  du du + dv dv: 2 |du| |delta du| + 2 |dv| |delta dv| + (one rounding per square, one for the sum: 2u (du^2 + dv^2)); fl(thr^2): u thr^2.
  DECIDED when
      |du^2 + dv^2 - thr^2| > 2u (|du| (|U| + |du|) + |dv| (|V| + |dv|)) + 4u (du^2 + dv^2 + thr^2).

Outside the window the fp32 evaluation and this float64 one agree; inside it either answer is accepted."""
import numpy as np

import twoview_support as TS

U32 = 2.0 ** -24
KINDS = ('fundamental', 'homography')
MAX_UNDECIDED = 1e-4


def _hom(k):
    k = np.asarray(k, np.float64).reshape(-1, 2)
    return k[:, 0], k[:, 1]


def model_valid(model):
    M = np.asarray(model, np.float64).reshape(3, 3)
    return bool(np.isfinite(M).all() and np.abs(M).max() > 0)


def gate(k1, k2, model, kind, thr):
    """(passes, decided), two (n1, n2) bool arrays: the float64 gate and whether its margin is outside the fp32 error window."""
    assert kind in KINDS
    x0, y0 = _hom(k1)
    x1, y1 = _hom(k2)
    n1, n2 = len(x0), len(x1)
    if not model_valid(model):
        return np.zeros((n1, n2), bool), np.ones((n1, n2), bool)
    M = np.asarray(model, np.float64).reshape(3, 3)
    t2 = float(thr) * float(thr)
    with np.errstate(all='ignore'):
        if kind == 'fundamental':
            M = M / np.abs(M).max()                      # (the gate does not depend on the model's scale; the kernel scales the same way)
            l0, l1, l2 = (M[r, 0] * x0 + M[r, 1] * y0 + M[r, 2] for r in range(3))
            m0, m1 = (M[0, c] * x1 + M[1, c] * y1 + M[2, c] for c in range(2))
            rhs = t2 * ((l0 * l0 + l1 * l1)[:, None] + (m0 * m0 + m1 * m1)[None, :])
            a, b = l0[:, None] * x1[None, :], l1[:, None] * y1[None, :]
            e = (a + b) + l2[:, None]
            margin = rhs - e * e
            bound = 2 * np.abs(e) * 4 * U32 * (np.abs(a) + np.abs(b) + np.abs(l2)[:, None]) + 4 * U32 * (e * e + rhs)
            return margin >= 0, np.abs(margin) > bound
        w = M[2, 0] * x0 + M[2, 1] * y0 + M[2, 2]
        good = np.isfinite(w) & (np.abs(w) > np.finfo(np.float64).eps * np.linalg.norm(M[2]))
        ws = np.where(good, w, 1.0)
        Uu, Vv = (M[0, 0] * x0 + M[0, 1] * y0 + M[0, 2]) / ws, (M[1, 0] * x0 + M[1, 1] * y0 + M[1, 2]) / ws
        du, dv = Uu[:, None] - x1[None, :], Vv[:, None] - y1[None, :]
        d2 = du * du + dv * dv
        margin = t2 - d2
        bound = 2 * U32 * (np.abs(du) * (np.abs(Uu)[:, None] + np.abs(du)) + np.abs(dv) * (np.abs(Vv)[:, None] + np.abs(dv))) + 4 * U32 * (d2 + t2)
        return (margin >= 0) & good[:, None], (np.abs(margin) > bound) | ~good[:, None]


def gate_fp32(k1, k2, model, kind, thr):
    """The kernel's evaluation in numpy: constants in float64 rounded to fp32 once, the per-element arithmetic in fp32 (no fused operations)."""
    x0, y0 = _hom(k1)
    x1, y1 = _hom(k2)
    n1, n2 = len(x0), len(x1)
    if not model_valid(model):
        return np.zeros((n1, n2), bool)
    M = np.asarray(model, np.float64).reshape(3, 3)
    t2 = float(thr) * float(thr)
    f = np.float32
    xf, yf = x1.astype(f)[None, :], y1.astype(f)[None, :]
    with np.errstate(all='ignore'):
        if kind == 'fundamental':
            mx = np.abs(M).max()
            l0, l1, l2 = ((M[r, 0] * x0 + M[r, 1] * y0 + M[r, 2]) / mx for r in range(3))
            m0, m1 = ((M[0, c] * x1 + M[1, c] * y1 + M[2, c]) / mx for c in range(2))
            rho, gam = (t2 * (l0 * l0 + l1 * l1)).astype(f)[:, None], (t2 * (m0 * m0 + m1 * m1)).astype(f)[None, :]
            e = (l0.astype(f)[:, None] * xf + l1.astype(f)[:, None] * yf) + l2.astype(f)[:, None]
            return e * e <= rho + gam
        w = M[2, 0] * x0 + M[2, 1] * y0 + M[2, 2]
        good = np.isfinite(w) & (np.abs(w) > np.finfo(np.float64).eps * np.linalg.norm(M[2]))
        ws = np.where(good, w, 1.0)
        Uu = np.where(good, (M[0, 0] * x0 + M[0, 1] * y0 + M[0, 2]) / ws, np.nan).astype(f)[:, None]
        Vv = np.where(good, (M[1, 0] * x0 + M[1, 1] * y0 + M[1, 2]) / ws, np.nan).astype(f)[:, None]
        du, dv = Uu - xf, Vv - yf
        return du * du + dv * dv <= f(t2)


def guided_mnn(d1, d2, k1, k2, model, kind, thr, min_cossim=-1.0):
    """Brute force in float64: (idx0, idx1) of the mutual nearest neighbours among the passing elements, lowest index on ties."""
    passes, _ = gate(k1, k2, model, kind, thr)
    s = np.asarray(d1, np.float64) @ np.asarray(d2, np.float64).T
    s = np.where(passes, s, -np.inf)
    if s.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    j = s.argmax(1)
    i = s.argmax(0)
    rows = np.arange(s.shape[0])
    v = s[rows, j]
    keep = (i[j] == rows) & np.isfinite(v)
    if min_cossim > 0:
        keep &= v > min_cossim
    return rows[keep].astype(np.int64), j[keep].astype(np.int64)


def check_guided_mnn_fp64(d1, d2, k1, k2, model, kind, thr, i0, i1, min_cossim=-1.0, rtol=2e-6, max_undecided=MAX_UNDECIDED):
    """adversarial.check_mnn_fp64 with a gate window.  Asserts: (1) every reported pair passes the gate or is undecided and is a row and a
    column maximum (tie allowance rtol, as the parity contract has it) among the decided-passing elements; (2) every pair that is
    decided-passing and strictly wins its row and column among the passing-or-undecided elements is reported; (3) idx0 ascends.
    Condition: at most max_undecided of the case's elements are undecided.  Returns (pairs that had to be reported, undecided elements)."""
    passes, decided = gate(k1, k2, model, kind, thr)
    n_und = int((~decided).sum())
    assert n_und <= max_undecided * decided.size, f"{n_und} of {decided.size} elements inside the fp32 window: not a usable case"
    s = np.asarray(d1, np.float64) @ np.asarray(d2, np.float64).T
    tol = rtol * max(1.0, float(np.abs(s).max()))
    i0 = np.asarray(i0, np.int64)
    i1 = np.asarray(i1, np.int64)
    assert len(i0) == len(i1) and (len(i0) < 2 or (np.diff(i0) > 0).all()), "idx0 does not ascend"
    assert ((i0 >= 0) & (i0 < s.shape[0]) & (i1 >= 0) & (i1 < s.shape[1])).all()
    sure = passes & decided
    maybe = sure | ~decided
    sd = np.where(sure, s, -np.inf)
    sm = np.where(maybe, s, -np.inf)
    v = s[i0, i1]
    assert maybe[i0, i1].all(), "a reported pair fails the gate"
    assert (v >= sd.max(1)[i0] - tol).all() and (v >= sd.max(0)[i1] - tol).all(), "a reported pair is not a mutual maximum among the passing elements"
    if min_cossim > 0:
        assert (v > min_cossim - tol).all()
    j = sm.argmax(1)
    rows = np.arange(s.shape[0])
    srt = np.sort(sm, axis=1)
    csrt = np.sort(sm, axis=0)
    with np.errstate(invalid='ignore'):       # (-inf) - (-inf): a row / column nothing passes in is not strict
        row_strict = (srt[:, -1] - (srt[:, -2] if s.shape[1] > 1 else -np.inf)) > tol
        col_strict = (csrt[-1] - (csrt[-2] if s.shape[0] > 1 else -np.inf)) > tol
    must = [i for i in rows if sure[i, j[i]] and row_strict[i] and col_strict[j[i]] and sm[:, j[i]].argmax() == i
            and (min_cossim <= 0 or s[i, j[i]] > min_cossim + tol)]
    got = dict(zip(i0.tolist(), i1.tolist()))
    missing = [i for i in must if got.get(int(i)) != int(j[i])]
    assert not missing, f"{len(missing)} strict guided mutual matches not reported, e.g. rows {missing[:3]}"
    return len(must), n_und


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def unit_rows(rng, n):
    d = rng.normal(size=(n, 64))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _assemble(rng, p0, p1, n1, n2, size0, size1, desc_noise):
    """n1 / n2 key-points and unit descriptors around the true correspondences p0 <-> p1 (their descriptors agree up to desc_noise), the rest
    unrelated points with unrelated descriptors; image 1 in a random order.  Returns k1, d1, k2, d2, truth (row of image 1 per true row of image 0)."""
    nt = min(len(p0), n1, n2)
    k1 = np.r_[p0[:nt], np.c_[rng.uniform(0, size0[1], n1 - nt), rng.uniform(0, size0[0], n1 - nt)]].astype(np.float32)
    k2 = np.r_[p1[:nt], np.c_[rng.uniform(0, size1[1], n2 - nt), rng.uniform(0, size1[0], n2 - nt)]].astype(np.float32)
    d1 = unit_rows(rng, n1)
    d2 = unit_rows(rng, n2)
    t = d1[:nt].astype(np.float64) + desc_noise * rng.normal(size=(nt, 64))
    d2[:nt] = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
    perm = rng.permutation(n2)
    inv = np.empty(n2, np.int64)
    inv[perm] = np.arange(n2)
    return k1, d1, np.ascontiguousarray(k2[perm]), np.ascontiguousarray(d2[perm]), inv[:nt]


def epipolar_scene(pair, n1, n2, seed, noise=0.5, desc_noise=0.03):
    """Pair `pair` of the MegaDepth-1500 fixture: min(n1, n2) * 3 / 4 true correspondences (at least one), the rest clutter.  Returns a dict:
    k1, d1, k2, d2, truth, model (the true F, unit Frobenius norm), kind."""
    rng = np.random.default_rng(seed)
    f = TS.fixture()
    nt = max(1, (3 * min(n1, n2)) // 4)
    p0, p1, _ = TS.fixture_pair(f, pair, nt, noise, 0.0, rng)
    k1, d1, k2, d2, truth = _assemble(rng, p0, p1, n1, n2, tuple(f["size0_hw"][pair]), tuple(f["size1_hw"][pair]), desc_noise)
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, truth=truth, model=TS.true_F(f["K0"][pair], f["K1"][pair], f["T_0to1"][pair]), kind='fundamental')


def planar_scene(n1, n2, seed, noise=0.5, desc_noise=0.03):
    """TS.homography_pair with clutter: the same dict, model = the true H, kind 'homography'."""
    rng = np.random.default_rng(seed)
    nt = max(1, (3 * min(n1, n2)) // 4)
    p0, p1, H, _ = TS.homography_pair(nt, 0.0, noise, seed)
    k1, d1, k2, d2, truth = _assemble(rng, p0, p1, n1, n2, (480.0, 640.0), (480.0, 640.0), desc_noise)
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, truth=truth, model=H, kind='homography')


def scene(kind, n1, n2, seed):
    return epipolar_scene(7, n1, n2, seed) if kind == 'fundamental' else planar_scene(n1, n2, seed)


def add_distractors(s, rng):
    """Every image-0 descriptor of a true correspondence gets an exact copy at a random place in image 1 (appended): the plain arg-max takes
    the copy (similarity 1), the gate removes it."""
    nt = len(s['truth'])
    h, w = (float(s['k2'][:, 1].max()) + 1.0, float(s['k2'][:, 0].max()) + 1.0)
    out = dict(s)
    out['k2'] = np.r_[s['k2'], np.c_[rng.uniform(0, w, nt), rng.uniform(0, h, nt)].astype(np.float32)]
    out['d2'] = np.r_[s['d2'], s['d1'][:nt]]
    return out


def distractor_scene(n=512, pair=7, seed=7):
    """The fixture of the issue: pair 7, n true correspondences at 0.5 px noise and nothing else, plus an exact descriptor copy per image-0
    point at a random place in image 1."""
    rng = np.random.default_rng(seed)
    f = TS.fixture()
    p0, p1, _ = TS.fixture_pair(f, pair, n, 0.5, 0.0, rng)
    k1, d1, k2, d2, truth = _assemble(rng, p0, p1, n, n, tuple(f["size0_hw"][pair]), tuple(f["size1_hw"][pair]), 0.03)
    s = dict(k1=k1, d1=d1, k2=k2, d2=d2, truth=truth, model=TS.true_F(f["K0"][pair], f["K1"][pair], f["T_0to1"][pair]), kind='fundamental')
    return add_distractors(s, rng)


def true_matches(s, i0, i1):
    """How many reported pairs are true correspondences of the scene."""
    t = s['truth']
    i0 = np.asarray(i0)
    i1 = np.asarray(i1)
    m = i0 < len(t)
    return int((t[i0[m]] == i1[m]).sum())


def horizontal_fixture():
    """Exactly representable: M = [[0,0,0],[0,0,-1],[0,1,0]] (horizontal epipolar lines) and half-pixel coordinates -- l = (0, -1, y0),
    rho = gamma = 1, e = y0 - y1, so the Sampson error is |y1 - y0| / sqrt(2) and every quantity of the gate is exact in fp32 and float64.
    Row i of image 0 at y = 8 i; image 1 holds, for every row, four scaled copies of the row's descriptor at dy = 0.5, 1, 1.5, 2 below it,
    the farther the more similar: the match of row i is the farthest copy the gate still passes (column 4 i + k at a threshold that admits
    dy_k and not dy_k+1), so the comparison at the threshold itself decides the result."""
    n = 6
    rng = np.random.default_rng(11)
    d1 = unit_rows(rng, n)
    dys = np.array([0.5, 1.0, 1.5, 2.0])
    k1 = np.c_[np.arange(n) * 16.0 + 3.5, np.arange(n) * 8.0].astype(np.float32)
    k2, d2 = [], []
    for i in range(n):
        for r, dy in enumerate(dys):
            k2.append((k1[i, 0] + 2.0 * r, k1[i, 1] + dy))
            d2.append(d1[i] * np.float32(0.5 + 0.125 * r))       # larger dy, larger similarity: 0.5, 0.625, 0.75, 0.875 (exact scalings)
    M = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    return dict(k1=k1, d1=d1, k2=np.array(k2, np.float32), d2=np.array(d2, np.float32), model=M, kind='fundamental', dys=dys)


def translation_fixture():
    """Exactly representable: H = a pure dyadic translation, so (U, V) and the transfer error are exact.  Same layout as horizontal_fixture,
    the copies at distance 3, 4, 5 (the (3,4,5) triangle) and 6 from the transferred point."""
    n = 6
    rng = np.random.default_rng(12)
    d1 = unit_rows(rng, n)
    offs = np.array([[3.0, 0.0], [0.0, 4.0], [3.0, 4.0], [6.0, 0.0]])
    dist = np.array([3.0, 4.0, 5.0, 6.0])
    k1 = np.c_[np.arange(n) * 32.0 + 1.5, np.arange(n) * 24.0 + 0.25].astype(np.float32)
    H = np.array([[1.0, 0, 12.5], [0, 1, -7.25], [0, 0, 1]])
    k2, d2 = [], []
    for i in range(n):
        for r in range(4):
            k2.append((k1[i, 0] + 12.5 + offs[r, 0], k1[i, 1] - 7.25 + offs[r, 1]))
            d2.append(d1[i] * np.float32(0.5 + 0.125 * r))
    return dict(k1=k1, d1=d1, k2=np.array(k2, np.float32), d2=np.array(d2, np.float32), model=H, kind='homography', dys=dist)


def sampson_threshold_at(dy):
    """A threshold that the horizontal fixture's element at |y1 - y0| = dy meets exactly or by one rounding: the float64 nearest dy / sqrt(2),
    moved up by one ulp if its square falls short (thr^2 * 2 >= dy^2 must hold in float64 for the restatement to pass it)."""
    t = dy / np.sqrt(2.0)
    while t * t * 2.0 < dy * dy:
        t = np.nextafter(t, np.inf)
    return float(t)
