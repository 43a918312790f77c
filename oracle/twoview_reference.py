"""What the three float64 numpy restatements of the two-view estimators share: oracle/homography_oracle.py (4 points, MAGSAC++ quality),
tests/pose_reference.py (5 points, MSAC cost) and tests/fundamental_reference.py (7 points, MAGSAC++ quality).

TEST INFRASTRUCTURE ONLY.  Nothing under ``accelerated_features_amd/`` may import this module, and it imports nothing from ``tests/``.

It is the host-side counterpart of csrc/ransac_common.hpp and csrc/twoview_math.hpp and repeats them operation for operation (numpy never
fuses a multiply and an add; every product and sum here is rounded once, as in the device files with fp contraction off), so what the
kernels compute is comparable with it bit for bit.  The common rules, stated once:

  * draws: draw d of hypothesis ``it`` of pair p is the upper half of splitmix64-finaliser(seed + golden * (((p << 20) + it) * 16 + d + 1))
    scaled to [0, n); a sample is m distinct indices in draw order, duplicates are redrawn, 16 draws at most; a sample that runs out of
    draws yields no model (``mix64``, ``sample_distinct``: rs::mix64, rs::draw_index, rs::sample_distinct<M>);
  * a hypothesis with several candidate models counts with its best one, the lower index on ties; hypotheses are visited in order; a
    strictly better value makes a new best and bounds the loop by ceil(log(1 - confidence) / log(1 - w^m)), w = the best's inlier ratio,
    w^m multiplied left to right; the loop stops at it >= max(min_iters, bound) (``iterations_needed``, ``stopping_rule``:
    rs::iterations_needed<M>, rs::hyp_best, rs::scan_stopping_rule);
  * floating-point totals over a workgroup are taken in one fixed order: thread i % 256 adds its terms in index order, 8 segments of 32
    threads are added in index order, then the tree ((q0+q1)+(q2+q3))+((q4+q5)+(q6+q7)) (``block_sums``, ``hartley_conditioning``:
    rs::block_sums<N>, rs::hartley_conditioning);
  * MAGSAC++ qualities are sums of 20-bit fixed-point table entries over the bins of r^2, so they are integers and carry no order
    (``table_bin``, ``quality``: rs::bin_of and the score kernels); a 64-bit value leaves as two signed 32-bit words (``info_words``:
    rs::write_info);
  * the geometry both epipolar solvers use (``finite``, ``cross``, ``dot``, ``pmul``, ``sampson``, ``gauss_jordan`` with its pivot
    threshold: is_finite, cross3, dot3, pmul, sampson, gauss_jordan of twoview_math.hpp).

What differs stays with each restatement: the solvers, MSAC cost against MAGSAC++ quality, the refinements, and the homography's
evaluation of its whole hypothesis list at once (it hands ``stopping_rule`` one block).
"""
import math

import numpy as np

MAX_DRAWS = 16               # generator draws per sample before it is given up
NBINS = 4096                 # bins of the MAGSAC++ tables over r^2 in [0, t_max^2)
BLOCK = 256                  # hypotheses built and scored together by the lazy estimators
PIVOT_EPS = 1e-12            # gauss_jordan: a pivot below it (or not finite) is a degenerate system
SQRT2 = 1.41421356237309504880
GOLDEN = np.uint64(0x9e3779b97f4a7c15)


# ---- draws ----------------------------------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def draw_index(seed, pair, its, draw, n):
    """Draw ``draw`` of hypotheses ``its`` (uint64 array) of pair ``pair``: splitmix64 finaliser of a counter, upper 32 bits scaled to [0, n)."""
    with np.errstate(over="ignore"):
        counter = (np.uint64(pair) * np.uint64(1 << 20) + its) * np.uint64(MAX_DRAWS) + np.uint64(draw)
        h = mix64(np.uint64(seed) + GOLDEN * (counter + np.uint64(1)))
    return (((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def sample_distinct(seed, pair, its, n, m):
    """Sample indices (H, m) and ok (H,) of hypotheses ``its`` of pair ``pair`` with n correspondences: m distinct indices per hypothesis,
    draws consumed in order, duplicates redrawn (-1 in the slots a sample that ran out of draws did not fill)."""
    its = np.asarray(its, np.uint64)
    H = its.shape[0]
    idx = np.full((H, m), -1, np.int64)
    slot = np.zeros(H, np.int64)
    for d in range(MAX_DRAWS):
        c = draw_index(seed, pair, its, d, n)
        dup = np.zeros(H, bool)
        for k in range(m - 1):
            dup |= (slot > k) & (c == idx[:, k])
        take = (slot < m) & ~dup
        for k in range(m):
            idx[:, k] = np.where(take & (slot == k), c, idx[:, k])
        slot += take
    return idx, slot >= m


# ---- the loop's bound and the stopping rule -----------------------------------------------------------------------------------------------
def iterations_needed(inliers, n, log1mc, max_iters, m):
    w = inliers / n
    wm = w
    for _ in range(1, m):
        wm = wm * w
    p = 1.0 - wm
    if p <= 0.0:
        return 1
    if p >= 1.0:
        return max_iters
    k = math.ceil(log1mc / math.log(p))
    return k if k < max_iters else max_iters


def stopping_rule(hyp, n, log1mc, max_iters, m, lower, min_iters=0, block=BLOCK):
    """The sequential loop over hypotheses 0 .. max_iters - 1, built ``block`` at a time and only while the loop still reaches them:
    hyp(its) -> (values (H, C) int64, inlier counts (H, C), models (H, C, ...), ncand (H,)).  lower: a lower value is better (a cost) or a
    higher one (a quality; a model of quality 0 never wins).  Returns (winner or -1, its value, a copy of its model or None, the number of
    iterations the loop ran)."""
    pick = np.argmin if lower else np.argmax
    best, best_v, best_model, stop, it = -1, (1 << 64) - 1 if lower else 0, None, max_iters, 0
    for base in range(0, max_iters, block):
        its = np.arange(base, min(base + block, max_iters))
        vals, cnts, models, nc = hyp(its)
        for i, h in enumerate(its):
            if h >= max(stop, min_iters):
                return best, best_v, best_model, int(h)
            if nc[i] > 0:
                c = int(pick(vals[i, :nc[i]]))               # first extremum: the lower index on ties
                v = int(vals[i, c])
                if (v < best_v) if lower else (v > best_v):
                    best, best_v, best_model = int(h), v, models[i, c].copy()
                    stop = min(stop, iterations_needed(int(cnts[i, c]), n, log1mc, max_iters, m))
            it = int(h) + 1
    return best, best_v, best_model, it


def info_words(v):
    """The two signed 32-bit info words (low, high) of a 64-bit value."""
    word = lambda u: u - (1 << 32) if u >= 1 << 31 else u      # noqa: E731
    return word(v & 0xffffffff), word((v >> 32) & 0xffffffff)


# ---- MAGSAC++ table lookups -------------------------------------------------------------------------------------------------------------
def table_bin(r2, tmax2, bin_scale):
    """(r2 < tmax2, bin of r2 in the tables; bin 0 where it is not)."""
    with np.errstate(invalid="ignore"):
        near = r2 < tmax2
        return near, np.minimum(np.where(near, r2 * bin_scale, 0.0).astype(np.int64), NBINS - 1)


def quality(r2, thr2, tmax2, bin_scale, stab):
    """(integer MAGSAC++ quality, inlier count at thr2) per row of r2 (..., n); the caller forms thr2 and tmax2."""
    near, b = table_bin(r2, tmax2, bin_scale)
    with np.errstate(invalid="ignore"):
        return np.where(near, stab[b].astype(np.int64), 0).sum(axis=-1), (r2 < thr2).sum(axis=-1)


# ---- the geometry of twoview_math.hpp (arrays broadcast; the kernel's operation order) ------------------------------------------------------
def finite(v):
    return (v - v) == 0.0


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def pmul(a, b):
    c = [0.0] * (len(a) + len(b) - 1)
    for i in range(len(a)):
        for j in range(len(b)):
            c[i + j] = c[i + j] + a[i] * b[j]
    return c


def sampson_terms(M, a, b, c, d):
    """num, den and (f0, f1) of the Sampson error num^2 / den of (a, b) <-> (c, d) under the 3x3 matrix M (9 entries, row-major)."""
    e0 = (M[0] * a + M[1] * b) + M[2]
    e1 = (M[3] * a + M[4] * b) + M[5]
    e2 = (M[6] * a + M[7] * b) + M[8]
    f0 = (M[0] * c + M[3] * d) + M[6]
    f1 = (M[1] * c + M[4] * d) + M[7]
    num = (c * e0 + d * e1) + e2
    den = ((e0 * e0 + e1 * e1) + f0 * f0) + f1 * f1
    return num, den, (f0, f1)


def sampson(M, a, b, c, d):
    num, den, _ = sampson_terms(M, a, b, c, d)
    return num * num / den


def gauss_jordan(M):
    """In place on (H, rows, cols), partial pivoting on the first `rows` columns.  Returns ok (H,)."""
    H, rows, cols = M.shape
    ok = np.ones(H, bool)
    ar = np.arange(H)
    for c in range(rows):
        a = np.abs(M[:, c:, c])
        first_nan = np.isnan(a[:, 0])
        cmp = np.where(np.isnan(a), -np.inf, a)
        p = np.where(first_nan, 0, np.argmax(cmp, axis=1)) + c
        best = a[ar, p - c]
        ok &= best >= PIVOT_EPS
        rc, rp = M[ar, c].copy(), M[ar, p].copy()
        M[ar, p] = rc
        M[ar, c] = rp
        inv = 1.0 / M[:, c, c]
        M[:, c, c + 1:] = M[:, c, c + 1:] * inv[:, None]
        M[:, c, c] = 1.0
        f = M[:, :, c].copy()
        upd = M[:, :, c + 1:] - f[:, :, None] * M[:, c:c + 1, c + 1:]
        others = np.arange(rows) != c
        M[:, others, c + 1:] = upd[:, others]
        M[:, others, c] = 0.0
    return ok


# ---- fixed-order sums -----------------------------------------------------------------------------------------------------------------
def block_sums(C):
    """The select kernels' fixed-order totals of per-correspondence terms C (n, K): thread i % 256 in index order, 8 segments of 32 threads, a tree."""
    n, K = C.shape
    R = -(-n // 256)
    Cp = np.zeros((max(R, 1) * 256, K))
    Cp[:n] = C
    acc = np.zeros((256, K))
    for r in range(R):
        acc = acc + Cp[r * 256:(r + 1) * 256]
    part = np.zeros((8, K))
    for j in range(8):
        s = np.zeros(K)
        for i in range(32):
            s = s + acc[32 * j + i]
        part[j] = s
    q = part
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))


def hartley_conditioning(P0, P1):
    """The Hartley similarities (cx0, cy0, s0, cx1, cy1, s1) of fp64 pixel arrays (n, 2): centroids, then sqrt(2) / (mean distance to them)."""
    n = P0.shape[0]
    c = block_sums(np.c_[P0, P1]) if n else np.zeros(4)
    dn = float(max(n, 1))
    cx0, cy0, cx1, cy1 = (float(v) / dn for v in c)
    with np.errstate(all="ignore"):
        ax, ay, bx, by = P0[:, 0] - cx0, P0[:, 1] - cy0, P1[:, 0] - cx1, P1[:, 1] - cy1
        d = block_sums(np.c_[np.sqrt(ax * ax + ay * ay), np.sqrt(bx * bx + by * by)]) if n else np.zeros(2)
        s0 = SQRT2 / (float(d[0]) / dn) if d[0] > 0.0 else 1.0
        s1 = SQRT2 / (float(d[1]) / dn) if d[1] > 0.0 else 1.0
    return (cx0, cy0, s0, cx1, cy1, s1)
