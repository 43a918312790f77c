// Relative pose from the match lists: the device side of the evaluation's
//     pose, info = poselib.estimate_relative_pose(kpts0, kpts1, cam0, cam1, {"max_epipolar_error": thr}, {})
// (modules/eval/megadepth1500.py and scannet1500.py of the reference).  poselib is not available offline and its source is not part of the
// reference tree, so nothing here is pinned to it: what is implemented is the published estimator -- RANSAC over Nister's five-point solver
// (Nister, PAMI 2004) with an MSAC score on the Sampson error and a Gauss-Newton refinement of the winner.  The specification (DESIGN.md 3.10;
// tests/pose_reference.py is a numpy restatement of it, operation for operation, and tests/test_relpose_emulated.py compiles the solver
// below on the host and holds it to that restatement bit for bit):
//   * calibration: pixel (u, v) of pair p -> ((u - cx) / fx, (v - cy) / fy) in fp64 with pair p's PINHOLE intrinsics (K row-major 3x3);
//     the threshold in these units is thr_n = max_epipolar_error / (0.5 (f0 + f1)), f = (fx + fy) / 2 of each camera -- our choice;
//   * sample: 5 distinct correspondences, drawn as ransac_common.hpp states (splitmix64 of (seed, pair, hypothesis, draw); duplicates
//     are redrawn, 16 draws at most; a sample that runs out of draws yields no model);
//   * minimal solver (relpose_solve): null space of the 5x9 epipolar constraint matrix by Gauss-Jordan with partial pivoting (a pivot
//     below tv::PIVOT_EPS of twoview_math.hpp, or not finite: no model), its four vectors orthonormalised by modified Gram-Schmidt, E = x X + y Y + z Z + W; the 10 cubic constraints det E = 0 and (E E' - tr(E E')/2 I) E = 0
//     (the trace constraint halved) as a 10x20 matrix in Nister's monomial order, Gauss-Jordan with partial pivoting on its first 10
//     columns; B(z) from rows (x^2 z, x^2), (y^2 z, y^2), (xyz, xy); det B(z) (degree 10) made monic; real roots by a Sturm sequence
//     (Cauchy bound, STURM_STEPS bisections on the root count per root, then SIGN_STEPS bisections on the sign of the polynomial, then
//     NEWTON_STEPS Newton steps, each kept only if it lowers |p|: the Sturm counts of a badly scaled polynomial can be off), in ascending order; (x, y) from the cross product of two rows of B(z) (the pair with the largest |third component|);
//   * decomposition without an SVD: t = the cross product of two columns of E (largest norm), R = cof(E) / s^2 -+ [t]x E / s with
//     s^2 = tr(E E') / 2 (cof(E) = t t' R: its rows are cross products of E's rows, and [t]x E = (t t' - I) R for E = [t]x R, |t| = 1), the four poses (Ra, t) (Ra, -t) (Rb, t)
//     (Rb, -t); the first that puts the 5 sample points in front of both cameras is the root's candidate, none: the root is dropped;
//   * only + - * / sqrt in all of it (no exp / log / trig), with every product and sum rounded once (fp contraction off in this file);
//   * score of a candidate: E = [t]x R, Sampson error r^2 = (x2' E x1)^2 / ((E x1)_1^2 + (E x1)_2^2 + (E' x2)_1^2 + (E' x2)_2^2); MSAC cost
//     floor(min(r^2, thr_n^2) / thr_n^2 * 2^20) summed as u64 (no summation order); inlier: r^2 < thr_n^2 (NaN: never); a hypothesis
//     costs the minimum over its candidates (ties: the lower root);
//   * stopping rule: hypotheses in order, a strictly lower cost makes a new best and bounds the loop by ceil(log(1 - p) / log(1 - w^5)),
//     w = inlier ratio of the best; the loop stops at it >= max(min_iterations, bound) (rs::scan_stopping_rule of ransac_common.hpp);
//   * refinement of the winner: up to 10 Gauss-Newton steps on R <- R cay(w), t <- normalise(t + d1 b1 + d2 b2) (b1, b2 from t and the
//     axis of its smallest component) over the inliers, residual x2' E x1 weighted by 1 / (Sampson denominator) at the step's start,
//     5x5 normal equations by Cholesky; a step is kept only if it strictly lowers the integer cost, the first rejected step ends it;
//     the sums are fixed-order block reductions (rs::block_sums; the restatement repeats that order), so the refined pose is reproducible too;
//   * mask: r^2 < thr_n^2 under the final pose; found = at least 5 inliers; R, t (unit), E = [t]x R, mask: zeros when not found.
//
// What makes it a device algorithm is what made the homography one: hypothesis `it` is a function of (seed, pair, it) alone, so every
// hypothesis is built and scored at once and the loop's stopping rule is applied to the cost list afterwards.
//
// The register budget.  The solver's working set is the 10x20 matrix (200 fp64 = 400 VGPRs), the quadratic entries of E E' (60 fp64), the
// sample (20 fp64) and the 66 Sturm coefficients.  Register arrays with runtime indices (the pivot row) go to scratch, which the library
// does not allow; a lane-parallel elimination (lane = column) needs a pivot search and a row broadcast per column through DPP / readlane
// for 10 + 5 columns and leaves the root isolation -- the longest part, serial per root -- on one lane of 20.  So the working set lives in
// a per-thread slice of LDS: SLICE = 280 fp64 per hypothesis, element k of thread j at lds[k * 64 + j] (consecutive lanes, consecutive
// banks), 64 hypotheses per workgroup = 140 KiB: one workgroup per CU, one wave per CU, latency-bound: 2048 hypotheses in flight per
// XCD (32 CUs), 16384 on the chip.  The linear entries of E (36 fp64) stay in registers for the whole solve.
//
// Launches per call (R workspace: per hypothesis 10 candidate poses + 10 costs + 10 inlier counts + the candidate count):
//   relpose_zero_kernel   : costs, counts, candidate counts zeroed
//   relpose_solve_kernel  : thread = hypothesis: sample, solver, candidates into the workspace      (hypotheses 0..255 first)
//   relpose_score_kernel  : thread = hypothesis, its candidates in turn against a chunk of correspondences in LDS, u64 atomics
//   relpose_bound_kernel  : the bound the loop reaches from the records among the first 256; the later blocks are solved and scored
//                           only below max(min_iterations, bound)
//   relpose_select_kernel : one workgroup per pair: stopping rule over the cost list (tiles in LDS), refinement, mask, outputs
//
// The threshold sweep (xfh_estimate_relpose_sweep: the twelve RANSAC thresholds of modules/eval/scannet1500.py in one call).  Slice j of
// a sweep IS the estimate above at threshold j -- the same specification, bit for bit.  What the T estimates share is computed once: a
// hypothesis is a function of (seed, pair, it) alone, so one solve per hypothesis serves every threshold (candidate poses stored once,
// 960 B), and the Sampson error of a (candidate, correspondence) is evaluated once and clamped T times.  Only the cost / count lists
// (T x 120 B per hypothesis, (P, iters_pad, 10, T)), the bounds and the select step are per threshold:
//   relpose_sweep_zero_kernel  : the lists, candidate counts zeroed
//   relpose_solve_kernel       : unchanged; the later blocks are solved below the pair's LARGEST bound over the thresholds
//   relpose_sweep_score_kernel : as relpose_score_kernel, T costs and T counts per residual.  The thresholds arrive sorted in descending
//                                order (the host sorts; `slot` maps threshold j to its place), so the T tests nest: a residual at or above
//                                the largest threshold -- most of them, under a wrong model -- takes one comparison.  Such a residual costs exactly
//                                2^20 (thr2 / thr2 = 1), so only the inliers' costs rp_cost(r2, thr2_j), division included, are summed and
//                                2^20 x (residuals - inliers) is added at the end; integer sums, the same total.  The accumulators stay in
//                                registers: the nest is unrolled at compile time over a padded size (4, 8, 12, 16; padding: thr2 = 0,
//                                never taken)
//   relpose_bound_kernel       : one bound per (pair, threshold) from the records among the first 256, and their maximum per pair
//   relpose_select_kernel      : one workgroup per (pair, threshold) on that threshold's lists (stride T); the single call is T = 1
// Hypotheses that the sweep solves and scores at or beyond threshold j's own bound (below the pair's largest) do not change slice j:
// rs::scan_stopping_rule never looks at an entry at or beyond the loop's stop, and that stop is at most threshold j's bound when the
// loop runs past the first 256 hypotheses (every record among them is one the loop sees) and lies inside the first 256 -- which are
// always solved and scored -- otherwise.
#include "ransac_common.hpp"
#include "twoview_math.hpp"

#pragma clang fp contract(off)

namespace xfh {
namespace rp {
using rs::HYP_PER_WG, rs::PTS_PER_WG, rs::SEL_TILE, rs::SEL_CACHE;
constexpr int LO_ITERS = 10, MAX_ITERS = 16384, MAX_THR = 16, MAX_CAND = 10;
constexpr int SLICE = 280, SOLVE_WG = 64, NSUM = 20;
}  // namespace rp

// ---- solver begin (host-compilable: tests/test_relpose_emulated.py slices it out behind the slice of twoview_math.hpp and drops the
// __device__ qualifiers) ----
namespace rp {
constexpr int STURM_STEPS = 48, SIGN_STEPS = 48, NEWTON_STEPS = 4;
constexpr int CAND_DOUBLES = 12;             // R (row-major) + t of one candidate pose
}  // namespace rp
// slice layout (fp64 elements): [0, 200) the 10x20 matrix (first the 5x9 one, last the Sturm sequence), [200, 260) the six quadratic
// entries of E E' - tr/2 I, [260, 280) the sample: x1[5] y1[5] x2[5] y2[5]
constexpr int RP_M = 0, RP_Q = 200, RP_PTS = 260;
// monomials: linear (x, y, z, 1); quadratic (x2, y2, z2, xy, xz, yz, x, y, z, 1); cubic in Nister's order
// (x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1); LL / QL: index of the product monomial
constexpr int RP_LL[4][4] = {{0, 3, 4, 6}, {3, 1, 5, 7}, {4, 5, 2, 8}, {6, 7, 8, 9}};
constexpr int RP_QL[10][4] = {{0, 2, 4, 5}, {3, 1, 6, 7}, {10, 13, 16, 17}, {2, 3, 8, 9}, {4, 8, 10, 11},
                              {8, 6, 13, 14}, {5, 9, 11, 12}, {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};
constexpr int RP_SYM[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};

// E = [t]x R
__device__ inline void rp_pose_E(const double* R, const double* t, double* E) {
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}
// MSAC cost in 2^-20 units of thr2; NaN counts as the cap
__device__ inline unsigned rp_cost(double r2, double thr2) {
    const double m = r2 < thr2 ? r2 : thr2;
    return (unsigned)floor(m / thr2 * 1048576.0);
}
__device__ inline double rp_horner(const double* a, int deg, double x) {
    double v = a[deg];
    for (int i = deg - 1; i >= 0; --i) v = v * x + a[i];
    return v;
}
template <class S>
__device__ inline double rp_horner_s(S s, int off, int deg, double x) {
    double v = s[off + deg];
    for (int i = deg - 1; i >= 0; --i) v = v * x + s[off + i];
    return v;
}
// sign changes of the Sturm sequence at x (sequence k has degree 10 - k, at offset RP_M + 11 k - k (k - 1) / 2)
template <class S>
__device__ inline int rp_sturm_changes(S s, double x) {
    int n = 0, off = RP_M;
    bool have = false, prev = false;
    for (int k = 0; k <= 10; ++k) {
        const double v = rp_horner_s(s, off, 10 - k, x);
        if (v != 0.0) {
            const bool g = v > 0.0;
            if (have && g != prev) ++n;
            prev = g; have = true;
        }
        off += 11 - k;
    }
    return n;
}
// candidate poses of the sample in S[RP_PTS ..]: out[12 c ..] = R (row-major), t (unit); returns their number (0: no model)
template <class S>
__device__ inline int relpose_solve(S s, double* out) {
    // ---- 5x9 constraint matrix, rows x2_i x1_j (E row-major), in the M area
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double a = s[RP_PTS + k], b = s[RP_PTS + 5 + k], c = s[RP_PTS + 10 + k], d = s[RP_PTS + 15 + k];
        const double r[9] = {c * a, c * b, c, d * a, d * b, d, a, b, 1.0};
#pragma unroll
        for (int j = 0; j < 9; ++j) s[RP_M + 9 * k + j] = r[j];
    }
    if (!tv::gauss_jordan(s, RP_M, 5, 9)) return 0;
    // null basis v_k = (-C[:, k], e_k) of the reduced matrix, orthonormalised by modified Gram-Schmidt (k = 0..3 in order, sums over the
    // 9 entries in index order): the raw basis is badly scaled for a sizeable fraction of samples, which the degree-10 polynomial inherits
    // (the true z stops being one of its roots); E entry m is then the linear polynomial (x, y, z, 1) -> e[m][0..3] = v_0..3[m]
    double e[9][4];
#pragma unroll
    for (int m = 0; m < 9; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) e[m][k] = m < 5 ? -s[RP_M + 9 * m + 5 + k] : (m - 5 == k ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < k; ++j) {
            double d = 0.0;
#pragma unroll
            for (int m = 0; m < 9; ++m) d = d + e[m][k] * e[m][j];
#pragma unroll
            for (int m = 0; m < 9; ++m) e[m][k] = e[m][k] - d * e[m][j];
        }
        double nn = 0.0;
#pragma unroll
        for (int m = 0; m < 9; ++m) nn = nn + e[m][k] * e[m][k];
        nn = sqrt(nn);
#pragma unroll
        for (int m = 0; m < 9; ++m) e[m][k] = e[m][k] / nn;
    }
    // ---- the 10x20 cubic constraints
#pragma unroll
    for (int j = 0; j < 200; ++j) s[RP_M + j] = 0.0;
    {   // row 0: det E by the first row's cofactors
        const int cof[3][4] = {{4, 8, 5, 7}, {3, 8, 5, 6}, {3, 7, 4, 6}};
        const double sg[3] = {1.0, -1.0, 1.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double q[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) q[k] = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) q[RP_LL[i][j]] = q[RP_LL[i][j]] + e[cof[c][0]][i] * e[cof[c][1]][j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) q[RP_LL[i][j]] = q[RP_LL[i][j]] - e[cof[c][2]][i] * e[cof[c][3]][j];
#pragma unroll
            for (int i = 0; i < 10; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double p = q[i] * e[c][j];
                    s[RP_M + RP_QL[i][j]] = sg[c] > 0.0 ? s[RP_M + RP_QL[i][j]] + p : s[RP_M + RP_QL[i][j]] - p;
                }
        }
    }
    // E E' (upper triangle) into the Q area, then minus tr / 2 on the diagonal
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double q[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) q[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[RP_LL[i][j]] = q[RP_LL[i][j]] + e[3 * a + k][i] * e[3 * b + k][j];
#pragma unroll
            for (int k = 0; k < 10; ++k) s[RP_Q + 10 * RP_SYM[a][b] + k] = q[k];
        }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const double h = 0.5 * ((s[RP_Q + k] + s[RP_Q + 30 + k]) + s[RP_Q + 50 + k]);
        s[RP_Q + k] = s[RP_Q + k] - h;
        s[RP_Q + 30 + k] = s[RP_Q + 30 + k] - h;
        s[RP_Q + 50 + k] = s[RP_Q + 50 + k] - h;
    }
    // rows 1..9: (Lambda E)_ij = sum_k Lambda_ik E_kj
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int row = 1 + 3 * i + j;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 10; ++a) {
                    const double qa = s[RP_Q + 10 * RP_SYM[i][k] + a];
#pragma unroll
                    for (int b = 0; b < 4; ++b) s[RP_M + 20 * row + RP_QL[a][b]] = s[RP_M + 20 * row + RP_QL[a][b]] + qa * e[3 * k + j][b];
                }
        }
    if (!tv::gauss_jordan(s, RP_M, 10, 20)) return 0;
    // ---- B(z): rows k = r4 - z r5, l = r6 - z r7, m = r8 - z r9 of the tail (xz2 xz x yz2 yz y z3 z2 z 1); x, y parts degree 3, constant 4
    double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int u = RP_M + 20 * (4 + 2 * r) + 10, v = RP_M + 20 * (5 + 2 * r) + 10;
        bx[r][0] = s[u + 2]; bx[r][1] = s[u + 1] - s[v + 2]; bx[r][2] = s[u + 0] - s[v + 1]; bx[r][3] = -s[v + 0];
        by[r][0] = s[u + 5]; by[r][1] = s[u + 4] - s[v + 5]; by[r][2] = s[u + 3] - s[v + 4]; by[r][3] = -s[v + 3];
        b1[r][0] = s[u + 9]; b1[r][1] = s[u + 8] - s[v + 9]; b1[r][2] = s[u + 7] - s[v + 8]; b1[r][3] = s[u + 6] - s[v + 7]; b1[r][4] = -s[v + 6];
    }
    // det B = bx0 (by1 b12 - b11 by2) - by0 (bx1 b12 - b11 bx2) + b10 (bx1 by2 - by1 bx2)
    double p[11];
    {
        double t1[8], t2[8], c1[8], c2[8], c3[7], w[11];
        tv::pmul(by[1], 3, b1[2], 4, t1); tv::pmul(b1[1], 4, by[2], 3, t2);
#pragma unroll
        for (int k = 0; k < 8; ++k) c1[k] = t1[k] - t2[k];
        tv::pmul(bx[1], 3, b1[2], 4, t1); tv::pmul(b1[1], 4, bx[2], 3, t2);
#pragma unroll
        for (int k = 0; k < 8; ++k) c2[k] = t1[k] - t2[k];
        tv::pmul(bx[1], 3, by[2], 3, t1); tv::pmul(by[1], 3, bx[2], 3, t2);
#pragma unroll
        for (int k = 0; k < 7; ++k) c3[k] = t1[k] - t2[k];
        tv::pmul(bx[0], 3, c1, 7, p);
        tv::pmul(by[0], 3, c2, 7, w);
#pragma unroll
        for (int k = 0; k < 11; ++k) p[k] = p[k] - w[k];
        tv::pmul(b1[0], 4, c3, 6, w);
#pragma unroll
        for (int k = 0; k < 11; ++k) p[k] = p[k] + w[k];
    }
    // ---- Sturm sequence of the monic polynomial into the M area
    const double lead = p[10];
    if (!(fabs(lead) > 0.0) || !tv::is_finite(lead)) return 0;
    double bound = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const double v = k == 10 ? 1.0 : p[k] / lead;
        s[RP_M + k] = v;
        const double av = fabs(v);
        if (k < 10 && av > bound) bound = av;
    }
    bound = 1.0 + bound;
#pragma unroll
    for (int k = 0; k < 10; ++k) s[RP_M + 11 + k] = (double)(k + 1) * s[RP_M + k + 1];
    bool fin = tv::is_finite(bound);
    {
        int oa = RP_M, ob = RP_M + 11;                     // a: degree d + 1, b: degree d
        for (int d = 9; d >= 1; --d) {
            const int oc = ob + d + 1;                     // -rem(a, b): degree d - 1
            const double q1 = s[oa + d + 1] / s[ob + d];
            // t = a - q1 x b (degree d): t[0] = a[0], t[i] = a[i] - q1 b[i-1]; q0 = t[d] / b[d]; -rem = -(t - q0 b)
            const double q0 = (s[oa + d] - q1 * s[ob + d - 1]) / s[ob + d];
            for (int i = 0; i < d; ++i) {
                const double ti = i == 0 ? s[oa] : s[oa + i] - q1 * s[ob + i - 1];
                s[oc + i] = -(ti - q0 * s[ob + i]);
            }
            oa = ob; ob = oc;
        }
        for (int k = 0; k < 66; ++k) fin = fin && tv::is_finite(s[RP_M + k]);
    }
    if (!fin) return 0;
    const int v_lo = rp_sturm_changes(s, -bound), v_hi = rp_sturm_changes(s, bound);
    int nroots = v_lo - v_hi;
    nroots = nroots < 0 ? 0 : (nroots > 10 ? 10 : nroots);
    int ncand = 0;
    for (int k = 0; k < nroots; ++k) {
        double lo = -bound, hi = bound;
        for (int it = 0; it < rp::STURM_STEPS; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (v_lo - rp_sturm_changes(s, mid) > k) hi = mid; else lo = mid;
        }
        const double flo = rp_horner_s(s, RP_M, 10, lo), fhi = rp_horner_s(s, RP_M, 10, hi);
        if ((flo > 0.0) != (fhi > 0.0)) {
            const bool slo = flo > 0.0;
            for (int it = 0; it < rp::SIGN_STEPS; ++it) {
                const double mid = 0.5 * (lo + hi);
                if ((rp_horner_s(s, RP_M, 10, mid) > 0.0) == slo) lo = mid; else hi = mid;
            }
        }
        double z = 0.5 * (lo + hi);
        for (int it = 0; it < rp::NEWTON_STEPS; ++it) {    // polish: Newton steps, each kept only if it lowers |p|
            const double f = rp_horner_s(s, RP_M, 10, z), df = rp_horner_s(s, RP_M + 11, 9, z);
            const double zn = z - f / df;
            const double fn = rp_horner_s(s, RP_M, 10, zn);
            if (fabs(fn) < fabs(f)) z = zn;
        }
        // ---- (x, y) from B(z)
        double rows[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { rows[r][0] = rp_horner(bx[r], 3, z); rows[r][1] = rp_horner(by[r], 3, z); rows[r][2] = rp_horner(b1[r], 4, z); }
        double cr[3][3];
        tv::cross3(rows[0], rows[1], cr[0]); tv::cross3(rows[0], rows[2], cr[1]); tv::cross3(rows[1], rows[2], cr[2]);
        const double a0 = fabs(cr[0][2]), a1 = fabs(cr[1][2]), a2 = fabs(cr[2][2]);
        const int pick = a2 > (a1 > a0 ? a1 : a0) ? 2 : (a1 > a0 ? 1 : 0);
        const double pm = pick == 0 ? a0 : (pick == 1 ? a1 : a2);
        const double v[3] = {pick == 0 ? cr[0][0] : (pick == 1 ? cr[1][0] : cr[2][0]), pick == 0 ? cr[0][1] : (pick == 1 ? cr[1][1] : cr[2][1]),
                             pick == 0 ? cr[0][2] : (pick == 1 ? cr[1][2] : cr[2][2])};
        if (!(pm > 0.0)) continue;
        const double x = v[0] / v[2], y = v[1] / v[2];
        double E[9];
        bool ok = tv::is_finite(x) && tv::is_finite(y);
#pragma unroll
        for (int m = 0; m < 9; ++m) { E[m] = ((x * e[m][0] + y * e[m][1]) + z * e[m][2]) + e[m][3]; ok = ok && tv::is_finite(E[m]); }
        if (!ok) continue;
        // ---- decomposition
        double s2 = 0.0;
#pragma unroll
        for (int m = 0; m < 9; ++m) s2 = s2 + E[m] * E[m];
        s2 = s2 * 0.5;
        double c01[3], c02[3], c12[3];
        const double k0[3] = {E[0], E[3], E[6]}, k1[3] = {E[1], E[4], E[7]}, k2[3] = {E[2], E[5], E[8]};     // columns: t' E = 0
        tv::cross3(k0, k1, c01); tv::cross3(k0, k2, c02); tv::cross3(k1, k2, c12);
        const double n01 = tv::dot3(c01, c01), n02 = tv::dot3(c02, c02), n12 = tv::dot3(c12, c12);
        const int tp = n12 > (n02 > n01 ? n02 : n01) ? 2 : (n02 > n01 ? 1 : 0);
        const double nt = tp == 0 ? n01 : (tp == 1 ? n02 : n12);
        double tc[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) tc[m] = tp == 0 ? c01[m] : (tp == 1 ? c02[m] : c12[m]);
        if (!(nt > 0.0) || !(s2 > 0.0)) continue;
        const double tn = sqrt(nt), sc = sqrt(s2);
        const double t[3] = {tc[0] / tn, tc[1] / tn, tc[2] / tn};
        double cof[9], te[9], Ra[9], Rb[9];
        tv::cross3(E + 3, E + 6, cof); tv::cross3(E + 6, E, cof + 3); tv::cross3(E, E + 3, cof + 6);
        rp_pose_E(E, t, te);                               // [t]x E (the same products as [t]x R)
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            const double a = cof[m] / s2, b = te[m] / sc;
            Ra[m] = a - b; Rb[m] = a + b;
        }
        // ---- cheirality of the 5 sample points, poses in the order (Ra, t) (Ra, -t) (Rb, t) (Rb, -t)
        int chosen = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double R[9];
#pragma unroll
            for (int m = 0; m < 9; ++m) R[m] = q < 2 ? Ra[m] : Rb[m];
            const double sg = (q & 1) ? -1.0 : 1.0;
            const double tq[3] = {sg * t[0], sg * t[1], sg * t[2]};
            bool front = true;
            for (int i = 0; i < 5; ++i) {
                const double x1[3] = {s[RP_PTS + i], s[RP_PTS + 5 + i], 1.0};
                const double x2[3] = {s[RP_PTS + 10 + i], s[RP_PTS + 15 + i], 1.0};
                const double rx[3] = {(R[0] * x1[0] + R[1] * x1[1]) + R[2], (R[3] * x1[0] + R[4] * x1[1]) + R[5], (R[6] * x1[0] + R[7] * x1[1]) + R[8]};
                double u[3], w[3], g[3], h[3];
                tv::cross3(x2, rx, u); tv::cross3(x2, tq, w); tv::cross3(rx, tq, g); tv::cross3(rx, x2, h);
                front = front && (-tv::dot3(w, u) > 0.0) && (tv::dot3(g, h) > 0.0);
            }
            chosen = chosen < 0 && front ? q : chosen;
        }
        if (chosen < 0) continue;
        const double sg = (chosen & 1) ? -1.0 : 1.0;
        double* o = out + rp::CAND_DOUBLES * ncand;
#pragma unroll
        for (int m = 0; m < 9; ++m) o[m] = chosen < 2 ? Ra[m] : Rb[m];
#pragma unroll
        for (int m = 0; m < 3; ++m) o[9 + m] = sg * t[m];
        ++ncand;
    }
    return ncand;
}
// ---- solver end ----

struct RpArgs {
    const float* p0;          // (P, kcap, 2): the correspondences (idx0 == NULL, kcap == cap) or the key-point lists they index
    const float* p1;
    const int64_t* idx0;      // (P, cap) rows of p0 / p1 of correspondence i, or NULL
    const int64_t* idx1;
    const int32_t* counts;
    const double* K0;         // (P, 3, 3)
    const double* K1;
    int n_const, P, cap, kcap, iters, iters_pad, min_iters;
    int chunk;
    int T;                    // thresholds (1: the single call); outputs are (P, T, ...)
    double max_err[rp::MAX_THR];        // in descending order
    unsigned char slot[rp::MAX_THR];    // threshold j of the caller is max_err[slot[j]]
    double log1mp;
    unsigned long long seed;
    double* cand;             // (P, iters_pad, 10, 12)
    unsigned long long* hcost;   // (P, iters_pad, 10, T)
    unsigned* hcnt;              // (P, iters_pad, 10, T)
    int* ncand;                  // (P, iters_pad)
    int* bound;                  // (P, T)
    int* bound_max;              // (P): the largest over the thresholds (T = 1: bound itself)
    double* R;
    double* t;
    double* E;
    unsigned char* mask;
    int32_t* info;
};

// the pair's correspondences in normalised coordinates: the view of ransac_common.hpp and the calibration
struct RpPair {
    rs::PairView pts;
    double fx0, fy0, cx0, cy0, fx1, fy1, cx1, cy1, thr2;
    // thr2: of threshold max_err[slot]
    __device__ RpPair(const RpArgs& a, int pair, int slot = 0) : pts(a, pair) {
        const double* k0 = a.K0 + (size_t)pair * 9;
        const double* k1 = a.K1 + (size_t)pair * 9;
        fx0 = k0[0]; cx0 = k0[2]; fy0 = k0[4]; cy0 = k0[5];
        fx1 = k1[0]; cx1 = k1[2]; fy1 = k1[4]; cy1 = k1[5];
        thr2 = thr2_of(a.max_err[slot]);
    }
    // the squared threshold in normalised units
    __device__ inline double thr2_of(double max_err) const {
        const double thr = max_err / (0.5 * ((fx0 + fy0) * 0.5 + (fx1 + fy1) * 0.5));
        return thr * thr;
    }
    // normalised coordinates (x1, y1, x2, y2) of correspondence i
    __device__ inline double4 get(int i) const {
        const float4 q = pts.get(i);
        return make_double4(((double)q.x - cx0) / fx0, ((double)q.y - cy0) / fy0, ((double)q.z - cx1) / fx1, ((double)q.w - cy1) / fy1);
    }
};

__global__ __launch_bounds__(256) void relpose_zero_kernel(RpArgs a, size_t nhyp) {
    rs::zero_hypotheses<rp::MAX_CAND>(a.ncand, a.hcost, a.hcnt, nhyp);
}

// hypotheses [it_base + 64 blockIdx.x, + 64) of pair blockIdx.y; only below the pair's bound when `use_bound`
__global__ __launch_bounds__(64) void relpose_solve_kernel(RpArgs a, int it_base, int use_bound) {
    extern __shared__ __attribute__((aligned(16))) double rp_lds[];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int it = it_base + blockIdx.x * rp::SOLVE_WG + tid;
    const int n = rs::pair_count(a, pair);
    if (n < 5 || it >= a.iters) return;
    if (use_bound && a.bound_max[pair] <= it) return;
    const RpPair pp(a, pair);
    int idx[5] = {-1, -1, -1, -1, -1};
    if (!rs::sample_distinct(a.seed, pair, it, n, idx)) return;
    tv::Slice<rp::SOLVE_WG> s{rp_lds + tid};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double4 q = pp.get(idx[k]);
        s[RP_PTS + k] = q.x; s[RP_PTS + 5 + k] = q.y; s[RP_PTS + 10 + k] = q.z; s[RP_PTS + 15 + k] = q.w;
    }
    const size_t h = (size_t)pair * a.iters_pad + it;
    a.ncand[h] = relpose_solve(s, a.cand + h * rp::MAX_CAND * rp::CAND_DOUBLES);
}

// Hypotheses [256 (blockIdx.x + blk0), + 256) of pair blockIdx.z against correspondences [chunk blockIdx.y, + chunk)
__global__ __launch_bounds__(256) void relpose_score_kernel(RpArgs a, int blk0, int use_bound) {
    __shared__ double4 spt[rp::PTS_PER_WG];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const int c0 = blockIdx.y * a.chunk;
    const int it0 = (blockIdx.x + blk0) * rp::HYP_PER_WG;
    if (n < 5 || c0 >= n) return;
    if (use_bound && a.bound[pair] <= it0) return;
    const RpPair pp(a, pair);
    const int c1 = min(c0 + a.chunk, n);
    for (int i = tid; i < c1 - c0; i += 256) spt[i] = pp.get(c0 + i);
    __syncthreads();
    const int it = it0 + tid;
    if (it >= a.iters) return;
    const size_t h = (size_t)pair * a.iters_pad + it;
    const int nc = a.ncand[h];
    const int m = c1 - c0;
    for (int c = 0; c < nc; ++c) {
        const double* o = a.cand + (h * rp::MAX_CAND + c) * rp::CAND_DOUBLES;
        double Rm[9], tv[3], E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[k] = o[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[k] = o[9 + k];
        rp_pose_E(Rm, tv, E);
        unsigned long long sc = 0;
        unsigned cnt = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const double4 q = spt[i];
            const double r2 = tv::sampson(E, q.x, q.y, q.z, q.w);
            sc += rp_cost(r2, pp.thr2);
            cnt += r2 < pp.thr2 ? 1u : 0u;
        }
        atomicAdd(a.hcost + h * rp::MAX_CAND + c, sc);
        atomicAdd(a.hcnt + h * rp::MAX_CAND + c, cnt);
    }
}

// ---- the threshold sweep's zero and score ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relpose_sweep_zero_kernel(RpArgs a, size_t nhyp) {
    const size_t nlist = nhyp * rp::MAX_CAND * a.T;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < nlist; j += (size_t)gridDim.x * 256) {
        a.hcost[j] = 0ull; a.hcnt[j] = 0u;
        if (j < nhyp) a.ncand[j] = 0;
    }
}

// r2 against thresholds J.. of the descending list: cost and count of the inliers only
template <int J, int TP>
__device__ inline void rp_sweep_add(double r2, const double (&thr2)[TP], unsigned (&sc)[TP], unsigned (&cnt)[TP]) {
    if constexpr (J < TP) {
        if (r2 < thr2[J]) {
            sc[J] += rp_cost(r2, thr2[J]);
            ++cnt[J];
            rp_sweep_add<J + 1, TP>(r2, thr2, sc, cnt);
        }
    }
}

// relpose_score_kernel for a.T <= TP thresholds at once (the lists in the order of a.max_err).  A chunk holds at most PTS_PER_WG = 512
// correspondences and an inlier costs less than 2^20, so the inliers' cost of a chunk fits 32 bits.
template <int TP>
__global__ __launch_bounds__(256) void relpose_sweep_score_kernel(RpArgs a, int blk0, int use_bound) {
    __shared__ double4 spt[rp::PTS_PER_WG];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const int c0 = blockIdx.y * a.chunk;
    const int it0 = (blockIdx.x + blk0) * rp::HYP_PER_WG;
    if (n < 5 || c0 >= n) return;
    if (use_bound && a.bound_max[pair] <= it0) return;
    const RpPair pp(a, pair);
    double thr2[TP];
#pragma unroll
    for (int j = 0; j < TP; ++j) thr2[j] = j < a.T ? pp.thr2_of(a.max_err[j]) : 0.0;
    const int c1 = min(c0 + a.chunk, n);
    for (int i = tid; i < c1 - c0; i += 256) spt[i] = pp.get(c0 + i);
    __syncthreads();
    const int it = it0 + tid;
    if (it >= a.iters) return;
    const size_t h = (size_t)pair * a.iters_pad + it;
    const int nc = a.ncand[h];
    const int m = c1 - c0;
    for (int c = 0; c < nc; ++c) {
        const double* o = a.cand + (h * rp::MAX_CAND + c) * rp::CAND_DOUBLES;
        double Rm[9], tv[3], E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[k] = o[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[k] = o[9 + k];
        rp_pose_E(Rm, tv, E);
        unsigned sc[TP], cnt[TP];
#pragma unroll
        for (int j = 0; j < TP; ++j) { sc[j] = 0u; cnt[j] = 0u; }
#pragma unroll 2
        for (int i = 0; i < m; ++i) {
            const double4 q = spt[i];
            rp_sweep_add<0, TP>(tv::sampson(E, q.x, q.y, q.z, q.w), thr2, sc, cnt);
        }
        const size_t l = (h * rp::MAX_CAND + c) * a.T;
#pragma unroll
        for (int j = 0; j < TP; ++j)
            if (j < a.T) {
                atomicAdd(a.hcost + l + j, (unsigned long long)sc[j] + ((unsigned long long)(m - (int)cnt[j]) << 20));
                atomicAdd(a.hcnt + l + j, cnt[j]);
            }
    }
}

// After the first 256 hypotheses: the index below which the loop can still visit hypotheses = max(min_iters, rs::hypotheses_bound over
// the records (strict prefix minima of the cost) among them); a hypothesis costs the minimum over its candidates (rs::hyp_best)
// -- per threshold, and the largest of them per pair (what the later blocks are solved and scored below)
__global__ __launch_bounds__(256) void relpose_bound_kernel(RpArgs a) {
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    int bmax = 0;
    for (int j = 0; j < a.T; ++j) {
        unsigned long long cost = ~0ull;
        unsigned cnt = 0;
        int cand = 0;
        const bool has = tid < a.iters && n >= 5 && rs::hyp_best<rp::MAX_CAND, true>(a.ncand, a.hcost + j, a.hcnt + j, (size_t)pair * a.iters_pad + tid, cost, cnt, cand, a.T);
        const int bmin = rs::hypotheses_bound<5, true>(has, cost, cnt, n, a.log1mp, a.iters);
        const int b = bmin > a.min_iters ? bmin : a.min_iters;
        if (tid == 0) a.bound[pair * a.T + j] = b;
        bmax = b > bmax ? b : bmax;
        __syncthreads();                                     // hypotheses_bound's shared words read by everybody before the next threshold
    }
    if (tid == 0) a.bound_max[pair] = bmax;
}

// ---- selection, refinement, mask --------------------------------------------------------------------------------------------------------
// one Gauss-Newton step from (R, t) with the 20 sums (H upper triangle row-major, then g); false if the normal equations are not positive
__device__ inline bool rp_gn_update(const double (&sm)[rp::NSUM], const double* R, const double* t, const double* b1, const double* b2, double* Rn, double* tn) {
    double H[5][5], L[5][5], g[5], y[5], d[5];
    int k = 0;
    for (int i = 0; i < 5; ++i)
        for (int j = i; j < 5; ++j) { H[i][j] = sm[k]; H[j][i] = sm[k]; ++k; }
    for (int i = 0; i < 5; ++i) g[i] = sm[15 + i];
    for (int j = 0; j < 5; ++j) {
        double dj = H[j][j];
        for (int q = 0; q < j; ++q) dj = dj - L[j][q] * L[j][q];
        if (!(dj > 0.0)) return false;
        L[j][j] = sqrt(dj);
        for (int i = j + 1; i < 5; ++i) {
            double v = H[i][j];
            for (int q = 0; q < j; ++q) v = v - L[i][q] * L[j][q];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 5; ++i) {
        double v = -g[i];
        for (int q = 0; q < i; ++q) v = v - L[i][q] * y[q];
        y[i] = v / L[i][i];
    }
    for (int i = 4; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < 5; ++q) v = v - L[q][i] * d[q];
        d[i] = v / L[i][i];
    }
    // R cay(w)
    const double w[3] = {d[0], d[1], d[2]};
    const double n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double f = 1.0 / (1.0 + 0.25 * n2);
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double Cm[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double w2 = w[i] * w[j] - (i == j ? n2 : 0.0);
            Cm[3 * i + j] = (i == j ? 1.0 : 0.0) + f * (W[3 * i + j] + 0.5 * w2);
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (R[3 * i] * Cm[j] + R[3 * i + 1] * Cm[3 + j]) + R[3 * i + 2] * Cm[6 + j];
    double tv[3];
    for (int i = 0; i < 3; ++i) tv[i] = (t[i] + d[3] * b1[i]) + d[4] * b2[i];
    const double nn = sqrt(tv::dot3(tv, tv));
    for (int i = 0; i < 3; ++i) tn[i] = tv[i] / nn;
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && tv::is_finite(Rn[i]);
    for (int i = 0; i < 3; ++i) fin = fin && tv::is_finite(tn[i]);
    return fin;
}
// tangent basis of the unit vector t: b1 = normalise(t x e_k), k the axis of the smallest |t_k| (the first on ties), b2 = t x b1
__device__ inline void rp_tangent(const double* t, double* b1, double* b2) {
    int k = 0;
    if (fabs(t[1]) < fabs(t[k])) k = 1;
    if (fabs(t[2]) < fabs(t[k])) k = 2;
    const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double c[3];
    tv::cross3(t, ek, c);
    const double nn = sqrt(tv::dot3(c, c));
    for (int i = 0; i < 3; ++i) b1[i] = c[i] / nn;
    tv::cross3(t, b1, b2);
}

// workgroup (pair, j): threshold j of the caller on its own cost / count lists
__global__ __launch_bounds__(256) void relpose_select_kernel(RpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double pose_sh[12];
    __shared__ unsigned long long sc_sh;
    __shared__ unsigned cnt_sh;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int slot = a.slot[blockIdx.y];
    const size_t out = (size_t)pair * a.T + blockIdx.y;
    const int n = rs::pair_count(a, pair);
    unsigned char* mask = a.mask + out * a.cap;
    int32_t* info = a.info + out * 8;

    // ---- the stopping rule of the sequential loop, over tiles of the cost list
    int best, best_cand, iters_run;
    rs::scan_stopping_rule<5, true>(lds_raw, n, a.iters, a.min_iters, a.log1mp,
                                    [&](int it, unsigned long long& c, unsigned& k, int& cd) {
                                        return rs::hyp_best<rp::MAX_CAND, true>(a.ncand, a.hcost + slot, a.hcnt + slot, (size_t)pair * a.iters_pad + it, c, k, cd, a.T);
                                    },
                                    best, best_cand, iters_run);
    if (best >= 0 && tid < 12) pose_sh[tid] = a.cand[(((size_t)pair * a.iters_pad + best) * rp::MAX_CAND + best_cand) * rp::CAND_DOUBLES + tid];
    __syncthreads();
    double* Rout = a.R + out * 9;
    double* tout = a.t + out * 3;
    double* Eout = a.E + out * 9;
    if (best < 0) {
        rs::write_nothing_found(mask, a.cap, info, iters_run, n);
        if (tid < 9) { Rout[tid] = 0.0; Eout[tid] = 0.0; }
        if (tid < 3) tout[tid] = 0.0;
        return;
    }
    const RpPair pp(a, pair, slot);
    const double thr2 = pp.thr2;
    double* red = reinterpret_cast<double*>(lds_raw);         // the tiles are dead: reduction buffer from here on
    double4* spt = reinterpret_cast<double4*>(lds_raw + (rs::block_sums_bytes(rp::NSUM) + 31 & ~(size_t)31));
    for (int i = tid; i < min(n, rp::SEL_CACHE); i += 256) spt[i] = pp.get(i);
    __syncthreads();
    auto for_each = [&](auto&& f) { rs::for_each_cached(spt, n, [&](int i) { return pp.get(i); }, f); };
    double Rc[9], tcur[3], Rb[9], tb[3];
    for (int k = 0; k < 9; ++k) { Rc[k] = pose_sh[k]; Rb[k] = Rc[k]; }
    for (int k = 0; k < 3; ++k) { tcur[k] = pose_sh[9 + k]; tb[k] = tcur[k]; }
    unsigned long long c_best = ~0ull;
    int lo_accepted = 0;
    for (int step = 0; step <= rp::LO_ITERS; ++step) {
        if (tid == 0) sc_sh = 0ull;
        __syncthreads();
        double E[9], b1[3], b2[3];
        rp_pose_E(Rc, tcur, E);
        rp_tangent(tcur, b1, b2);
        double sm[rp::NSUM];
        for (int k = 0; k < rp::NSUM; ++k) sm[k] = 0.0;
        unsigned long long sc = 0;
        for_each([&](int, const double4& q) {
            const double pa = q.x, pb = q.y, pc = q.z, pd = q.w;
            const double e0 = (E[0] * pa + E[1] * pb) + E[2], e1 = (E[3] * pa + E[4] * pb) + E[5], e2 = (E[6] * pa + E[7] * pb) + E[8];
            const double f0 = (E[0] * pc + E[3] * pd) + E[6], f1 = (E[1] * pc + E[4] * pd) + E[7], f2 = (E[2] * pc + E[5] * pd) + E[8];
            const double num = (pc * e0 + pd * e1) + e2;
            const double den = ((e0 * e0 + e1 * e1) + f0 * f0) + f1 * f1;
            const double r2 = num * num / den;
            sc += rp_cost(r2, thr2);
            if (r2 < thr2) {
                const double w = 1.0 / den;
                const double rx0 = (Rc[0] * pa + Rc[1] * pb) + Rc[2], rx1 = (Rc[3] * pa + Rc[4] * pb) + Rc[5], rx2 = (Rc[6] * pa + Rc[7] * pb) + Rc[8];
                const double g0 = rx1 - rx2 * pd, g1 = rx2 * pc - rx0, g2 = rx0 * pd - rx1 * pc;
                const double J[5] = {pb * f2 - f1, f0 - pa * f2, pa * f1 - pb * f0, (b1[0] * g0 + b1[1] * g1) + b1[2] * g2, (b2[0] * g0 + b2[1] * g1) + b2[2] * g2};
                int k = 0;
                for (int i = 0; i < 5; ++i) {
                    const double wj = w * J[i];
                    for (int j = i; j < 5; ++j) { sm[k] = sm[k] + wj * J[j]; ++k; }
                    sm[15 + i] = sm[15 + i] + wj * num;
                }
            }
        });
        atomicAdd(&sc_sh, sc);
        rs::block_sums(sm, red);                              // (its barriers also publish sc_sh)
        const unsigned long long c_now = sc_sh;
        if (step > 0 && !(c_now < c_best)) break;
        for (int k = 0; k < 9; ++k) Rb[k] = Rc[k];
        for (int k = 0; k < 3; ++k) tb[k] = tcur[k];
        if (step > 0) ++lo_accepted;
        c_best = c_now;
        if (step == rp::LO_ITERS) break;
        double Rn[9], tn2[3];
        if (!rp_gn_update(sm, Rc, tcur, b1, b2, Rn, tn2)) break;
        for (int k = 0; k < 9; ++k) Rc[k] = Rn[k];
        for (int k = 0; k < 3; ++k) tcur[k] = tn2[k];
        __syncthreads();                                     // sc_sh read by everybody before it is cleared again
    }
    // ---- inlier mask under the final pose
    double Eb[9];
    rp_pose_E(Rb, tb, Eb);
    __syncthreads();
    if (tid == 0) cnt_sh = 0u;
    __syncthreads();
    unsigned cn = 0;
    for_each([&](int, const double4& q) { cn += tv::sampson(Eb, q.x, q.y, q.z, q.w) < thr2 ? 1u : 0u; });
    atomicAdd(&cnt_sh, cn);
    __syncthreads();
    const int n_in = (int)cnt_sh;
    const bool found = n_in >= 5;
    for_each([&](int i, const double4& q) { mask[i] = found && tv::sampson(Eb, q.x, q.y, q.z, q.w) < thr2 ? 1 : 0; });
    for (int i = n + tid; i < a.cap; i += 256) mask[i] = 0;
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) { Rout[k] = found ? Rb[k] : 0.0; Eout[k] = found ? Eb[k] : 0.0; }
        for (int k = 0; k < 3; ++k) tout[k] = found ? tb[k] : 0.0;
        rs::write_info(info, found, best, iters_run, n_in, lo_accepted, n, c_best);
    }
}

size_t relpose_workspace_bytes(int P, int max_iters) {
    const size_t pad = (size_t)ceil_div(max_iters, 256) * 256;
    const size_t per = (size_t)rp::MAX_CAND * rp::CAND_DOUBLES * 8 + (size_t)rp::MAX_CAND * 12 + 4;
    return (size_t)P * pad * per + (size_t)P * 4 + 1024;
}
size_t relpose_sweep_workspace_bytes(int P, int max_iters, int T) {
    const size_t pad = (size_t)ceil_div(max_iters, 256) * 256;
    const size_t per = (size_t)rp::MAX_CAND * rp::CAND_DOUBLES * 8 + (size_t)T * rp::MAX_CAND * 12 + 4;
    return (size_t)P * pad * per + (size_t)P * (T + 1) * 4 + 1024;
}

// T thresholds in the caller's order; T = 1 is the single call, kernel for kernel
int launch_estimate_relpose_sweep(const float* p0, const float* p1, const int64_t* idx0, const int64_t* idx1, int kcap, const int32_t* counts, int n_const,
                                  int P, int cap, const double* K0, const double* K1, const double* max_errs, int T, int min_iters, int max_iters,
                                  double success_prob, unsigned long long seed, double* R, double* t, double* E, unsigned char* mask, int32_t* info,
                                  void* ws, hipStream_t st) {
    if (max_iters < 1 || max_iters > rp::MAX_ITERS || P > 65535 || T < 1 || T > rp::MAX_THR) return -1;
    RpArgs a;
    a.p0 = p0; a.p1 = p1; a.idx0 = idx0; a.idx1 = idx1; a.kcap = idx0 ? kcap : cap; a.counts = counts; a.n_const = n_const; a.P = P; a.cap = cap;
    a.K0 = K0; a.K1 = K1; a.iters = max_iters; a.iters_pad = ceil_div(max_iters, 256) * 256; a.min_iters = min_iters < 0 ? 0 : min_iters;
    a.log1mp = log(1.0 - success_prob); a.seed = seed;
    a.T = T;
    int order[rp::MAX_THR];                                  // the thresholds in descending order (stable: repeated values keep their order)
    for (int j = 0; j < T; ++j) {
        int k = j;
        for (; k > 0 && max_errs[order[k - 1]] < max_errs[j]; --k) order[k] = order[k - 1];
        order[k] = j;
    }
    for (int k = 0; k < rp::MAX_THR; ++k) { a.max_err[k] = k < T ? max_errs[order[k]] : 0.0; a.slot[k] = 0; }
    for (int k = 0; k < T; ++k) a.slot[order[k]] = (unsigned char)k;
    unsigned char* w = static_cast<unsigned char*>(ws);
    const size_t nhyp = (size_t)P * a.iters_pad;
    a.cand = reinterpret_cast<double*>(w); w += nhyp * rp::MAX_CAND * rp::CAND_DOUBLES * 8;
    a.hcost = reinterpret_cast<unsigned long long*>(w); w += nhyp * rp::MAX_CAND * T * 8;
    a.hcnt = reinterpret_cast<unsigned*>(w); w += nhyp * rp::MAX_CAND * T * 4;
    a.ncand = reinterpret_cast<int*>(w); w += nhyp * 4;
    a.bound = reinterpret_cast<int*>(w);
    a.bound_max = T == 1 ? a.bound : a.bound + (size_t)P * T;
    a.R = R; a.t = t; a.E = E; a.mask = mask; a.info = info;
    a.chunk = rs::score_chunk(P, cap);
    const int nblk = ceil_div(max_iters, rp::HYP_PER_WG), nch = ceil_div(cap, a.chunk);
    auto score = [&](int blocks, int blk0, int use_bound) {
        const dim3 grid(blocks, nch, P);
        if (T == 1) relpose_score_kernel<<<grid, 256, 0, st>>>(a, blk0, use_bound);
        else if (T <= 4) relpose_sweep_score_kernel<4><<<grid, 256, 0, st>>>(a, blk0, use_bound);
        else if (T <= 8) relpose_sweep_score_kernel<8><<<grid, 256, 0, st>>>(a, blk0, use_bound);
        else if (T <= 12) relpose_sweep_score_kernel<12><<<grid, 256, 0, st>>>(a, blk0, use_bound);
        else relpose_sweep_score_kernel<16><<<grid, 256, 0, st>>>(a, blk0, use_bound);
    };
    if (T == 1) {
        const size_t zg = (nhyp + 255) / 256;
        relpose_zero_kernel<<<(unsigned)(zg > 2048 ? 2048 : zg), 256, 0, st>>>(a, nhyp);
    } else {
        const size_t zg = (nhyp * rp::MAX_CAND * T + 255) / 256;
        relpose_sweep_zero_kernel<<<(unsigned)(zg > 8192 ? 8192 : zg), 256, 0, st>>>(a, nhyp);
    }
    const size_t solve_lds = (size_t)rp::SLICE * rp::SOLVE_WG * sizeof(double);
    static AttrMask attr_solve = 0, attr_sel = 0;
    set_max_dynamic_lds(reinterpret_cast<const void*>(relpose_solve_kernel), (int)solve_lds, attr_solve);
    const int first = max_iters < rp::HYP_PER_WG ? max_iters : rp::HYP_PER_WG;
    relpose_solve_kernel<<<dim3(ceil_div(first, rp::SOLVE_WG), P), rp::SOLVE_WG, solve_lds, st>>>(a, 0, 0);
    score(1, 0, 0);
    if (nblk > 1) {
        relpose_bound_kernel<<<P, 256, 0, st>>>(a);
        relpose_solve_kernel<<<dim3(ceil_div(max_iters - rp::HYP_PER_WG, rp::SOLVE_WG), P), rp::SOLVE_WG, solve_lds, st>>>(a, rp::HYP_PER_WG, 1);
        score(nblk - 1, 1, 1);
    }
    const size_t red = (rs::block_sums_bytes(rp::NSUM) + 31) & ~(size_t)31;
    const size_t tiles = (size_t)rp::SEL_TILE * 16;
    const size_t front = red > tiles ? red : tiles;
    const size_t lds = (front > red ? front : red) + (size_t)rp::SEL_CACHE * sizeof(double4);
    set_max_dynamic_lds(reinterpret_cast<const void*>(relpose_select_kernel), (int)lds, attr_sel);
    relpose_select_kernel<<<dim3(P, T), 256, lds, st>>>(a);
    return 0;
}

int launch_estimate_relpose(const float* p0, const float* p1, const int64_t* idx0, const int64_t* idx1, int kcap, const int32_t* counts, int n_const,
                            int P, int cap, const double* K0, const double* K1, double max_err, int min_iters, int max_iters, double success_prob,
                            unsigned long long seed, double* R, double* t, double* E, unsigned char* mask, int32_t* info, void* ws, hipStream_t st) {
    return launch_estimate_relpose_sweep(p0, p1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, &max_err, 1, min_iters, max_iters, success_prob, seed,
                                         R, t, E, mask, info, ws, st);
}

}  // namespace xfh
