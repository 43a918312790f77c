// Fundamental matrix from the match lists: the device side of
//     F, inliers = cv2.findFundamentalMat(points1, points2, cv2.USAC_MAGSAC, thr, confidence, maxIters)
// for uncalibrated, non-planar pairs.  The reference never calls it; it completes the two-view models next to the homography
// (k_homography.hip) and the essential matrix (k_relpose.hip).  OpenCV is not available offline: what is implemented is the published
// estimator -- RANSAC over the 7-point solver with the oriented epipolar constraint (Chum, Werner, Matas 2004), the MAGSAC++ quality and
// sigma-consensus++ re-weighted refinement (Barath et al., CVPR 2020).  The specification (tests/fundamental_reference.py
// restates it in numpy operation for operation, tests/test_fundamental_emulated.py compiles the solver below on the host and holds it
// to that restatement bit for bit):
//   * conditioning: per pair a Hartley similarity, centroid c then scale s = sqrt(2) / (mean distance to c), both from fixed-order block
//     sums (fundamental_prep_kernel, rs::hartley_conditioning of ransac_common.hpp); x_n = (x - c) s.  The solver works in normalised coordinates, the score in pixels;
//   * sample: 7 distinct correspondences, drawn as ransac_common.hpp states (splitmix64 of (seed, pair, hypothesis, draw); duplicates
//     are redrawn, 16 draws at most; a sample that runs out of draws yields no model);
//   * minimal solver (fm_solve): null space (F1, F2) of the 7x9 constraint matrix by Gauss-Jordan with partial pivoting (a pivot below
//     tv::PIVOT_EPS of twoview_math.hpp or not finite: no model); det(F2 + a (F1 - F2)) = c3 a^3 + c2 a^2 + c1 a + c0 by polynomial products in a fixed order,
//     made monic (c3 zero or not finite: no model); its real roots with + - * / sqrt only: the derivative's roots split [-B, B]
//     (B = 1 + max |a_k|, Cauchy) into monotone brackets, each bracket with a sign change gets BISECT_STEPS bisections on the sign, then
//     NEWTON_STEPS Newton steps, each kept only if it lowers |p|; roots in ascending order, at most 3;
//   * oriented epipolar constraint: e' = the cross product of two columns of F (the pair with the largest norm), the root is dropped
//     unless (e' x x1) . (F x0) has one strict sign over the 7 sample points;
//   * score of a candidate (F back in pixels, F = T1' Fn T0): Sampson error r^2 = (x1' F x0)^2 / ((F x0)_1^2 + (F x0)_2^2 + (F' x1)_1^2
//     + (F' x1)_2^2); MAGSAC++ quality = sum over r^2 < (2 thr)^2 of the 20-bit table entry of r^2's bin (the homography's tables:
//     n = 4 degrees of freedom, k = 3.64, sigma_max = 2 thr / k, 4096 bins), summed as u64 (no summation order); inlier: r^2 < thr^2
//     (NaN: never); a hypothesis scores the best of its candidates (ties: the lower root);
//   * stopping rule: hypotheses in order, a strictly better quality bounds the loop by ceil(log(1 - confidence) / log(1 - w^7))
//     (rs::scan_stopping_rule of ransac_common.hpp);
//   * refinement of the winner: up to LO_ITERS re-weighted 8-point fits (Hartley-normalised, weights w(r) / w(0) from the same bins),
//     the 45 sums of the 9x9 normal matrix from fixed-order block reductions (rs::block_sums), its smallest eigenvector by cyclic Jacobi (JACOBI_SWEEPS
//     sweeps), rank 2 by removing the smallest singular value (smallest eigenvector v of Fn' Fn, Fn <- Fn - (Fn v) v'), each step kept
//     only if it raises the quality;
//   * mask: r^2 < thr^2 under the final F; found = at least 7 inliers; F scaled to unit Frobenius norm, then divided by F[2,2] when
//     |F[2,2]| > FLT_EPSILON; zeros when nothing is found;
//   * FM_8POINT: one unit-weight 8-point fit on all n >= 8 points; FM_7POINT: the solver on exactly 7 points, every real root (no
//     oriented check), up to 3 models stacked; the mask is all ones for the points used, as cv2 writes it.
// Only + - * / sqrt in the geometry, every product and sum rounded once (fp contraction off in this file).
//
// The register budget.  The solver's runtime-indexed state is the 7x9 matrix (pivot rows) and the sample: 91 fp64 in a per-thread slice
// of LDS (element k of thread j at lds[k * 64 + j]), 64 hypotheses per workgroup = 46.6 KiB, three workgroups per CU; the null vectors,
// the cubic and the candidates stay in registers.  The refinement's 9x9 Jacobi runs on one thread of the pair's workgroup, in LDS.
//
// Launches per call (workspace: tables, per pair the conditioning and the bound, per hypothesis 3 candidates + 3 scores + 3 counts + the
// candidate count):
//   homog_tables_kernel         : quality / weight tables of this threshold (k_homography.hip, through launch_homography_tables)
//   fundamental_zero_kernel     : scores, counts, candidate counts zeroed
//   fundamental_prep_kernel     : one workgroup per pair: the Hartley conditioning
//   fundamental_solve_kernel    : thread = hypothesis: sample, solver, candidates into the workspace      (hypotheses 0..255 first)
//   fundamental_score_kernel    : thread = hypothesis, its candidates in turn against a chunk of correspondences in LDS, u64 atomics
//   fundamental_bound_kernel    : the bound the loop reaches from the records among the first 256; later blocks run only below it
//   fundamental_select_kernel   : one workgroup per pair: stopping rule over the score list (tiles in LDS), refinement, mask, outputs
#include "ransac_common.hpp"
#include "twoview_math.hpp"

#pragma clang fp contract(off)

namespace xfh {
namespace fm {
using rs::NBINS, rs::HYP_PER_WG, rs::PTS_PER_WG, rs::SEL_TILE, rs::SEL_CACHE;
constexpr int LO_ITERS = 5, MAX_ITERS = 16384, SOLVE_WG = 64, NSUM = 45;
constexpr double MAX_THR_FACTOR = 2.0;          // the tables (k = 3.64, 4096 bins) are the homography's
constexpr int METHOD_7POINT = 1, METHOD_8POINT = 2, METHOD_MAGSAC = 38;
}  // namespace fm

// ---- fm solver begin (host-compilable: tests/test_fundamental_emulated.py slices it out behind the slice of twoview_math.hpp and drops
// the __device__ qualifiers) ----
namespace fm {
constexpr int MAX_CAND = 3, SLICE = 91, BISECT_STEPS = 64, NEWTON_STEPS = 3, JACOBI_SWEEPS = 10;
constexpr double FLT_EPS = 1.1920928955078125e-07, FIT_RANK_EPS = 1e-12;
}  // namespace fm
// slice layout (fp64 elements): [0, 63) the 7x9 constraint matrix, [63, 91) the sample: x0[7] y0[7] x1[7] y1[7] (normalised)
constexpr int FM_M = 0, FM_PTS = 63;

// the pair's Hartley similarities: x_n = (x - cx) s
struct FmNorm {
    double cx0, cy0, s0, cx1, cy1, s1;
};

// monic cubic x^3 + a2 x^2 + a1 x + a0 and its derivative (b2 = 2 a2)
__device__ inline double fm_cubic(const double* a, double x) { return ((x + a[2]) * x + a[1]) * x + a[0]; }
__device__ inline double fm_dcubic(const double* a, double b2, double x) { return (3.0 * x + b2) * x + a[1]; }

// real roots of the monic cubic, ascending; returns their number (0..3)
__device__ inline int fm_cubic_roots(const double* a, double* roots) {
    double bound = fabs(a[0]);
    bound = fabs(a[1]) > bound ? fabs(a[1]) : bound;
    bound = fabs(a[2]) > bound ? fabs(a[2]) : bound;
    bound = 1.0 + bound;
    if (!tv::is_finite(bound)) return 0;
    // brackets [e0, e1], [e1, e2], [e2, e3]: split at the derivative's roots when it has two, else one bracket [-B, B]
    double e[4] = {-bound, bound, bound, bound};
    const double disc = a[2] * a[2] - 3.0 * a[1];
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        e[1] = (-a[2] - sq) / 3.0;
        e[2] = (-a[2] + sq) / 3.0;
    }
    const double b2 = 2.0 * a[2];
    int nr = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double lo = e[j], hi = e[j + 1];
        const double flo = fm_cubic(a, lo), fhi = fm_cubic(a, hi);
        if ((flo > 0.0) == (fhi > 0.0)) continue;
        const bool slo = flo > 0.0;
        for (int it = 0; it < fm::BISECT_STEPS; ++it) {
            const double mid = 0.5 * (lo + hi);
            if ((fm_cubic(a, mid) > 0.0) == slo) lo = mid; else hi = mid;
        }
        double z = 0.5 * (lo + hi);
        for (int it = 0; it < fm::NEWTON_STEPS; ++it) {       // polish: Newton steps, each kept only if it lowers |p|
            const double f = fm_cubic(a, z), df = fm_dcubic(a, b2, z);
            const double zn = z - f / df;
            if (fabs(fm_cubic(a, zn)) < fabs(f)) z = zn;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) roots[k] = k == nr ? z : roots[k];     // (a register array: no runtime index)
        ++nr;
    }
    return nr;
}

// Hartley-normalised F -> pixels: Fp = T1' Fn T0, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
__device__ inline void fm_denormalise(const double* Fn, const FmNorm& t, double* Fp) {
    const double tx0 = t.s0 * t.cx0, ty0 = t.s0 * t.cy0, tx1 = t.s1 * t.cx1, ty1 = t.s1 * t.cy1;
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = Fn[3 * i] * t.s0;
        G[3 * i + 1] = Fn[3 * i + 1] * t.s0;
        G[3 * i + 2] = Fn[3 * i + 2] - (Fn[3 * i] * tx0 + Fn[3 * i + 1] * ty0);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Fp[j] = t.s1 * G[j];
        Fp[3 + j] = t.s1 * G[3 + j];
        Fp[6 + j] = G[6 + j] - (tx1 * G[j] + ty1 * G[3 + j]);
    }
}

// candidate F (pixels, row-major) of the 7-point sample in S[FM_PTS ..] into out[9 c ..]; returns their number (0: no model)
template <class S>
__device__ inline int fm_solve(S s, const FmNorm& nt, bool oriented, double* out) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double a = s[FM_PTS + k], b = s[FM_PTS + 7 + k], c = s[FM_PTS + 14 + k], d = s[FM_PTS + 21 + k];
        const double r[9] = {c * a, c * b, c, d * a, d * b, d, a, b, 1.0};
#pragma unroll
        for (int j = 0; j < 9; ++j) s[FM_M + 9 * k + j] = r[j];
    }
    if (!tv::gauss_jordan(s, FM_M, 7, 9)) return 0;
    // null vectors (-C[:, k], e_k) of the reduced matrix [I | C]; F(a) = F2 + a D, D = F1 - F2
    double f2[9], D[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) {
        const double v1 = m < 7 ? -s[FM_M + 9 * m + 7] : (m == 7 ? 1.0 : 0.0);
        const double v2 = m < 7 ? -s[FM_M + 9 * m + 8] : (m == 8 ? 1.0 : 0.0);
        f2[m] = v2;
        D[m] = v1 - v2;
    }
    // det F(a) = m0 (m4 m8 - m5 m7) - m1 (m3 m8 - m5 m6) + m2 (m3 m7 - m4 m6), entries m_i = f2_i + a D_i
    double c[4];
    {
        double m[9][2];
#pragma unroll
        for (int i = 0; i < 9; ++i) { m[i][0] = f2[i]; m[i][1] = D[i]; }
        double t1[3], t2[3], q0[3], q1[3], q2[3], w[4];
        tv::pmul(m[4], 1, m[8], 1, t1); tv::pmul(m[5], 1, m[7], 1, t2);
#pragma unroll
        for (int k = 0; k < 3; ++k) q0[k] = t1[k] - t2[k];
        tv::pmul(m[3], 1, m[8], 1, t1); tv::pmul(m[5], 1, m[6], 1, t2);
#pragma unroll
        for (int k = 0; k < 3; ++k) q1[k] = t1[k] - t2[k];
        tv::pmul(m[3], 1, m[7], 1, t1); tv::pmul(m[4], 1, m[6], 1, t2);
#pragma unroll
        for (int k = 0; k < 3; ++k) q2[k] = t1[k] - t2[k];
        tv::pmul(m[0], 1, q0, 2, c);
        tv::pmul(m[1], 1, q1, 2, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = c[k] - w[k];
        tv::pmul(m[2], 1, q2, 2, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = c[k] + w[k];
    }
    const double lead = c[3];
    if (!(fabs(lead) > 0.0) || !tv::is_finite(lead)) return 0;
    const double a[3] = {c[0] / lead, c[1] / lead, c[2] / lead};
    double roots[3] = {0.0, 0.0, 0.0};
    const int nr = fm_cubic_roots(a, roots);
    int ncand = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (r >= nr) continue;
        const double z = roots[r];
        double Fn[9];
        bool ok = true;
#pragma unroll
        for (int m = 0; m < 9; ++m) { Fn[m] = f2[m] + z * D[m]; ok = ok && tv::is_finite(Fn[m]); }
        if (!ok) continue;
        if (oriented) {
            // epipole e' in image 1 (e'' F = 0): the cross product of two columns of F, the pair with the largest norm
            const double k0[3] = {Fn[0], Fn[3], Fn[6]}, k1[3] = {Fn[1], Fn[4], Fn[7]}, k2[3] = {Fn[2], Fn[5], Fn[8]};
            double c01[3], c02[3], c12[3];
            tv::cross3(k0, k1, c01); tv::cross3(k0, k2, c02); tv::cross3(k1, k2, c12);
            const double n01 = tv::dot3(c01, c01), n02 = tv::dot3(c02, c02), n12 = tv::dot3(c12, c12);
            const int tp = n12 > (n02 > n01 ? n02 : n01) ? 2 : (n02 > n01 ? 1 : 0);
            const double ne = tp == 0 ? n01 : (tp == 1 ? n02 : n12);
            double ep[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) ep[k] = tp == 0 ? c01[k] : (tp == 1 ? c02[k] : c12[k]);
            if (!(ne > 0.0)) continue;
            int pos = 0, neg = 0;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const double xa = s[FM_PTS + i], xb = s[FM_PTS + 7 + i];
                const double x1[3] = {s[FM_PTS + 14 + i], s[FM_PTS + 21 + i], 1.0};
                const double fx[3] = {(Fn[0] * xa + Fn[1] * xb) + Fn[2], (Fn[3] * xa + Fn[4] * xb) + Fn[5], (Fn[6] * xa + Fn[7] * xb) + Fn[8]};
                double ex[3];
                tv::cross3(ep, x1, ex);
                const double v = tv::dot3(ex, fx);
                pos += v > 0.0 ? 1 : 0;
                neg += v < 0.0 ? 1 : 0;
            }
            if (pos != 7 && neg != 7) continue;
        }
        double Fp[9];
        fm_denormalise(Fn, nt, Fp);
#pragma unroll
        for (int m = 0; m < 9; ++m) ok = ok && tv::is_finite(Fp[m]);
        if (!ok) continue;
        double* o = out + 9 * ncand;
#pragma unroll
        for (int m = 0; m < 9; ++m) o[m] = Fp[m];
        ++ncand;
    }
    return ncand;
}

// cyclic Jacobi on the symmetric N x N matrix A (row-major, both triangles), V <- its eigenvectors (columns), JACOBI_SWEEPS sweeps
template <int N, class S>
__device__ inline void fm_jacobi(S A, S V) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sw = 0; sw < fm::JACOBI_SWEEPS; ++sw)
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double app = A[p * N + p], aqq = A[q * N + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double r = sqrt(theta * theta + 1.0);
                const double t = theta >= 0.0 ? 1.0 / (theta + r) : -1.0 / (r - theta);
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < N; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    const double np = c * akp - sn * akq, nq = sn * akp + c * akq;
                    A[k * N + p] = np; A[p * N + k] = np;
                    A[k * N + q] = nq; A[q * N + k] = nq;
                }
                A[p * N + p] = app - t * apq;
                A[q * N + q] = aqq + t * apq;
                A[p * N + q] = 0.0;
                A[q * N + p] = 0.0;
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - sn * vkq;
                    V[k * N + q] = sn * vkp + c * vkq;
                }
            }
}
template <int N, class S>
__device__ inline int fm_smallest(S A) {
    int m = 0;
    for (int k = 1; k < N; ++k)
        if (A[k * N + k] < A[m * N + m]) m = k;
    return m;
}

// 8-point fit from the 45 sums of w a a' (upper triangle, row-major; a = the constraint row of a normalised correspondence): smallest
// eigenvector, rank 2, back to pixels.  A, V: 81 fp64 each of working space (LDS on the device).  false if the normal matrix has rank
// below 8 (second smallest eigenvalue <= FIT_RANK_EPS x the largest) or the result is not finite.
template <class S>
__device__ inline bool fm_fit8(const double* sm, S A, S V, const FmNorm& nt, double* Fp) {
    int k = 0;
    for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j) { A[9 * i + j] = sm[k]; A[9 * j + i] = sm[k]; ++k; }
    fm_jacobi<9>(A, V);
    int m = fm_smallest<9>(A);
    // rank of the normal matrix below 8 (e.g. collinear points): the second smallest eigenvalue vanishes against the largest
    double l2 = 0.0, lmax = 0.0;
    bool first = true;
    for (int i = 0; i < 9; ++i) {
        const double d = A[9 * i + i];
        lmax = d > lmax ? d : lmax;
        if (i != m && (first || d < l2)) { l2 = d; first = false; }
    }
    if (!(l2 > fm::FIT_RANK_EPS * lmax)) return false;
    double Fn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Fn[i] = V[9 * i + m];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[3 * i + j] = (Fn[i] * Fn[j] + Fn[3 + i] * Fn[3 + j]) + Fn[6 + i] * Fn[6 + j];
    fm_jacobi<3>(A, V);
    m = fm_smallest<3>(A);
    const double v[3] = {V[m], V[3 + m], V[6 + m]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double u = (Fn[3 * i] * v[0] + Fn[3 * i + 1] * v[1]) + Fn[3 * i + 2] * v[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) Fn[3 * i + j] = Fn[3 * i + j] - u * v[j];
    }
    fm_denormalise(Fn, nt, Fp);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && tv::is_finite(Fp[i]);
    return fin;
}

// output scaling: unit Frobenius norm, then F[2,2] = 1 when |F[2,2]| > FLT_EPSILON
__device__ inline void fm_scale_out(const double* F, double* o) {
    double nn = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) nn = nn + F[k] * F[k];
    nn = sqrt(nn);
    double g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = F[k] / nn;
    const double d = g[8];
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = fabs(d) > fm::FLT_EPS ? g[k] / d : g[k];
}
// ---- fm solver end ----

struct FmArgs {
    const float* p0;          // (P, kcap, 2): the correspondences (idx0 == NULL, kcap == cap) or the key-point lists they index
    const float* p1;
    const int64_t* idx0;      // (P, cap) rows of p0 / p1 of correspondence i, or NULL
    const int64_t* idx1;
    const int32_t* counts;
    int n_const, P, cap, kcap, iters, iters_pad, method, chunk;
    double thr2, tmax2, bin_scale, log1mc;
    unsigned long long seed;
    const unsigned* stab;
    const double* wtab;
    double* norm;                 // (P, 8): cx0 cy0 s0 cx1 cy1 s1
    double* cand;                 // (P, iters_pad, 3, 9)
    unsigned long long* hscore;   // (P, iters_pad, 3)
    unsigned* hcnt;               // (P, iters_pad, 3)
    int* ncand;                   // (P, iters_pad)
    int* bound;                   // (P)
    double* F;                    // (P, 3, 9)
    unsigned char* mask;
    int32_t* info;
};

__device__ inline FmNorm fm_norm(const FmArgs& a, int pair) {
    const double* q = a.norm + (size_t)pair * 8;
    return FmNorm{q[0], q[1], q[2], q[3], q[4], q[5]};
}
// minimum number of correspondences of the method
__device__ inline int fm_min_n(const FmArgs& a) { return a.method == fm::METHOD_8POINT ? 8 : 7; }

__global__ __launch_bounds__(256) void fundamental_zero_kernel(FmArgs a, size_t nhyp) {
    rs::zero_hypotheses<fm::MAX_CAND>(a.ncand, a.hscore, a.hcnt, nhyp);
}

// one workgroup per pair: the Hartley conditioning of both point sets
__global__ __launch_bounds__(256) void fundamental_prep_kernel(FmArgs a) {
    __shared__ double red[rs::block_sums_bytes(4) / sizeof(double)];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const rs::PairView pts(a, pair);
    double nt[6];
    rs::hartley_conditioning([&](auto&& f) { for (int i = tid; i < n; i += 256) f(i, pts.get(i)); }, (double)(n > 0 ? n : 1), red, nt);
    if (tid == 0) {
        double* o = a.norm + (size_t)pair * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = k < 6 ? nt[k] : 0.0;
    }
}

// hypotheses [it_base + 64 blockIdx.x, + 64) of pair blockIdx.y; only below the pair's bound when `use_bound`.  FM_7POINT: hypothesis 0
// is the 7 points in order, every real root kept.
__global__ __launch_bounds__(64) void fundamental_solve_kernel(FmArgs a, int it_base, int use_bound) {
    extern __shared__ __attribute__((aligned(16))) double fm_lds[];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int it = it_base + blockIdx.x * fm::SOLVE_WG + tid;
    const int n = rs::pair_count(a, pair);
    const bool seven = a.method == fm::METHOD_7POINT;
    if (seven ? (n != 7 || it != 0) : (n < 7 || it >= a.iters)) return;
    if (use_bound && a.bound[pair] <= it) return;
    const rs::PairView pts(a, pair);
    int idx[7] = {0, 1, 2, 3, 4, 5, 6};
    if (!seven && !rs::sample_distinct(a.seed, pair, it, n, idx)) return;
    const FmNorm nt = fm_norm(a, pair);
    tv::Slice<fm::SOLVE_WG> s{fm_lds + tid};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float4 q = pts.get(idx[k]);
        s[FM_PTS + k] = ((double)q.x - nt.cx0) * nt.s0;
        s[FM_PTS + 7 + k] = ((double)q.y - nt.cy0) * nt.s0;
        s[FM_PTS + 14 + k] = ((double)q.z - nt.cx1) * nt.s1;
        s[FM_PTS + 21 + k] = ((double)q.w - nt.cy1) * nt.s1;
    }
    const size_t h = (size_t)pair * a.iters_pad + it;
    a.ncand[h] = fm_solve(s, nt, !seven, a.cand + h * fm::MAX_CAND * 9);
}

// Hypotheses [256 (blockIdx.x + blk0), + 256) of pair blockIdx.z against correspondences [chunk blockIdx.y, + chunk)
__global__ __launch_bounds__(256) void fundamental_score_kernel(FmArgs a, int blk0, int use_bound) {
    __shared__ unsigned stab[fm::NBINS];
    __shared__ float4 spt[fm::PTS_PER_WG];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const int c0 = blockIdx.y * a.chunk;
    const int it0 = (blockIdx.x + blk0) * fm::HYP_PER_WG;
    if (n < 7 || c0 >= n) return;
    if (use_bound && a.bound[pair] <= it0) return;
    const rs::PairView pts(a, pair);
    const int c1 = min(c0 + a.chunk, n);
#pragma unroll
    for (int k = 0; k < fm::NBINS / 256; ++k) stab[tid + 256 * k] = a.stab[tid + 256 * k];
    for (int i = tid; i < c1 - c0; i += 256) spt[i] = pts.get(c0 + i);
    __syncthreads();
    const int it = it0 + tid;
    if (it >= a.iters) return;
    const size_t h = (size_t)pair * a.iters_pad + it;
    const int nc = a.ncand[h];
    const int m = c1 - c0;
    for (int c = 0; c < nc; ++c) {
        const double* o = a.cand + (h * fm::MAX_CAND + c) * 9;
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = o[k];
        unsigned long long sc = 0;
        unsigned cnt = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const float4 q = spt[i];
            const double r2 = tv::sampson(F, q.x, q.y, q.z, q.w);
            const bool near = r2 < a.tmax2;
            const unsigned e = stab[rs::bin_of(near ? r2 : 0.0, a.bin_scale)];
            sc += near ? e : 0u;
            cnt += r2 < a.thr2 ? 1u : 0u;
        }
        atomicAdd(a.hscore + h * fm::MAX_CAND + c, sc);
        atomicAdd(a.hcnt + h * fm::MAX_CAND + c, cnt);
    }
}

// After the first 256 hypotheses: rs::hypotheses_bound over the records (strict prefix maxima of the quality) among them; a hypothesis
// scores the maximum over its candidates (rs::hyp_best)
__global__ __launch_bounds__(256) void fundamental_bound_kernel(FmArgs a) {
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    unsigned long long q = 0;
    unsigned cnt = 0;
    int cand = 0;
    const bool has = tid < a.iters && n >= 7 && rs::hyp_best<fm::MAX_CAND, false>(a.ncand, a.hscore, a.hcnt, (size_t)pair * a.iters_pad + tid, q, cnt, cand);
    const int bmin = rs::hypotheses_bound<7, false>(has, q, cnt, n, a.log1mc, a.iters);
    if (tid == 0) a.bound[pair] = bmin;
}

// ---- selection, refinement, mask --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fundamental_select_kernel(FmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double jA[81], jV[81], fsh[9];
    __shared__ unsigned long long sc_sh;
    __shared__ unsigned cnt_sh;
    __shared__ int ok_sh;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const rs::PairView pts(a, pair);
    unsigned char* mask = a.mask + (size_t)pair * a.cap;
    int32_t* info = a.info + pair * 8;
    double* Fout = a.F + (size_t)pair * fm::MAX_CAND * 9;
    const bool robust = a.method == fm::METHOD_MAGSAC;

    // ---- FM_7POINT: the candidates of hypothesis 0 as they are
    if (a.method == fm::METHOD_7POINT) {
        const size_t h = (size_t)pair * a.iters_pad;
        const int nc = n == 7 ? a.ncand[h] : 0;
        if (tid < fm::MAX_CAND) {
            double o[9];
            if (tid < nc) fm_scale_out(a.cand + (h * fm::MAX_CAND + tid) * 9, o);
            for (int k = 0; k < 9; ++k) Fout[9 * tid + k] = tid < nc ? o[k] : 0.0;
        }
        for (int i = tid; i < a.cap; i += 256) mask[i] = nc > 0 && i < n ? 1 : 0;
        if (tid < 8) info[tid] = tid == 0 ? (nc > 0 ? 1 : 0) : tid == 1 ? -1 : tid == 2 ? nc : tid == 3 ? (nc > 0 ? n : 0) : tid == 5 ? n : 0;
        return;
    }

    // ---- the stopping rule of the sequential loop, over tiles of the score list
    int best = -1, best_cand = -1, iters_run = 0;
    if (robust) {
        rs::scan_stopping_rule<7, false>(lds_raw, n, a.iters, 0, a.log1mc,
                                         [&](int it, unsigned long long& q, unsigned& k, int& cd) {
                                             return rs::hyp_best<fm::MAX_CAND, false>(a.ncand, a.hscore, a.hcnt, (size_t)pair * a.iters_pad + it, q, k, cd);
                                         },
                                         best, best_cand, iters_run);
        if (best >= 0 && tid < 9) fsh[tid] = a.cand[(((size_t)pair * a.iters_pad + best) * fm::MAX_CAND + best_cand) * 9 + tid];
        __syncthreads();
    }
    if (robust ? best < 0 : n < 8) {
        rs::write_nothing_found(mask, a.cap, info, iters_run, n);
        if (tid < 27) Fout[tid] = 0.0;
        return;
    }
    const FmNorm nt = fm_norm(a, pair);
    double* red = reinterpret_cast<double*>(lds_raw);         // the tiles are dead: reduction buffer from here on
    float4* spt = reinterpret_cast<float4*>(lds_raw + (rs::block_sums_bytes(fm::NSUM) + 31 & ~(size_t)31));
    for (int i = tid; i < min(n, fm::SEL_CACHE); i += 256) spt[i] = pts.get(i);
    __syncthreads();
    auto for_each = [&](auto&& f) { rs::for_each_cached(spt, n, [&](int i) { return pts.get(i); }, f); };
    // the 45 weighted sums of a a' of one pass; weight w(r)/w(0) of the bin of r^2 under F (FM_8POINT: 1 for every point), quality into sc_sh
    auto pass = [&](const double* F, double (&sm)[fm::NSUM]) {
        for (int k = 0; k < fm::NSUM; ++k) sm[k] = 0.0;
        unsigned long long sc = 0;
        for_each([&](int, const float4& q) {
            double w = 1.0;
            if (robust) {
                const double r2 = tv::sampson(F, q.x, q.y, q.z, q.w);
                if (!(r2 < a.tmax2)) return;
                const int b = rs::bin_of(r2, a.bin_scale);
                sc += a.stab[b];
                w = a.wtab[b];
            }
            const double x0 = ((double)q.x - nt.cx0) * nt.s0, y0 = ((double)q.y - nt.cy0) * nt.s0;
            const double x1 = ((double)q.z - nt.cx1) * nt.s1, y1 = ((double)q.w - nt.cy1) * nt.s1;
            const double r[9] = {x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double wi = w * r[i];
#pragma unroll
                for (int j = i; j < 9; ++j) { sm[k] = sm[k] + wi * r[j]; ++k; }
            }
        });
        atomicAdd(&sc_sh, sc);
        rs::block_sums(sm, red);                               // (its barriers also publish sc_sh)
    };
    // one fit from the sums on thread 0 (LDS Jacobi), result into fsh / ok_sh
    auto fit = [&](const double (&sm)[fm::NSUM]) {
        if (tid == 0) {
            double Fp[9];
            ok_sh = fm_fit8(sm, static_cast<double*>(jA), static_cast<double*>(jV), nt, Fp) ? 1 : 0;
            for (int k = 0; k < 9; ++k) fsh[k] = Fp[k];
        }
        __syncthreads();
    };
    double Fb[9];
    unsigned long long s_best = 0;
    int lo_accepted = 0;
    bool model = true;
    if (!robust) {                                            // FM_8POINT: one unit-weight fit on all points
        if (tid == 0) sc_sh = 0ull;
        __syncthreads();
        double sm[fm::NSUM];
        pass(nullptr, sm);
        fit(sm);
        model = ok_sh != 0;
        for (int k = 0; k < 9; ++k) Fb[k] = fsh[k];
    } else {
        double Fc[9];
        for (int k = 0; k < 9; ++k) { Fc[k] = fsh[k]; Fb[k] = Fc[k]; }
        // ---- sigma-consensus++: re-weighted 8-point fits while the quality rises
        for (int step = 0; step <= fm::LO_ITERS; ++step) {
            if (tid == 0) sc_sh = 0ull;
            __syncthreads();
            double sm[fm::NSUM];
            pass(Fc, sm);
            const unsigned long long s_now = sc_sh;
            if (s_now <= s_best) break;
            for (int k = 0; k < 9; ++k) Fb[k] = Fc[k];
            s_best = s_now;
            lo_accepted = step;
            if (step == fm::LO_ITERS) break;
            __syncthreads();                                  // sc_sh and fsh read by everybody before they change
            fit(sm);
            if (!ok_sh) break;
            for (int k = 0; k < 9; ++k) Fc[k] = fsh[k];
            __syncthreads();
        }
    }
    // ---- inlier mask under the final F
    __syncthreads();
    if (tid == 0) cnt_sh = 0u;
    __syncthreads();
    unsigned cn = 0;
    if (robust) {
        for_each([&](int, const float4& q) { cn += tv::sampson(Fb, q.x, q.y, q.z, q.w) < a.thr2 ? 1u : 0u; });
        atomicAdd(&cnt_sh, cn);
    }
    __syncthreads();
    const int n_in = robust ? (int)cnt_sh : (model ? n : 0);
    const bool found = robust ? n_in >= 7 : model;
    for_each([&](int i, const float4& q) { mask[i] = found && (!robust || tv::sampson(Fb, q.x, q.y, q.z, q.w) < a.thr2) ? 1 : 0; });
    for (int i = n + tid; i < a.cap; i += 256) mask[i] = 0;
    if (tid == 0) {
        double o[9];
        fm_scale_out(Fb, o);
        for (int k = 0; k < 27; ++k) Fout[k] = found && k < 9 ? o[k] : 0.0;
        rs::write_info(info, found, robust ? best : -1, robust ? iters_run : (found ? 1 : 0), found ? n_in : 0, lo_accepted, n, s_best);
    }
}

static size_t fm_align(size_t v) { return (v + 255) & ~(size_t)255; }

size_t fundamental_workspace_bytes(int P, int max_iters) {
    const size_t pad = (size_t)ceil_div(max_iters, 256) * 256;
    const size_t nhyp = (size_t)P * pad;
    return fm_align((size_t)fm::NBINS * 12) + fm_align((size_t)P * 64) + fm_align((size_t)P * 4) + fm_align(nhyp * fm::MAX_CAND * 72) +
           fm_align(nhyp * fm::MAX_CAND * 8) + fm_align(nhyp * fm::MAX_CAND * 4) + fm_align(nhyp * 4);
}

int launch_find_fundamental(const float* p0, const float* p1, const int64_t* idx0, const int64_t* idx1, int kcap, const int32_t* counts, int n_const,
                            int P, int cap, int method, double thr, int max_iters, double confidence, unsigned long long seed, double* F,
                            unsigned char* mask, int32_t* info, void* ws, hipStream_t st) {
    if (max_iters < 1 || max_iters > fm::MAX_ITERS || P > 65535) return -1;
    if (method != fm::METHOD_MAGSAC && method != fm::METHOD_7POINT && method != fm::METHOD_8POINT) return -1;
    FmArgs a;
    a.p0 = p0; a.p1 = p1; a.idx0 = idx0; a.idx1 = idx1; a.kcap = idx0 ? kcap : cap; a.counts = counts; a.n_const = n_const; a.P = P; a.cap = cap;
    a.iters = method == fm::METHOD_MAGSAC ? max_iters : 1;
    a.iters_pad = ceil_div(max_iters, 256) * 256; a.method = method;
    const double t_max = fm::MAX_THR_FACTOR * thr;
    a.thr2 = thr * thr; a.tmax2 = t_max * t_max; a.bin_scale = fm::NBINS / (t_max * t_max); a.log1mc = log(1.0 - confidence); a.seed = seed;
    unsigned char* w = static_cast<unsigned char*>(ws);
    const size_t nhyp = (size_t)P * a.iters_pad;
    double* wtab = reinterpret_cast<double*>(w);
    unsigned* stab = reinterpret_cast<unsigned*>(w + (size_t)fm::NBINS * 8);
    a.wtab = wtab; a.stab = stab; w += fm_align((size_t)fm::NBINS * 12);
    a.norm = reinterpret_cast<double*>(w); w += fm_align((size_t)P * 64);
    a.bound = reinterpret_cast<int*>(w); w += fm_align((size_t)P * 4);
    a.cand = reinterpret_cast<double*>(w); w += fm_align(nhyp * fm::MAX_CAND * 72);
    a.hscore = reinterpret_cast<unsigned long long*>(w); w += fm_align(nhyp * fm::MAX_CAND * 8);
    a.hcnt = reinterpret_cast<unsigned*>(w); w += fm_align(nhyp * fm::MAX_CAND * 4);
    a.ncand = reinterpret_cast<int*>(w);
    a.F = F; a.mask = mask; a.info = info;
    static AttrMask attr_sel = 0;
    const size_t red = (rs::block_sums_bytes(fm::NSUM) + 31) & ~(size_t)31;
    const size_t tiles = (size_t)fm::SEL_TILE * 16;
    const size_t sel_lds = (red > tiles ? red : tiles) + (size_t)fm::SEL_CACHE * sizeof(float4);
    set_max_dynamic_lds(reinterpret_cast<const void*>(fundamental_select_kernel), (int)sel_lds, attr_sel);
    fundamental_prep_kernel<<<P, 256, 0, st>>>(a);
    if (method == fm::METHOD_8POINT) {
        fundamental_select_kernel<<<P, 256, sel_lds, st>>>(a);
        return 0;
    }
    const size_t solve_lds = (size_t)fm::SLICE * fm::SOLVE_WG * sizeof(double);
    if (method == fm::METHOD_7POINT) {
        fundamental_zero_kernel<<<P, 256, 0, st>>>(a, nhyp);
        fundamental_solve_kernel<<<dim3(1, P), fm::SOLVE_WG, solve_lds, st>>>(a, 0, 0);
        fundamental_select_kernel<<<P, 256, sel_lds, st>>>(a);
        return 0;
    }
    launch_homography_tables(thr, stab, wtab, st);
    const size_t zg = (nhyp + 255) / 256;
    fundamental_zero_kernel<<<(unsigned)(zg > 2048 ? 2048 : zg), 256, 0, st>>>(a, nhyp);
    a.chunk = rs::score_chunk(P, cap);
    const int nblk = ceil_div(max_iters, fm::HYP_PER_WG), nch = ceil_div(cap, a.chunk);
    const int first = max_iters < fm::HYP_PER_WG ? max_iters : fm::HYP_PER_WG;
    fundamental_solve_kernel<<<dim3(ceil_div(first, fm::SOLVE_WG), P), fm::SOLVE_WG, solve_lds, st>>>(a, 0, 0);
    fundamental_score_kernel<<<dim3(1, nch, P), 256, 0, st>>>(a, 0, 0);
    if (nblk > 1) {
        fundamental_bound_kernel<<<P, 256, 0, st>>>(a);
        fundamental_solve_kernel<<<dim3(ceil_div(max_iters - fm::HYP_PER_WG, fm::SOLVE_WG), P), fm::SOLVE_WG, solve_lds, st>>>(a, fm::HYP_PER_WG, 1);
        fundamental_score_kernel<<<dim3(nblk - 1, nch, P), 256, 0, st>>>(a, 1, 1);
    }
    fundamental_select_kernel<<<P, 256, sel_lds, st>>>(a);
    return 0;
}

}  // namespace xfh
