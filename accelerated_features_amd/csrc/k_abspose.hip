// Absolute camera pose from 2D-3D correspondences: the device side of
//     pose, info = poselib.estimate_absolute_pose(points2D, points3D, camera, {"max_reproj_error": thr}, {})
// (what hloc runs for the Aachen localisation benchmark of the XFeat paper; the 3D side may also be the key-points of a reference image
// lifted through its depth map, as modules/dataset/megadepth/megadepth_warper.py::warp_kpts lifts them).  poselib is not available offline
// and its source is not part of the reference tree, so nothing here is pinned to it: what is implemented is the published estimator --
// RANSAC over a P3P solver (the classical quartic in a depth ratio, Grunert 1841 / Haralick et al., IJCV 1994) with an MSAC score on the
// reprojection error and a Gauss-Newton refinement of the winner.  The specification (tests/abspose_reference.py is a numpy
// restatement of it, operation for operation, and tests/test_abspose_emulated.py compiles the solver below on the host and holds it to that
// restatement bit for bit):
//   * inputs of pair p: 2D points (cap2 rows of 2 fp32 pixels in the query image), 3D points (cap3 rows of 3 fp32, any world frame),
//     correspondence i = (row i, row i) or, with index lists, (row idx2d[i] of the 2D points, row idx3d[i] of the 3D points); the two sides
//     have capacities of their own (ApView; rs::PairView is for two 2D sets of one capacity);
//   * calibration: pixel (u, v) -> x = ((u - cx) / fx, (v - cy) / fy) in fp64 with pair p's PINHOLE intrinsics (K row-major 3x3); the
//     threshold in these units is thr_n = max_reproj_error / ((fx + fy) / 2) -- our choice, as for the relative pose;
//   * sample: 3 distinct correspondences, drawn as ransac_common.hpp states (rs::sample_distinct<3>); a sample that runs out of draws or
//     holds a non-finite coordinate yields no model;
//   * minimal solver (ap_solve): unit bearings f_i = (x_i, y_i, 1) / |.|; squared sides a2 = |P2 - P3|^2, b2 = |P1 - P3|^2,
//     c2 = |P1 - P2|^2 (b2 = 0: no model) taken relative to b2, ra = a2 / b2, rc = c2 / b2, so that every constant below is free of the
//     world's unit; cosines ca = f2.f3, cb = f1.f3, cg = f1.f2.  With the depths s2 = u s1, s3 = v s1 and q(v) = v^2 - 2 cb v + 1 the three
//     cosine-law equations, s1^2 eliminated, give u = N(v) / D(v),
//         N = (v^2 - 1) + (rc - ra) q(v),   D = 2 (ca v - cg),   and the quartic   N^2 - 2 cg N D + (1 - rc q) D^2 = 0
//     (the elimination on b2 N, b2 D divided through by b2).  Its products are tv::pmul's.  A leading coefficient below ap::LEAD_EPS in
//     magnitude, or anything non-finite: no model.  The real roots of the quartic made monic, in ascending order, by the root isolation of
//     the five-point solver at degree 4: Cauchy bound 1 + max |coefficient|, the Sturm sequence (15 coefficients, in registers).  Its last
//     term, a constant, decides whether two close roots count as real: where it is below ap::SQFREE_EPS of the two terms it is the
//     difference of, its sign is rounding noise around a (nearly) double root, and it takes the sign that counts more real roots, the
//     positive one on ties (so a double root is found, possibly twice, and never lost; a pair that is in truth complex leaves the place
//     where |p| is smallest, which the later steps drop or score as any other candidate.  On random quartics with a double root the
//     ratio stays below 2e-10, with simple roots above 7e-8),
//     STURM_STEPS bisections on the root count per root, SIGN_STEPS bisections on the sign of the polynomial where it changes over the
//     bracket, NEWTON_STEPS Newton steps, each kept only if it lowers |p|.  A root with |D(v)| < ap::DEN_EPS is dropped.  (u, v) is then
//     polished by POLISH_STEPS Newton steps on the two equations themselves, F1 = u^2 + v^2 - 2 ca u v - ra q(v) and
//     F2 = 1 + u^2 - 2 cg u - rc q(v), each kept only if it lowers |F1| + |F2| (u = N / D loses digits where D is small; measured on
//     20 000 noise-free samples the worst reprojection of a candidate falls from 7e-4 to 1e-11 and no true pose is missed).  The pair is
//     kept if |F1| + |F2| <= ap::RES_EPS (it solves the equations: not the place a complex pair left), v > 0, u > 0, q(v) > 0; then s1 = sqrt(b2 / q(v)), s2 = u s1, s3 = v s1 and the camera points C_i = s_i f_i;
//   * R, t without an SVD: the orthonormal frame of a triangle (A, B, C) is e1 = (B - A) / |.|, e3 = (e1 x (C - A)) / |.|, e2 = e3 x e1;
//     R = [frame of C1 C2 C3] [frame of P1 P2 P3]', t = C1 - R P1.  A triangle with |e1 x (C - A)|^2 <= ap::COLLINEAR_EPS2 |C - A|^2
//     (the sine of the angle at A below 1e-4: collinear points, which leave the rotation about their line free) or a zero first side gives no model; a non-finite pose is dropped.  At most 4 candidates per hypothesis, in root order;
//   * only + - * / sqrt in all of it, every product and sum rounded once (fp contraction off in this file);
//   * score of a candidate: Y = R X + t; r^2 = |x - Y_xy (1 / Y_z)|^2 (one division per residual) when Y_z > 0, otherwise (and when anything is not finite) the
//     correspondence is never an inlier and costs the cap; MSAC cost floor(min(r^2, thr_n^2) / thr_n^2 * 2^20) summed as u64 (no
//     summation order); inlier: r^2 < thr_n^2; a hypothesis costs the minimum over its candidates (ties: the lower root; rs::hyp_best);
//   * stopping rule: rs::scan_stopping_rule<3, true>; the later blocks run below rs::hypotheses_bound<3, true> of the first 256;
//   * refinement of the winner: up to 10 Gauss-Newton steps on R <- R cay(w) (the update multiplies on the RIGHT, as the relative pose's),
//     t <- t + d over the inliers, residual e = (Y_x (1 / Y_z) - x, Y_y (1 / Y_z) - y), J = de / d(w, d) with dY/dw_k = R (e_k x X), dY/dd = I;
//     the 27 sums -- the upper triangle of J'J row-major (21), then J'e (6) -- are fixed-order block reductions (rs::block_sums), the 6x6
//     normal equations are solved by Cholesky; a step is kept only if it strictly lowers the integer cost, the first rejected step ends it;
//   * outputs: R (row-major), t with X_cam = R X_world + t (t is a length in the world's unit: not normalised), mask r^2 < thr_n^2 under
//     the final pose, info = the family's 8 words; found = at least 3 inliers; fewer than 3 correspondences or no model:
//     rs::write_nothing_found and zeros in R, t.
//
// Registers, not LDS.  The working set of ap_solve is the sample (15 fp64), the bearings and frames (27), the quartic's factors (~20) and
// the Sturm sequence (15); no array is indexed at run time (the Sturm sequence is a struct of fixed-size arrays, every loop over it is
// unrolled, a root's index only enters a comparison), so nothing goes to scratch and the 140 KiB LDS slices of the five-point solver are
// not needed: thread = hypothesis, 256 per workgroup, the candidates written straight to the workspace.
//
// Launches per call (workspace: per hypothesis 4 candidate poses of 12 fp64 + 4 costs + 4 inlier counts + the candidate count):
//   abspose_zero_kernel   : costs, counts, candidate counts zeroed
//   abspose_solve_kernel  : thread = hypothesis: sample, ap_solve, candidates into the workspace      (hypotheses 0..255 first)
//   abspose_score_kernel  : thread = hypothesis, its candidates in turn against a chunk of correspondences in LDS, u64 atomics
//   abspose_bound_kernel  : the bound the loop reaches from the records among the first 256; the later blocks are solved and scored
//                           only below max(min_iterations, bound)
//   abspose_select_kernel : one workgroup per pair: stopping rule over the cost list (tiles in LDS), refinement, mask, outputs
#include "ransac_common.hpp"
#include "twoview_math.hpp"

#pragma clang fp contract(off)

namespace xfh {
namespace ap {
using rs::HYP_PER_WG, rs::PTS_PER_WG, rs::SEL_TILE, rs::SEL_CACHE;
constexpr int LO_ITERS = 10, MAX_ITERS = 16384, MAX_CAND = 4, NSUM = 27;
}  // namespace ap

// ---- solver begin (host-compilable: tests/test_abspose_emulated.py slices it out behind the slice of twoview_math.hpp and drops the
// __device__ qualifiers) ----
namespace ap {
constexpr int STURM_STEPS = 48, SIGN_STEPS = 48, NEWTON_STEPS = 4, POLISH_STEPS = 3;
constexpr int CAND_DOUBLES = 12;             // R (row-major) + t of one candidate pose
constexpr double LEAD_EPS = 1e-12;           // the quartic's leading coefficient (dimensionless: cosines and side ratios)
constexpr double DEN_EPS = 1e-12;            // |D(v)| of u = N / D
constexpr double COLLINEAR_EPS2 = 1e-8;      // sin^2 of the triangle's angle at its first corner
constexpr double RES_EPS = 1e-10;            // |F1| + |F2| of a kept (u, v)
constexpr double SQFREE_EPS = 1e-9;          // the Sturm sequence's last term relative to the two terms it is the difference of
}  // namespace ap

// MSAC cost in 2^-20 units of thr2; NaN counts as the cap
__device__ inline unsigned ap_cost(double r2, double thr2) {
    const double m = r2 < thr2 ? r2 : thr2;
    return (unsigned)floor(m / thr2 * 1048576.0);
}
// squared reprojection error of X under (R, t) against (x, y); behind the camera (or Y_z not a number): 1e300, never an inlier
__device__ inline double ap_residual2(const double* R, const double* t, double x, double y, double X0, double X1, double X2) {
    const double Y0 = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
    const double Y1 = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    const double Y2 = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
    const double iz = 1.0 / Y2;                               // one division per residual: the projection is Y_xy * (1 / Y_z)
    const double dx = x - Y0 * iz, dy = y - Y1 * iz;
    return Y2 > 0.0 ? dx * dx + dy * dy : 1e300;
}
template <int DEG>
__device__ inline double ap_horner(const double (&a)[DEG + 1], double x) {
    double v = a[DEG];
#pragma unroll
    for (int i = DEG - 1; i >= 0; --i) v = v * x + a[i];
    return v;
}
// the Sturm sequence of a monic quartic: s0 the polynomial, s1 its derivative, s2 .. s4 the negated remainders (ascending powers)
struct ApSturm {
    double s0[5], s1[4], s2[3], s3[2], s4[1];
};
// c = -rem(a, b), a of degree D + 1, b of degree D, c of degree D - 1
template <int D>
__device__ inline void ap_sturm_rem(const double (&a)[D + 2], const double (&b)[D + 1], double (&c)[D]) {
    const double q1 = a[D + 1] / b[D];
    const double q0 = (a[D] - q1 * b[D - 1]) / b[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double ti = i == 0 ? a[0] : a[i] - q1 * b[i > 0 ? i - 1 : 0];
        c[i] = -(ti - q0 * b[i]);
    }
}
// sign changes of the sequence at x (zeros skipped)
__device__ inline int ap_sturm_changes(const ApSturm& q, double x) {
    const double v[5] = {ap_horner<4>(q.s0, x), ap_horner<3>(q.s1, x), ap_horner<2>(q.s2, x), ap_horner<1>(q.s3, x), q.s4[0]};
    int n = 0;
    bool have = false, prev = false;
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (v[k] != 0.0) {
            const bool g = v[k] > 0.0;
            if (have && g != prev) ++n;
            prev = g; have = true;
        }
    return n;
}
// the two cosine-law equations left of the three after s1 is eliminated: F1 = u^2 + v^2 - 2 ca u v - ra q(v), F2 = 1 + u^2 - 2 cg u - rc q(v)
__device__ inline void ap_cosine_laws(double u, double v, double ra, double rc, double ca, double cg, double q1, double& F1, double& F2) {
    const double qv = (v + q1) * v + 1.0;
    F1 = ((u * u + v * v) - (2.0 * ca) * (u * v)) - ra * qv;
    F2 = ((1.0 + u * u) - (2.0 * cg) * u) - rc * qv;
}
// orthonormal frame (e1, e2, e3) of the triangle (A, B, C); false: degenerate (a zero first side, collinear)
__device__ inline bool ap_frame(const double* A, const double* B, const double* Cc, double* e1, double* e2, double* e3) {
    return tv::triangle_frame(A, B, Cc, ap::COLLINEAR_EPS2, e1, e2, e3);
}
// candidate poses of the sample: x[3], y[3] normalised image coordinates, X[9] the 3D points (point-major); out[12 c ..] = R (row-major),
// t; returns their number (0: no model)
__device__ inline int ap_solve(const double* x, const double* y, const double* X, double* out) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) fin = fin && tv::is_finite(x[k]) && tv::is_finite(y[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && tv::is_finite(X[k]);
    if (!fin) return 0;
    // ---- bearings, sides, cosines
    double f[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double nn = sqrt((x[i] * x[i] + y[i] * y[i]) + 1.0);
        f[i][0] = x[i] / nn; f[i][1] = y[i] / nn; f[i][2] = 1.0 / nn;
    }
    const double d23[3] = {X[3] - X[6], X[4] - X[7], X[5] - X[8]};
    const double d13[3] = {X[0] - X[6], X[1] - X[7], X[2] - X[8]};
    const double d12[3] = {X[0] - X[3], X[1] - X[4], X[2] - X[5]};
    const double a2 = tv::dot3(d23, d23), b2 = tv::dot3(d13, d13), c2 = tv::dot3(d12, d12);
    if (!(b2 > 0.0)) return 0;
    const double ra = a2 / b2, rc = c2 / b2;
    const double ca = tv::dot3(f[1], f[2]), cb = tv::dot3(f[0], f[2]), cg = tv::dot3(f[0], f[1]);
    // ---- the world triangle's frame
    double ep[3][3];
    if (!ap_frame(X, X + 3, X + 6, ep[0], ep[1], ep[2])) return 0;
    // ---- the quartic in v (ascending powers)
    const double q1 = -2.0 * cb;                              // q = (1, q1, 1)
    const double kk = rc - ra;
    const double N[3] = {kk - 1.0, kk * q1, 1.0 + kk};
    const double D[2] = {-(2.0 * cg), 2.0 * ca};
    const double g[3] = {1.0 - rc, -(rc * q1), -rc};          // 1 - rc q
    const double m = 2.0 * cg;
    double NN[5], ND[4], DD[3], gDD[5], p[5];
    tv::pmul(N, 2, N, 2, NN); tv::pmul(N, 2, D, 1, ND); tv::pmul(D, 1, D, 1, DD); tv::pmul(g, 2, DD, 2, gDD);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = (NN[k] - m * ND[k]) + gDD[k];
    p[4] = NN[4] + gDD[4];
    // ---- Sturm sequence of the monic polynomial
    const double lead = p[4];
    if (!(fabs(lead) >= ap::LEAD_EPS) || !tv::is_finite(lead)) return 0;
    ApSturm st;
    double bound = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double v = k == 4 ? 1.0 : p[k] / lead;
        st.s0[k] = v;
        const double av = fabs(v);
        if (k < 4 && av > bound) bound = av;
    }
    bound = 1.0 + bound;
#pragma unroll
    for (int k = 0; k < 4; ++k) st.s1[k] = (double)(k + 1) * st.s0[k + 1];
    ap_sturm_rem<3>(st.s0, st.s1, st.s2);
    ap_sturm_rem<2>(st.s1, st.s2, st.s3);
    ap_sturm_rem<1>(st.s2, st.s3, st.s4);
    bool noise;
    {   // a last term that is all cancellation: its sign is rounding noise (see the header)
        const double r1 = st.s2[2] / st.s3[1];
        const double r0 = (st.s2[1] - r1 * st.s3[0]) / st.s3[1];
        noise = fabs(st.s4[0]) <= ap::SQFREE_EPS * (fabs(st.s2[0]) + fabs(r0 * st.s3[0]));
    }
    fin = tv::is_finite(bound);
#pragma unroll
    for (int k = 0; k < 5; ++k) fin = fin && tv::is_finite(st.s0[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) fin = fin && tv::is_finite(st.s1[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) fin = fin && tv::is_finite(st.s2[k]);
    fin = fin && tv::is_finite(st.s3[0]) && tv::is_finite(st.s3[1]) && tv::is_finite(st.s4[0]);
    if (!fin) return 0;
    if (noise) {                                             // the sign that counts more real roots (the positive one on ties)
        const double s4 = fabs(st.s4[0]);
        st.s4[0] = s4;
        const int n_pos = ap_sturm_changes(st, -bound) - ap_sturm_changes(st, bound);
        st.s4[0] = -s4;
        const int n_neg = ap_sturm_changes(st, -bound) - ap_sturm_changes(st, bound);
        st.s4[0] = n_neg > n_pos ? -s4 : s4;
    }
    const int v_lo = ap_sturm_changes(st, -bound), v_hi = ap_sturm_changes(st, bound);
    int nroots = v_lo - v_hi;
    nroots = nroots < 0 ? 0 : (nroots > 4 ? 4 : nroots);
    int ncand = 0;
    for (int k = 0; k < nroots; ++k) {
        double lo = -bound, hi = bound;
        for (int it = 0; it < ap::STURM_STEPS; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (v_lo - ap_sturm_changes(st, mid) > k) hi = mid; else lo = mid;
        }
        const double flo = ap_horner<4>(st.s0, lo), fhi = ap_horner<4>(st.s0, hi);
        if ((flo > 0.0) != (fhi > 0.0)) {
            const bool slo = flo > 0.0;
            for (int it = 0; it < ap::SIGN_STEPS; ++it) {
                const double mid = 0.5 * (lo + hi);
                if ((ap_horner<4>(st.s0, mid) > 0.0) == slo) lo = mid; else hi = mid;
            }
        }
        double v = 0.5 * (lo + hi);
        for (int it = 0; it < ap::NEWTON_STEPS; ++it) {    // polish: Newton steps, each kept only if it lowers |p|
            const double fv = ap_horner<4>(st.s0, v), df = ap_horner<3>(st.s1, v);
            const double vn = v - fv / df;
            const double fn = ap_horner<4>(st.s0, vn);
            if (fabs(fn) < fabs(fv)) v = vn;
        }
        // ---- depths
        const double Dv = D[1] * v + D[0];
        const double Nv = (N[2] * v + N[1]) * v + N[0];
        if (!(fabs(Dv) >= ap::DEN_EPS)) continue;
        double u = Nv / Dv;
        for (int it = 0; it < ap::POLISH_STEPS; ++it) {    // polish (u, v) on the two cosine-law equations, each step kept only if it lowers |F1| + |F2|
            double F1, F2, G1, G2;
            ap_cosine_laws(u, v, ra, rc, ca, cg, q1, F1, F2);
            const double dq = 2.0 * v + q1;
            const double a11 = 2.0 * u - (2.0 * ca) * v, a12 = (2.0 * v - (2.0 * ca) * u) - ra * dq;
            const double a21 = 2.0 * u - 2.0 * cg, a22 = -(rc * dq);
            const double det = a11 * a22 - a12 * a21;
            const double un = u - (F1 * a22 - F2 * a12) / det;
            const double vn = v - (a11 * F2 - a21 * F1) / det;
            ap_cosine_laws(un, vn, ra, rc, ca, cg, q1, G1, G2);
            if (fabs(G1) + fabs(G2) < fabs(F1) + fabs(F2)) { u = un; v = vn; }
        }
        {
            double F1, F2;
            ap_cosine_laws(u, v, ra, rc, ca, cg, q1, F1, F2);
            if (!(fabs(F1) + fabs(F2) <= ap::RES_EPS)) continue;
        }
        const double qv = (v + q1) * v + 1.0;
        if (!(v > 0.0) || !(u > 0.0) || !(qv > 0.0)) continue;
        const double s1 = sqrt(b2 / qv);
        const double sd[3] = {s1, u * s1, v * s1};
        double Cp[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Cp[i][j] = sd[i] * f[i][j];
        // ---- pose from the two frames
        double ec[3][3];
        if (!ap_frame(Cp[0], Cp[1], Cp[2], ec[0], ec[1], ec[2])) continue;
        double R[9], t[3];
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                R[3 * i + j] = (ec[0][i] * ep[0][j] + ec[1][i] * ep[1][j]) + ec[2][i] * ep[2][j];
                ok = ok && tv::is_finite(R[3 * i + j]);
            }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            t[i] = Cp[0][i] - ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]);
            ok = ok && tv::is_finite(t[i]);
        }
        if (!ok) continue;
        double* o = out + ap::CAND_DOUBLES * ncand;
#pragma unroll
        for (int j = 0; j < 9; ++j) o[j] = R[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) o[9 + j] = t[j];
        ++ncand;
    }
    return ncand;
}
// ---- solver end ----

struct ApArgs {
    const float* p2;          // (P, cap2, 2): the 2D points of the correspondences (idx2 == NULL, cap2 == cap) or the key-point lists they index
    const float* p3;          // (P, cap3, 3): the 3D points likewise
    const int64_t* idx2;      // (P, cap) rows of p2 / p3 of correspondence i, or NULL
    const int64_t* idx3;
    const int32_t* counts;
    const double* K;          // (P, 3, 3)
    int n_const, P, cap, cap2, cap3, iters, iters_pad, min_iters;
    int chunk;
    double max_err;
    double log1mp;
    unsigned long long seed;
    double* cand;             // (P, iters_pad, 4, 12)
    unsigned long long* hcost;   // (P, iters_pad, 4)
    unsigned* hcnt;              // (P, iters_pad, 4)
    int* ncand;                  // (P, iters_pad)
    int* bound;                  // (P)
    double* R;
    double* t;
    unsigned char* mask;
    int32_t* info;
};

// one correspondence: normalised image coordinates and the 3D point
struct ApPt {
    double x, y, X0, X1, X2;
};

// the 2D-3D correspondences of one pair: two sides with capacities of their own, through the index lists when given
struct ApView {
    const float* p2;
    const float* p3;
    const int64_t* i2;
    const int64_t* i3;
    __device__ ApView(const ApArgs& a, int pair)
        : p2(a.p2 + (size_t)pair * a.cap2 * 2), p3(a.p3 + (size_t)pair * a.cap3 * 3), i2(a.idx2 ? a.idx2 + (size_t)pair * a.cap : nullptr),
          i3(a.idx3 ? a.idx3 + (size_t)pair * a.cap : nullptr) {}
    __device__ inline float2 get2(int i) const {
        const size_t r = i2 ? (size_t)i2[i] : (size_t)i;
        return *reinterpret_cast<const float2*>(p2 + 2 * r);
    }
    __device__ inline float3 get3(int i) const {
        const size_t r = i3 ? (size_t)i3[i] : (size_t)i;
        return make_float3(p3[3 * r], p3[3 * r + 1], p3[3 * r + 2]);
    }
};

// the view and the calibration
struct ApPair {
    ApView pts;
    double fx, fy, cx, cy, thr2;
    __device__ ApPair(const ApArgs& a, int pair) : pts(a, pair) {
        const double* k = a.K + (size_t)pair * 9;
        fx = k[0]; cx = k[2]; fy = k[4]; cy = k[5];
        const double thr = a.max_err / ((fx + fy) * 0.5);
        thr2 = thr * thr;
    }
    __device__ inline ApPt get(int i) const {
        const float2 q = pts.get2(i);
        const float3 w = pts.get3(i);
        return ApPt{((double)q.x - cx) / fx, ((double)q.y - cy) / fy, (double)w.x, (double)w.y, (double)w.z};
    }
};

__global__ __launch_bounds__(256) void abspose_zero_kernel(ApArgs a, size_t nhyp) {
    rs::zero_hypotheses<ap::MAX_CAND>(a.ncand, a.hcost, a.hcnt, nhyp);
}

// hypotheses [it_base + 256 blockIdx.x, + 256) of pair blockIdx.y; only below the pair's bound when `use_bound`
__global__ __launch_bounds__(256) void abspose_solve_kernel(ApArgs a, int it_base, int use_bound) {
    const int pair = blockIdx.y;
    const int it = it_base + blockIdx.x * ap::HYP_PER_WG + threadIdx.x;
    const int n = rs::pair_count(a, pair);
    if (n < 3 || it >= a.iters) return;
    if (use_bound && a.bound[pair] <= it) return;
    const ApPair pp(a, pair);
    int idx[3] = {-1, -1, -1};
    if (!rs::sample_distinct(a.seed, pair, it, n, idx)) return;
    double x[3], y[3], X[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const ApPt q = pp.get(idx[k]);
        x[k] = q.x; y[k] = q.y; X[3 * k] = q.X0; X[3 * k + 1] = q.X1; X[3 * k + 2] = q.X2;
    }
    const size_t h = (size_t)pair * a.iters_pad + it;
    a.ncand[h] = ap_solve(x, y, X, a.cand + h * ap::MAX_CAND * ap::CAND_DOUBLES);
}

// Hypotheses [256 (blockIdx.x + blk0), + 256) of pair blockIdx.z against correspondences [chunk blockIdx.y, + chunk)
__global__ __launch_bounds__(256) void abspose_score_kernel(ApArgs a, int blk0, int use_bound) {
    __shared__ ApPt spt[ap::PTS_PER_WG];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const int c0 = blockIdx.y * a.chunk;
    const int it0 = (blockIdx.x + blk0) * ap::HYP_PER_WG;
    if (n < 3 || c0 >= n) return;
    if (use_bound && a.bound[pair] <= it0) return;
    const ApPair pp(a, pair);
    const int c1 = min(c0 + a.chunk, n);
    for (int i = tid; i < c1 - c0; i += 256) spt[i] = pp.get(c0 + i);
    __syncthreads();
    const int it = it0 + tid;
    if (it >= a.iters) return;
    const size_t h = (size_t)pair * a.iters_pad + it;
    const int nc = a.ncand[h];
    const int m = c1 - c0;
    for (int c = 0; c < nc; ++c) {
        const double* o = a.cand + (h * ap::MAX_CAND + c) * ap::CAND_DOUBLES;
        double Rm[9], tm[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[k] = o[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tm[k] = o[9 + k];
        unsigned long long sc = 0;
        unsigned cnt = 0;
#pragma unroll 4
        for (int i = 0; i < m; ++i) {
            const ApPt q = spt[i];
            const double r2 = ap_residual2(Rm, tm, q.x, q.y, q.X0, q.X1, q.X2);
            sc += ap_cost(r2, pp.thr2);
            cnt += r2 < pp.thr2 ? 1u : 0u;
        }
        atomicAdd(a.hcost + h * ap::MAX_CAND + c, sc);
        atomicAdd(a.hcnt + h * ap::MAX_CAND + c, cnt);
    }
}

// After the first 256 hypotheses: the index below which the loop can still visit hypotheses = max(min_iters, rs::hypotheses_bound over
// the records (strict prefix minima of the cost) among them); a hypothesis costs the minimum over its candidates (rs::hyp_best)
__global__ __launch_bounds__(256) void abspose_bound_kernel(ApArgs a) {
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    unsigned long long cost = ~0ull;
    unsigned cnt = 0;
    int cand = 0;
    const bool has = tid < a.iters && n >= 3 && rs::hyp_best<ap::MAX_CAND, true>(a.ncand, a.hcost, a.hcnt, (size_t)pair * a.iters_pad + tid, cost, cnt, cand);
    const int bmin = rs::hypotheses_bound<3, true>(has, cost, cnt, n, a.log1mp, a.iters);
    if (tid == 0) a.bound[pair] = bmin > a.min_iters ? bmin : a.min_iters;
}

// ---- selection, refinement, mask --------------------------------------------------------------------------------------------------------
// one Gauss-Newton step from (R, t) with the 27 sums (H upper triangle row-major, then g); false if the normal equations are not positive
__device__ inline bool ap_gn_update(const double (&sm)[ap::NSUM], const double* R, const double* t, double* Rn, double* tn) {
    double H[6][6], L[6][6], g[6], y[6], d[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { H[i][j] = sm[k]; H[j][i] = sm[k]; ++k; }
    for (int i = 0; i < 6; ++i) g[i] = sm[21 + i];
    for (int j = 0; j < 6; ++j) {
        double dj = H[j][j];
        for (int q = 0; q < j; ++q) dj = dj - L[j][q] * L[j][q];
        if (!(dj > 0.0)) return false;
        L[j][j] = sqrt(dj);
        for (int i = j + 1; i < 6; ++i) {
            double v = H[i][j];
            for (int q = 0; q < j; ++q) v = v - L[i][q] * L[j][q];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
        for (int q = 0; q < i; ++q) v = v - L[i][q] * y[q];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < 6; ++q) v = v - L[q][i] * d[q];
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
    for (int i = 0; i < 3; ++i) tn[i] = t[i] + d[3 + i];
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && tv::is_finite(Rn[i]);
    for (int i = 0; i < 3; ++i) fin = fin && tv::is_finite(tn[i]);
    return fin;
}

__global__ __launch_bounds__(256) void abspose_select_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double pose_sh[12];
    __shared__ unsigned long long sc_sh;
    __shared__ unsigned cnt_sh;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    unsigned char* mask = a.mask + (size_t)pair * a.cap;
    int32_t* info = a.info + (size_t)pair * 8;

    // ---- the stopping rule of the sequential loop, over tiles of the cost list
    int best, best_cand, iters_run;
    rs::scan_stopping_rule<3, true>(lds_raw, n, a.iters, a.min_iters, a.log1mp,
                                    [&](int it, unsigned long long& c, unsigned& k, int& cd) {
                                        return rs::hyp_best<ap::MAX_CAND, true>(a.ncand, a.hcost, a.hcnt, (size_t)pair * a.iters_pad + it, c, k, cd);
                                    },
                                    best, best_cand, iters_run);
    if (best >= 0 && tid < 12) pose_sh[tid] = a.cand[(((size_t)pair * a.iters_pad + best) * ap::MAX_CAND + best_cand) * ap::CAND_DOUBLES + tid];
    __syncthreads();
    double* Rout = a.R + (size_t)pair * 9;
    double* tout = a.t + (size_t)pair * 3;
    if (best < 0) {
        rs::write_nothing_found(mask, a.cap, info, iters_run, n);
        if (tid < 9) Rout[tid] = 0.0;
        if (tid < 3) tout[tid] = 0.0;
        return;
    }
    const ApPair pp(a, pair);
    const double thr2 = pp.thr2;
    double* red = reinterpret_cast<double*>(lds_raw);         // the tiles are dead: reduction buffer from here on
    ApPt* spt = reinterpret_cast<ApPt*>(lds_raw + (rs::block_sums_bytes(ap::NSUM) + 31 & ~(size_t)31));
    for (int i = tid; i < min(n, ap::SEL_CACHE); i += 256) spt[i] = pp.get(i);
    __syncthreads();
    auto for_each = [&](auto&& f) { rs::for_each_cached(spt, n, [&](int i) { return pp.get(i); }, f); };
    double Rc[9], tcur[3], Rb[9], tb[3];
    for (int k = 0; k < 9; ++k) { Rc[k] = pose_sh[k]; Rb[k] = Rc[k]; }
    for (int k = 0; k < 3; ++k) { tcur[k] = pose_sh[9 + k]; tb[k] = tcur[k]; }
    unsigned long long c_best = ~0ull;
    int lo_accepted = 0;
    for (int step = 0; step <= ap::LO_ITERS; ++step) {
        if (tid == 0) sc_sh = 0ull;
        __syncthreads();
        double sm[ap::NSUM];
        for (int k = 0; k < ap::NSUM; ++k) sm[k] = 0.0;
        unsigned long long sc = 0;
        for_each([&](int, const ApPt& q) {
            const double Y0 = ((Rc[0] * q.X0 + Rc[1] * q.X1) + Rc[2] * q.X2) + tcur[0];
            const double Y1 = ((Rc[3] * q.X0 + Rc[4] * q.X1) + Rc[5] * q.X2) + tcur[1];
            const double Y2 = ((Rc[6] * q.X0 + Rc[7] * q.X1) + Rc[8] * q.X2) + tcur[2];
            const double iz = 1.0 / Y2;
            const double px = Y0 * iz, py = Y1 * iz;
            const double dx = q.x - px, dy = q.y - py;
            const double r2 = Y2 > 0.0 ? dx * dx + dy * dy : 1e300;
            sc += ap_cost(r2, thr2);
            if (r2 < thr2) {
                const double e0 = px - q.x, e1 = py - q.y;
                // G_k = R (e_k x X): e_0 x X = (0, -X2, X1), e_1 x X = (X2, 0, -X0), e_2 x X = (-X1, X0, 0)
                const double G[3][3] = {{Rc[2] * q.X1 - Rc[1] * q.X2, Rc[5] * q.X1 - Rc[4] * q.X2, Rc[8] * q.X1 - Rc[7] * q.X2},
                                        {Rc[0] * q.X2 - Rc[2] * q.X0, Rc[3] * q.X2 - Rc[5] * q.X0, Rc[6] * q.X2 - Rc[8] * q.X0},
                                        {Rc[1] * q.X0 - Rc[0] * q.X1, Rc[4] * q.X0 - Rc[3] * q.X1, Rc[7] * q.X0 - Rc[6] * q.X1}};
                const double ax = -(px * iz), ay = -(py * iz);      // de0/dY = (iz, 0, ax), de1/dY = (0, iz, ay)
                const double J0[6] = {iz * G[0][0] + ax * G[0][2], iz * G[1][0] + ax * G[1][2], iz * G[2][0] + ax * G[2][2], iz, 0.0, ax};
                const double J1[6] = {iz * G[0][1] + ay * G[0][2], iz * G[1][1] + ay * G[1][2], iz * G[2][1] + ay * G[2][2], 0.0, iz, ay};
                int k = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
#pragma unroll
                    for (int j = i; j < 6; ++j) { sm[k] = sm[k] + (J0[i] * J0[j] + J1[i] * J1[j]); ++k; }
                    sm[21 + i] = sm[21 + i] + (J0[i] * e0 + J1[i] * e1);
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
        if (step == ap::LO_ITERS) break;
        double Rn[9], tn2[3];
        if (!ap_gn_update(sm, Rc, tcur, Rn, tn2)) break;
        for (int k = 0; k < 9; ++k) Rc[k] = Rn[k];
        for (int k = 0; k < 3; ++k) tcur[k] = tn2[k];
        __syncthreads();                                     // sc_sh read by everybody before it is cleared again
    }
    // ---- inlier mask under the final pose
    __syncthreads();
    if (tid == 0) cnt_sh = 0u;
    __syncthreads();
    unsigned cn = 0;
    for_each([&](int, const ApPt& q) { cn += ap_residual2(Rb, tb, q.x, q.y, q.X0, q.X1, q.X2) < thr2 ? 1u : 0u; });
    atomicAdd(&cnt_sh, cn);
    __syncthreads();
    const int n_in = (int)cnt_sh;
    const bool found = n_in >= 3;
    for_each([&](int i, const ApPt& q) { mask[i] = found && ap_residual2(Rb, tb, q.x, q.y, q.X0, q.X1, q.X2) < thr2 ? 1 : 0; });
    for (int i = n + tid; i < a.cap; i += 256) mask[i] = 0;
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) Rout[k] = found ? Rb[k] : 0.0;
        for (int k = 0; k < 3; ++k) tout[k] = found ? tb[k] : 0.0;
        rs::write_info(info, found, best, iters_run, n_in, lo_accepted, n, c_best);
    }
}

size_t abspose_workspace_bytes(int P, int max_iters) {
    const size_t pad = (size_t)ceil_div(max_iters, 256) * 256;
    const size_t per = (size_t)ap::MAX_CAND * ap::CAND_DOUBLES * 8 + (size_t)ap::MAX_CAND * 12 + 4;
    return (size_t)P * pad * per + (size_t)P * 4 + 1024;
}

int launch_estimate_abspose(const float* p2, const float* p3, const int64_t* idx2, const int64_t* idx3, int cap2, int cap3, const int32_t* counts,
                            int n_const, int P, int cap, const double* K, double max_err, int min_iters, int max_iters, double success_prob,
                            unsigned long long seed, double* R, double* t, unsigned char* mask, int32_t* info, void* ws, hipStream_t st) {
    if (max_iters < 1 || max_iters > ap::MAX_ITERS || P > 65535) return -1;
    ApArgs a;
    a.p2 = p2; a.p3 = p3; a.idx2 = idx2; a.idx3 = idx3; a.cap2 = idx2 ? cap2 : cap; a.cap3 = idx3 ? cap3 : cap; a.counts = counts; a.n_const = n_const;
    a.P = P; a.cap = cap; a.K = K; a.iters = max_iters; a.iters_pad = ceil_div(max_iters, 256) * 256; a.min_iters = min_iters < 0 ? 0 : min_iters;
    a.max_err = max_err; a.log1mp = log(1.0 - success_prob); a.seed = seed;
    unsigned char* w = static_cast<unsigned char*>(ws);
    const size_t nhyp = (size_t)P * a.iters_pad;
    a.cand = reinterpret_cast<double*>(w); w += nhyp * ap::MAX_CAND * ap::CAND_DOUBLES * 8;
    a.hcost = reinterpret_cast<unsigned long long*>(w); w += nhyp * ap::MAX_CAND * 8;
    a.hcnt = reinterpret_cast<unsigned*>(w); w += nhyp * ap::MAX_CAND * 4;
    a.ncand = reinterpret_cast<int*>(w); w += nhyp * 4;
    a.bound = reinterpret_cast<int*>(w);
    a.R = R; a.t = t; a.mask = mask; a.info = info;
    a.chunk = rs::score_chunk(P, cap);
    const int nblk = ceil_div(max_iters, ap::HYP_PER_WG), nch = ceil_div(cap, a.chunk);
    const size_t zg = (nhyp + 255) / 256;
    abspose_zero_kernel<<<(unsigned)(zg > 2048 ? 2048 : zg), 256, 0, st>>>(a, nhyp);
    abspose_solve_kernel<<<dim3(1, P), 256, 0, st>>>(a, 0, 0);
    abspose_score_kernel<<<dim3(1, nch, P), 256, 0, st>>>(a, 0, 0);
    if (nblk > 1) {
        abspose_bound_kernel<<<P, 256, 0, st>>>(a);
        abspose_solve_kernel<<<dim3(nblk - 1, P), 256, 0, st>>>(a, ap::HYP_PER_WG, 1);
        abspose_score_kernel<<<dim3(nblk - 1, nch, P), 256, 0, st>>>(a, 1, 1);
    }
    const size_t red = (rs::block_sums_bytes(ap::NSUM) + 31) & ~(size_t)31;
    const size_t tiles = (size_t)ap::SEL_TILE * 16;
    const size_t lds = (red > tiles ? red : tiles) + (size_t)ap::SEL_CACHE * sizeof(ApPt);
    static AttrMask attr_sel = 0;
    set_max_dynamic_lds(reinterpret_cast<const void*>(abspose_select_kernel), (int)lds, attr_sel);
    abspose_select_kernel<<<P, 256, lds, st>>>(a);
    return 0;
}

}  // namespace xfh
