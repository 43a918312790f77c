// Two-view structure: the 3D points that the correspondences of a pair see under a relative pose (triangulation), and the pose of an
// essential matrix chosen by those points (what cv2.recoverPose does for modules/eval/scannet1500.py:84 of the reference: decompose E into
// four poses, keep the one that puts the points in front of both cameras).  cv2 is not available offline, so nothing here is pinned to it:
// what is implemented is the published method -- Lindstrom's optimal two-view correction ("Triangulation made easy", CVPR 2010, variant
// niter2 with its closing step solved exactly) followed by the closed-form depths of the corrected rays.  The specification (tests/structure_reference.py is a
// numpy restatement of it, operation for operation, and tests/test_structure_emulated.py compiles the solver below on the host and holds
// it to that restatement bit for bit):
//   * inputs of pair p: two point lists (cap rows of 2 fp32 pixels) or, with index lists, two key-point lists (kcap rows) and correspondence
//     i = (row idx0[i] of image 0, row idx1[i] of image 1); an index outside [0, kcap) makes the correspondence "not finite"; PINHOLE
//     intrinsics K0, K1 (row-major 3x3); a pose with X1 = R X0 + t and E = [t]x R (tg_pose_E: the formula of k_relpose.hip's rp_pose_E);
//   * calibration: x0 = ((u0 - cx0) / fx0, (v0 - cy0) / fy0, 1), x1 likewise with K1, in fp64;
//   * correction onto x1' E x0 = 0 (tg_correct).  With S = [[1,0,0],[0,1,0]] and Et = S E S':
//         n = S E x0, n' = S E' x1, a = n . (Et n'), b = (n.n + n'.n') / 2, c = x1' E x0, d = sqrt(b^2 - a c),
//         lambda = c / (b + d), D1 = lambda n, D0 = lambda n', n1 = n - Et D0, n1' = n' - Et' D1 (the gradients at the corrected pair),
//         then the second step along them: a1 = n1 . (Et n1'), b1 = (n1.n + n1'.n') / 2, lambda1 = c / (b1 + sqrt(b1^2 - a1 c)),
//         y1 = x1 - lambda1 n1, y0 = x0 - lambda1 n1'  (third components stay 1).
//     lambda1 is the root of the constraint along (n1', n1), a1 l^2 - 2 b1 l + c = 0, so the pair meets the constraint to rounding; niter2
//     closes with the approximation lambda 2 d / (n1.n1 + n1'.n1') of that root instead, which leaves up to 1.4e-2 px of epipolar
//     distance for pairs near an epipole at 10 px of noise; the directions, and with them the optimality, are niter2's.
//     The displacement does not depend on the scale or sign of E in exact arithmetic and not on its sign in floating point;
//   * depths (tg_depths): r = R y0, z = y1 x r, zz = z.z, l0 = -(z . (y1 x t)) / zz, l1 = (z . (t x r)) / zz, X = l0 y0 in camera 0's frame
//     and the unit of t; l0 and l1 are the z-depths in the two cameras;
//   * status, the first failing gate wins: 0 valid; 1 masked out by the input mask (rows at or beyond the pair's count are written as 1
//     too and are not counted in info); 2 not finite (a coordinate that is not finite, an index out of range, an unusable pose = an entry
//     that is not finite, R all zero, t all zero; zz not > 0; X or l1 not finite); 3 behind (l0 <= 0 or l1 <= 0); 4 far (l0 or l1 >
//     max_depth); 5 reprojection (max(e0^2, e1^2) > max_reproj_error^2, e0^2 = ((y0.x - x0.x) fx0)^2 + ((y0.y - x0.y) fy0)^2, e1^2 alike);
//     6 parallax (cos = (r.y1) / sqrt((r.r)(y1.y1)) > cos_min; the host passes cos_min = cos(min_parallax_deg): no trigonometry here);
//   * outputs per correspondence: X as 3 fp32, NaN unless the status is 0 (the convention of unproject_keypoints); the status; the
//     reprojection error sqrt(max(e0^2, e1^2)) as fp32, NaN for status 1 and 2;
//   * pose from E (tg_decompose): E at any scale or sign; s^2 = tr(E E') / 2, t = the cross product of two columns of E (largest norm)
//     made unit, R = cof(E) / s^2 -+ [t]x E / s, the poses in the order (Ra, t) (Ra, -t) (Rb, t) (Rb, -t) -- the decomposition inside
//     relpose_solve of k_relpose.hip, restated here (a DUPLICATE: that one works on the LDS slice of a hypothesis and its emulated tests
//     hold it bit for bit, so it is left alone), each R then moved to the nearest rotation by three Newton-Schulz steps (tg_orthonormalise:
//     the result is the SVD decomposition's rotation when E = K1' F K0 is essential only nearly).  E with an entry that is not finite, s^2 or the cross product not > 0, or a pose that is
//     not finite: unusable.  The correction runs once on E / s and the four depth solves reuse it; pose q gets the vote of every
//     correspondence that passes gates 1-4 under it with max_depth = distance_thresh (cv2.recoverPose's: depth in (0, distance_thresh) in
//     both cameras); the winner is the highest count, ties to the lowest pose index; an unusable E or a best count of 0: found = 0, zeros;
//   * only + - * / sqrt in all of it, every product and sum rounded once (fp contraction off in this file).
//
// Launches per call (no workspace):
//   triangulate_kernel   : thread = correspondence, grid = (chunks of 256 of cap, P); the pair's pose and intrinsics through LDS once per
//                          workgroup; per-pair status counts by wave ballots + popcount, one integer atomic per wave and status (integer
//                          sums carry no order: info is reproducible); optional scatter of the valid points to image 0's key-point rows
//   recover_pose_kernel  : one workgroup per pair: decomposition, the four votes (integer LDS atomics), the winner, its mask and points
#include "ransac_common.hpp"
#include "twoview_math.hpp"

#pragma clang fp contract(off)

namespace xfh {

// ---- solver begin (host-compilable: tests/test_structure_emulated.py slices it out behind the slice of twoview_math.hpp and drops the
// __device__ qualifiers) ----
namespace tg {
constexpr int VALID = 0, MASKED = 1, NOT_FINITE = 2, BEHIND = 3, FAR = 4, REPROJ = 5, PARALLAX = 6, NSTATUS = 7;
constexpr int POLAR_STEPS = 3;              // tg_orthonormalise
}  // namespace tg

// E = [t]x R
__device__ inline void tg_pose_E(const double* R, const double* t, double* E) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}
// a pose that can triangulate: every entry finite, R not all zero (what "not found" pairs carry), t not zero
__device__ inline bool tg_pose_ok(const double* R, const double* t) {
    bool fin = true, rnz = false, tnz = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) { fin = fin && tv::is_finite(R[k]); rnz = rnz || R[k] != 0.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { fin = fin && tv::is_finite(t[k]); tnz = tnz || t[k] != 0.0; }
    return fin && rnz && tnz;
}
// a correspondence after calibration and correction: y0, y1 the corrected rays (third component 1), e2 = max(e0^2, e1^2) in pixels^2
struct TgRays {
    double y0x, y0y, y1x, y1y, e2;
    bool fin;                                              // the four pixel coordinates are finite
};
// cal = fx0 fy0 cx0 cy0 fx1 fy1 cx1 cy1
__device__ inline TgRays tg_correct(const double* E, const double* cal, double u0, double v0, double u1, double v1) {
    TgRays q;
    q.fin = tv::is_finite(u0) && tv::is_finite(v0) && tv::is_finite(u1) && tv::is_finite(v1);
    const double x0x = (u0 - cal[2]) / cal[0], x0y = (v0 - cal[3]) / cal[1];
    const double x1x = (u1 - cal[6]) / cal[4], x1y = (v1 - cal[7]) / cal[5];
    double n0 = (E[0] * x0x + E[1] * x0y) + E[2], n1 = (E[3] * x0x + E[4] * x0y) + E[5];            // n  = S E x0
    double m0 = (E[0] * x1x + E[3] * x1y) + E[6], m1 = (E[1] * x1x + E[4] * x1y) + E[7];            // n' = S E' x1
    const double a = n0 * (E[0] * m0 + E[1] * m1) + n1 * (E[3] * m0 + E[4] * m1);
    const double b = 0.5 * ((n0 * n0 + n1 * n1) + (m0 * m0 + m1 * m1));
    const double c = (x1x * n0 + x1y * n1) + ((E[6] * x0x + E[7] * x0y) + E[8]);
    const double d = sqrt(b * b - a * c);
    double lam = c / (b + d);
    const double d1x = lam * n0, d1y = lam * n1, d0x = lam * m0, d0y = lam * m1;
    const double p0 = n0, p1 = n1, q0 = m0, q1 = m1;     // the gradients at the measured pair
    n0 = n0 - (E[0] * d0x + E[1] * d0y); n1 = n1 - (E[3] * d0x + E[4] * d0y);
    m0 = m0 - (E[0] * d1x + E[3] * d1y); m1 = m1 - (E[1] * d1x + E[4] * d1y);
    const double a1 = n0 * (E[0] * m0 + E[1] * m1) + n1 * (E[3] * m0 + E[4] * m1);
    const double b1 = 0.5 * ((n0 * p0 + n1 * p1) + (m0 * q0 + m1 * q1));
    lam = c / (b1 + sqrt(b1 * b1 - a1 * c));
    q.y1x = x1x - lam * n0; q.y1y = x1y - lam * n1;
    q.y0x = x0x - lam * m0; q.y0y = x0y - lam * m1;
    const double ax = (q.y0x - x0x) * cal[0], ay = (q.y0y - x0y) * cal[1];
    const double bx = (q.y1x - x1x) * cal[4], by = (q.y1y - x1y) * cal[5];
    const double e0 = ax * ax + ay * ay, e1 = bx * bx + by * by;
    q.e2 = e0 > e1 ? e0 : e1;
    return q;
}
// depths l0, l1 of the corrected rays under (R, t), zz = |y1 x R y0|^2 and r = R y0
__device__ inline void tg_depths(const double* R, const double* t, const TgRays& q, double& l0, double& l1, double& zz, double* r) {
    const double y1[3] = {q.y1x, q.y1y, 1.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = (R[3 * i] * q.y0x + R[3 * i + 1] * q.y0y) + R[3 * i + 2];
    double z[3], a[3], b[3];
    tv::cross3(y1, r, z); tv::cross3(y1, t, a); tv::cross3(t, r, b);
    zz = tv::dot3(z, z);
    l0 = -tv::dot3(z, a) / zz;
    l1 = tv::dot3(z, b) / zz;
}
// gates 2-4 (what the pose vote shares with the triangulation); X = l0 y0
__device__ inline int tg_depth_status(bool usable, const TgRays& q, double l0, double l1, double zz, double max_depth, double* X) {
    X[0] = l0 * q.y0x; X[1] = l0 * q.y0y; X[2] = l0;
    const bool fin = usable && q.fin && zz > 0.0 && tv::is_finite(X[0]) && tv::is_finite(X[1]) && tv::is_finite(X[2]) && tv::is_finite(l1);
    if (!fin) return tg::NOT_FINITE;
    if (!(l0 > 0.0) || !(l1 > 0.0)) return tg::BEHIND;
    if (l0 > max_depth || l1 > max_depth) return tg::FAR;
    return tg::VALID;
}
// the per-correspondence function: status, X3 (NaN unless valid), err (NaN when masked or not finite); gate = l0, l1, e2, cos for the tests
__device__ inline int tg_point(const double* R, const double* t, const double* E, bool usable, const double* cal, double u0, double v0, double u1,
                               double v1, bool masked, double thr2, double cos_min, double max_depth, float* X3, float& err, double* gate) {
    const TgRays q = tg_correct(E, cal, u0, v0, u1, v1);
    double l0, l1, zz, r[3], X[3];
    tg_depths(R, t, q, l0, l1, zz, r);
    int st = tg_depth_status(usable, q, l0, l1, zz, max_depth, X);
    const double y1[3] = {q.y1x, q.y1y, 1.0};
    const double cosv = tv::dot3(r, y1) / sqrt(tv::dot3(r, r) * tv::dot3(y1, y1));
    if (st == tg::VALID && q.e2 > thr2) st = tg::REPROJ;
    if (st == tg::VALID && cosv > cos_min) st = tg::PARALLAX;
    if (masked) st = tg::MASKED;
    const float nanv = __builtin_nanf("");
    const bool ok = st == tg::VALID;
    X3[0] = ok ? (float)X[0] : nanv; X3[1] = ok ? (float)X[1] : nanv; X3[2] = ok ? (float)X[2] : nanv;
    err = st == tg::MASKED || st == tg::NOT_FINITE ? nanv : (float)sqrt(q.e2);
    gate[0] = l0; gate[1] = l1; gate[2] = q.e2; gate[3] = cosv;
    return st;
}
// The rotation nearest to R (its polar factor) by tg::POLAR_STEPS Newton-Schulz steps R <- R (3 I - R'R) / 2: for an E that is essential
// only nearly (K1' F K0 of an estimated F: two singular values that differ) cof(E) / s^2 -+ [t]x E / s is U W diag(s1/s, s2/s, s1 s2/s^2) V',
// a rotation times a symmetric factor near I, and its polar factor U W V' is the rotation of the SVD decomposition (each step squares the
// distance from orthonormal: 1e-2 -> 1e-4 -> 1e-8 -> 1e-16); an essential E's R moves in its last bits only
__device__ inline void tg_orthonormalise(double* R) {
    for (int it = 0; it < tg::POLAR_STEPS; ++it) {
        double M[9], Rn[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) M[3 * i + j] = (i == j ? 1.5 : 0.0) - 0.5 * ((R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rn[3 * r + j] = (R[3 * r] * M[j] + R[3 * r + 1] * M[3 + j]) + R[3 * r + 2] * M[6 + j];
#pragma unroll
        for (int m = 0; m < 9; ++m) R[m] = Rn[m];
    }
}
// The four poses of E at any scale or sign: Ra, Rb, t (unit) -- (Ra, t) (Ra, -t) (Rb, t) (Rb, -t) -- and En = E / s; false: unusable.
// (The decomposition of k_relpose.hip's relpose_solve, restated.)
__device__ inline bool tg_decompose(const double* E, double* Ra, double* Rb, double* t, double* En) {
    bool ok = true;
    double s2 = 0.0;
#pragma unroll
    for (int m = 0; m < 9; ++m) { ok = ok && tv::is_finite(E[m]); s2 = s2 + E[m] * E[m]; }
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
    ok = ok && nt > 0.0 && s2 > 0.0;
    const double tn = sqrt(nt), sc = sqrt(s2);
#pragma unroll
    for (int m = 0; m < 3; ++m) t[m] = tc[m] / tn;
    double cof[9], te[9];
    tv::cross3(E + 3, E + 6, cof); tv::cross3(E + 6, E, cof + 3); tv::cross3(E, E + 3, cof + 6);
    tg_pose_E(E, t, te);                                   // [t]x E (the same products as [t]x R)
#pragma unroll
    for (int m = 0; m < 9; ++m) {
        const double a = cof[m] / s2, b = te[m] / sc;
        Ra[m] = a - b; Rb[m] = a + b;
        En[m] = E[m] / sc;
    }
    tg_orthonormalise(Ra);
    tg_orthonormalise(Rb);
#pragma unroll
    for (int m = 0; m < 9; ++m) ok = ok && tv::is_finite(Ra[m]) && tv::is_finite(Rb[m]) && tv::is_finite(En[m]);
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && tv::is_finite(t[m]);
    return ok;
}
// status of gates 2-4 of one corrected correspondence under pose Q of the four (compile time: no pose is indexed at run time); X under it
template <int Q>
__device__ inline int tg_vote(const double* Ra, const double* Rb, const double* t, bool usable, const TgRays& q, double max_depth, double* X) {
    const double sg = (Q & 1) ? -1.0 : 1.0;
    const double tq[3] = {sg * t[0], sg * t[1], sg * t[2]};
    double l0, l1, zz, r[3];
    tg_depths(Q < 2 ? Ra : Rb, tq, q, l0, l1, zz, r);
    return tg_depth_status(usable, q, l0, l1, zz, max_depth, X);
}
// the winner of the four counts: the highest, ties to the lowest pose index
__device__ inline int tg_winner(int c0, int c1, int c2, int c3) {
    int w = 0, best = c0;
    if (c1 > best) { w = 1; best = c1; }
    if (c2 > best) { w = 2; best = c2; }
    if (c3 > best) { w = 3; best = c3; }
    return w;
}
// ---- solver end ----

struct TgArgs {
    const float* p0;          // (P, kcap, 2): the correspondences (idx0 == NULL, kcap == cap) or the key-point lists they index
    const float* p1;
    const int64_t* idx0;      // (P, cap) rows of p0 / p1 of correspondence i, or NULL
    const int64_t* idx1;
    const int32_t* counts;
    const double* K0;         // (P, 3, 3)
    const double* K1;
    const double* R;          // triangulate: (P, 3, 3), (P, 3)
    const double* t;
    const double* E;          // recover pose: (P, 3, 3)
    const unsigned char* mask_in;   // (P, cap) or NULL
    int n_const, P, cap, kcap;
    double thr2, cos_min, max_depth;
    float* X;                 // (P, cap, 3) (recover pose: or NULL)
    float* Xref;              // (P, kcap, 3) or NULL, pre-filled with NaN
    unsigned char* status;
    float* err;
    int32_t* info;
    double* Rout;             // recover pose
    double* tout;
    int32_t* good;
    unsigned char* mask_out;
};

// correspondence i of a pair through the index lists when given; false: an index outside [0, kcap).  r0 = its row of image 0
struct TgView {
    const float* p0;
    const float* p1;
    const int64_t* i0;
    const int64_t* i1;
    unsigned long long kcap;
    __device__ TgView(const TgArgs& a, int pair)
        : p0(a.p0 + (size_t)pair * a.kcap * 2), p1(a.p1 + (size_t)pair * a.kcap * 2), i0(a.idx0 ? a.idx0 + (size_t)pair * a.cap : nullptr),
          i1(a.idx1 ? a.idx1 + (size_t)pair * a.cap : nullptr), kcap((unsigned long long)a.kcap) {}
    __device__ inline bool get(int i, float4& q, unsigned long long& r0) const {
        r0 = i0 ? (unsigned long long)i0[i] : (unsigned long long)i;
        const unsigned long long r1 = i1 ? (unsigned long long)i1[i] : (unsigned long long)i;
        const bool in = r0 < kcap && r1 < kcap;              // (a negative index is a huge unsigned one)
        const float nanv = __builtin_nanf("");
        q = make_float4(nanv, nanv, nanv, nanv);
        if (in) {
            const float2 a = *reinterpret_cast<const float2*>(p0 + 2 * r0);
            const float2 b = *reinterpret_cast<const float2*>(p1 + 2 * r1);
            q = make_float4(a.x, a.y, b.x, b.y);
        }
        return in;
    }
};

// cal = fx0 fy0 cx0 cy0 fx1 fy1 cx1 cy1 of a pair: entry j of that list is entry tg_cal_src(j) of K0 (j < 4) or K1
__device__ inline int tg_cal_src(int j) {
    const int k = j & 3;
    return k == 0 ? 0 : (k == 1 ? 4 : (k == 2 ? 2 : 5));
}

__global__ __launch_bounds__(256) void triangulate_kernel(TgArgs a) {
    __shared__ double ps[20];                              // R (9), t (3), cal (8)
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const int i = blockIdx.x * 256 + tid;
    if (tid < 9) ps[tid] = a.R[(size_t)pair * 9 + tid];
    else if (tid < 12) ps[tid] = a.t[(size_t)pair * 3 + (tid - 9)];
    else if (tid < 20) ps[tid] = (tid < 16 ? a.K0 : a.K1)[(size_t)pair * 9 + tg_cal_src(tid - 12)];
    __syncthreads();
    double R[9], t[3], cal[8], E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = ps[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ps[9 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) cal[k] = ps[12 + k];
    tg_pose_E(R, t, E);
    const bool usable = tg_pose_ok(R, t);
    const bool counted = i < n;                            // (n <= cap)
    int st = tg::MASKED;
    if (counted) {
        const TgView pts(a, pair);
        float4 q;
        unsigned long long r0;
        const bool in = pts.get(i, q, r0);
        const bool masked = a.mask_in && a.mask_in[(size_t)pair * a.cap + i] == 0;
        float X3[3], err;
        double gate[4];
        st = tg_point(R, t, E, usable, cal, (double)q.x, (double)q.y, (double)q.z, (double)q.w, masked, a.thr2, a.cos_min, a.max_depth, X3, err, gate);
        const size_t o = (size_t)pair * a.cap + i;
        a.X[3 * o] = X3[0]; a.X[3 * o + 1] = X3[1]; a.X[3 * o + 2] = X3[2];
        a.status[o] = (unsigned char)st;
        a.err[o] = err;
        if (a.Xref && st == tg::VALID && in) {
            float* ref = a.Xref + ((size_t)pair * a.kcap + (size_t)r0) * 3;
            ref[0] = X3[0]; ref[1] = X3[1]; ref[2] = X3[2];
        }
    } else if (i < a.cap) {                                // beyond the pair's count: written, not counted
        const size_t o = (size_t)pair * a.cap + i;
        const float nanv = __builtin_nanf("");
        a.X[3 * o] = nanv; a.X[3 * o + 1] = nanv; a.X[3 * o + 2] = nanv;
        a.status[o] = (unsigned char)tg::MASKED;
        a.err[o] = nanv;
    }
    // ---- status counts: one ballot per status, one atomic per wave and status
    int32_t* info = a.info + (size_t)pair * 8;
    const bool lead = (tid & 63) == 0;
#pragma unroll
    for (int s = 0; s < tg::NSTATUS; ++s) {
        const unsigned long long m = __ballot(counted && st == s);
        if (lead && m) atomicAdd(info + 1 + s, (int)__popcll(m));
    }
    if (blockIdx.x == 0 && tid == 0) info[0] = n;          // (the counts were zeroed before the launch; nobody adds to word 0)
}

__global__ __launch_bounds__(256) void recover_pose_kernel(TgArgs a) {
    __shared__ double es[20];                              // E (9), 3 unused, cal (8)
    __shared__ int cnt[4];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    if (tid < 9) es[tid] = a.E[(size_t)pair * 9 + tid];
    else if (tid >= 12 && tid < 20) es[tid] = (tid < 16 ? a.K0 : a.K1)[(size_t)pair * 9 + tg_cal_src(tid - 12)];
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    double Ein[9], cal[8], Ra[9], Rb[9], t[3], En[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ein[k] = es[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) cal[k] = es[12 + k];
    const bool usable = tg_decompose(Ein, Ra, Rb, t, En);
    const TgView pts(a, pair);
    const unsigned char* mask_in = a.mask_in ? a.mask_in + (size_t)pair * a.cap : nullptr;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int i = tid; i < n; i += 256) {
        float4 q;
        unsigned long long r0;
        pts.get(i, q, r0);
        if (mask_in && mask_in[i] == 0) continue;
        const TgRays ry = tg_correct(En, cal, (double)q.x, (double)q.y, (double)q.z, (double)q.w);
        double X[3];
        c0 += tg_vote<0>(Ra, Rb, t, usable, ry, a.max_depth, X) == tg::VALID ? 1 : 0;
        c1 += tg_vote<1>(Ra, Rb, t, usable, ry, a.max_depth, X) == tg::VALID ? 1 : 0;
        c2 += tg_vote<2>(Ra, Rb, t, usable, ry, a.max_depth, X) == tg::VALID ? 1 : 0;
        c3 += tg_vote<3>(Ra, Rb, t, usable, ry, a.max_depth, X) == tg::VALID ? 1 : 0;
    }
    if (c0) atomicAdd(&cnt[0], c0);
    if (c1) atomicAdd(&cnt[1], c1);
    if (c2) atomicAdd(&cnt[2], c2);
    if (c3) atomicAdd(&cnt[3], c3);
    __syncthreads();
    const int g0 = cnt[0], g1 = cnt[1], g2 = cnt[2], g3 = cnt[3];
    const int w = tg_winner(g0, g1, g2, g3);
    const int best = w == 0 ? g0 : (w == 1 ? g1 : (w == 2 ? g2 : g3));
    const bool found = usable && best > 0;
    // ---- the winner's mask and points
    double Rw[9], tw[3];
    const double sg = (w & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rw[k] = w < 2 ? Ra[k] : Rb[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tw[k] = sg * t[k];
    unsigned char* mask = a.mask_out + (size_t)pair * a.cap;
    float* Xo = a.X ? a.X + (size_t)pair * a.cap * 3 : nullptr;
    const float nanv = __builtin_nanf("");
    for (int i = tid; i < a.cap; i += 256) {
        bool pass = false;
        double X[3] = {0.0, 0.0, 0.0};
        if (found && i < n && !(mask_in && mask_in[i] == 0)) {
            float4 q;
            unsigned long long r0;
            pts.get(i, q, r0);
            const TgRays ry = tg_correct(En, cal, (double)q.x, (double)q.y, (double)q.z, (double)q.w);
            double l0, l1, zz, r[3];
            tg_depths(Rw, tw, ry, l0, l1, zz, r);
            pass = tg_depth_status(usable, ry, l0, l1, zz, a.max_depth, X) == tg::VALID;
        }
        mask[i] = pass ? 1 : 0;
        if (Xo) { Xo[3 * i] = pass ? (float)X[0] : nanv; Xo[3 * i + 1] = pass ? (float)X[1] : nanv; Xo[3 * i + 2] = pass ? (float)X[2] : nanv; }
    }
    if (tid == 0) {
        double* Ro = a.Rout + (size_t)pair * 9;
        double* to = a.tout + (size_t)pair * 3;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ro[k] = found ? Rw[k] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) to[k] = found ? tw[k] : 0.0;
        int32_t* good = a.good + (size_t)pair * 4;
        good[0] = usable ? g0 : 0; good[1] = usable ? g1 : 0; good[2] = usable ? g2 : 0; good[3] = usable ? g3 : 0;
        int32_t* info = a.info + (size_t)pair * 8;         // the family's words: found, winner (pose index), 0, votes of the winner, 0, n, 0, 0
        info[0] = found ? 1 : 0; info[1] = found ? w : -1; info[2] = 0; info[3] = found ? best : 0; info[4] = 0; info[5] = n; info[6] = 0; info[7] = 0;
    }
}

static TgArgs tg_args(const float* p0, const float* p1, const int64_t* idx0, const int64_t* idx1, int kcap, const int32_t* counts, int n_const, int P,
                      int cap, const double* K0, const double* K1, const unsigned char* mask_in) {
    TgArgs a = {};
    a.p0 = p0; a.p1 = p1; a.idx0 = idx0; a.idx1 = idx1; a.kcap = idx0 ? kcap : cap; a.counts = counts; a.n_const = n_const; a.P = P; a.cap = cap;
    a.K0 = K0; a.K1 = K1; a.mask_in = mask_in;
    return a;
}

int launch_triangulate(const float* p0, const float* p1, const int64_t* idx0, const int64_t* idx1, int kcap, const int32_t* counts, int n_const, int P,
                       int cap, const double* K0, const double* K1, const double* R, const double* t, const unsigned char* mask_in,
                       double max_reproj_error, double cos_min, double max_depth, float* X, unsigned char* status, float* err, int32_t* info,
                       float* Xref, hipStream_t st) {
    if (P < 1 || P > 65535 || cap < 1) return -1;
    TgArgs a = tg_args(p0, p1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, mask_in);
    a.R = R; a.t = t; a.thr2 = max_reproj_error * max_reproj_error; a.cos_min = cos_min; a.max_depth = max_depth;
    a.X = X; a.status = status; a.err = err; a.info = info; a.Xref = idx0 ? Xref : nullptr;
    if (hipMemsetAsync(info, 0, (size_t)P * 8 * sizeof(int32_t), st) != hipSuccess) return -1;
    if (a.Xref && hipMemsetAsync(a.Xref, 0xFF, (size_t)P * a.kcap * 3 * sizeof(float), st) != hipSuccess) return -1;     // all ones: a NaN
    triangulate_kernel<<<dim3(ceil_div(cap, 256), P), 256, 0, st>>>(a);
    return 0;
}

int launch_recover_pose(const float* p0, const float* p1, const int64_t* idx0, const int64_t* idx1, int kcap, const int32_t* counts, int n_const, int P,
                        int cap, const double* K0, const double* K1, const double* E, const unsigned char* mask_in, double distance_thresh, double* R,
                        double* t, int32_t* good, unsigned char* mask, float* X, int32_t* info, hipStream_t st) {
    if (P < 1 || P > 65535 || cap < 1) return -1;
    TgArgs a = tg_args(p0, p1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, mask_in);
    a.E = E; a.max_depth = distance_thresh; a.Rout = R; a.tout = t; a.good = good; a.mask_out = mask; a.X = X; a.info = info;
    recover_pose_kernel<<<P, 256, 0, st>>>(a);
    return 0;
}

// ================================================================================================================================================
// Multi-view triangulation of key-point tracks (tests/multiview_reference.py restates it operation for operation,
// tests/tracks_reference.py restates the anchored form on that restatement's functions, and tests/test_multiview_emulated.py and
// tests/test_tracks_emulated.py compile the slice below, behind the slice above, on the host and hold it to them bit for bit).
// A call holds S scenes of up to V <= 32 views with PINHOLE intrinsics K_v and world -> camera poses x_v = R_v X + t_v;
// tracks[s, k, v] = the row of view v's key-point table that track k sees, or -1.  One per-track function, mv_track<FIRST>, in two
// instantiations that differ in the anchor view a alone: <false> a = 0, the reference view (a track is then a row of its table: 3.16);
// <true> a = the lowest view of the observed set, for tracks that view 0 need not see (3.18).  A track with a = 0 gets the same bits from
// both.  Per track:
//   * observed set O: views v < n_views[s] with a table entry in range, a finite pixel and a usable pose (entries finite, R not all zero;
//     t = 0 is a pose here); |O| < 2 or a not in O (which only <false> can meet): status 1;
//   * hypotheses, exhaustive: for v in O, v > a ascending, Rrel = R_v R_a', trel = t_v - Rrel t_a (zero: skipped), E = tg_pose_E (mv_pair:
//     <false> reads the three from view v's staged block, <true> calls it per hypothesis on the two staged poses), the point of
//     the pair (a, v) by tg_correct / tg_depths / tg_depth_status with max_depth, moved to the world frame X = R_a' (X_ca - t_a), scored by
//     MSAC sum_{w in O} min(e_w^2, thr^2) (e_w^2 the squared pixel reprojection error of X in w; thr^2 where the depth in w is not > 0 or e_w^2
//     is not finite); the lowest score wins, ties to the lowest v; no valid hypothesis: the failure code (2, 3, 4) of the lowest-v hypothesis
//     tried (the error is then that pair's correction, as tg_point's), none tried: 2;
//   * inliers I: w in O with depth > 0 and e_w^2 <= thr^2 under the winner, a 32-bit mask; a not in I or |I| < min_views: status 5;
//   * refit: mv::GN_ITERS Gauss-Newton steps on sum_{w in I} e_w^2(X), I fixed, the 3x3 normal equations summed in ascending w and solved by
//     cofactors; a step is kept only if it lowers the cost, otherwise the iteration stops;
//   * final gates on the refined X over I, the first failing one wins: 2 not finite; 3 depth <= 0 in an inlier view; 4 depth > max_depth in one;
//     5 max e_w^2 > thr^2; 6 min_{w in I \ {a}} cos(X - c_a, X - c_w) > cos_min (c_w = -R_w' t_w);
//   * outputs: X as 3 fp32 (NaN unless the status is 0), the status, |I|, I, sqrt(max_{w in I} e_w^2) as fp32 (NaN for status 1 and 2).
// Only + - * / sqrt, every product and sum rounded once, every sum over views in ascending view order.
//
// Launches (no workspace):
//   track_scatter_kernel            : thread = match i of the pair (view 0, view v), grid = (chunks of 256 of max(cap, K), V - 1, S): an integer
//                                     atomicMax onto the table pre-filled with -1 (duplicate reference rows resolve to the largest candidate
//                                     row: reproducible); the threads of v = 1 also write column 0
//   triangulate_views_kernel<FIRST> : thread = track, grid = (chunks of 256 of K, S); the first V threads of a workgroup put the per-view block
//                                     (mv::STRIDE doubles: R, t, calibration, centre, pose flag by mv_stage_pose and, for <false>, Rrel, trel,
//                                     E of the pair (0, v) by mv_stage_view; <true> leaves those three unwritten and unread; 10.3 KB at
//                                     V = 32) into LDS once; every lane reads the same LDS address in the view loops (broadcasts); the
//                                     observations are re-read from global memory through the track table inside the loops; status counts
//                                     as triangulate_kernel's

// ---- views solver begin (host-compilable: tests/test_multiview_emulated.py and tests/test_tracks_emulated.py slice it out behind the solver
// slice above) ----
namespace mv {
constexpr int MAX_VIEWS = 32;
constexpr int GN_ITERS = 5;                 // the refit's steps (the cost stops moving after 3 at 0.5 - 2 px of noise)
constexpr int UNOBSERVED = 1;               // the other status codes are tg::'s
// the per-view block of doubles
constexpr int ROT = 0, TRA = 9, CAL = 12, CEN = 16, OK = 19, RREL = 20, TREL = 29, ESS = 32, STRIDE = 41;
}  // namespace mv

// the first ba::STRIDE = 20 doubles of the per-view block of view v (ROT, TRA, CAL, CEN, OK): Rv (9), tv (3) its pose, Kv (9, row-major) its
// intrinsics
__device__ inline void mv_stage_pose(const double* Rv, const double* tv, const double* Kv, double* o) {
    bool fin = true, rnz = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) { o[mv::ROT + k] = Rv[k]; fin = fin && tv::is_finite(Rv[k]); rnz = rnz || Rv[k] != 0.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[mv::TRA + k] = tv[k]; fin = fin && tv::is_finite(tv[k]); }
    o[mv::CAL] = Kv[0]; o[mv::CAL + 1] = Kv[4]; o[mv::CAL + 2] = Kv[2]; o[mv::CAL + 3] = Kv[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[mv::CEN + i] = -((Rv[i] * tv[0] + Rv[3 + i] * tv[1]) + Rv[6 + i] * tv[2]);
    o[mv::OK] = fin && rnz ? 1.0 : 0.0;
}
// the pair (a, v): Rrel = Rv Ra', trel = tv - Rrel ta, E = [trel]x Rrel
__device__ inline void mv_pair(const double* Ra, const double* ta, const double* Rv, const double* tv, double* Rrel, double* trel, double* E) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rrel[3 * i + j] = (Rv[3 * i] * Ra[3 * j] + Rv[3 * i + 1] * Ra[3 * j + 1]) + Rv[3 * i + 2] * Ra[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) trel[i] = tv[i] - ((Rrel[3 * i] * ta[0] + Rrel[3 * i + 1] * ta[1]) + Rrel[3 * i + 2] * ta[2]);
    tg_pose_E(Rrel, trel, E);
}
// the whole per-view block of view v for the reference instantiation: mv_stage_pose and the pair (0, v); R0, t0 the pose of view 0
__device__ inline void mv_stage_view(const double* Rv, const double* tv, const double* Kv, const double* R0, const double* t0, double* o) {
    mv_stage_pose(Rv, tv, Kv, o);
    double Rrel[9], trel[3], E[9];
    mv_pair(R0, t0, Rv, tv, Rrel, trel, E);
#pragma unroll
    for (int k = 0; k < 9; ++k) { o[mv::RREL + k] = Rrel[k]; o[mv::ESS + k] = E[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) o[mv::TREL + k] = trel[k];
}
// squared pixel reprojection error of the world point X in the view of block p against the pixel (u, v); z = its depth there
__device__ inline double mv_reproj(const double* p, const double* X, double u, double v, double& z) {
    const double x = ((p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]) + p[mv::TRA];
    const double y = ((p[3] * X[0] + p[4] * X[1]) + p[5] * X[2]) + p[mv::TRA + 1];
    z = ((p[6] * X[0] + p[7] * X[1]) + p[8] * X[2]) + p[mv::TRA + 2];
    const double du = (p[mv::CAL] * (x / z) + p[mv::CAL + 2]) - u, dv = (p[mv::CAL + 1] * (y / z) + p[mv::CAL + 3]) - v;
    return du * du + dv * dv;
}
// the cost sum_{w in I} e_w^2 at X and its normal equations: A = J'J as (00 01 02 11 12 22), g = J'r.  obs(w, u, v) reads the pixel of view w.
template <class Obs>
__device__ inline double mv_normal(const double* vd, int nv, const Obs& obs, unsigned I, const double* X, double* A, double* g) {
    double cost = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = 0.0;
    for (int w = 0; w < nv; ++w) {
        if (!((I >> w) & 1u)) continue;
        const double* p = vd + w * mv::STRIDE;
        double u, v;
        obs(w, u, v);
        const double x = ((p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]) + p[mv::TRA];
        const double y = ((p[3] * X[0] + p[4] * X[1]) + p[5] * X[2]) + p[mv::TRA + 1];
        const double z = ((p[6] * X[0] + p[7] * X[1]) + p[8] * X[2]) + p[mv::TRA + 2];
        const double a = x / z, b = y / z;
        const double du = (p[mv::CAL] * a + p[mv::CAL + 2]) - u, dv = (p[mv::CAL + 1] * b + p[mv::CAL + 3]) - v;
        cost = cost + (du * du + dv * dv);
        const double ju0 = p[mv::CAL] * ((p[0] - a * p[6]) / z), ju1 = p[mv::CAL] * ((p[1] - a * p[7]) / z), ju2 = p[mv::CAL] * ((p[2] - a * p[8]) / z);
        const double jv0 = p[mv::CAL + 1] * ((p[3] - b * p[6]) / z), jv1 = p[mv::CAL + 1] * ((p[4] - b * p[7]) / z), jv2 = p[mv::CAL + 1] * ((p[5] - b * p[8]) / z);
        A[0] = A[0] + (ju0 * ju0 + jv0 * jv0); A[1] = A[1] + (ju0 * ju1 + jv0 * jv1); A[2] = A[2] + (ju0 * ju2 + jv0 * jv2);
        A[3] = A[3] + (ju1 * ju1 + jv1 * jv1); A[4] = A[4] + (ju1 * ju2 + jv1 * jv2); A[5] = A[5] + (ju2 * ju2 + jv2 * jv2);
        g[0] = g[0] + (ju0 * du + jv0 * dv); g[1] = g[1] + (ju1 * du + jv1 * dv); g[2] = g[2] + (ju2 * du + jv2 * dv);
    }
    return cost;
}
// the Gauss-Newton step -A^-1 g of the symmetric A (00 01 02 11 12 22) by cofactors
__device__ inline void mv_step(const double* A, const double* g, double* d) {
    const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
    const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
    const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
    d[0] = -(((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det);
    d[1] = -(((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det);
    d[2] = -(((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det);
}
struct MvResult {
    float X[3], err;           // NaN unless the status is 0; NaN for status 1 and 2
    int status, n_inliers;
    unsigned inliers;          // bit v = view v
    int winner;                // the view of the winning hypothesis, -1: none
    double score;              // its MSAC score (0 without a winner)
    double cost0, cost1;       // the refit's cost before and after (0 without a refit)
};
// the per-track function: vd the per-view blocks, nv = n_views[s], obs(w, u, v) = the pixel of view w through the track table (false: no
// entry in range; u, v then NaN).  The anchor a is view 0, which has to be observed (the reference instantiation: Rrel, trel, E of the
// pair (0, v) are read from view v's block, mv_stage_view), or with FIRST the lowest observed view (the pair (a, v) by mv_pair per
// hypothesis from the two blocks, which need mv_stage_pose alone).  MvResult::winner is the view of the winning hypothesis.
template <bool FIRST, class Obs>
__device__ inline MvResult mv_track(const double* vd, int nv, const Obs& obs, double thr2, double cos_min, double max_depth, int min_views) {
    const float nanv = __builtin_nanf("");
    MvResult o;
    o.X[0] = nanv; o.X[1] = nanv; o.X[2] = nanv; o.err = nanv;
    o.status = mv::UNOBSERVED; o.n_inliers = 0; o.inliers = 0u; o.winner = -1; o.score = 0.0; o.cost0 = 0.0; o.cost1 = 0.0;
    // ---- the observed set and the anchor
    unsigned O = 0u;
    int nobs = 0, low = -1;
    for (int w = 0; w < nv; ++w) {
        double u, v;
        const bool in = obs(w, u, v);
        if (in && tv::is_finite(u) && tv::is_finite(v) && vd[w * mv::STRIDE + mv::OK] != 0.0) { O |= 1u << w; ++nobs; low = low < 0 ? w : low; }
    }
    const int an = FIRST ? low : 0;
    if (nobs < 2 || (!FIRST && !(O & 1u))) return o;        // (the lowest view of O is in O: only view 0 can be a missing anchor)
    // ---- the hypotheses of the pairs (a, v)
    const double* pa = vd + an * mv::STRIDE;
    double ua, va;
    obs(an, ua, va);
    double Ra[9], ta[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ra[k] = pa[mv::ROT + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ta[k] = pa[mv::TRA + k];
    int first = -1;
    double first_e2 = 0.0, best = 0.0, X[3] = {0.0, 0.0, 0.0};
    for (int v = an + 1; v < nv; ++v) {
        if (!((O >> v) & 1u)) continue;
        const double* p = vd + v * mv::STRIDE;
        double Rrel[9], trel[3], E[9], cal[8];
        // the pair (a, v): computed here or staged (the staged Rrel and E are read behind the skip: in front of it hipcc gives each of the
        // loop's LDS reads an address register of its own)
        if (FIRST) {
            mv_pair(Ra, ta, p + mv::ROT, p + mv::TRA, Rrel, trel, E);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) trel[k] = p[mv::TREL + k];
        }
        if (trel[0] == 0.0 && trel[1] == 0.0 && trel[2] == 0.0) continue;
        if (!FIRST) {
#pragma unroll
            for (int k = 0; k < 9; ++k) { Rrel[k] = p[mv::RREL + k]; E[k] = p[mv::ESS + k]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { cal[k] = pa[mv::CAL + k]; cal[4 + k] = p[mv::CAL + k]; }
        double uv, vv;
        obs(v, uv, vv);
        const TgRays q = tg_correct(E, cal, ua, va, uv, vv);
        double l0, l1, zz, r[3], Xc[3];
        tg_depths(Rrel, trel, q, l0, l1, zz, r);
        const int st = tg_depth_status(true, q, l0, l1, zz, max_depth, Xc);
        if (first < 0) { first = st; first_e2 = q.e2; }
        if (st != tg::VALID) continue;
        const double d[3] = {Xc[0] - ta[0], Xc[1] - ta[1], Xc[2] - ta[2]};
        double Xw[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) Xw[i] = (Ra[i] * d[0] + Ra[3 + i] * d[1]) + Ra[6 + i] * d[2];
        double sc = 0.0;
        for (int w = an; w < nv; ++w) {
            if (!((O >> w) & 1u)) continue;
            double u, vpx, z;
            obs(w, u, vpx);
            const double e2 = mv_reproj(vd + w * mv::STRIDE, Xw, u, vpx, z);
            sc = sc + (z > 0.0 && tv::is_finite(e2) && e2 < thr2 ? e2 : thr2);
        }
        if (o.winner < 0 || sc < best) { o.winner = v; best = sc; X[0] = Xw[0]; X[1] = Xw[1]; X[2] = Xw[2]; }
    }
    if (o.winner < 0) {
        o.status = first < 0 ? tg::NOT_FINITE : first;
        if (o.status != tg::NOT_FINITE) o.err = (float)sqrt(first_e2);
        return o;
    }
    o.score = best;
    // ---- the inliers of the winner
    unsigned I = 0u;
    int ni = 0;
    double emax = 0.0;
    for (int w = an; w < nv; ++w) {
        if (!((O >> w) & 1u)) continue;
        double u, vpx, z;
        obs(w, u, vpx);
        const double e2 = mv_reproj(vd + w * mv::STRIDE, X, u, vpx, z);
        if (z > 0.0 && e2 <= thr2) { I |= 1u << w; ++ni; emax = e2 > emax ? e2 : emax; }
    }
    o.inliers = I; o.n_inliers = ni;
    if (!((I >> an) & 1u) || ni < min_views) { o.status = tg::REPROJ; o.err = (float)sqrt(emax); return o; }
    // ---- the refit on the fixed inlier set
    double A[6], g[3];
    double cost = mv_normal(vd, nv, obs, I, X, A, g);
    o.cost0 = cost;
    for (int it = 0; it < mv::GN_ITERS; ++it) {
        double d[3], An[6], gn[3];
        mv_step(A, g, d);
        const double Xn[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
        const double cn = mv_normal(vd, nv, obs, I, Xn, An, gn);
        if (!(cn < cost)) break;
        cost = cn; X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = An[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = gn[k];
    }
    o.cost1 = cost;
    // ---- the final gates
    bool fin = tv::is_finite(X[0]) && tv::is_finite(X[1]) && tv::is_finite(X[2]), behind = false, far = false;
    double cmin = 2.0;
    emax = 0.0;
    const double a[3] = {X[0] - pa[mv::CEN], X[1] - pa[mv::CEN + 1], X[2] - pa[mv::CEN + 2]};
    const double aa = tv::dot3(a, a);
    for (int w = an; w < nv; ++w) {
        if (!((I >> w) & 1u)) continue;
        const double* p = vd + w * mv::STRIDE;
        double u, vpx, z;
        obs(w, u, vpx);
        const double e2 = mv_reproj(p, X, u, vpx, z);
        fin = fin && tv::is_finite(e2) && tv::is_finite(z);
        behind = behind || !(z > 0.0);
        far = far || z > max_depth;
        emax = e2 > emax ? e2 : emax;
        if (w > an) {
            const double b[3] = {X[0] - p[mv::CEN], X[1] - p[mv::CEN + 1], X[2] - p[mv::CEN + 2]};
            const double c = tv::dot3(a, b) / sqrt(aa * tv::dot3(b, b));
            cmin = c < cmin ? c : cmin;
        }
    }
    o.status = !fin ? tg::NOT_FINITE : (behind ? tg::BEHIND : (far ? tg::FAR : (emax > thr2 ? tg::REPROJ : (cmin > cos_min ? tg::PARALLAX : tg::VALID))));
    if (o.status != tg::NOT_FINITE) o.err = (float)sqrt(emax);
    if (o.status == tg::VALID) { o.X[0] = (float)X[0]; o.X[1] = (float)X[1]; o.X[2] = (float)X[2]; }
    return o;
}
// ---- views solver end ----

struct MvArgs {
    const float* kpts;        // (S, V, kcap, 2)
    const int32_t* tracks;    // (S, K, V)
    const int32_t* n_views;   // (S,) or NULL: V
    const double* Ks;         // (S, V, 3, 3)
    const double* Rs;         // (S, V, 3, 3)
    const double* ts;         // (S, V, 3)
    int K, V, kcap, min_views;
    double thr2, cos_min, max_depth;
    float* X;                 // (S, K, 3)
    unsigned char* status;    // (S, K)
    unsigned char* n_inliers;
    int32_t* inliers;
    float* err;
    int32_t* info;            // (S, 8)
};

// the pixel of view w of a track through its row of the table
struct MvObs {
    const int32_t* row;       // (V,)
    const float* kp;          // (V, kcap, 2)
    unsigned kcap;
    __device__ inline bool operator()(int w, double& u, double& v) const {
        const unsigned r = (unsigned)row[w];                 // (-1 is a huge unsigned one)
        const bool in = r < kcap;
        const float nanv = __builtin_nanf("");
        float2 q = make_float2(nanv, nanv);
        if (in) q = *reinterpret_cast<const float2*>(kp + ((size_t)w * kcap + r) * 2);
        u = (double)q.x; v = (double)q.y;
        return in;
    }
};

template <bool FIRST>
__global__ __launch_bounds__(256) void triangulate_views_kernel(MvArgs a) {
    __shared__ double vd[mv::MAX_VIEWS * mv::STRIDE];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int k = blockIdx.x * 256 + tid;
    int nv = a.n_views ? a.n_views[s] : a.V;
    nv = nv < 0 ? 0 : (nv > a.V ? a.V : nv);
    if (tid < a.V) {
        const size_t v = (size_t)s * a.V + tid, v0 = (size_t)s * a.V;
        if (FIRST) mv_stage_pose(a.Rs + v * 9, a.ts + v * 3, a.Ks + v * 9, vd + tid * mv::STRIDE);
        else mv_stage_view(a.Rs + v * 9, a.ts + v * 3, a.Ks + v * 9, a.Rs + v0 * 9, a.ts + v0 * 3, vd + tid * mv::STRIDE);
    }
    __syncthreads();
    const bool counted = k < a.K;
    int st = -1;
    if (counted) {
        const size_t o = (size_t)s * a.K + k;
        MvObs obs;
        obs.row = a.tracks + o * a.V; obs.kp = a.kpts + (size_t)s * a.V * a.kcap * 2; obs.kcap = (unsigned)a.kcap;
        const MvResult r = mv_track<FIRST>(vd, nv, obs, a.thr2, a.cos_min, a.max_depth, a.min_views);
        st = r.status;
        a.X[3 * o] = r.X[0]; a.X[3 * o + 1] = r.X[1]; a.X[3 * o + 2] = r.X[2];
        a.status[o] = (unsigned char)st;
        a.n_inliers[o] = (unsigned char)r.n_inliers;
        a.inliers[o] = (int32_t)r.inliers;
        a.err[o] = r.err;
    }
    // ---- status counts: one ballot per status, one atomic per wave and status
    int32_t* info = a.info + (size_t)s * 8;
    const bool lead = (tid & 63) == 0;
#pragma unroll
    for (int c = 0; c < tg::NSTATUS; ++c) {
        const unsigned long long m = __ballot(counted && st == c);
        if (lead && m) atomicAdd(info + 1 + c, (int)__popcll(m));
    }
    if (blockIdx.x == 0 && tid == 0) info[0] = a.K;        // (the counts were zeroed before the launch; nobody adds to word 0)
}

// tracks (S, K, V) pre-filled with -1: column 0 = k, column v >= 1 = the largest row of view v that the list of the pair (0, v) gives row k
__global__ __launch_bounds__(256) void track_scatter_kernel(const int64_t* idx_ref, const int64_t* idx_view, const int32_t* n_matches, int V, int cap, int K,
                                                            int kcap, int32_t* tracks) {
    const int s = blockIdx.z, v = blockIdx.y + 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int32_t* tab = tracks + (size_t)s * K * V;
    if (v == 1 && i < K) tab[(size_t)i * V] = i;
    const size_t pair = (size_t)s * (V - 1) + (v - 1);
    int n = cap > 0 ? n_matches[pair] : 0;
    n = n > cap ? cap : n;
    if (i >= n) return;
    const unsigned long long r0 = (unsigned long long)idx_ref[pair * cap + i], r1 = (unsigned long long)idx_view[pair * cap + i];
    if (r0 < (unsigned long long)K && r1 < (unsigned long long)kcap) atomicMax(tab + (size_t)r0 * V + v, (int)r1);
}

int launch_build_tracks(const int64_t* idx_ref, const int64_t* idx_view, const int32_t* n_matches, int S, int V, int cap, int K, int kcap, int32_t* tracks,
                        hipStream_t st) {
    if (S < 1 || S > 65535 || V < 2 || V > mv::MAX_VIEWS || cap < 0 || K < 1 || kcap < 1) return -1;
    if (hipMemsetAsync(tracks, 0xFF, (size_t)S * K * V * sizeof(int32_t), st) != hipSuccess) return -1;       // all ones: -1
    track_scatter_kernel<<<dim3(ceil_div(cap > K ? cap : K, 256), V - 1, S), 256, 0, st>>>(idx_ref, idx_view, n_matches, V, cap, K, kcap, tracks);
    return 0;
}

int launch_triangulate_views(const float* kpts, int kcap, const int32_t* tracks, const int32_t* n_views, int S, int K, int V, const double* Ks,
                             const double* Rs, const double* ts, double max_reproj_error, double cos_min, double max_depth, int min_views, float* X,
                             unsigned char* status, unsigned char* n_inliers, int32_t* inliers, float* err, int32_t* info, bool first,
                             hipStream_t st) {
    if (S < 1 || S > 65535 || K < 1 || V < 2 || V > mv::MAX_VIEWS || kcap < 1) return -1;
    MvArgs a = {};
    a.kpts = kpts; a.tracks = tracks; a.n_views = n_views; a.Ks = Ks; a.Rs = Rs; a.ts = ts; a.K = K; a.V = V; a.kcap = kcap; a.min_views = min_views;
    a.thr2 = max_reproj_error * max_reproj_error; a.cos_min = cos_min; a.max_depth = max_depth;
    a.X = X; a.status = status; a.n_inliers = n_inliers; a.inliers = inliers; a.err = err; a.info = info;
    if (hipMemsetAsync(info, 0, (size_t)S * 8 * sizeof(int32_t), st) != hipSuccess) return -1;
    if (first) triangulate_views_kernel<true><<<dim3(ceil_div(K, 256), S), 256, 0, st>>>(a);
    else triangulate_views_kernel<false><<<dim3(ceil_div(K, 256), S), 256, 0, st>>>(a);
    return 0;
}

// ================================================================================================================================================
// Bundle adjustment of the poses of the free views and the points of the valid tracks (tests/bundle_reference.py restates it
// operation for operation and tests/test_bundle_emulated.py compiles the slice below, behind the two slices above, on the host and holds it
// to that restatement bit for bit).  Levenberg-Marquardt with Marquardt scaling on sum rho(e_w), e_w^2 = mv_reproj's, rho = Huber's at c pixels:
//   * observations, fixed at the input state: (k, w) with bit w of inlier_views[k], w < n_views, a table entry in range, a finite pixel, a
//     usable pose, a finite input point, depth > 0 and a finite e_w^2; a track with fewer than 2 is not refined and its observations are
//     dropped; a view is free when it is not in fixed_views and keeps at least ba::MIN_VIEW_OBS observations;
//   * parameters: R <- R cay(w), t <- t + d (ba_pose_update: the update inside k_abspose.hip's ap_gn_update, restated) and X <- X + dX;
//     dY/dw_j = R (e_j x X), dY/dd = I, dY/dX = R, the projection's derivative as mv_normal's;
//   * one step at damping lambda, opl = 1 + lambda: per point V_k = sum_w wt Jp'Jp, g_k = -sum_w wt Jp'r in ascending w, the diagonal of V_k
//     times opl, its inverse by cofactors (mv_step on the unit vectors); a determinant that is not finite or not > 0 holds the point for the
//     step.  Reduced camera system, n = 6 V, lower triangle packed: block (w, v), v <= w, = [v == w] U_v* - sum_k Y_wk W_vk' with
//     W_vk = wt Jc'Jp (6x3), Y_wk = W_wk V_k*^-1, the diagonal of U_v times opl term by term; rhs_v = sum_k (-wt Jc'r - Y_vk g_k); sums over
//     tracks by rs::block_sums (thread i of 256 takes tracks i, i + 256, ...); rows of held views are identity and zero.  Cholesky with every
//     element's subtractions in ascending column order, forward substitution ascending, back substitution descending; a pivot that is not
//     > 0 or not finite fails the step.  Candidate points dX_k = V_k*^-1 (g_k - sum_w W_wk' d_w) over the free views in ascending w;
//   * the candidate's cost is the robust sum (per track ascending w, per chunk of 256 tracks block_sums, chunks ascending); a depth <= 0 or a
//     value that is not finite rejects; only a strictly lower finite cost is accepted: lambda <- max(lambda / 10, 1e-10), else
//     lambda <- min(10 lambda, 1e10); a scene ends after max_iterations rounds, on a rejection with lambda at the ceiling, or when an
//     accepted step lowers the cost by less than ba::FTOL relative.
// Only + - * / sqrt, every product and sum rounded once, no floating-point atomics.
//
// Launches per call (workspace: bundle_workspace_bytes): ba_init_kernel (thread = track: masks, fp64 points, per-view counts by integer
// atomics, cost partials), ba_setup_kernel (workgroup = scene: pose state, free views, status), then max_iterations rounds of ba_point_kernel
// (thread = track: V_k*^-1, g_k: 72 B), ba_schur_kernel (workgroup = (view pair v <= w, scene): the Jacobians of the two views recomputed from
// the poses in LDS, 36 or 42 block sums), ba_solve_kernel (workgroup = scene: the packed triangle in LDS, 148 KB at V = 32; candidate poses),
// ba_update_kernel (thread = track: candidate point and cost partials), ba_decide_kernel (scene: accept or reject on the double-buffered
// state), and ba_final_kernel (outputs).  The workgroups of a finished scene return at once; nothing synchronises with the host.

// ---- bundle solver begin (host-compilable: tests/test_bundle_emulated.py slices it out behind the two slices above) ----
namespace ba {
constexpr int MIN_VIEW_OBS = 6;             // fewer observations than the 6 parameters of a pose: the view is held
constexpr int STRIDE = 20;                  // the per-view block: what mv_stage_pose writes (mv_reproj reads mv::ROT, mv::TRA, mv::CAL of it)
constexpr double FTOL = 1e-8;               // noise-free scenes stop moving by more than 9.3e-9 relative once they are down to rounding
constexpr double LAMBDA0 = 1e-3, LAMBDA_MIN = 1e-10, LAMBDA_MAX = 1e10;
constexpr int ST_OK = 0, ST_NOTHING = 1, ST_NOT_FINITE = 2;
}  // namespace ba

// Huber's rho of e^2 at c pixels (c = +inf: e^2) and the weight of the observation
__device__ inline double ba_rho(double e2, double c, double& wt) {
    const double e = sqrt(e2);
    const bool far = e > c;
    wt = far ? c / e : 1.0;
    return far ? (2.0 * c) * e - c * c : e2;
}
// the observation set of a track at the input state (a mask of views; fewer than 2: none)
template <class Obs>
__device__ inline unsigned ba_mask(const double* vd, int nv, const Obs& obs, unsigned inl, const double* X) {
    const bool xfin = tv::is_finite(X[0]) && tv::is_finite(X[1]) && tv::is_finite(X[2]);
    unsigned M = 0u;
    int n = 0;
    for (int w = 0; w < nv; ++w) {
        if (!((inl >> w) & 1u)) continue;
        double u, v, z;
        const bool in = obs(w, u, v);
        const double* p = vd + w * ba::STRIDE;
        if (!(in && tv::is_finite(u) && tv::is_finite(v) && p[mv::OK] != 0.0 && xfin)) continue;
        const double e2 = mv_reproj(p, X, u, v, z);
        if (z > 0.0 && tv::is_finite(e2)) { M |= 1u << w; ++n; }
    }
    return n >= 2 ? M : 0u;
}
// the robust cost of a track over its observations M; bad: an observation with depth <= 0 or a value that is not finite
template <class Obs>
__device__ inline double ba_cost(const double* vd, int nv, const Obs& obs, unsigned M, const double* X, double c, bool& bad) {
    double cost = 0.0;
    bad = false;
    for (int w = 0; w < nv; ++w) {
        if (!((M >> w) & 1u)) continue;
        double u, v, z, wt;
        obs(w, u, v);
        const double e2 = mv_reproj(vd + w * ba::STRIDE, X, u, v, z);
        bad = bad || !(z > 0.0) || !tv::is_finite(e2);
        cost = cost + ba_rho(e2, c, wt);
    }
    return cost;
}
// one observation: residual (du, dv), weight, Jp = d(du, dv)/dX (u row, v row), Jc = d(du, dv)/d(w, d) (u row, v row)
struct BaTerm {
    double du, dv, wt;
    double jp[6], jc[12];
};
__device__ inline void ba_term(const double* p, const double* X, double u, double v, double c, BaTerm& o) {
    double z;
    const double e2 = mv_reproj(p, X, u, v, z);
    ba_rho(e2, c, o.wt);
    const double x = ((p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]) + p[mv::TRA];
    const double y = ((p[3] * X[0] + p[4] * X[1]) + p[5] * X[2]) + p[mv::TRA + 1];
    const double a = x / z, b = y / z;
    o.du = (p[mv::CAL] * a + p[mv::CAL + 2]) - u; o.dv = (p[mv::CAL + 1] * b + p[mv::CAL + 3]) - v;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        o.jp[j] = p[mv::CAL] * ((p[j] - a * p[6 + j]) / z);
        o.jp[3 + j] = p[mv::CAL + 1] * ((p[3 + j] - b * p[6 + j]) / z);
    }
    const double gu0 = p[mv::CAL] / z, gu2 = -((p[mv::CAL] * a) / z), gv1 = p[mv::CAL + 1] / z, gv2 = -((p[mv::CAL + 1] * b) / z);
    // dY/dw_j = R (e_j x X): component i
    const double d20 = p[8] * X[1] - p[7] * X[2], d21 = p[6] * X[2] - p[8] * X[0], d22 = p[7] * X[0] - p[6] * X[1];
    const double d00 = p[2] * X[1] - p[1] * X[2], d01 = p[0] * X[2] - p[2] * X[0], d02 = p[1] * X[0] - p[0] * X[1];
    const double d10 = p[5] * X[1] - p[4] * X[2], d11 = p[3] * X[2] - p[5] * X[0], d12 = p[4] * X[0] - p[3] * X[1];
    o.jc[0] = gu0 * d00 + gu2 * d20; o.jc[1] = gu0 * d01 + gu2 * d21; o.jc[2] = gu0 * d02 + gu2 * d22;
    o.jc[3] = gu0; o.jc[4] = 0.0; o.jc[5] = gu2;
    o.jc[6] = gv1 * d10 + gv2 * d20; o.jc[7] = gv1 * d11 + gv2 * d21; o.jc[8] = gv1 * d12 + gv2 * d22;
    o.jc[9] = 0.0; o.jc[10] = gv1; o.jc[11] = gv2;
}
// V_k*^-1 (00 01 02 11 12 22) and g_k of a track at opl = 1 + lambda; false: the point is held for this step
template <class Obs>
__device__ inline bool ba_point(const double* vd, int nv, const Obs& obs, unsigned M, const double* X, double c, double opl, double* Vi, double* g) {
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    for (int w = 0; w < nv; ++w) {
        if (!((M >> w) & 1u)) continue;
        double u, v;
        obs(w, u, v);
        BaTerm t;
        ba_term(vd + w * ba::STRIDE, X, u, v, c, t);
        A[0] = A[0] + t.wt * (t.jp[0] * t.jp[0] + t.jp[3] * t.jp[3]); A[1] = A[1] + t.wt * (t.jp[0] * t.jp[1] + t.jp[3] * t.jp[4]);
        A[2] = A[2] + t.wt * (t.jp[0] * t.jp[2] + t.jp[3] * t.jp[5]); A[3] = A[3] + t.wt * (t.jp[1] * t.jp[1] + t.jp[4] * t.jp[4]);
        A[4] = A[4] + t.wt * (t.jp[1] * t.jp[2] + t.jp[4] * t.jp[5]); A[5] = A[5] + t.wt * (t.jp[2] * t.jp[2] + t.jp[5] * t.jp[5]);
        s[0] = s[0] + t.wt * (t.jp[0] * t.du + t.jp[3] * t.dv); s[1] = s[1] + t.wt * (t.jp[1] * t.du + t.jp[4] * t.dv);
        s[2] = s[2] + t.wt * (t.jp[2] * t.du + t.jp[5] * t.dv);
    }
    g[0] = -s[0]; g[1] = -s[1]; g[2] = -s[2];
    A[0] = A[0] * opl; A[3] = A[3] * opl; A[5] = A[5] * opl;
    const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
    const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
    const double e0[3] = {-1.0, 0.0, 0.0}, e1[3] = {0.0, -1.0, 0.0}, e2[3] = {0.0, 0.0, -1.0};
    double q0[3], q1[3], q2[3];
    mv_step(A, e0, q0); mv_step(A, e1, q1); mv_step(A, e2, q2);
    Vi[0] = q0[0]; Vi[1] = q0[1]; Vi[2] = q0[2]; Vi[3] = q1[1]; Vi[4] = q1[2]; Vi[5] = q2[2];
    return tv::is_finite(det) && det > 0.0;
}
// W = wt Jc'Jp (6 rows of 3) of an observation, Y = W V^-1
__device__ inline void ba_W(const BaTerm& t, double* W) {
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) W[3 * a + c] = t.wt * (t.jc[a] * t.jp[c] + t.jc[6 + a] * t.jp[3 + c]);
}
__device__ inline void ba_Y(const double* W, const double* Vi, double* Y) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        Y[3 * a] = (W[3 * a] * Vi[0] + W[3 * a + 1] * Vi[1]) + W[3 * a + 2] * Vi[2];
        Y[3 * a + 1] = (W[3 * a] * Vi[1] + W[3 * a + 1] * Vi[3]) + W[3 * a + 2] * Vi[4];
        Y[3 * a + 2] = (W[3 * a] * Vi[2] + W[3 * a + 1] * Vi[4]) + W[3 * a + 2] * Vi[5];
    }
}
// one track's term of block (row view, column view) of the reduced system: acc[6 a + b] (row 6 w + a, column 6 v + b); DIAG (row == column
// view): also acc[36 + a], the right-hand side.  A held point takes no part in the products with V^-1.
template <bool DIAG>
__device__ inline void ba_pair_add(const BaTerm& tr, const BaTerm& tc, const double* Vi, const double* g, bool held, double opl, double* acc) {
    double Wr[18], Wc[18], Y[18];
    ba_W(tr, Wr);
    ba_W(tc, Wc);
    ba_Y(Wr, Vi, Y);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const double s = held ? 0.0 : (Y[3 * a] * Wc[3 * b] + Y[3 * a + 1] * Wc[3 * b + 1]) + Y[3 * a + 2] * Wc[3 * b + 2];
            if (DIAG) {
                const double u = tr.wt * (tr.jc[a] * tr.jc[b] + tr.jc[6 + a] * tr.jc[6 + b]);
                acc[6 * a + b] = acc[6 * a + b] + ((a == b ? u * opl : u) - s);
            } else {
                acc[6 * a + b] = acc[6 * a + b] - s;
            }
        }
        if (DIAG) {
            const double r = -(tr.wt * (tr.jc[a] * tr.du + tr.jc[6 + a] * tr.dv));
            const double yg = held ? 0.0 : (Y[3 * a] * g[0] + Y[3 * a + 1] * g[1]) + Y[3 * a + 2] * g[2];
            acc[36 + a] = acc[36 + a] + (r - yg);
        }
    }
}
// Cholesky of the packed lower triangle L (entry (i, j), j <= i, at i (i + 1) / 2 + j) in place (the diagonal keeps the pivots' squares, piv
// their roots), then r <- the solution of L L' d = r.  Thread tid of nt; sync() is the workgroup's barrier (the host: one thread, nothing).
// false: a pivot that is not > 0 or not finite (the same on every thread).
template <class Sync>
__device__ inline bool ba_cholesky_solve(double* L, double* r, double* piv, int n, int tid, int nt, const Sync& sync) {
    sync();
    for (int j = 0; j < n; ++j) {
        const double* rj = L + (size_t)j * (j + 1) / 2;
        for (int i = j + tid; i < n; i += nt) {
            double* ri = L + (size_t)i * (i + 1) / 2;
            double v = ri[j];
            for (int q = 0; q < j; ++q) v = v - ri[q] * rj[q];
            ri[j] = v;
        }
        sync();
        const double d = rj[j];
        if (!(d > 0.0) || !tv::is_finite(d)) return false;
        const double pj = sqrt(d);
        if (tid == 0) piv[j] = pj;
        for (int i = j + 1 + tid; i < n; i += nt) {
            double* ri = L + (size_t)i * (i + 1) / 2;
            ri[j] = ri[j] / pj;
        }
        sync();
    }
    for (int q = 0; q < n; ++q) {                           // forward: every row's subtractions in ascending q
        if (tid == 0) r[q] = r[q] / piv[q];
        sync();
        const double yq = r[q];
        for (int i = q + 1 + tid; i < n; i += nt) r[i] = r[i] - L[(size_t)i * (i + 1) / 2 + q] * yq;
        sync();
    }
    for (int q = n - 1; q >= 0; --q) {                      // back: every row's subtractions in descending q
        if (tid == 0) r[q] = r[q] / piv[q];
        sync();
        const double dq = r[q];
        const double* rq = L + (size_t)q * (q + 1) / 2;
        for (int i = tid; i < q; i += nt) r[i] = r[i] - rq[i] * dq;
        sync();
    }
    return true;
}
// R cay(w), t + d of d6 = (w, d) (the update inside k_abspose.hip's ap_gn_update, restated)
__device__ inline void ba_pose_update(const double* R, const double* t, const double* d6, double* Rn, double* tn) {
    const double w0 = d6[0], w1 = d6[1], w2 = d6[2];
    const double n2 = (w0 * w0 + w1 * w1) + w2 * w2;
    const double f = 1.0 / (1.0 + 0.25 * n2);
    const double w[3] = {w0, w1, w2};
    const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double Cm[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double ww = w[i] * w[j] - (i == j ? n2 : 0.0);
            Cm[3 * i + j] = (i == j ? 1.0 : 0.0) + f * (W[3 * i + j] + 0.5 * ww);
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (R[3 * i] * Cm[j] + R[3 * i + 1] * Cm[3 + j]) + R[3 * i + 2] * Cm[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) tn[i] = t[i] + d6[3 + i];
}
// the candidate point of a track: X + V^-1 (g - sum_w W_wk' d_w) over its observations in the free views, ascending w; held: X
template <class Obs>
__device__ inline void ba_point_step(const double* vd, int nv, const Obs& obs, unsigned M, unsigned free_views, const double* X, double c,
                                     const double* Vi, const double* g, bool held, const double* dcam, double* Xn) {
    double q0 = g[0], q1 = g[1], q2 = g[2];
    for (int w = 0; w < nv; ++w) {
        if (!(((M & free_views) >> w) & 1u)) continue;
        double u, v, W[18];
        obs(w, u, v);
        BaTerm t;
        ba_term(vd + w * ba::STRIDE, X, u, v, c, t);
        ba_W(t, W);
        const double* d = dcam + 6 * w;
        q0 = q0 - (((((W[0] * d[0] + W[3] * d[1]) + W[6] * d[2]) + W[9] * d[3]) + W[12] * d[4]) + W[15] * d[5]);
        q1 = q1 - (((((W[1] * d[0] + W[4] * d[1]) + W[7] * d[2]) + W[10] * d[3]) + W[13] * d[4]) + W[16] * d[5]);
        q2 = q2 - (((((W[2] * d[0] + W[5] * d[1]) + W[8] * d[2]) + W[11] * d[3]) + W[14] * d[4]) + W[17] * d[5]);
    }
    const double dx = (Vi[0] * q0 + Vi[1] * q1) + Vi[2] * q2, dy = (Vi[1] * q0 + Vi[3] * q1) + Vi[4] * q2, dz = (Vi[2] * q0 + Vi[4] * q1) + Vi[5] * q2;
    Xn[0] = held ? X[0] : X[0] + dx; Xn[1] = held ? X[1] : X[1] + dy; Xn[2] = held ? X[2] : X[2] + dz;
}
// the decision of a round: the state words lambda, cost; returns accepted; done: the scene has ended
__device__ inline bool ba_decide(bool failed, double cand, double& lambda, double& cost, bool& done) {
    const bool accept = !failed && tv::is_finite(cand) && cand < cost;
    if (accept) {
        done = cost - cand < ba::FTOL * cost;
        cost = cand;
        const double l = lambda / 10.0;
        lambda = l > ba::LAMBDA_MIN ? l : ba::LAMBDA_MIN;
    } else {
        done = lambda >= ba::LAMBDA_MAX;
        const double l = 10.0 * lambda;
        lambda = l < ba::LAMBDA_MAX ? l : ba::LAMBDA_MAX;
    }
    return accept;
}
// ---- bundle solver end ----

struct BaCtrl {               // per scene
    double lambda, cost, cost0;
    int32_t cur, done, iters, accepted, status, free_views, failed, bad, n_refined, n_obs;
};
struct BaArgs {
    const float* kpts;        // (S, V, kcap, 2)
    const int32_t* tracks;    // (S, K, V)
    const int32_t* inliers;   // (S, K)
    const float* X0;          // (S, K, 3)
    const int32_t* n_views;   // (S,) or NULL
    const double* Ks;         // (S, V, 3, 3)
    const double* Rs;
    const double* ts;
    int S, K, V, kcap, nch;
    unsigned fixed;
    double huber;
    // workspace
    BaCtrl* ctrl;             // (S,)
    int32_t* counts;          // (S, 32) observations per view
    double* pose;             // (S, 2, V, 12)
    double* X;                // (S, 2, K, 3)
    uint32_t* mask;           // (S, K)
    unsigned char* held;      // (S, K)
    double* pv;               // (S, K, 9): V*^-1 (6), g (3)
    double* sys;              // (S, n (n + 1) / 2 + n), n = 6 V: the packed triangle, then the right-hand side
    double* dcam;             // (S, n)
    double* partial;          // (S, nch)
    // outputs
    double* Rout;
    double* tout;
    float* Xout;
    unsigned char* refined;
    int32_t* free_out;
    double* cost_out;         // (S, 2)
    int32_t* info;            // (S, 8)
};

__device__ inline int ba_nv(const BaArgs& a, int s) {
    int nv = a.n_views ? a.n_views[s] : a.V;
    return nv < 0 ? 0 : (nv > a.V ? a.V : nv);
}
__device__ inline MvObs ba_obs(const BaArgs& a, size_t o, int s) {
    MvObs obs;
    obs.row = a.tracks + o * a.V; obs.kp = a.kpts + (size_t)s * a.V * a.kcap * 2; obs.kcap = (unsigned)a.kcap;
    return obs;
}
// the view blocks of scene s from buffer `which` of the pose state into LDS
__device__ inline void ba_stage_state(const BaArgs& a, int s, int which, double* vd) {
    const int tid = threadIdx.x;
    if (tid < a.V) {
        const double* p = a.pose + (((size_t)s * 2 + which) * a.V + tid) * 12;
        mv_stage_pose(p, p + 9, a.Ks + ((size_t)s * a.V + tid) * 9, vd + tid * ba::STRIDE);
    }
}

__global__ __launch_bounds__(256) void ba_init_kernel(BaArgs a) {
    __shared__ double vd[mv::MAX_VIEWS * ba::STRIDE];
    __shared__ double red[rs::block_sums_bytes(1) / sizeof(double)];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int k = blockIdx.x * 256 + tid;
    const int nv = ba_nv(a, s);
    if (tid < a.V) {
        const size_t v = (size_t)s * a.V + tid;
        mv_stage_pose(a.Rs + v * 9, a.ts + v * 3, a.Ks + v * 9, vd + tid * ba::STRIDE);
    }
    __syncthreads();
    unsigned M = 0u;
    double cost[1] = {0.0};
    if (k < a.K) {
        const size_t o = (size_t)s * a.K + k;
        const double X[3] = {(double)a.X0[3 * o], (double)a.X0[3 * o + 1], (double)a.X0[3 * o + 2]};
        const MvObs obs = ba_obs(a, o, s);
        M = ba_mask(vd, nv, obs, (unsigned)a.inliers[o], X);
        bool bad;
        if (M) cost[0] = ba_cost(vd, nv, obs, M, X, a.huber, bad);
        double* Xs = a.X + ((size_t)s * 2 * a.K + k) * 3;
        Xs[0] = X[0]; Xs[1] = X[1]; Xs[2] = X[2];
        a.mask[o] = M;
    }
    const bool lead = (tid & 63) == 0;
    int nobs = 0;
    for (int w = 0; w < a.V; ++w) {
        const unsigned long long m = __ballot((M >> w) & 1u);
        if (lead && m) { atomicAdd(a.counts + (size_t)s * 32 + w, (int)__popcll(m)); nobs += (int)__popcll(m); }
    }
    const unsigned long long m = __ballot(M != 0u);
    if (lead && m) atomicAdd(&a.ctrl[s].n_refined, (int)__popcll(m));
    if (lead && nobs) atomicAdd(&a.ctrl[s].n_obs, nobs);
    rs::block_sums(cost, red);
    if (tid == 0) a.partial[(size_t)s * a.nch + blockIdx.x] = cost[0];
}

// (the workspace's control words and counts were zeroed before ba_init_kernel)
__global__ __launch_bounds__(64) void ba_setup_kernel(BaArgs a) {
    const int s = blockIdx.x, tid = threadIdx.x;
    if (tid < a.V) {
        const size_t v = (size_t)s * a.V + tid;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            double* p = a.pose + (((size_t)s * 2 + b) * a.V + tid) * 12;
#pragma unroll
            for (int k = 0; k < 9; ++k) p[k] = a.Rs[v * 9 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[9 + k] = a.ts[v * 3 + k];
        }
    }
    if (tid == 0) {
        BaCtrl& c = a.ctrl[s];
        unsigned fr = 0u;
        for (int v = 0; v < a.V; ++v)
            if (!((a.fixed >> v) & 1u) && a.counts[(size_t)s * 32 + v] >= ba::MIN_VIEW_OBS) fr |= 1u << v;
        double cost = 0.0;
        for (int j = 0; j < a.nch; ++j) cost = cost + a.partial[(size_t)s * a.nch + j];
        c.free_views = (int32_t)fr;
        c.cost0 = cost; c.cost = cost; c.lambda = ba::LAMBDA0;
        c.status = (fr == 0u || c.n_refined == 0) ? ba::ST_NOTHING : (tv::is_finite(cost) ? ba::ST_OK : ba::ST_NOT_FINITE);
        c.done = c.status != ba::ST_OK;
    }
}

__global__ __launch_bounds__(256) void ba_point_kernel(BaArgs a) {
    __shared__ double vd[mv::MAX_VIEWS * ba::STRIDE];
    const int s = blockIdx.y, tid = threadIdx.x;
    const BaCtrl c = a.ctrl[s];
    if (c.done) return;
    ba_stage_state(a, s, c.cur, vd);
    __syncthreads();
    const int k = blockIdx.x * 256 + tid;
    if (k >= a.K) return;
    const size_t o = (size_t)s * a.K + k;
    const unsigned M = a.mask[o];
    if (!M) return;
    const double* Xs = a.X + (((size_t)s * 2 + c.cur) * a.K + k) * 3;
    const double X[3] = {Xs[0], Xs[1], Xs[2]};
    double Vi[6], g[3];
    const bool ok = ba_point(vd, ba_nv(a, s), ba_obs(a, o, s), M, X, a.huber, 1.0 + c.lambda, Vi, g);
    double* pv = a.pv + o * 9;
#pragma unroll
    for (int j = 0; j < 6; ++j) pv[j] = Vi[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) pv[6 + j] = g[j];
    a.held[o] = ok ? 0 : 1;
}

// the term of track k in block (w, v): the pixel of a view through the table, as MvObs
template <bool DIAG>
__device__ inline void ba_schur_block(const BaArgs& a, int s, int v, int w, const BaCtrl& c, const double* pvw /* LDS: blocks of v and w */, double* red,
                                      double* out, double* rhs) {
    constexpr int N = DIAG ? 42 : 36;
    const int tid = threadIdx.x;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    const double opl = 1.0 + c.lambda;
    const unsigned need = (1u << v) | (1u << w);
    const float* kp = a.kpts + (size_t)s * a.V * a.kcap * 2;
    for (int k = tid; k < a.K; k += 256) {
        const size_t o = (size_t)s * a.K + k;
        if ((a.mask[o] & need) != need) continue;
        const double* Xs = a.X + (((size_t)s * 2 + c.cur) * a.K + k) * 3;
        const double X[3] = {Xs[0], Xs[1], Xs[2]};
        const int32_t* row = a.tracks + o * a.V;
        const float2 qv = *reinterpret_cast<const float2*>(kp + ((size_t)v * a.kcap + (unsigned)row[v]) * 2);
        const double* pv = a.pv + o * 9;
        const double Vi[6] = {pv[0], pv[1], pv[2], pv[3], pv[4], pv[5]}, g[3] = {pv[6], pv[7], pv[8]};
        const bool held = a.held[o] != 0;
        BaTerm tc;
        ba_term(pvw, X, (double)qv.x, (double)qv.y, a.huber, tc);
        if (DIAG) {
            ba_pair_add<true>(tc, tc, Vi, g, held, opl, acc);
        } else {
            const float2 qw = *reinterpret_cast<const float2*>(kp + ((size_t)w * a.kcap + (unsigned)row[w]) * 2);
            BaTerm tr;
            ba_term(pvw + ba::STRIDE, X, (double)qw.x, (double)qw.y, a.huber, tr);
            ba_pair_add<false>(tr, tc, Vi, g, held, opl, acc);
        }
    }
    rs::block_sums(acc, red);
    // entry (6 w + i, 6 v + j) of the packed triangle (the diagonal block: j <= i)
#pragma unroll
    for (int e = 0; e < 36; ++e) {
        const int i = e / 6, j = e % 6;
        if (tid == e && (!DIAG || j <= i)) out[(size_t)(6 * w + i) * (6 * w + i + 1) / 2 + 6 * v + j] = acc[e];
    }
    if (DIAG) {
#pragma unroll
        for (int e = 0; e < 6; ++e)
            if (tid == 36 + e) rhs[6 * v + e] = acc[36 + e];
    }
}

__global__ __launch_bounds__(256) void ba_schur_kernel(BaArgs a) {
    __shared__ double pvw[2 * ba::STRIDE];
    __shared__ double red[rs::block_sums_bytes(42) / sizeof(double)];
    const int s = blockIdx.y, tid = threadIdx.x;
    const BaCtrl c = a.ctrl[s];
    if (c.done) return;
    int w = 0, rest = blockIdx.x;                          // pair index = w (w + 1) / 2 + v, v <= w
    while (rest > w) { rest -= w + 1; ++w; }
    const int v = rest;
    const int n = 6 * a.V;
    double* out = a.sys + (size_t)s * ((size_t)n * (n + 1) / 2 + n);
    double* rhs = out + (size_t)n * (n + 1) / 2;
    const unsigned fr = (unsigned)c.free_views;
    if (!((fr >> v) & 1u) || !((fr >> w) & 1u)) {          // a held view: its rows are identity and zero
        if (tid < 36) {
            const int i = tid / 6, j = tid % 6;
            if (v != w || j <= i) out[(size_t)(6 * w + i) * (6 * w + i + 1) / 2 + 6 * v + j] = (v == w && i == j) ? 1.0 : 0.0;
        } else if (tid < 42 && v == w) {
            rhs[6 * v + (tid - 36)] = 0.0;
        }
        return;
    }
    if (tid < 2) {
        const int x = tid == 0 ? v : w;
        const double* p = a.pose + (((size_t)s * 2 + c.cur) * a.V + x) * 12;
        mv_stage_pose(p, p + 9, a.Ks + ((size_t)s * a.V + x) * 9, pvw + tid * ba::STRIDE);
    }
    __syncthreads();
    if (v == w) ba_schur_block<true>(a, s, v, w, c, pvw, red, out, rhs);
    else ba_schur_block<false>(a, s, v, w, c, pvw, red, out, rhs);
}

struct BaBarrier {
    __device__ inline void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(256) void ba_solve_kernel(BaArgs a) {
    extern __shared__ double lds[];                        // the packed triangle, the right-hand side, the pivots
    const int s = blockIdx.x, tid = threadIdx.x;
    const BaCtrl c = a.ctrl[s];
    if (c.done) return;
    const int n = 6 * a.V;
    const size_t tri = (size_t)n * (n + 1) / 2;
    double* L = lds;
    double* r = lds + tri;
    double* piv = r + n;
    const double* src = a.sys + (size_t)s * (tri + n);
    for (size_t i = tid; i < tri + n; i += 256) lds[i] = src[i];
    const bool ok = ba_cholesky_solve(L, r, piv, n, tid, 256, BaBarrier());
    if (!ok) {
        if (tid == 0) a.ctrl[s].failed = 1;
        return;
    }
    if (tid < n) a.dcam[(size_t)s * n + tid] = r[tid];
    if (tid < a.V) {
        const double* p = a.pose + (((size_t)s * 2 + c.cur) * a.V + tid) * 12;
        double* q = a.pose + (((size_t)s * 2 + (1 - c.cur)) * a.V + tid) * 12;
        double R[9], t[3], d6[6], Rn[9], tn[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = p[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = p[9 + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) d6[k] = r[6 * tid + k];
        ba_pose_update(R, t, d6, Rn, tn);
        const bool fr = ((unsigned)c.free_views >> tid) & 1u;
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = fr ? Rn[k] : R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[9 + k] = fr ? tn[k] : t[k];
    }
}

__global__ __launch_bounds__(256) void ba_update_kernel(BaArgs a) {
    __shared__ double vd[mv::MAX_VIEWS * ba::STRIDE];      // the current poses
    __shared__ double vc[mv::MAX_VIEWS * ba::STRIDE];      // the candidate poses
    __shared__ double dc[6 * mv::MAX_VIEWS];
    __shared__ double red[rs::block_sums_bytes(1) / sizeof(double)];
    const int s = blockIdx.y, tid = threadIdx.x;
    const BaCtrl c = a.ctrl[s];
    if (c.done || c.failed) return;
    const int n = 6 * a.V;
    ba_stage_state(a, s, c.cur, vd);
    ba_stage_state(a, s, 1 - c.cur, vc);
    if (tid < n) dc[tid] = a.dcam[(size_t)s * n + tid];
    __syncthreads();
    const int k = blockIdx.x * 256 + tid;
    double cost[1] = {0.0};
    bool bad = false;
    if (k < a.K) {
        const size_t o = (size_t)s * a.K + k;
        const unsigned M = a.mask[o];
        if (M) {
            const double* Xs = a.X + (((size_t)s * 2 + c.cur) * a.K + k) * 3;
            double* Xc = a.X + (((size_t)s * 2 + (1 - c.cur)) * a.K + k) * 3;
            const double X[3] = {Xs[0], Xs[1], Xs[2]};
            const double* pv = a.pv + o * 9;
            const double Vi[6] = {pv[0], pv[1], pv[2], pv[3], pv[4], pv[5]}, g[3] = {pv[6], pv[7], pv[8]};
            const MvObs obs = ba_obs(a, o, s);
            const int nv = ba_nv(a, s);
            double Xn[3];
            ba_point_step(vd, nv, obs, M, (unsigned)c.free_views, X, a.huber, Vi, g, a.held[o] != 0, dc, Xn);
            Xc[0] = Xn[0]; Xc[1] = Xn[1]; Xc[2] = Xn[2];
            cost[0] = ba_cost(vc, nv, obs, M, Xn, a.huber, bad);
        }
    }
    const unsigned long long m = __ballot(bad);
    if ((tid & 63) == 0 && m) atomicOr(&a.ctrl[s].bad, 1);
    rs::block_sums(cost, red);
    if (tid == 0) a.partial[(size_t)s * a.nch + blockIdx.x] = cost[0];
}

__global__ __launch_bounds__(64) void ba_decide_kernel(BaArgs a) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.S) return;
    BaCtrl& c = a.ctrl[s];
    if (c.done) return;
    const bool failed = c.failed != 0 || c.bad != 0;
    double cand = 0.0;
    if (!failed)
        for (int j = 0; j < a.nch; ++j) cand = cand + a.partial[(size_t)s * a.nch + j];
    double lambda = c.lambda, cost = c.cost;
    bool done;
    const bool accept = ba_decide(failed, cand, lambda, cost, done);
    c.lambda = lambda; c.cost = cost;
    c.iters += 1;
    if (accept) { c.accepted += 1; c.cur = 1 - c.cur; }
    c.done = done ? 1 : 0;
    c.failed = 0; c.bad = 0;
}

__global__ __launch_bounds__(256) void ba_final_kernel(BaArgs a) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const BaCtrl c = a.ctrl[s];
    const int k = blockIdx.x * 256 + tid;
    const bool ran = c.status == ba::ST_OK;
    if (k < a.K) {
        const size_t o = (size_t)s * a.K + k;
        const bool ref = ran && a.mask[o] != 0u;
        const double* Xs = a.X + (((size_t)s * 2 + c.cur) * a.K + k) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float x = ref ? (float)Xs[j] : a.X0[3 * o + j];
            a.Xout[3 * o + j] = x;
        }
        a.refined[o] = ref ? 1 : 0;
    }
    if (blockIdx.x != 0) return;
    if (tid < a.V) {
        const size_t v = (size_t)s * a.V + tid;
        const double* p = a.pose + (((size_t)s * 2 + c.cur) * a.V + tid) * 12;
#pragma unroll
        for (int j = 0; j < 9; ++j) a.Rout[v * 9 + j] = p[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) a.tout[v * 3 + j] = p[9 + j];
    }
    if (tid == 0) {
        a.free_out[s] = c.free_views;
        a.cost_out[2 * s] = c.cost0; a.cost_out[2 * s + 1] = c.cost;
        int nf = 0;
        for (int v = 0; v < a.V; ++v) nf += (c.free_views >> v) & 1;
        int32_t* info = a.info + (size_t)s * 8;
        info[0] = ran ? c.n_refined : 0; info[1] = c.n_obs; info[2] = nf; info[3] = c.iters; info[4] = c.accepted; info[5] = c.status;
        info[6] = 0; info[7] = 0;
    }
}

static size_t ba_align(size_t x) { return (x + 255) & ~(size_t)255; }
// the workspace's parts in order: ctrl, counts, pose, X, mask, held, pv, sys, dcam, partial
static size_t ba_layout(int S, int K, int V, size_t* off) {
    const size_t n = 6 * (size_t)V, nch = (size_t)ceil_div(K, 256);
    const size_t sz[10] = {(size_t)S * sizeof(BaCtrl), (size_t)S * 32 * 4, (size_t)S * 2 * V * 12 * 8, (size_t)S * 2 * K * 3 * 8, (size_t)S * K * 4,
                           (size_t)S * K, (size_t)S * K * 9 * 8, (size_t)S * (n * (n + 1) / 2 + n) * 8, (size_t)S * n * 8, (size_t)S * nch * 8};
    size_t at = 0;
    for (int i = 0; i < 10; ++i) { if (off) off[i] = at; at += ba_align(sz[i]); }
    return at;
}
size_t bundle_workspace_bytes(int S, int K, int V) { return ba_layout(S, K, V, nullptr); }

int launch_bundle_adjust(const float* kpts, int kcap, const int32_t* tracks, const int32_t* inlier_views, const float* points3d, const int32_t* n_views,
                         int S, int K, int V, const double* Ks, const double* Rs, const double* ts, unsigned fixed_views, int max_iterations,
                         double huber_px, double* Rs_out, double* ts_out, float* points3d_out, unsigned char* refined, int32_t* free_views, double* cost,
                         int32_t* info, void* ws, hipStream_t st) {
    if (S < 1 || S > 65535 || K < 1 || V < 2 || V > mv::MAX_VIEWS || kcap < 1 || max_iterations < 0) return -1;
    size_t off[10];
    ba_layout(S, K, V, off);
    char* w = static_cast<char*>(ws);
    BaArgs a = {};
    a.kpts = kpts; a.tracks = tracks; a.inliers = inlier_views; a.X0 = points3d; a.n_views = n_views; a.Ks = Ks; a.Rs = Rs; a.ts = ts;
    a.S = S; a.K = K; a.V = V; a.kcap = kcap; a.nch = ceil_div(K, 256); a.fixed = fixed_views; a.huber = huber_px;
    a.ctrl = reinterpret_cast<BaCtrl*>(w + off[0]); a.counts = reinterpret_cast<int32_t*>(w + off[1]); a.pose = reinterpret_cast<double*>(w + off[2]);
    a.X = reinterpret_cast<double*>(w + off[3]); a.mask = reinterpret_cast<uint32_t*>(w + off[4]); a.held = reinterpret_cast<unsigned char*>(w + off[5]);
    a.pv = reinterpret_cast<double*>(w + off[6]); a.sys = reinterpret_cast<double*>(w + off[7]); a.dcam = reinterpret_cast<double*>(w + off[8]);
    a.partial = reinterpret_cast<double*>(w + off[9]);
    a.Rout = Rs_out; a.tout = ts_out; a.Xout = points3d_out; a.refined = refined; a.free_out = free_views; a.cost_out = cost; a.info = info;
    if (hipMemsetAsync(w, 0, off[2], st) != hipSuccess) return -1;                // the control words and the counts
    const int n = 6 * V;
    const int lds = (int)(((size_t)n * (n + 1) / 2 + 2 * (size_t)n) * sizeof(double));
    static AttrMask attr_done{0};
    set_max_dynamic_lds(reinterpret_cast<const void*>(ba_solve_kernel), 160 * 1024, attr_done);
    const dim3 per_track(a.nch, S);
    ba_init_kernel<<<per_track, 256, 0, st>>>(a);
    ba_setup_kernel<<<S, 64, 0, st>>>(a);
    for (int it = 0; it < max_iterations; ++it) {
        ba_point_kernel<<<per_track, 256, 0, st>>>(a);
        ba_schur_kernel<<<dim3(V * (V + 1) / 2, S), 256, 0, st>>>(a);
        ba_solve_kernel<<<S, 256, lds, st>>>(a);
        ba_update_kernel<<<per_track, 256, 0, st>>>(a);
        ba_decide_kernel<<<ceil_div(S, 64), 64, 0, st>>>(a);
    }
    ba_final_kernel<<<per_track, 256, 0, st>>>(a);
    return 0;
}

// ================================================================================================================================================
// Pose-graph initialisation: the world -> camera poses of the V <= 32 views of a scene from the relative poses of P pairs of views (DESIGN.md
// 3.19; tests/posegraph_reference.py restates it operation for operation and tests/test_posegraph_emulated.py compiles the slice below, behind
// the three slices above, on the host and holds it to that restatement bit for bit).  Edge p = (a, b) carries R_rel, t_rel with
// x_b = R_rel x_a + t_rel (R_rel = R_b R_a', t_rel parallel to R_b (c_a - c_b), c_v = -R_v' t_v) and a weight.  Gauge R_0 = I, c_0 = 0.
//   * an edge is valid when a != b, both views are in [0, n_views), the weight is finite and > 0 and R_rel is finite; a valid edge has a
//     direction when t_rel is finite and n2 = (t0 t0 + t1 t1) + t2 t2 is finite and > 0;
//   * spanning tree: view 0 is reached; repeat: of the valid edges with exactly one reached endpoint the largest weight, ties to the lowest
//     pair index; the new view's rotation is R_b = R_rel R_a or R_a = R_rel' R_b (every entry (x y + x y) + x y).  Views never reached are
//     unregistered (NaN poses, bit of `registered` clear) and the valid edges between them drop out; the edges left are the active ones.  The
//     unknowns are the registered views but 0, ascending, numbered compactly: n_r views;
//   * rotations, `iterations` rounds on R_v <- R_v cay(delta_v) (ba_pose_update): the residual of an active edge is r = 2 vec(q), q the
//     quaternion of E = R_b' (R_rel R_a) by the branch on the trace and the largest diagonal entry (s = 2 sqrt(.), the component of the branch
//     s / 4, the others a sum or difference of two entries over s), divided by its norm, its sign that of a scalar part >= 0;
//     |r| = sqrt((r0 r0 + r1 r1) + r2 r2).  The factor of round k: Huber's (|r| > c ? c / |r| : 1) for k < iterations - redescend, Cauchy's
//     c c / (c c + |r| |r|) for the later rounds, w_p = weight_p factor.  To first order r' = r + delta_a - delta_b: the round solves the
//     weighted graph Laplacian (packed lower triangle over the unknowns: diagonal + w_p at both ends, entry (a, b) - w_p; right-hand sides
//     - w_p r at a, + w_p r at b, one per coordinate) by ba_cholesky_solve, once per coordinate on a copy of the triangle; a failed
//     factorisation leaves the rotations of the round as they are.  After the last round the residuals and factors are taken once more
//     with the last round's loss: those are the final rotation factors;
//   * positions, the rotations fixed: d_p = R_b' (t_rel / sqrt(n2)) is the direction of c_a - c_b.  Round k: w_p = weight_p factor over the
//     active edges with a direction, factor 1 in round 0 and else from rho = |e - (d.e) d| / |e| (d.e > 0, else 1) of e = c_a - c_b at the
//     positions of the round before, with c = pos_scale_sin and the losses as above.  M: 3x3 blocks + w_p (I - d d') on the diagonal of both
//     ends and - w_p (I - d d') between them (entry (x, y): w_p ((x == y) - d_x d_y)); g: + w_p d at a, - w_p d at b; view 0 is left out:
//     n = 3 n_r.  mu = tr(M) / (g.g), both summed in ascending index; A = M + (mu g_i) g_j; solve A c = g by ba_cholesky_solve.  The
//     rigidity test: the smallest pivot^2 / (the entry of A's diagonal before the factorisation) must be >= min_pivot_ratio.  The scale:
//     c <- c / s, s = sum_p w_p d_p.(c_a - c_b) / sum_p w_p.  A failed factorisation or test, mu or s not finite or not > 0: the scene's
//     status is ROTATIONS_ONLY, the positions of every view but 0 NaN, the position factors 0.  After the last round the residuals and
//     factors once more (the final position factors), then t_v = -(R_v c_v);
//   * sums: every entry of a matrix or vector adds its edges in ascending pair index; every sum over edges is taken in rs::block_sums'
//     order (pg_sum: slot i of 256 adds the edges i, i + 256, ..., 8 segments of 32 slots in order, the tree over the 8);
//   * info: valid edges, registered views, valid edges with a direction, active edges with a final rotation factor < 0.5, position edges
//     with a final position factor < 0.5, n = 3 n_r, status, 0.  Status: NOTHING (no valid edge at view 0: R_0 = I, t_0 = 0, the rest NaN),
//     else NOT_FINITE (an output of a registered view is not finite), else ROTATIONS_ONLY, else OK.
// Only + - * / sqrt, every product and sum rounded once, no floating-point atomics: two calls give the same bits.
//
// One launch per call: pose_graph_kernel, one workgroup of 256 per scene, runs the tree and all the rounds without leaving.  LDS: the packed
// 93 x 93 triangle with its right-hand side, pivots and diagonal (36.3 KB; the rotation rounds keep their 31 x 31 systems in its front),
// the rotations and centres (3 KB), the sums' and the tree's selection buffers.  Per-edge keys, weights, residuals, directions and the
// sums' terms live in the workspace (pose_graph_workspace_bytes).

// pg_run is pg_run_with(PgEdgesOnly): the position rounds call the hooks of a Terms argument (prepare, weights, assemble, finish), empty here; the
// baseline ratios of posescale_body.hpp are the other Terms.
// ---- pose graph begin (host-compilable: tests/test_posegraph_emulated.py slices it out behind the three slices above) ----
namespace pg {
constexpr int ST_OK = 0, ST_NOTHING = 1, ST_ROTATIONS_ONLY = 2, ST_NOT_FINITE = 3;
constexpr int MAXU = mv::MAX_VIEWS - 1, NPOS = 3 * MAXU, TRI = NPOS * (NPOS + 1) / 2;
// the scene's fp64 LDS: the position system, then the state
constexpr int L_SYS = 0, L_RHS = TRI, L_PIV = L_RHS + NPOS, L_DIAG = L_PIV + NPOS, L_ROT = L_DIAG + NPOS, L_CEN = L_ROT + 9 * mv::MAX_VIEWS;
constexpr int L_RED = L_CEN + 3 * mv::MAX_VIEWS, L_BW = L_RED + 264, L_SC = L_BW + 256, L_END = L_SC + 8;
// the rotation rounds inside L_SYS: the triangle, its working copy, three right-hand sides of 32, the pivots
constexpr int R_TRI = 0, R_WORK = 512, R_RHS = 1024, R_PIV = 1120;
// the scene's int LDS: the tree's selection, compact index of a view (-1: none), view of a compact index, the tree's edges, words
constexpr int I_BP = 0, I_IDX = 256, I_VIEW = 288, I_TREE = 320, I_REG = 352, I_NR = 353, I_END = 360;
constexpr int K_DIR = 1 << 16, K_ACTIVE = 1 << 17;          // key of a valid edge: a | b << 8 | flags; -1: not valid
constexpr int HUBER = 0, CAUCHY = 1;
}  // namespace pg

struct PgScene {
    const int32_t* pairs;     // (P, 2)
    const double* Rrel;       // (P, 9)
    const double* trel;       // (P, 3)
    const double* weight;     // (P,)
    int nv, P, V, iterations, redescend;
    double crot, cpos, min_ratio;
    double* Rs;               // (V, 9)
    double* ts;               // (V, 3)
    int32_t* registered;      // (1,)
    double* factor;           // (P, 2)
    int32_t* info;            // (8,)
    int32_t* key;             // workspace (P,)
    double* wcur;             // (P,)
    double* res;              // (P, 3)
    double* dir;              // (P, 3)
    double* ta;               // (P,)
    double* tb;               // (P,)
    double* lds;              // pg::L_END
    int* ldi;                 // pg::I_END
};

// the total of x[0 .. P) in rs::block_sums' order, on every thread
template <class Sync>
__device__ inline double pg_sum(const double* x, int P, double* red, int tid, int nt, const Sync& sync) {
    sync();
    for (int i = tid; i < 256; i += nt) {
        double t = 0.0;
        for (int p = i; p < P; p += 256) t = t + x[p];
        red[i] = t;
    }
    sync();
    for (int j = tid; j < 8; j += nt) {
        double t = 0.0;
        for (int i = 0; i < 32; ++i) t = t + red[32 * j + i];
        red[256 + j] = t;
    }
    sync();
    const double* q = red + 256;
    return (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7])));
}
__device__ inline double pg_factor(double x, double c, int kind) {
    if (kind == pg::CAUCHY) return (c * c) / (c * c + x * x);
    return x > c ? c / x : 1.0;
}
__device__ inline int pg_kind(const PgScene& s, int k) { return k < s.iterations - s.redescend ? pg::HUBER : pg::CAUCHY; }
// C = A B, or A' B with TA
template <bool TA>
__device__ inline void pg_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = TA ? (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j] : (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
// the key of edge p: valid, views, direction
__device__ inline int pg_edge_key(const int32_t* pairs, const double* Rrel, const double* trel, const double* weight, int nv, int p) {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const double w = weight[p];
    bool ok = a != b && a >= 0 && a < nv && b >= 0 && b < nv && tv::is_finite(w) && w > 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && tv::is_finite(Rrel[(size_t)9 * p + k]);
    const double t0 = trel[(size_t)3 * p], t1 = trel[(size_t)3 * p + 1], t2 = trel[(size_t)3 * p + 2];
    const double n2 = (t0 * t0 + t1 * t1) + t2 * t2;
    const bool dir = tv::is_finite(t0) && tv::is_finite(t1) && tv::is_finite(t2) && tv::is_finite(n2) && n2 > 0.0;
    return ok ? (a | (b << 8) | (dir ? pg::K_DIR : 0)) : -1;
}
// the keys of the edges
template <class Sync>
__device__ inline void pg_keys(const PgScene& s, int tid, int nt, const Sync& sync) {
    for (int p = tid; p < s.P; p += nt) s.key[p] = pg_edge_key(s.pairs, s.Rrel, s.trel, s.weight, s.nv, p);
    sync();
}
// the spanning tree: rotations of the reached views in LDS, the mask, the compact numbering; marks the active edges
template <class Sync>
__device__ inline void pg_tree(const PgScene& s, int tid, int nt, const Sync& sync) {
    double* rot = s.lds + pg::L_ROT;
    double* bw = s.lds + pg::L_BW;
    int* bp = s.ldi + pg::I_BP;
    for (int i = tid; i < 9 * mv::MAX_VIEWS; i += nt) rot[i] = (i % 9) % 4 == 0 ? 1.0 : 0.0;
    for (int i = tid; i < 3 * mv::MAX_VIEWS; i += nt) s.lds[pg::L_CEN + i] = 0.0;
    for (int i = tid; i < 32; i += nt) s.ldi[pg::I_TREE + i] = -1;
    if (tid == 0) s.ldi[pg::I_REG] = 1;
    sync();
    for (int step = 0; step + 1 < s.nv; ++step) {
        const unsigned reg = (unsigned)s.ldi[pg::I_REG];
        for (int i = tid; i < 256; i += nt) {
            double w = -1.0;
            int at = -1;
            for (int p = i; p < s.P; p += 256) {
                const int k = s.key[p];
                if (k < 0) continue;
                if (((reg >> (k & 255)) & 1u) == ((reg >> ((k >> 8) & 255)) & 1u)) continue;
                const double wp = s.weight[p];
                if (wp > w) { w = wp; at = p; }
            }
            bw[i] = w; bp[i] = at;
        }
        sync();
        for (int h = 128; h > 0; h >>= 1) {
            for (int i = tid; i < h; i += nt) {
                const double w0 = bw[i], w1 = bw[i + h];
                const int p0 = bp[i], p1 = bp[i + h];
                const bool second = p1 >= 0 && (p0 < 0 || w1 > w0 || (w1 == w0 && p1 < p0));
                if (second) { bw[i] = w1; bp[i] = p1; }
            }
            sync();
        }
        const int p = bp[0];
        if (p < 0) break;
        if (tid == 0) {
            const int k = s.key[p], a = k & 255, b = (k >> 8) & 255;
            double Rr[9], Rn[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) Rr[j] = s.Rrel[(size_t)9 * p + j];
            if ((reg >> a) & 1u) {
                pg_mul<false>(Rr, rot + 9 * a, Rn);
#pragma unroll
                for (int j = 0; j < 9; ++j) rot[9 * b + j] = Rn[j];
                s.ldi[pg::I_REG] = (int)(reg | (1u << b));
            } else {
                pg_mul<true>(Rr, rot + 9 * b, Rn);
#pragma unroll
                for (int j = 0; j < 9; ++j) rot[9 * a + j] = Rn[j];
                s.ldi[pg::I_REG] = (int)(reg | (1u << a));
            }
            s.ldi[pg::I_TREE + step] = p;
        }
        sync();
    }
    sync();
    const unsigned reg = (unsigned)s.ldi[pg::I_REG];
    if (tid == 0) {
        int n = 0;
        s.ldi[pg::I_IDX] = -1;
        for (int v = 1; v < mv::MAX_VIEWS; ++v) {
            const bool in = (reg >> v) & 1u;
            s.ldi[pg::I_IDX + v] = in ? n : -1;
            if (in) { s.ldi[pg::I_VIEW + n] = v; ++n; }
        }
        s.ldi[pg::I_NR] = n;
    }
    for (int p = tid; p < s.P; p += nt) {
        const int k = s.key[p];
        if (k >= 0 && ((reg >> (k & 255)) & 1u) && ((reg >> ((k >> 8) & 255)) & 1u)) s.key[p] = k | pg::K_ACTIVE;
    }
    sync();
}
// r = 2 vec(q) of E, q of unit norm with a scalar part >= 0
__device__ inline void pg_rot_residual(const double* E, double* r) {
    const double tr = (E[0] + E[4]) + E[8];
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        const double h = sqrt(tr + 1.0) * 2.0;
        qw = 0.25 * h; qx = (E[7] - E[5]) / h; qy = (E[2] - E[6]) / h; qz = (E[3] - E[1]) / h;
    } else if (E[0] > E[4] && E[0] > E[8]) {
        const double h = sqrt(((1.0 + E[0]) - E[4]) - E[8]) * 2.0;
        qw = (E[7] - E[5]) / h; qx = 0.25 * h; qy = (E[1] + E[3]) / h; qz = (E[2] + E[6]) / h;
    } else if (E[4] > E[8]) {
        const double h = sqrt(((1.0 + E[4]) - E[0]) - E[8]) * 2.0;
        qw = (E[2] - E[6]) / h; qx = (E[1] + E[3]) / h; qy = 0.25 * h; qz = (E[5] + E[7]) / h;
    } else {
        const double h = sqrt(((1.0 + E[8]) - E[0]) - E[4]) * 2.0;
        qw = (E[3] - E[1]) / h; qx = (E[2] + E[6]) / h; qy = (E[5] + E[7]) / h; qz = 0.25 * h;
    }
    const double nq = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    const double sg = qw < 0.0 ? -2.0 : 2.0;
    r[0] = sg * (qx / nq); r[1] = sg * (qy / nq); r[2] = sg * (qz / nq);
}
// the residuals, factors and weights of the active edges at the rotations in LDS
template <class Sync>
__device__ inline void pg_rot_weights(const PgScene& s, int kind, int tid, int nt, const Sync& sync) {
    const double* rot = s.lds + pg::L_ROT;
    for (int p = tid; p < s.P; p += nt) {
        const int k = s.key[p];
        double f = 0.0, r[3] = {0.0, 0.0, 0.0};
        if (k >= 0 && (k & pg::K_ACTIVE)) {
            double Rr[9], M1[9], E[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) Rr[j] = s.Rrel[(size_t)9 * p + j];
            pg_mul<false>(Rr, rot + 9 * (k & 255), M1);
            pg_mul<true>(rot + 9 * ((k >> 8) & 255), M1, E);
            pg_rot_residual(E, r);
            f = pg_factor(sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]), s.crot, kind);
        }
        s.res[(size_t)3 * p] = r[0]; s.res[(size_t)3 * p + 1] = r[1]; s.res[(size_t)3 * p + 2] = r[2];
        s.factor[(size_t)2 * p] = f;
        s.wcur[p] = s.weight[p] * f;
    }
    sync();
}
// the view pair (i >= j, compact) of slot t of the packed triangle of blocks
__device__ inline void pg_slot(int t, int& i, int& j) {
    i = 0;
    while (t > i) { t -= i + 1; ++i; }
    j = t;
}
// the Laplacian of a rotation round and its three right-hand sides
template <class Sync>
__device__ inline void pg_rot_assemble(const PgScene& s, int tid, int nt, const Sync& sync) {
    const int nr = s.ldi[pg::I_NR];
    double* T = s.lds + pg::L_SYS + pg::R_TRI;
    double* rhs = s.lds + pg::L_SYS + pg::R_RHS;
    for (int t = tid; t < nr * (nr + 1) / 2; t += nt) {
        int i, j;
        pg_slot(t, i, j);
        const int vi = s.ldi[pg::I_VIEW + i], vj = s.ldi[pg::I_VIEW + j];
        double acc = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0;
        for (int p = 0; p < s.P; ++p) {
            const int k = s.key[p];
            if (k < 0 || !(k & pg::K_ACTIVE)) continue;
            const int a = k & 255, b = (k >> 8) & 255;
            if (i == j) {
                if (a != vi && b != vi) continue;
                const double w = s.wcur[p];
                acc = acc + w;
                const double r0 = w * s.res[(size_t)3 * p], r1 = w * s.res[(size_t)3 * p + 1], r2 = w * s.res[(size_t)3 * p + 2];
                if (a == vi) { h0 = h0 - r0; h1 = h1 - r1; h2 = h2 - r2; }
                else { h0 = h0 + r0; h1 = h1 + r1; h2 = h2 + r2; }
            } else if ((a == vi && b == vj) || (a == vj && b == vi)) {
                acc = acc - s.wcur[p];
            }
        }
        T[i * (i + 1) / 2 + j] = acc;
        if (i == j) { rhs[i] = h0; rhs[32 + i] = h1; rhs[64 + i] = h2; }
    }
    sync();
}
// the three solves of a rotation round (the solutions replace the right-hand sides) and the update of the rotations
template <class Sync>
__device__ inline void pg_rot_solve(const PgScene& s, int tid, int nt, const Sync& sync) {
    const int nr = s.ldi[pg::I_NR];
    const double* T = s.lds + pg::L_SYS + pg::R_TRI;
    double* Wk = s.lds + pg::L_SYS + pg::R_WORK;
    double* rhs = s.lds + pg::L_SYS + pg::R_RHS;
    double* piv = s.lds + pg::L_SYS + pg::R_PIV;
    double* rot = s.lds + pg::L_ROT;
    bool ok = true;
    for (int x = 0; x < 3; ++x) {
        for (int t = tid; t < nr * (nr + 1) / 2; t += nt) Wk[t] = T[t];
        ok = ba_cholesky_solve(Wk, rhs + 32 * x, piv, nr, tid, nt, sync) && ok;
        sync();
    }
    if (ok) {
        for (int i = tid; i < nr; i += nt) {
            const int v = s.ldi[pg::I_VIEW + i];
            const double d6[6] = {rhs[i], rhs[32 + i], rhs[64 + i], 0.0, 0.0, 0.0}, t0[3] = {0.0, 0.0, 0.0};
            double R[9], Rn[9], tn[3];
#pragma unroll
            for (int j = 0; j < 9; ++j) R[j] = rot[9 * v + j];
            ba_pose_update(R, t0, d6, Rn, tn);
#pragma unroll
            for (int j = 0; j < 9; ++j) rot[9 * v + j] = Rn[j];
        }
    }
    sync();
}
// the directions of the active edges that have one
template <class Sync>
__device__ inline void pg_directions(const PgScene& s, int tid, int nt, const Sync& sync) {
    const double* rot = s.lds + pg::L_ROT;
    for (int p = tid; p < s.P; p += nt) {
        const int k = s.key[p];
        double d[3] = {0.0, 0.0, 0.0};
        if (k >= 0 && (k & pg::K_ACTIVE) && (k & pg::K_DIR)) {
            const double t0 = s.trel[(size_t)3 * p], t1 = s.trel[(size_t)3 * p + 1], t2 = s.trel[(size_t)3 * p + 2];
            const double n = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
            const double u0 = t0 / n, u1 = t1 / n, u2 = t2 / n;
            const double* Rb = rot + 9 * ((k >> 8) & 255);
#pragma unroll
            for (int x = 0; x < 3; ++x) d[x] = (Rb[x] * u0 + Rb[3 + x] * u1) + Rb[6 + x] * u2;
        }
        s.dir[(size_t)3 * p] = d[0]; s.dir[(size_t)3 * p + 1] = d[1]; s.dir[(size_t)3 * p + 2] = d[2];
    }
    sync();
}
// the factors and weights of the position edges: 1 with `first`, else from the centres in LDS
template <class Sync>
__device__ inline void pg_pos_weights(const PgScene& s, int kind, bool first, int tid, int nt, const Sync& sync) {
    const double* cen = s.lds + pg::L_CEN;
    for (int p = tid; p < s.P; p += nt) {
        const int k = s.key[p];
        double f = 0.0;
        if (k >= 0 && (k & pg::K_ACTIVE) && (k & pg::K_DIR)) {
            f = 1.0;
            if (!first) {
                const double* ca = cen + 3 * (k & 255);
                const double* cb = cen + 3 * ((k >> 8) & 255);
                const double d0 = s.dir[(size_t)3 * p], d1 = s.dir[(size_t)3 * p + 1], d2 = s.dir[(size_t)3 * p + 2];
                const double e0 = ca[0] - cb[0], e1 = ca[1] - cb[1], e2 = ca[2] - cb[2];
                const double pr = (d0 * e0 + d1 * e1) + d2 * e2;
                const double q0 = e0 - pr * d0, q1 = e1 - pr * d1, q2 = e2 - pr * d2;
                const double rho = pr > 0.0 ? sqrt((q0 * q0 + q1 * q1) + q2 * q2) / sqrt((e0 * e0 + e1 * e1) + e2 * e2) : 1.0;
                f = pg_factor(rho, s.cpos, kind);
            }
        }
        s.factor[(size_t)2 * p + 1] = f;
        s.wcur[p] = s.weight[p] * f;
    }
    sync();
}
// M (packed, n = 3 n_r) and g of a position round
template <class Sync>
__device__ inline void pg_pos_assemble(const PgScene& s, int tid, int nt, const Sync& sync) {
    const int nr = s.ldi[pg::I_NR];
    double* T = s.lds + pg::L_SYS;
    double* g = s.lds + pg::L_RHS;
    for (int t = tid; t < nr * (nr + 1) / 2; t += nt) {
        int i, j;
        pg_slot(t, i, j);
        const int vi = s.ldi[pg::I_VIEW + i], vj = s.ldi[pg::I_VIEW + j];
        double B[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, h[3] = {0.0, 0.0, 0.0};
        for (int p = 0; p < s.P; ++p) {
            const int k = s.key[p];
            if (k < 0 || !(k & pg::K_ACTIVE) || !(k & pg::K_DIR)) continue;
            const int a = k & 255, b = (k >> 8) & 255;
            const bool diag = i == j && (a == vi || b == vi), off = i != j && ((a == vi && b == vj) || (a == vj && b == vi));
            if (!diag && !off) continue;
            const double w = s.wcur[p];
            const double d[3] = {s.dir[(size_t)3 * p], s.dir[(size_t)3 * p + 1], s.dir[(size_t)3 * p + 2]};
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) {
                    const double m = w * ((x == y ? 1.0 : 0.0) - d[x] * d[y]);
                    B[3 * x + y] = diag ? B[3 * x + y] + m : B[3 * x + y] - m;
                }
            if (diag) {
#pragma unroll
                for (int x = 0; x < 3; ++x) h[x] = a == vi ? h[x] + w * d[x] : h[x] - w * d[x];
            }
        }
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y)
                if (i != j || y <= x) T[(3 * i + x) * (3 * i + x + 1) / 2 + 3 * j + y] = B[3 * x + y];
        if (i == j) { g[3 * i] = h[0]; g[3 * i + 1] = h[1]; g[3 * i + 2] = h[2]; }
    }
    sync();
}
// A = M + (mu g) g', A c = g, the rigidity test, the scale; the centres of the views into LDS.  false: the positions are not determined
template <class Sync>
__device__ inline bool pg_pos_solve(const PgScene& s, int tid, int nt, const Sync& sync) {
    const int nr = s.ldi[pg::I_NR], n = 3 * nr;
    double* T = s.lds + pg::L_SYS;
    double* g = s.lds + pg::L_RHS;
    double* piv = s.lds + pg::L_PIV;
    double* dg = s.lds + pg::L_DIAG;
    double* cen = s.lds + pg::L_CEN;
    double* sc = s.lds + pg::L_SC;
    if (tid == 0) {
        double trm = 0.0, gg = 0.0;
        for (int i = 0; i < n; ++i) { trm = trm + T[i * (i + 1) / 2 + i]; gg = gg + g[i] * g[i]; }
        sc[0] = trm / gg;
    }
    sync();
    const double mu = sc[0];
    if (!(tv::is_finite(mu) && mu > 0.0)) return false;
    for (int i = tid; i < n; i += nt) {
        const double mg = mu * g[i];
        for (int j = 0; j <= i; ++j) T[i * (i + 1) / 2 + j] = T[i * (i + 1) / 2 + j] + mg * g[j];
        dg[i] = T[i * (i + 1) / 2 + i];
    }
    const bool ok = ba_cholesky_solve(T, g, piv, n, tid, nt, sync);
    sync();
    if (!ok) return false;
    if (tid == 0) {
        double lo = T[0] / dg[0];
        for (int i = 1; i < n; ++i) {
            const double q = T[i * (i + 1) / 2 + i] / dg[i];
            lo = q < lo ? q : lo;
        }
        sc[1] = lo;
    }
    sync();
    if (!(sc[1] >= s.min_ratio)) return false;
    for (int i = tid; i < n; i += nt) cen[3 * s.ldi[pg::I_VIEW + i / 3] + i % 3] = g[i];
    sync();
    for (int p = tid; p < s.P; p += nt) {
        const int k = s.key[p];
        double a = 0.0, b = 0.0;
        if (k >= 0 && (k & pg::K_ACTIVE) && (k & pg::K_DIR)) {
            const double* ca = cen + 3 * (k & 255);
            const double* cb = cen + 3 * ((k >> 8) & 255);
            const double e0 = ca[0] - cb[0], e1 = ca[1] - cb[1], e2 = ca[2] - cb[2];
            b = s.wcur[p];
            a = b * ((s.dir[(size_t)3 * p] * e0 + s.dir[(size_t)3 * p + 1] * e1) + s.dir[(size_t)3 * p + 2] * e2);
        }
        s.ta[p] = a; s.tb[p] = b;
    }
    const double sa = pg_sum(s.ta, s.P, s.lds + pg::L_RED, tid, nt, sync);
    const double sb = pg_sum(s.tb, s.P, s.lds + pg::L_RED, tid, nt, sync);
    const double scale = sa / sb;
    if (!(tv::is_finite(scale) && scale > 0.0)) return false;
    for (int i = tid; i < n; i += nt) {
        double* c = cen + 3 * s.ldi[pg::I_VIEW + i / 3] + i % 3;
        *c = *c / scale;
    }
    sync();
    return true;
}
// the counts of info: valid edges (0), with a direction (1), final rotation factor < 0.5 (2), final position factor < 0.5 (3)
template <class Sync>
__device__ inline int pg_count(const PgScene& s, int what, int tid, int nt, const Sync& sync) {
    for (int p = tid; p < s.P; p += nt) {
        const int k = s.key[p];
        const bool act = k >= 0 && (k & pg::K_ACTIVE), dir = k >= 0 && (k & pg::K_DIR);
        bool c = k >= 0;
        if (what == 1) c = dir;
        if (what == 2) c = act && s.factor[(size_t)2 * p] < 0.5;
        if (what == 3) c = act && dir && s.factor[(size_t)2 * p + 1] < 0.5;
        s.ta[p] = c ? 1.0 : 0.0;
    }
    return (int)pg_sum(s.ta, s.P, s.lds + pg::L_RED, tid, nt, sync);
}
// what the position rounds add to the edges' terms: nothing (pg_run), or the baseline ratios of posescale_body.hpp (pg_run_ratios)
struct PgEdgesOnly {
    template <class Sync> __device__ inline void prepare(const PgScene&, int, int, const Sync&) const {}
    template <class Sync> __device__ inline void weights(const PgScene&, int, bool, int, int, const Sync&) const {}
    template <class Sync> __device__ inline void assemble(const PgScene&, int, int, const Sync&) const {}
    template <class Sync> __device__ inline void finish(const PgScene&, bool, int, int, const Sync&) const {}
};
// the whole scene
template <class Sync, class Terms>
__device__ inline void pg_run_with(const PgScene& s, const Terms& x, int tid, int nt, const Sync& sync) {
    const double zero = s.min_ratio - s.min_ratio, nan = zero / zero;            // (NaN either way)
    pg_keys(s, tid, nt, sync);
    pg_tree(s, tid, nt, sync);
    x.prepare(s, tid, nt, sync);
    const int nr = s.ldi[pg::I_NR];
    const unsigned reg = (unsigned)s.ldi[pg::I_REG];
    const int last = pg_kind(s, s.iterations - 1);
    bool pos = false;
    if (nr > 0) {
        for (int k = 0; k < s.iterations; ++k) {
            pg_rot_weights(s, pg_kind(s, k), tid, nt, sync);
            pg_rot_assemble(s, tid, nt, sync);
            pg_rot_solve(s, tid, nt, sync);
        }
        pg_rot_weights(s, last, tid, nt, sync);
        pg_directions(s, tid, nt, sync);
        pos = true;
        for (int k = 0; k < s.iterations && pos; ++k) {
            pg_pos_weights(s, pg_kind(s, k), k == 0, tid, nt, sync);
            x.weights(s, pg_kind(s, k), k == 0, tid, nt, sync);
            pg_pos_assemble(s, tid, nt, sync);
            x.assemble(s, tid, nt, sync);
            pos = pg_pos_solve(s, tid, nt, sync);
        }
        if (pos) {
            pg_pos_weights(s, last, false, tid, nt, sync);
            x.weights(s, last, false, tid, nt, sync);
        }
    } else {
        for (int p = tid; p < s.P; p += nt) s.factor[(size_t)2 * p] = 0.0;
    }
    x.finish(s, pos, tid, nt, sync);
    if (!pos) {
        for (int p = tid; p < s.P; p += nt) s.factor[(size_t)2 * p + 1] = 0.0;
        sync();
    }
    const int n_valid = pg_count(s, 0, tid, nt, sync), n_dir = pg_count(s, 1, tid, nt, sync);
    const int n_rot = pg_count(s, 2, tid, nt, sync), n_pos = pos ? pg_count(s, 3, tid, nt, sync) : 0;
    const double* rot = s.lds + pg::L_ROT;
    const double* cen = s.lds + pg::L_CEN;
    double* fin = s.lds + pg::L_BW;
    for (int v = tid; v < s.V; v += nt) {
        const bool in = (reg >> v) & 1u;
        bool f = true;
        const double* R = rot + 9 * v;
#pragma unroll
        for (int j = 0; j < 9; ++j) { s.Rs[9 * v + j] = in ? R[j] : nan; f = f && tv::is_finite(R[j]); }
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double t = -((R[3 * x] * cen[3 * v] + R[3 * x + 1] * cen[3 * v + 1]) + R[3 * x + 2] * cen[3 * v + 2]);
            const bool has = in && (pos || v == 0);
            s.ts[3 * v + x] = has ? (v == 0 ? 0.0 : t) : nan;
            f = f && (!has || tv::is_finite(t));
        }
        fin[v] = in && !f ? 1.0 : 0.0;
    }
    sync();
    if (tid == 0) {
        bool bad = false;
        int count = 0;
        for (int v = 0; v < s.V; ++v) { bad = bad || fin[v] != 0.0; count += (int)((reg >> v) & 1u); }
        s.registered[0] = (int32_t)reg;
        s.info[0] = n_valid; s.info[1] = count; s.info[2] = n_dir; s.info[3] = n_rot; s.info[4] = n_pos; s.info[5] = 3 * nr;
        s.info[6] = nr == 0 ? pg::ST_NOTHING : (bad ? pg::ST_NOT_FINITE : (pos ? pg::ST_OK : pg::ST_ROTATIONS_ONLY));
        s.info[7] = 0;
    }
}
template <class Sync>
__device__ inline void pg_run(const PgScene& s, int tid, int nt, const Sync& sync) { pg_run_with(s, PgEdgesOnly(), tid, nt, sync); }
// ---- pose graph end ----

struct PgArgs {
    const int32_t* pairs;     // (S, P, 2)
    const double* Rrel;       // (S, P, 9)
    const double* trel;       // (S, P, 3)
    const double* weight;     // (S, P)
    const int32_t* n_views;   // (S,) or NULL
    int P, V, iterations, redescend;
    double crot, cpos, min_ratio;
    double* Rs;
    double* ts;
    int32_t* registered;
    double* factor;
    int32_t* info;
    int32_t* key;             // workspace: (S, P) keys, then (S, 9, P) doubles
    double* wd;
};

// scene sc of a call; lds: pg::L_END doubles, ldi: pg::I_END ints
__device__ inline PgScene pg_scene_of(const PgArgs& a, size_t sc, double* lds, int* ldi) {
    const size_t P = (size_t)a.P;
    int nv = a.n_views ? a.n_views[sc] : a.V;
    nv = nv < 0 ? 0 : (nv > a.V ? a.V : nv);
    PgScene s;
    s.pairs = a.pairs + sc * P * 2; s.Rrel = a.Rrel + sc * P * 9; s.trel = a.trel + sc * P * 3; s.weight = a.weight + sc * P;
    s.nv = nv; s.P = a.P; s.V = a.V; s.iterations = a.iterations; s.redescend = a.redescend;
    s.crot = a.crot; s.cpos = a.cpos; s.min_ratio = a.min_ratio;
    s.Rs = a.Rs + sc * a.V * 9; s.ts = a.ts + sc * a.V * 3; s.registered = a.registered + sc; s.factor = a.factor + sc * P * 2; s.info = a.info + sc * 8;
    s.key = a.key + sc * P;
    double* w = a.wd + sc * 9 * P;
    s.wcur = w; s.res = w + P; s.dir = w + 4 * P; s.ta = w + 7 * P; s.tb = w + 8 * P;
    s.lds = lds; s.ldi = ldi;
    return s;
}

__global__ __launch_bounds__(256) void pose_graph_kernel(PgArgs a) {
    __shared__ double lds[pg::L_END];
    __shared__ int ldi[pg::I_END];
    pg_run(pg_scene_of(a, blockIdx.x, lds, ldi), (int)threadIdx.x, 256, BaBarrier());
}

// the workspace's parts in order: the keys, the per-edge doubles
static size_t pg_layout(int S, int P, size_t* off) {
    const size_t sz[2] = {(size_t)S * P * 4, (size_t)S * P * 9 * 8};
    size_t at = 0;
    for (int i = 0; i < 2; ++i) { if (off) off[i] = at; at += ba_align(sz[i]); }
    return at;
}
size_t pose_graph_workspace_bytes(int S, int P, int V) { (void)V; return pg_layout(S, P, nullptr); }

static PgArgs pg_args(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight, const int32_t* n_views, int S, int P, int V,
                      int iterations, int redescend, double rot_scale_rad, double pos_scale_sin, double min_pivot_ratio, double* Rs_out, double* ts_out,
                      int32_t* registered, double* edge_factor, int32_t* info, void* ws) {
    size_t off[2];
    pg_layout(S, P, off);
    char* w = static_cast<char*>(ws);
    PgArgs a = {};
    a.pairs = view_pairs; a.Rrel = R_rel; a.trel = t_rel; a.weight = weight; a.n_views = n_views; a.P = P; a.V = V; a.iterations = iterations;
    a.redescend = redescend; a.crot = rot_scale_rad; a.cpos = pos_scale_sin; a.min_ratio = min_pivot_ratio;
    a.Rs = Rs_out; a.ts = ts_out; a.registered = registered; a.factor = edge_factor; a.info = info;
    a.key = reinterpret_cast<int32_t*>(w + off[0]); a.wd = reinterpret_cast<double*>(w + off[1]);
    return a;
}

int launch_average_poses(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight, const int32_t* n_views, int S, int P,
                         int V, int iterations, int redescend, double rot_scale_rad, double pos_scale_sin, double min_pivot_ratio, double* Rs_out,
                         double* ts_out, int32_t* registered, double* edge_factor, int32_t* info, void* ws, hipStream_t st) {
    if (S < 1 || S > 65535 || P < 1 || V < 2 || V > mv::MAX_VIEWS || iterations < 1 || redescend < 0 || redescend > iterations) return -1;
    const PgArgs a = pg_args(view_pairs, R_rel, t_rel, weight, n_views, S, P, V, iterations, redescend, rot_scale_rad, pos_scale_sin, min_pivot_ratio, Rs_out,
                             ts_out, registered, edge_factor, info, ws);
    pose_graph_kernel<<<S, 256, 0, st>>>(a);
    return 0;
}

// the baseline ratios of the edge pairs that share a view and their terms in the position rounds
#include "posescale_body.hpp"

// ================================================================================================================================================
// Geometric verification of match lists under world poses (tests/verification_reference.py restates it operation for operation
// and tests/test_verification_emulated.py compiles the slice below, behind the solver and views-solver slices above, on the host): the
// epipolar test that relpose_select_kernel (k_relpose.hip) applies under its own estimate, for the pairs of a pair graph under the poses of
// the views -- for a pair whose own RANSAC failed but whose views are registered, and for a new selection under adjusted poses.
// Per pair p = (a, b) of scene s, once per workgroup:
//   * status 1: a == b or a view outside [0, n_views[s]) (n_views clamped to [0, V]; NULL: V); 2: the pose of a or b is not usable
//     (mv_stage_pose: an entry not finite, or R all zero); 3: trel == 0; they are tested in this order;
//   * Rrel = R_b R_a', trel = t_b - Rrel t_a, E = [trel]x Rrel (mv_pair); f = 0.5 ((fx_a + fy_a) 0.5 + (fx_b + fy_b) 0.5);
//     thr = max_epipolar_error / f, thr2 = thr thr (RpPair::thr2_of of k_relpose.hip).
// Per match i < n = n_matches[s, p] clamped to [0, cap], when the status is 0: it is EVALUATED when both rows are in [0, K) and the four
//   pixel coordinates are finite; then x = ((u - cx) / fx, (v - cy) / fy) per view in fp64 (RpPair::get), r2 = tv::sampson(E, x_a, x_b),
//   mask = r2 is finite and r2 < thr2, err = fp32 of sqrt(r2) f.  Every other entry of the (cap) row: mask 0, err NaN.
// pair_info: the status, n, the entries with mask 1, 0.  No cheirality test: the triangulation has its gates.
// Launch: verify_matches_kernel, one workgroup of 256 per pair (grid S P), thread 0 stages the pair in LDS, every thread walks the row in
// steps of 256; the kept entries are counted by wave ballots into four LDS words that only their own wave's first lane writes.

// ---- match verify begin (host-compilable with tests/emu/emu.hpp, behind the slices above) ----
namespace vm {
constexpr int ST_OK = 0, ST_PAIR = 1, ST_POSE = 2, ST_BASELINE = 3;       // pair_info word 0
constexpr int ESS = 0, CAL = 9, THR2 = 17, FOCAL = 18, L_END = 19;          // the staged pair: E, (fx, fy, cx, cy) of a and of b, thr2, f
constexpr unsigned NAN_BITS = 0x7fc00000u;
}  // namespace vm

struct VmArgs {
    const float* kpts;           // (S, V, K, 2)
    const int32_t* view_pairs;   // (S, P, 2)
    const int64_t* idx_a;        // (S, P, cap)
    const int64_t* idx_b;
    const int32_t* n_matches;    // (S, P)
    const int32_t* n_views;      // (S,) or null
    const double* Ks;            // (S, V, 9)
    const double* Rs;            // (S, V, 9)
    const double* ts;            // (S, V, 3)
    int P, cap, V, K;
    double max_err;
    unsigned char* mask;         // (S, P, cap)
    float* err;                  // (S, P, cap) or null
    int32_t* info;               // (S, P, 4)
};

__device__ inline bool vm_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the pair (a, b) of a scene with nv views: its status and, when that is 0, the vm::L_END doubles of o
__device__ inline int vm_stage_pair(int a, int b, int nv, const double* Ks, const double* Rs, const double* ts, double max_err, double* o) {
    if (a == b || (unsigned)a >= (unsigned)nv || (unsigned)b >= (unsigned)nv) return vm::ST_PAIR;
    double pa[mv::RREL], pb[mv::RREL];                     // (what mv_stage_pose writes: ROT, TRA, CAL, CEN, OK)
    mv_stage_pose(Rs + (size_t)a * 9, ts + (size_t)a * 3, Ks + (size_t)a * 9, pa);
    mv_stage_pose(Rs + (size_t)b * 9, ts + (size_t)b * 3, Ks + (size_t)b * 9, pb);
    if (pa[mv::OK] == 0.0 || pb[mv::OK] == 0.0) return vm::ST_POSE;
    double Rrel[9], trel[3];
    mv_pair(pa + mv::ROT, pa + mv::TRA, pb + mv::ROT, pb + mv::TRA, Rrel, trel, o + vm::ESS);
    if (trel[0] == 0.0 && trel[1] == 0.0 && trel[2] == 0.0) return vm::ST_BASELINE;
    // CAL of a staged pose is (fx, fy, cx, cy)
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[vm::CAL + k] = pa[mv::CAL + k]; o[vm::CAL + 4 + k] = pb[mv::CAL + k]; }
    const double f = 0.5 * ((o[vm::CAL] + o[vm::CAL + 1]) * 0.5 + (o[vm::CAL + 4] + o[vm::CAL + 5]) * 0.5);
    const double thr = max_err / f;
    o[vm::THR2] = thr * thr;
    o[vm::FOCAL] = f;
    return vm::ST_OK;
}

__global__ __launch_bounds__(256) void verify_matches_kernel(VmArgs a) {
    __shared__ double pr[vm::L_END];
    __shared__ int st_sh;
    __shared__ int wave_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pair = blockIdx.x, s = pair / (size_t)a.P;
    if (tid == 0) {
        int nv = a.n_views ? a.n_views[s] : a.V;
        nv = nv < 0 ? 0 : (nv > a.V ? a.V : nv);
        const size_t v0 = s * (size_t)a.V;
        st_sh = vm_stage_pair(a.view_pairs[2 * pair], a.view_pairs[2 * pair + 1], nv, a.Ks + v0 * 9, a.Rs + v0 * 9, a.ts + v0 * 3, a.max_err, pr);
    }
    __syncthreads();
    const int st = st_sh;
    int n = a.n_matches[pair];
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    const int live = st == vm::ST_OK ? n : 0;
    double E[9], cal[8];                                    // (LDS broadcasts; a pair that is not ok left pr unwritten)
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = live > 0 ? pr[vm::ESS + k] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cal[k] = live > 0 ? pr[vm::CAL + k] : 0.0;
    const double thr2 = live > 0 ? pr[vm::THR2] : 0.0, f = live > 0 ? pr[vm::FOCAL] : 0.0;
    // views in range: vm_stage_pair checked them for a live pair
    const int va = live > 0 ? a.view_pairs[2 * pair] : 0, vb = live > 0 ? a.view_pairs[2 * pair + 1] : 0;
    const float* ka = a.kpts + (s * (size_t)a.V + va) * a.K * 2;
    const float* kb = a.kpts + (s * (size_t)a.V + vb) * a.K * 2;
    const size_t base = pair * (size_t)a.cap;
    const float nanv = __uint_as_float(vm::NAN_BITS);
    int kept = 0;
    for (int b0 = 0; b0 < a.cap; b0 += 256) {               // (the trip count is the same for every thread: the ballot is the whole wave's)
        const int i = b0 + tid;
        bool in = false;
        float e = nanv;
        if (i < live) {
            const unsigned long long ra = (unsigned long long)a.idx_a[base + i], rb = (unsigned long long)a.idx_b[base + i];      // (-1 is a huge unsigned one)
            if (ra < (unsigned long long)a.K && rb < (unsigned long long)a.K) {
                const float2 q0 = *reinterpret_cast<const float2*>(ka + 2 * ra);
                const float2 q1 = *reinterpret_cast<const float2*>(kb + 2 * rb);
                if (vm_finite(q0.x) && vm_finite(q0.y) && vm_finite(q1.x) && vm_finite(q1.y)) {
                    const double r2 = tv::sampson(E, ((double)q0.x - cal[2]) / cal[0], ((double)q0.y - cal[3]) / cal[1], ((double)q1.x - cal[6]) / cal[4],
                                                  ((double)q1.y - cal[7]) / cal[5]);
                    in = tv::is_finite(r2) && r2 < thr2;
                    e = (float)(sqrt(r2) * f);
                }
            }
        }
        if (i < a.cap) {
            a.mask[base + i] = in ? 1 : 0;
            if (a.err) a.err[base + i] = e;
        }
        kept += (int)__popcll(__ballot(in));                // (the same in every lane of a wave)
    }
    if (lane == 0) wave_n[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        int32_t* info = a.info + pair * 4;
        info[0] = st; info[1] = n; info[2] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]); info[3] = 0;
    }
}
// ---- match verify end ----

int launch_verify_matches(const float* kpts, const int32_t* view_pairs, const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches,
                          const int32_t* n_views, int S, int P, int cap, int V, int K, const double* Ks, const double* Rs, const double* ts,
                          double max_epipolar_error, unsigned char* mask, float* err, int32_t* pair_info, hipStream_t st) {
    if (S < 1 || S > 65535 || P < 1 || cap < 1 || V < 2 || V > mv::MAX_VIEWS || K < 1) return -1;
    if ((long long)S * P > 0x7fffffffll) return -1;         // the grid is one-dimensional over the pairs
    VmArgs a = {};
    a.kpts = kpts; a.view_pairs = view_pairs; a.idx_a = idx_a; a.idx_b = idx_b; a.n_matches = n_matches; a.n_views = n_views; a.Ks = Ks; a.Rs = Rs; a.ts = ts;
    a.P = P; a.cap = cap; a.V = V; a.K = K; a.max_err = max_epipolar_error; a.mask = mask; a.err = err; a.info = pair_info;
    verify_matches_kernel<<<(unsigned)((long long)S * P), 256, 0, st>>>(a);
    return 0;
}

}  // namespace xfh
