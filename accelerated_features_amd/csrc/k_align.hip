// 3D-3D alignment: the similarity (or rigid) transform between two sets of corresponding 3D points,
//     B ~= s R A + t,   R a proper rotation, s > 0   (with_scale = 0: s = 1, the rigid case)
// -- the metric relative pose of an RGB-D pair (both key-point sets lifted through their depth maps), the scale between two reconstructions
// triangulated under baselines of their own, the registration of a reconstruction to a metric frame.  The estimator is RANSAC over a
// 3-point solver with a closed-form least-squares fit of the consensus set (Horn, JOSA A 1987: the rotation as the dominant eigenvector of
// a symmetric 4x4 matrix; Umeyama, PAMI 1991 for the scale).  The specification (tests/alignment_reference.py is a numpy
// restatement of it, operation for operation, and tests/test_alignment_emulated.py compiles the solver below on the host and holds it to
// that restatement bit for bit):
//   * inputs of pair p: points A (cap_a rows of 3 fp32), points B (cap_b rows of 3 fp32); correspondence i = (row i, row i) or, with index
//     lists, (row idx_a[i] of A, row idx_b[i] of B); the two sides have capacities of their own (AlView); an index outside its table makes
//     the correspondence NaN.  Rows may be NaN ("no point", as unproject_keypoints and the triangulation's scatter write them): such a
//     correspondence is never sampled into a model and never an inlier.  A correspondence travels as 6 fp64;
//   * threshold: max_error is a distance in B's unit, thr2 = max_error^2; it is not rescaled;
//   * sample: 3 distinct correspondences (rs::sample_distinct<3>); a sample that runs out of draws or holds a non-finite coordinate yields
//     no model;
//   * minimal solver (al_solve): the orthonormal frame of each triangle (tv::triangle_frame, the construction of DESIGN 3.12, with the
//     same collinearity test -- sin^2 at the first corner <= 1e-8 -- on both triangles; a zero first side: no model);
//     R = [frame of B1 B2 B3] [frame of A1 A2 A3]'; centroids ca = ((A1 + A2) + A3) / 3, cb likewise; va, vb = the sums of the squared
//     distances of the three points to their centroid; s = sqrt(vb / va) (va or vb not > 0, s not finite: no model; with_scale = 0: s = 1);
//     t = cb - s (R ca).  One candidate per hypothesis: 13 fp64 = R (row-major), t, s;
//   * score: r^2 = |B - ((sR) A + t)|^2 with sR = s R formed once per hypothesis; anything non-finite is never an inlier and costs the
//     cap; MSAC cost floor(min(r^2, thr2) / thr2 * 2^20) summed as u64 (the family's formula); inlier: r^2 < thr2; rs::hyp_best<1, true>;
//   * stopping rule: rs::scan_stopping_rule<3, true>; the later blocks run below rs::hypotheses_bound<3, true> of the first 256;
//   * refit (al_fit): closed form over the current inliers, in two passes so that the sums are centred (raw second moments cancel when
//     the cloud is far from the origin).  Pass 1: the 6 coordinate sums (rs::block_sums<6>) and the inlier count give the centroids
//     ca, cb = sums / count.  Pass 2: with x = A - ca, y = B - cb the 9 entries S[3 i + j] = sum x_i y_j and S[9] = sum |x|^2
//     (rs::block_sums<10>).  Horn's matrix
//         N = [ Sxx+Syy+Szz  Syz-Szy      Szx-Sxz      Sxy-Syx     ]
//             [              Sxx-Syy-Szz  Sxy+Syx      Szx+Sxz     ]
//             [                           -Sxx+Syy-Szz Syz+Szy     ]
//             [ (symmetric)                            -Sxx-Syy+Szz]
//     is diagonalised by cyclic Jacobi: JACOBI_SWEEPS = 8 sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a rotation is
//     skipped when N[p][q] is exactly 0; theta = (N[q][q] - N[p][p]) / (2 N[p][q]), t = sign(theta) / (|theta| + sqrt(theta^2 + 1))
//     (sign(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c; N[p][p] -= t N[p][q], N[q][q] += t N[p][q], rows / columns k != p, q:
//     (N[k][p], N[k][q]) <- (c N[k][p] - s N[k][q], s N[k][p] + c N[k][q]); the eigenvectors V (identity at the start) likewise on
//     their columns p, q.  The quaternion is the column of V at the largest diagonal entry (the lower index on ties); the rotation is the
//     quaternion's matrix divided by |q|^2, so it is a proper rotation whatever the clouds are (a mirrored cloud gets one, and no
//     consensus).  s = sum y . (R x) / sum |x|^2 from the same sums (with_scale = 0: 1; s not > 0 or not finite: no fit),
//     t = cb - s (R ca).  Agreement with an SVD fit: DESIGN 3.15;
//   * refit loop: up to LO_ITERS = 10 rounds of (inliers of the current model, al_fit, rescore); a refit is kept only if the integer cost
//     strictly drops, the first rejected (or failed) refit ends the loop; fewer than 3 inliers: no refit;
//   * only + - * / sqrt in all of it, every product and sum rounded once (fp contraction off in this file);
//   * outputs: R (row-major), t, s, the mask r^2 < thr2 under the final model, info = the family's 8 words; found = at least 3 inliers;
//     otherwise rs::write_nothing_found, zeros in R and t, s = 0.
//
// Registers, not LDS.  al_solve holds the sample (18 fp64), two frames (18) and the model (13); al_fit holds N (10 distinct entries) and
// V (16) with every index a compile-time constant (al_jacobi_rotate<P, Q> is instantiated six times), so nothing goes to scratch.
//
// Launches per call (workspace: per hypothesis 13 fp64, one cost, one inlier count, the candidate flag):
//   align_zero_kernel   : costs, counts, flags zeroed
//   align_solve_kernel  : thread = hypothesis: sample, al_solve, the model into the workspace             (hypotheses 0..255 first)
//   align_score_kernel  : thread = hypothesis (sR, t in 12 registers) against a chunk of correspondences in LDS, u64 atomics
//   align_bound_kernel  : the bound the loop reaches from the records among the first 256; the later blocks are solved and scored only
//                         below max(min_iterations, bound)
//   align_select_kernel : one workgroup per pair: stopping rule over the cost list (tiles in LDS), refit loop, mask, outputs.  LDS: the
//                         larger of the tiles (32 KiB) and the block_sums<10> buffer (20.8 KiB, in the dead tiles) + SEL_CACHE = 2048
//                         correspondences of 48 bytes (96 KiB) = 128 KiB of the CU's 160
#include "ransac_common.hpp"
#include "twoview_math.hpp"

#pragma clang fp contract(off)

namespace xfh {
namespace al {
using rs::HYP_PER_WG, rs::PTS_PER_WG, rs::SEL_TILE, rs::SEL_CACHE;
constexpr int LO_ITERS = 10, MAX_ITERS = 16384, NSUM1 = 6, NSUM2 = 10;
}  // namespace al

// ---- solver begin (host-compilable: tests/test_alignment_emulated.py slices it out behind the slice of twoview_math.hpp and drops the
// __device__ qualifiers) ----
namespace al {
constexpr int MODEL_DOUBLES = 13;            // R (row-major), t, s
constexpr int JACOBI_SWEEPS = 8;
constexpr double COLLINEAR_EPS2 = 1e-8;      // sin^2 of a triangle's angle at its first corner
}  // namespace al

// MSAC cost in 2^-20 units of thr2; NaN counts as the cap
__device__ inline unsigned al_cost(double r2, double thr2) {
    const double m = r2 < thr2 ? r2 : thr2;
    return (unsigned)floor(m / thr2 * 1048576.0);
}
// squared distance of b to (sR) a + t
__device__ inline double al_residual2(const double* sR, const double* t, double a0, double a1, double a2, double b0, double b1, double b2) {
    const double d0 = b0 - (((sR[0] * a0 + sR[1] * a1) + sR[2] * a2) + t[0]);
    const double d1 = b1 - (((sR[3] * a0 + sR[4] * a1) + sR[5] * a2) + t[1]);
    const double d2 = b2 - (((sR[6] * a0 + sR[7] * a1) + sR[8] * a2) + t[2]);
    return (d0 * d0 + d1 * d1) + d2 * d2;
}
// sR = s R of a model (R, t, s)
__device__ inline void al_scaled_rotation(const double* model, double* sR) {
#pragma unroll
    for (int k = 0; k < 9; ++k) sR[k] = model[12] * model[k];
}
// t = cb - s (R ca) into model[9..11]; false: something in the model is not finite
__device__ inline bool al_finish(const double* ca, const double* cb, double* model) {
    bool fin = tv::is_finite(model[12]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        model[9 + i] = cb[i] - model[12] * ((model[3 * i] * ca[0] + model[3 * i + 1] * ca[1]) + model[3 * i + 2] * ca[2]);
        fin = fin && tv::is_finite(model[9 + i]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && tv::is_finite(model[k]);
    return fin;
}
// the model of a sample: A[9], B[9] point-major; false: no model
__device__ inline bool al_solve(const double* A, const double* B, int with_scale, double* model) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && tv::is_finite(A[k]) && tv::is_finite(B[k]);
    if (!fin) return false;
    double ea[3][3], eb[3][3];
    if (!tv::triangle_frame(A, A + 3, A + 6, al::COLLINEAR_EPS2, ea[0], ea[1], ea[2])) return false;
    if (!tv::triangle_frame(B, B + 3, B + 6, al::COLLINEAR_EPS2, eb[0], eb[1], eb[2])) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) model[3 * i + j] = (eb[0][i] * ea[0][j] + eb[1][i] * ea[1][j]) + eb[2][i] * ea[2][j];
    double ca[3], cb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ca[k] = ((A[k] + A[3 + k]) + A[6 + k]) / 3.0;
        cb[k] = ((B[k] + B[3 + k]) + B[6 + k]) / 3.0;
    }
    double na[3], nb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double da[3] = {A[3 * i] - ca[0], A[3 * i + 1] - ca[1], A[3 * i + 2] - ca[2]};
        const double db[3] = {B[3 * i] - cb[0], B[3 * i + 1] - cb[1], B[3 * i + 2] - cb[2]};
        na[i] = tv::dot3(da, da);
        nb[i] = tv::dot3(db, db);
    }
    const double va = (na[0] + na[1]) + na[2], vb = (nb[0] + nb[1]) + nb[2];
    if (!(va > 0.0) || !(vb > 0.0)) return false;
    model[12] = with_scale ? sqrt(vb / va) : 1.0;
    return al_finish(ca, cb, model);
}
// one Jacobi rotation in the (P, Q) plane of the symmetric N with the eigenvectors V; every index is a compile-time constant
template <int P, int Q>
__device__ inline void al_jacobi_rotate(double (&N)[4][4], double (&V)[4][4]) {
    const double apq = N[P][Q];
    if (apq == 0.0) return;
    const double theta = (N[Q][Q] - N[P][P]) / (2.0 * apq);
    const double at = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / at;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    N[P][P] = N[P][P] - t * apq;
    N[Q][Q] = N[Q][Q] + t * apq;
    N[P][Q] = 0.0;
    N[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = N[k][P], akq = N[k][Q];
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            N[k][P] = np; N[P][k] = np;
            N[k][Q] = nq; N[Q][k] = nq;
        }
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}
// the least-squares model of a consensus set from its centred sums: S[3 i + j] = sum x_i y_j, S[9] = sum |x|^2 (x = A - ca, y = B - cb);
// false: no fit
__device__ inline bool al_fit(const double* S, const double* ca, const double* cb, int with_scale, double* model) {
    double N[4][4], V[4][4];
    N[0][0] = (S[0] + S[4]) + S[8];
    N[1][1] = (S[0] - S[4]) - S[8];
    N[2][2] = (S[4] - S[0]) - S[8];
    N[3][3] = (S[8] - S[0]) - S[4];
    N[0][1] = S[5] - S[7]; N[0][2] = S[6] - S[2]; N[0][3] = S[1] - S[3];
    N[1][2] = S[1] + S[3]; N[1][3] = S[6] + S[2]; N[2][3] = S[5] + S[7];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < i) N[i][j] = N[j][i];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < al::JACOBI_SWEEPS; ++sweep) {
        al_jacobi_rotate<0, 1>(N, V); al_jacobi_rotate<0, 2>(N, V); al_jacobi_rotate<0, 3>(N, V);
        al_jacobi_rotate<1, 2>(N, V); al_jacobi_rotate<1, 3>(N, V); al_jacobi_rotate<2, 3>(N, V);
    }
    double lam = N[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = N[k][k] > lam;
        lam = up ? N[k][k] : lam;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = up ? V[i][k] : q[i];
    }
    const double ww = q[0] * q[0], xx = q[1] * q[1], yy = q[2] * q[2], zz = q[3] * q[3];
    const double nq = ((ww + xx) + yy) + zz;
    const double wx = q[0] * q[1], wy = q[0] * q[2], wz = q[0] * q[3], xy = q[1] * q[2], xz = q[1] * q[3], yz = q[2] * q[3];
    model[0] = (((ww + xx) - yy) - zz) / nq; model[1] = (2.0 * (xy - wz)) / nq;        model[2] = (2.0 * (xz + wy)) / nq;
    model[3] = (2.0 * (xy + wz)) / nq;        model[4] = (((ww - xx) + yy) - zz) / nq; model[5] = (2.0 * (yz - wx)) / nq;
    model[6] = (2.0 * (xz - wy)) / nq;        model[7] = (2.0 * (yz + wx)) / nq;        model[8] = (((ww - xx) - yy) + zz) / nq;
    double sc = 1.0;
    if (with_scale) {
        double r[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] = (model[3 * i] * S[i] + model[3 * i + 1] * S[3 + i]) + model[3 * i + 2] * S[6 + i];
        sc = ((r[0] + r[1]) + r[2]) / S[9];
    }
    if (!(sc > 0.0)) return false;
    model[12] = sc;
    return al_finish(ca, cb, model);
}
// ---- solver end ----

struct AlArgs {
    const float* pa;          // (P, cap_a, 3): the points A of the correspondences (idx_a == NULL, cap_a == cap) or the table they index
    const float* pb;          // (P, cap_b, 3): the points B likewise
    const int64_t* idx_a;     // (P, cap) rows of pa / pb of correspondence i, or NULL
    const int64_t* idx_b;
    const int32_t* counts;
    int n_const, P, cap, cap_a, cap_b, iters, iters_pad, min_iters;
    int chunk, with_scale;
    double thr2;
    double log1mp;
    unsigned long long seed;
    double* model;            // (P, iters_pad, 13)
    unsigned long long* hcost;   // (P, iters_pad)
    unsigned* hcnt;              // (P, iters_pad)
    int* ncand;                  // (P, iters_pad): 1 = the hypothesis has a model
    int* bound;                  // (P)
    double* R;
    double* t;
    double* s;
    unsigned char* mask;
    int32_t* info;
};

// one correspondence
struct AlPt {
    double a0, a1, a2, b0, b1, b2;
};

// the 3D-3D correspondences of one pair: two tables with capacities of their own, through the index lists when given; a row outside its
// table reads as NaN
struct AlView {
    const float* pa;
    const float* pb;
    const int64_t* ia;
    const int64_t* ib;
    size_t cap_a, cap_b;
    __device__ AlView(const AlArgs& a, int pair)
        : pa(a.pa + (size_t)pair * a.cap_a * 3), pb(a.pb + (size_t)pair * a.cap_b * 3), ia(a.idx_a ? a.idx_a + (size_t)pair * a.cap : nullptr),
          ib(a.idx_b ? a.idx_b + (size_t)pair * a.cap : nullptr), cap_a((size_t)a.cap_a), cap_b((size_t)a.cap_b) {}
    __device__ inline AlPt get(int i) const {
        const size_t ra = ia ? (size_t)ia[i] : (size_t)i, rb = ib ? (size_t)ib[i] : (size_t)i;      // (a negative index wraps past the capacity)
        const double nan = __builtin_nan("");
        AlPt q{nan, nan, nan, nan, nan, nan};
        if (ra < cap_a && rb < cap_b) {
            q.a0 = (double)pa[3 * ra]; q.a1 = (double)pa[3 * ra + 1]; q.a2 = (double)pa[3 * ra + 2];
            q.b0 = (double)pb[3 * rb]; q.b1 = (double)pb[3 * rb + 1]; q.b2 = (double)pb[3 * rb + 2];
        }
        return q;
    }
};

__global__ __launch_bounds__(256) void align_zero_kernel(AlArgs a, size_t nhyp) {
    rs::zero_hypotheses<1>(a.ncand, a.hcost, a.hcnt, nhyp);
}

// hypotheses [it_base + 256 blockIdx.x, + 256) of pair blockIdx.y; only below the pair's bound when `use_bound`
__global__ __launch_bounds__(256) void align_solve_kernel(AlArgs a, int it_base, int use_bound) {
    const int pair = blockIdx.y;
    const int it = it_base + blockIdx.x * al::HYP_PER_WG + threadIdx.x;
    const int n = rs::pair_count(a, pair);
    if (n < 3 || it >= a.iters) return;
    if (use_bound && a.bound[pair] <= it) return;
    const AlView pp(a, pair);
    int idx[3] = {-1, -1, -1};
    if (!rs::sample_distinct(a.seed, pair, it, n, idx)) return;
    double A[9], B[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const AlPt q = pp.get(idx[k]);
        A[3 * k] = q.a0; A[3 * k + 1] = q.a1; A[3 * k + 2] = q.a2;
        B[3 * k] = q.b0; B[3 * k + 1] = q.b1; B[3 * k + 2] = q.b2;
    }
    double model[al::MODEL_DOUBLES];
    if (!al_solve(A, B, a.with_scale, model)) return;
    const size_t h = (size_t)pair * a.iters_pad + it;
    double* o = a.model + h * al::MODEL_DOUBLES;
#pragma unroll
    for (int k = 0; k < al::MODEL_DOUBLES; ++k) o[k] = model[k];
    a.ncand[h] = 1;
}

// Hypotheses [256 (blockIdx.x + blk0), + 256) of pair blockIdx.z against correspondences [chunk blockIdx.y, + chunk)
__global__ __launch_bounds__(256) void align_score_kernel(AlArgs a, int blk0, int use_bound) {
    __shared__ AlPt spt[al::PTS_PER_WG];
    const int pair = blockIdx.z, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    const int c0 = blockIdx.y * a.chunk;
    const int it0 = (blockIdx.x + blk0) * al::HYP_PER_WG;
    if (n < 3 || c0 >= n) return;
    if (use_bound && a.bound[pair] <= it0) return;
    const AlView pp(a, pair);
    const int c1 = min(c0 + a.chunk, n);
    for (int i = tid; i < c1 - c0; i += 256) spt[i] = pp.get(c0 + i);
    __syncthreads();
    const int it = it0 + tid;
    if (it >= a.iters) return;
    const size_t h = (size_t)pair * a.iters_pad + it;
    if (a.ncand[h] <= 0) return;
    const double* o = a.model + h * al::MODEL_DOUBLES;
    double md[al::MODEL_DOUBLES], sR[9], tm[3];
#pragma unroll
    for (int k = 0; k < al::MODEL_DOUBLES; ++k) md[k] = o[k];
    al_scaled_rotation(md, sR);
#pragma unroll
    for (int k = 0; k < 3; ++k) tm[k] = md[9 + k];
    const double thr2 = a.thr2;
    const int m = c1 - c0;
    unsigned long long sc = 0;
    unsigned cnt = 0;
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
        const AlPt q = spt[i];
        const double r2 = al_residual2(sR, tm, q.a0, q.a1, q.a2, q.b0, q.b1, q.b2);
        sc += al_cost(r2, thr2);
        cnt += r2 < thr2 ? 1u : 0u;
    }
    atomicAdd(a.hcost + h, sc);
    atomicAdd(a.hcnt + h, cnt);
}

// After the first 256 hypotheses: the index below which the loop can still visit hypotheses = max(min_iters, rs::hypotheses_bound over
// the records (strict prefix minima of the cost) among them)
__global__ __launch_bounds__(256) void align_bound_kernel(AlArgs a) {
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = rs::pair_count(a, pair);
    unsigned long long cost = ~0ull;
    unsigned cnt = 0;
    int cand = 0;
    const bool has = tid < a.iters && n >= 3 && rs::hyp_best<1, true>(a.ncand, a.hcost, a.hcnt, (size_t)pair * a.iters_pad + tid, cost, cnt, cand);
    const int bmin = rs::hypotheses_bound<3, true>(has, cost, cnt, n, a.log1mp, a.iters);
    if (tid == 0) a.bound[pair] = bmin > a.min_iters ? bmin : a.min_iters;
}

// ---- selection, refit, mask ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_select_kernel(AlArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double model_sh[al::MODEL_DOUBLES];
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
                                        return rs::hyp_best<1, true>(a.ncand, a.hcost, a.hcnt, (size_t)pair * a.iters_pad + it, c, k, cd);
                                    },
                                    best, best_cand, iters_run);
    if (best >= 0 && tid < al::MODEL_DOUBLES) model_sh[tid] = a.model[((size_t)pair * a.iters_pad + best) * al::MODEL_DOUBLES + tid];
    __syncthreads();
    double* Rout = a.R + (size_t)pair * 9;
    double* tout = a.t + (size_t)pair * 3;
    if (best < 0) {
        rs::write_nothing_found(mask, a.cap, info, iters_run, n);
        if (tid < 9) Rout[tid] = 0.0;
        if (tid < 3) tout[tid] = 0.0;
        if (tid == 0) a.s[pair] = 0.0;
        return;
    }
    const AlView pp(a, pair);
    const double thr2 = a.thr2;
    double* red = reinterpret_cast<double*>(lds_raw);         // the tiles are dead: reduction buffer from here on
    AlPt* spt = reinterpret_cast<AlPt*>(lds_raw + (size_t)al::SEL_TILE * 16);
    for (int i = tid; i < min(n, al::SEL_CACHE); i += 256) spt[i] = pp.get(i);
    __syncthreads();
    auto for_each = [&](auto&& f) { rs::for_each_cached(spt, n, [&](int i) { return pp.get(i); }, f); };
    double cur[al::MODEL_DOUBLES], bst[al::MODEL_DOUBLES], sR[9];
#pragma unroll
    for (int k = 0; k < al::MODEL_DOUBLES; ++k) { cur[k] = model_sh[k]; bst[k] = cur[k]; }
    unsigned long long c_best = ~0ull;
    int lo_accepted = 0;
    for (int step = 0; step <= al::LO_ITERS; ++step) {
        if (tid == 0) { sc_sh = 0ull; cnt_sh = 0u; }
        __syncthreads();
        // ---- pass 1: the cost of the current model, its inliers' count and coordinate sums
        al_scaled_rotation(cur, sR);
        double s1[al::NSUM1];
#pragma unroll
        for (int k = 0; k < al::NSUM1; ++k) s1[k] = 0.0;
        unsigned long long sc = 0;
        unsigned cn = 0;
        for_each([&](int, const AlPt& q) {
            const double r2 = al_residual2(sR, cur + 9, q.a0, q.a1, q.a2, q.b0, q.b1, q.b2);
            sc += al_cost(r2, thr2);
            if (r2 < thr2) {
                ++cn;
                s1[0] = s1[0] + q.a0; s1[1] = s1[1] + q.a1; s1[2] = s1[2] + q.a2;
                s1[3] = s1[3] + q.b0; s1[4] = s1[4] + q.b1; s1[5] = s1[5] + q.b2;
            }
        });
        atomicAdd(&sc_sh, sc);
        atomicAdd(&cnt_sh, cn);
        rs::block_sums(s1, red);                              // (its barriers also publish sc_sh, cnt_sh)
        const unsigned long long c_now = sc_sh;
        const unsigned n_cur = cnt_sh;
        if (step > 0 && !(c_now < c_best)) break;
#pragma unroll
        for (int k = 0; k < al::MODEL_DOUBLES; ++k) bst[k] = cur[k];
        if (step > 0) ++lo_accepted;
        c_best = c_now;
        if (step == al::LO_ITERS || n_cur < 3u) break;
        // ---- pass 2: the centred second moments of the same inliers
        const double dn = (double)n_cur;
        const double ca[3] = {s1[0] / dn, s1[1] / dn, s1[2] / dn}, cb[3] = {s1[3] / dn, s1[4] / dn, s1[5] / dn};
        double s2[al::NSUM2];
#pragma unroll
        for (int k = 0; k < al::NSUM2; ++k) s2[k] = 0.0;
        for_each([&](int, const AlPt& q) {
            const double r2 = al_residual2(sR, cur + 9, q.a0, q.a1, q.a2, q.b0, q.b1, q.b2);
            if (r2 < thr2) {
                const double x[3] = {q.a0 - ca[0], q.a1 - ca[1], q.a2 - ca[2]}, y[3] = {q.b0 - cb[0], q.b1 - cb[1], q.b2 - cb[2]};
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) s2[3 * i + j] = s2[3 * i + j] + x[i] * y[j];
                s2[9] = s2[9] + tv::dot3(x, x);
            }
        });
        rs::block_sums(s2, red);
        double nxt[al::MODEL_DOUBLES];
        if (!al_fit(s2, ca, cb, a.with_scale, nxt)) break;
#pragma unroll
        for (int k = 0; k < al::MODEL_DOUBLES; ++k) cur[k] = nxt[k];
        __syncthreads();                                     // sc_sh, cnt_sh read by everybody before they are cleared again
    }
    // ---- inlier mask under the final model
    __syncthreads();
    if (tid == 0) cnt_sh = 0u;
    __syncthreads();
    al_scaled_rotation(bst, sR);
    unsigned cn = 0;
    for_each([&](int, const AlPt& q) { cn += al_residual2(sR, bst + 9, q.a0, q.a1, q.a2, q.b0, q.b1, q.b2) < thr2 ? 1u : 0u; });
    atomicAdd(&cnt_sh, cn);
    __syncthreads();
    const int n_in = (int)cnt_sh;
    const bool found = n_in >= 3;
    for_each([&](int i, const AlPt& q) { mask[i] = found && al_residual2(sR, bst + 9, q.a0, q.a1, q.a2, q.b0, q.b1, q.b2) < thr2 ? 1 : 0; });
    for (int i = n + tid; i < a.cap; i += 256) mask[i] = 0;
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) Rout[k] = found ? bst[k] : 0.0;
        for (int k = 0; k < 3; ++k) tout[k] = found ? bst[9 + k] : 0.0;
        a.s[pair] = found ? bst[12] : 0.0;
        rs::write_info(info, found, best, iters_run, n_in, lo_accepted, n, c_best);
    }
}

size_t align_workspace_bytes(int P, int max_iters) {
    const size_t pad = (size_t)ceil_div(max_iters, 256) * 256;
    const size_t per = (size_t)al::MODEL_DOUBLES * 8 + 8 + 4 + 4;
    return (size_t)P * pad * per + (size_t)P * 4 + 1024;
}

int launch_estimate_alignment(const float* pa, const float* pb, const int64_t* idx_a, const int64_t* idx_b, int cap_a, int cap_b, const int32_t* counts,
                              int n_const, int P, int cap, int with_scale, double max_err, int min_iters, int max_iters, double success_prob,
                              unsigned long long seed, double* R, double* t, double* s, unsigned char* mask, int32_t* info, void* ws, hipStream_t st) {
    if (max_iters < 1 || max_iters > al::MAX_ITERS || P > 65535) return -1;
    AlArgs a;
    a.pa = pa; a.pb = pb; a.idx_a = idx_a; a.idx_b = idx_b; a.cap_a = idx_a ? cap_a : cap; a.cap_b = idx_b ? cap_b : cap; a.counts = counts;
    a.n_const = n_const; a.P = P; a.cap = cap; a.iters = max_iters; a.iters_pad = ceil_div(max_iters, 256) * 256;
    a.min_iters = min_iters < 0 ? 0 : min_iters; a.with_scale = with_scale ? 1 : 0;
    a.thr2 = max_err * max_err; a.log1mp = log(1.0 - success_prob); a.seed = seed;
    unsigned char* w = static_cast<unsigned char*>(ws);
    const size_t nhyp = (size_t)P * a.iters_pad;
    a.model = reinterpret_cast<double*>(w); w += nhyp * al::MODEL_DOUBLES * 8;
    a.hcost = reinterpret_cast<unsigned long long*>(w); w += nhyp * 8;
    a.hcnt = reinterpret_cast<unsigned*>(w); w += nhyp * 4;
    a.ncand = reinterpret_cast<int*>(w); w += nhyp * 4;
    a.bound = reinterpret_cast<int*>(w);
    a.R = R; a.t = t; a.s = s; a.mask = mask; a.info = info;
    a.chunk = rs::score_chunk(P, cap);
    const int nblk = ceil_div(max_iters, al::HYP_PER_WG), nch = ceil_div(cap, a.chunk);
    const size_t zg = (nhyp + 255) / 256;
    align_zero_kernel<<<(unsigned)(zg > 2048 ? 2048 : zg), 256, 0, st>>>(a, nhyp);
    align_solve_kernel<<<dim3(1, P), 256, 0, st>>>(a, 0, 0);
    align_score_kernel<<<dim3(1, nch, P), 256, 0, st>>>(a, 0, 0);
    if (nblk > 1) {
        align_bound_kernel<<<P, 256, 0, st>>>(a);
        align_solve_kernel<<<dim3(nblk - 1, P), 256, 0, st>>>(a, al::HYP_PER_WG, 1);
        align_score_kernel<<<dim3(nblk - 1, nch, P), 256, 0, st>>>(a, 1, 1);
    }
    static_assert(rs::block_sums_bytes(al::NSUM2) <= (size_t)al::SEL_TILE * 16, "the reduction buffer lives in the dead tiles");
    const size_t lds = (size_t)al::SEL_TILE * 16 + (size_t)al::SEL_CACHE * sizeof(AlPt);
    static AttrMask attr_sel = 0;
    set_max_dynamic_lds(reinterpret_cast<const void*>(align_select_kernel), (int)lds, attr_sel);
    align_select_kernel<<<P, 256, lds, st>>>(a);
    return 0;
}

}  // namespace xfh
