// RANSAC scaffolding shared by the three two-view estimators: k_homography.hip (4 points, MAGSAC++ quality), k_relpose.hip (5 points,
// MSAC cost) and k_fundamental.hip (7 points, MAGSAC++ quality).  This file IS the common part of their specification; the three numpy
// restatements that the test suite holds the estimators to (one per estimator, independent of each other) repeat it operation for operation:
//   * draws: draw d of hypothesis `it` of pair p is the upper half of splitmix64-finaliser(seed + golden * (((p << 20) + it) * 16 + d + 1))
//     scaled to [0, n); a sample is M distinct indices in draw order, duplicates are redrawn, 16 draws at most (draw_index,
//     sample_distinct); a sample that runs out of draws yields no model;
//   * a hypothesis with several candidate models counts with its best one, the lower index on ties (hyp_best);
//   * stopping rule: hypotheses in order; a strictly better value makes a new best and bounds the loop by
//     ceil(log(1 - confidence) / log(1 - w^M)), w = the best's inlier ratio, w^M multiplied left to right (iterations_needed); the loop
//     stops at it >= max(min_iters, bound) (scan_stopping_rule; the homography applies the same rule to its whole list at once);
//   * the first 256 hypotheses of every pair are built and scored first; the records among them bound the index the loop can still
//     reach, and the later blocks run only below that bound (hypotheses_bound);
//   * floating-point totals over a workgroup are taken in one fixed order (block_sums), so that they are reproducible.
// A hypothesis is a function of (seed, pair, it) alone: that is what lets every hypothesis be built and scored at once and the
// sequential loop's stopping rule be applied to the list of values afterwards.
// Device code only (LDS, barriers); the host-compilable geometry is in twoview_math.hpp.
#pragma once
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace xfh {
namespace rs {
constexpr int MAX_DRAWS = 16, NBINS = 4096;                    // NBINS: bins of the MAGSAC++ tables (homog_tables_kernel)
constexpr int HYP_PER_WG = 256, PTS_PER_WG = 512;              // score kernels: hypotheses x correspondences of one workgroup
constexpr int SEL_TILE = 2048, SEL_CACHE = 2048;               // select kernels: list entries per LDS tile, correspondences kept in LDS
constexpr int RED_PITCH = 257;

// ---- the correspondences of one pair --------------------------------------------------------------------------------------------------
// Args (HgArgs / RpArgs / FmArgs) carry p0, p1 (P, kcap, 2), idx0, idx1 (P, cap) or NULL, counts or NULL, n_const, cap, kcap
struct PairView {
    const float* p0;
    const float* p1;
    const int64_t* i0;
    const int64_t* i1;
    template <class Args>
    __device__ PairView(const Args& a, int pair)
        : p0(a.p0 + (size_t)pair * a.kcap * 2), p1(a.p1 + (size_t)pair * a.kcap * 2), i0(a.idx0 ? a.idx0 + (size_t)pair * a.cap : nullptr),
          i1(a.idx1 ? a.idx1 + (size_t)pair * a.cap : nullptr) {}
    // (x0, y0, x1, y1) of correspondence i, through the index lists when given
    __device__ inline float4 get(int i) const {
        const size_t r0 = i0 ? (size_t)i0[i] : (size_t)i, r1 = i1 ? (size_t)i1[i] : (size_t)i;
        const float2 q0 = *reinterpret_cast<const float2*>(p0 + 2 * r0);
        const float2 q1 = *reinterpret_cast<const float2*>(p1 + 2 * r1);
        return make_float4(q0.x, q0.y, q1.x, q1.y);
    }
};
template <class Args>
__device__ inline int pair_count(const Args& a, int pair) { return a.counts ? min(max(a.counts[pair], 0), a.cap) : a.n_const; }

// ---- draws ----------------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ inline int draw_index(unsigned long long seed, int pair, int it, int draw, int n) {
    const unsigned long long counter = ((unsigned long long)pair * (1ull << 20) + (unsigned long long)it) * MAX_DRAWS + (unsigned long long)draw;
    const unsigned long long h = mix64(seed + 0x9e3779b97f4a7c15ull * (counter + 1ull));
    return (int)(((h >> 32) * (unsigned long long)n) >> 32);
}
// the M distinct indices of hypothesis `it` into idx; false when the draws ran out.  (Select-by-compare: no runtime index into idx, which
// stays in registers.)
template <int M>
__device__ inline bool sample_distinct(unsigned long long seed, int pair, int it, int n, int (&idx)[M]) {
    int slot = 0;
#pragma unroll
    for (int d = 0; d < MAX_DRAWS; ++d) {
        const int c = draw_index(seed, pair, it, d, n);
        bool dup = false;
#pragma unroll
        for (int k = 0; k < M - 1; ++k) dup |= (slot > k) & (c == idx[k]);      // (no short circuit: branch-free)
        if (slot < M && !dup) {
#pragma unroll
            for (int k = 0; k < M; ++k) idx[k] = slot == k ? c : idx[k];
            ++slot;
        }
    }
    return slot == M;
}

// bin of r^2 in the MAGSAC++ tables
__device__ inline int bin_of(double r2, double bin_scale) {
    const int b = (int)(r2 * bin_scale);
    return b < NBINS - 1 ? b : NBINS - 1;
}

// ---- the loop's bound -----------------------------------------------------------------------------------------------------------------
// iterations the loop still needs once a model with `inliers` of n is the best one (the standard RANSAC bound for samples of M)
template <int M>
__device__ inline int iterations_needed(unsigned inliers, int n, double log1mc, int max_iters) {
    const double w = (double)inliers / (double)n;
    double wm = w;
#pragma unroll
    for (int k = 1; k < M; ++k) wm = wm * w;
    const double p = 1.0 - wm;
    if (p <= 0.0) return 1;
    if (p >= 1.0) return max_iters;
    const double k = ceil(log1mc / log(p));
    return k < (double)max_iters ? (int)k : max_iters;
}

template <bool LOWER>
__device__ inline bool better(unsigned long long v, unsigned long long than) { return LOWER ? v < than : v > than; }
template <bool LOWER>
__device__ inline unsigned long long worst() { return LOWER ? ~0ull : 0ull; }     // what no model is better than

// value of hypothesis h = the best of its candidates' (the lower index on ties) and that candidate's inlier count; false: no model.
// `stride`: entries per candidate in hval / hcnt (k_relpose.hip's threshold sweep keeps one per threshold and passes the lists offset
// to its own)
template <int MAX_CAND, bool LOWER>
__device__ inline bool hyp_best(const int* ncand, const unsigned long long* hval, const unsigned* hcnt, size_t h, unsigned long long& val,
                                unsigned& cnt, int& cand, size_t stride = 1) {
    const int nc = ncand[h];
    if (nc <= 0) return false;
    val = hval[h * MAX_CAND * stride];
    cnt = hcnt[h * MAX_CAND * stride];
    cand = 0;
    for (int c = 1; c < nc; ++c) {
        const unsigned long long v = hval[(h * MAX_CAND + c) * stride];
        if (better<LOWER>(v, val)) { val = v; cnt = hcnt[(h * MAX_CAND + c) * stride]; cand = c; }
    }
    return true;
}
template <int MAX_CAND>
__device__ inline void zero_hypotheses(int* ncand, unsigned long long* hval, unsigned* hcnt, size_t nhyp) {
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < nhyp; j += (size_t)gridDim.x * 256) {
        ncand[j] = 0;
#pragma unroll
        for (int c = 0; c < MAX_CAND; ++c) { hval[j * MAX_CAND + c] = 0ull; hcnt[j * MAX_CAND + c] = 0u; }
    }
}

// After the first 256 hypotheses (thread = hypothesis; has / val / cnt: its model, value and inlier count): an upper bound of the index
// the sequential loop stops at = min over the records (strict prefix optima of the value) among them of iterations_needed.  If the loop
// stops inside the first 256 the value does not matter (no later hypothesis is visited); if it does not, every record among the first 256
// is one the loop sees, so its own bound is <= this one.  Valid on every thread.
template <int M, bool LOWER>
__device__ inline int hypotheses_bound(bool has, unsigned long long val, unsigned cnt, int n, double log1mc, int iters) {
    __shared__ unsigned long long sc[256];
    __shared__ int bmin;
    const int tid = threadIdx.x;
    sc[tid] = has ? val : worst<LOWER>();
    if (tid == 0) bmin = iters;
    __syncthreads();
    unsigned long long before = worst<LOWER>();
    for (int j = 0; j < tid; ++j) before = better<LOWER>(sc[j], before) ? sc[j] : before;
    if (has && better<LOWER>(val, before)) atomicMin(&bmin, iterations_needed<M>(cnt, n, log1mc, iters));
    __syncthreads();
    return bmin;
}

// The stopping rule of the sequential loop over the list of hypothesis values, in tiles of SEL_TILE entries in LDS (`tiles`: SEL_TILE * 16
// bytes): all threads fetch a tile (hyp(it, val, cnt, cand) -> has a model), thread 0 walks it.  Every thread gets the winner (-1: none),
// its candidate and the number of iterations the loop ran.  Ends with a barrier; `tiles` is free afterwards.
template <int M, bool LOWER, class Hyp>
__device__ inline void scan_stopping_rule(unsigned char* tiles, int n, int iters, int min_iters, double log1mc, Hyp&& hyp, int& best, int& best_cand,
                                          int& iters_run) {
    __shared__ int sel[4];
    __shared__ unsigned long long best_sh;
    __shared__ int stop_sh, done_sh;
    const int tid = threadIdx.x;
    unsigned long long* tq = reinterpret_cast<unsigned long long*>(tiles);
    unsigned* tn = reinterpret_cast<unsigned*>(tiles + (size_t)SEL_TILE * 8);
    int* tk = reinterpret_cast<int*>(tiles + (size_t)SEL_TILE * 12);
    if (tid == 0) { sel[0] = -1; sel[1] = 0; sel[2] = -1; best_sh = worst<LOWER>(); stop_sh = iters; done_sh = n < M ? 1 : 0; }
    __syncthreads();
    for (int base = 0; base < iters; base += SEL_TILE) {
        if (done_sh) break;
        for (int i = tid; i < SEL_TILE; i += 256) {
            const int it = base + i;
            unsigned long long v = worst<LOWER>();
            unsigned k = 0;
            int cd = -1;
            if (it < iters && it < (stop_sh > min_iters ? stop_sh : min_iters) && !hyp(it, v, k, cd)) cd = -1;
            tq[i] = v; tn[i] = k; tk[i] = cd;
        }
        __syncthreads();
        if (tid == 0) {
            int it = base;
            int stop = stop_sh;
            for (; it < iters && it < base + SEL_TILE; ++it) {
                if (it >= (stop > min_iters ? stop : min_iters)) { done_sh = 1; break; }
                const int i = it - base;
                if (tk[i] >= 0 && better<LOWER>(tq[i], best_sh)) {
                    best_sh = tq[i]; sel[0] = it; sel[2] = tk[i];
                    const int need = iterations_needed<M>(tn[i], n, log1mc, iters);
                    stop = need < stop ? need : stop;
                }
            }
            sel[1] = it;
            stop_sh = stop;
            if (it >= iters) done_sh = 1;
        }
        __syncthreads();
    }
    __syncthreads();
    best = sel[0]; best_cand = sel[2]; iters_run = n < M ? 0 : sel[1];
}

// ---- fixed-order sums -----------------------------------------------------------------------------------------------------------------
// Totals of N per-thread values over the 256 threads of the workgroup, every thread gets them; the order of the additions is fixed: 8
// segments of 32 threads per value, each added in index order, then the tree ((q0+q1)+(q2+q3))+((q4+q5)+(q6+q7)) over the 8.  Through LDS
// as a transpose: thread (k, j) adds 32 of the 256 entries of row k, thread k the 8 partial sums -- ~40 dependent additions and four
// barriers.  (A butterfly of wave shuffles costs 6 steps x 2 ds_bpermute per value, each waited for: with it the homography's select
// kernel took 76-84 us instead of 52.)
template <int N>
__device__ inline void block_sums(double (&v)[N], double* buf /* N * RED_PITCH + 9 * N doubles */) {
    const int tid = threadIdx.x;
    double* part = buf + N * RED_PITCH;
    double* tot = part + N * 8;
    __syncthreads();                                       // buf free (previous use)
#pragma unroll
    for (int k = 0; k < N; ++k) buf[k * RED_PITCH + tid] = v[k];
    __syncthreads();
    for (int r = tid; r < N * 8; r += 256) {
        const int k = r >> 3, j = r & 7;
        const double* row = buf + k * RED_PITCH + j * 32;
        double t = 0.0;
        for (int i = 0; i < 32; ++i) t += row[i];            // (unrolled in full by the compiler: all 32 LDS reads issued before the first addition)
        part[r] = t;
    }
    __syncthreads();
    for (int k = tid; k < N; k += 256) {
        const double* q = part + k * 8;
        tot[k] = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7])));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = tot[k];
}
constexpr size_t block_sums_bytes(int n) { return ((size_t)n * RED_PITCH + 9 * (size_t)n) * sizeof(double); }

// Hartley conditioning of both point sets of a pair: centroids c, then s = sqrt(2) / (mean distance to c) (1 for coincident points), from
// block sums; each(f) calls f(i, float4 correspondence) for this thread's correspondences.  o = cx0 cy0 s0 cx1 cy1 s1, on every thread.
template <class Each>
__device__ inline void hartley_conditioning(Each&& each, double dn, double* red /* block_sums buffer for 4 */, double (&o)[6]) {
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    each([&](int, const float4& q) { c[0] += q.x; c[1] += q.y; c[2] += q.z; c[3] += q.w; });
    block_sums(c, red);
    const double cx0 = c[0] / dn, cy0 = c[1] / dn, cx1 = c[2] / dn, cy1 = c[3] / dn;
    double dd[2] = {0.0, 0.0};
    each([&](int, const float4& q) {
        const double ax = q.x - cx0, ay = q.y - cy0, bx = q.z - cx1, by = q.w - cy1;
        dd[0] += sqrt(ax * ax + ay * ay);
        dd[1] += sqrt(bx * bx + by * by);
    });
    block_sums(dd, red);
    o[0] = cx0; o[1] = cy0; o[2] = dd[0] > 0.0 ? 1.41421356237309504880 / (dd[0] / dn) : 1.0;
    o[3] = cx1; o[4] = cy1; o[5] = dd[1] > 0.0 ? 1.41421356237309504880 / (dd[1] / dn) : 1.0;
}

// ---- the select kernels' common ends ----------------------------------------------------------------------------------------------------
// this thread's correspondences tid, tid + 256, ... of the pair's n: the first SEL_CACHE from the LDS copy `spt` (every pass otherwise pays
// the index -> key-point round trip again), the rest through get(i)
template <class V, class Get, class F>
__device__ inline void for_each_cached(const V* spt, int n, Get&& get, F&& f) {
    for (int i = threadIdx.x; i < n; i += 256) f(i, i < SEL_CACHE ? spt[i] : get(i));
}
// nothing found: mask zeroed, info = (0, -1, iters_run, 0, 0, n, 0, 0); the model outputs are the caller's
__device__ inline void write_nothing_found(unsigned char* mask, int cap, int32_t* info, int iters_run, int n) {
    const int tid = threadIdx.x;
    for (int i = tid; i < cap; i += 256) mask[i] = 0;
    if (tid < 8) info[tid] = tid == 2 ? iters_run : (tid == 1 ? -1 : (tid == 5 ? n : 0));
}
// the 8 info words (one thread)
__device__ inline void write_info(int32_t* info, bool found, int best, int iters_run, int n_in, int lo_accepted, int n, unsigned long long value) {
    info[0] = found ? 1 : 0; info[1] = best; info[2] = iters_run; info[3] = n_in; info[4] = lo_accepted; info[5] = n;
    info[6] = (int)(value & 0xffffffffull); info[7] = (int)(value >> 32);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// correspondences per workgroup of a score kernel: few pairs take smaller chunks, so that one pair still spreads over the chip (integer
// scores: any split gives the same sums)
inline int score_chunk(int P, int cap) {
    int chunk = PTS_PER_WG;
    while (chunk > 64 && (long)P * ceil_div(cap, chunk) < 256) chunk >>= 1;
    return chunk;
}
}  // namespace rs
}  // namespace xfh
