// Guided matching: mutual nearest neighbours among the candidates that agree with a known two-view model (xfh_match_mnn_guided).
//
// The sweep is the exact kernel's (k_match.hip: 256 rows of D1 per workgroup, A fragments stationary, D2 staged through LDS 128 columns at a
// time, S = D1.D2^T produced tile by tile by v_mfma_f32_32x32x2_f32 and never stored) with ONE addition in front of its epilogue: element
// (i, j) is replaced by -inf unless key-point i of image 0 and key-point j of image 1 pass the gate.  Everything behind that is unchanged --
// running row maxima with strict >, one packed column key per lane per tile, 64-bit atomic max in L2, lowest index on ties -- so the keys
// have the layout of k_match.hip and its finalize kernel serves both (it rejects a row key whose value is -inf: a row nothing passed in).
//
// A separate file rather than a gate policy templated into mnn_sim_kernel: the exact kernel is the reference behind the shipped filter and
// the yardstick of its tests and timings; its code object stays byte for byte what it was, and the gate's registers and LDS (6 KB of
// constants) are paid by the guided kernel alone.
//
// Gate arithmetic (include/xfeat_hip.h has the contract).  guided_prep_kernel computes, once per call, in fp64 from the fp64 model:
//   fundamental  row i: l = M (x0_i, 1) / max|M|, (l0, l1, l2, thr^2 (l0^2 + l1^2))      column j: (x, y, thr^2 (m0^2 + m1^2)), m = M' (x1_j, 1) / max|M|
//   homography   row i: (U, V) = dehom(H (x0_i, 1))                                      column j: (x, y)
// rounded to fp32.  Per element, in fp32:  e = (l0 x + l1 y) + l2, pass iff e e <= rho' + gamma'   /   du = U - x, dv = V - y, pass iff du du + dv dv <= thr^2.
// Rows that may pass nothing (invalid model, w ~ 0) carry NaN constants: every comparison with them is false.  Padding lanes (rows >= n1, columns >= n2)
// load the constants of the last valid row / column, like their descriptors, so they tie with it and lose to its lower index.
#include <cfloat>
#include "../../include/xfeat_hip.h"
#include "kernels.hpp"

namespace xfh {

// ---- guided kernels begin
typedef float gm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int GM_ROWS = 256;   // rows of D1 per workgroup (8 waves x 32): k_match.hip's MT_ROWS
constexpr int GM_COLS = 128;   // columns of D2 per LDS fill
constexpr int GM_DS = 68;      // LDS row stride in floats
constexpr int GM_PREP = 256;   // points per workgroup of the prep kernel

__device__ inline int gpair_count(const int32_t* n, int idx, int cap) {
    if (!n) return cap;
    const int v = n[idx];
    return v < 0 ? 0 : (v > cap ? cap : v);
}

__device__ inline bool gm_finite(double v) { return fabs(v) <= DBL_MAX; }      // (false for NaN too)

// grid P * nb, block GM_PREP: thread t of pair p writes the constants of row t (t < n1) and of column t (t < n2)
__global__ __launch_bounds__(GM_PREP) void guided_prep_kernel(const float* __restrict__ k1, size_t ks1, const float* __restrict__ k2, size_t ks2,
                                                              const int32_t* __restrict__ n1p, const int32_t* __restrict__ n2p, int n_stride, int n_off2,
                                                              int N1, int N2, int nb, const double* __restrict__ models, int kind, double thr2,
                                                              float4* __restrict__ rowc, float4* __restrict__ colc) {
    const int p = blockIdx.x / nb;
    const int t = (blockIdx.x - p * nb) * GM_PREP + threadIdx.x;
    const int n1 = gpair_count(n1p, p * n_stride, N1);
    const int n2 = gpair_count(n2p, p * n_stride + n_off2, N2);
    double M[9], mx = 0.0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        M[i] = models[(size_t)p * 9 + i];
        ok = ok && gm_finite(M[i]);
        mx = fmax(mx, fabs(M[i]));
    }
    ok = ok && mx > 0.0;      // an all-zero model is "nothing found", not "everything passes"
    const float qn = __uint_as_float(0x7fc00000u);
    if (t < n1) {
        const double x = (double)k1[(size_t)p * ks1 + 2 * (size_t)t], y = (double)k1[(size_t)p * ks1 + 2 * (size_t)t + 1];
        float4 c = make_float4(qn, qn, qn, qn);
        if (kind == XFH_GUIDE_FUNDAMENTAL) {
            if (ok) {
                const double l0 = (M[0] * x + M[1] * y + M[2]) / mx, l1 = (M[3] * x + M[4] * y + M[5]) / mx, l2 = (M[6] * x + M[7] * y + M[8]) / mx;
                c = make_float4((float)l0, (float)l1, (float)l2, (float)(thr2 * (l0 * l0 + l1 * l1)));
            }
        } else {
            const double w = M[6] * x + M[7] * y + M[8];
            if (ok && gm_finite(w) && fabs(w) > DBL_EPSILON * sqrt(M[6] * M[6] + M[7] * M[7] + M[8] * M[8]))
                c = make_float4((float)((M[0] * x + M[1] * y + M[2]) / w), (float)((M[3] * x + M[4] * y + M[5]) / w), 0.f, 0.f);
        }
        rowc[(size_t)p * N1 + t] = c;
    }
    if (t < n2) {
        const float xf = k2[(size_t)p * ks2 + 2 * (size_t)t], yf = k2[(size_t)p * ks2 + 2 * (size_t)t + 1];
        float g = 0.f;
        if (kind == XFH_GUIDE_FUNDAMENTAL) {
            const double x = (double)xf, y = (double)yf;
            const double m0 = (M[0] * x + M[3] * y + M[6]) / mx, m1 = (M[1] * x + M[4] * y + M[7]) / mx;
            g = ok ? (float)(thr2 * (m0 * m0 + m1 * m1)) : qn;
        }
        colc[(size_t)p * N2 + t] = make_float4(xf, yf, g, 0.f);
    }
}

// 512 threads = 8 waves, 32 rows of D1 each; grid and mapping of mnn_sim_kernel.  KIND 0: fundamental, 1: homography.
template <int KIND>
__global__ __launch_bounds__(512, 4) void mnn_guided_kernel(const float* __restrict__ d1, size_t ps1, const float* __restrict__ d2, size_t ps2,
                                                         const int32_t* __restrict__ n1p, const int32_t* __restrict__ n2p, int n_stride, int n_off2,
                                                         int N1, int N2, int nrb, int P, const float4* __restrict__ rowc,
                                                         const float4* __restrict__ colc, float thr2, unsigned long long* __restrict__ rowkey,
                                                         unsigned long long* __restrict__ colbest_g) {
    __shared__ __attribute__((aligned(16))) float Dl[GM_COLS * GM_DS];
    __shared__ unsigned long long colbest[8][GM_COLS];
    __shared__ __attribute__((aligned(16))) float4 Rl[GM_ROWS];
    __shared__ __attribute__((aligned(16))) float4 Cl[GM_COLS];

    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int p, rb;
    if (!xcd_group_map(blockIdx.x, nrb, P, p, rb)) return;
    const int n1 = gpair_count(n1p, p * n_stride, N1);
    const int n2 = gpair_count(n2p, p * n_stride + n_off2, N2);
    const int row0 = rb * GM_ROWS;
    if (n1 <= 0 || n2 <= 0 || row0 >= n1) return;
    const float* A = d1 + (size_t)p * ps1;
    const float* Bm = d2 + (size_t)p * ps2;
    const int wrow0 = row0 + wave * 32;

    // row constants of the workgroup's 256 rows (clamped like the descriptor rows below); the first barrier of the column loop publishes them
    if (tid < GM_ROWS) Rl[tid] = rowc[(size_t)p * N1 + min(row0 + tid, n1 - 1)];

    // stationary A fragment (32 rows x K=64): step s uses k = s (lanes 0-31) / k = 32+s (lanes 32-63)
    float a[32];
    {
        const int row = min(wrow0 + l31, n1 - 1);
        const float4* src = reinterpret_cast<const float4*>(A + (size_t)row * 64 + 32 * half);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 v = src[q];
            a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
        }
    }
    // running row maxima per (lane, row) and the 32-column tile they were found in, two 16-bit tile numbers per register (the column is tile * 32 + l31;
    // N2 <= 2^21).  Full column numbers, as mnn_sim_kernel keeps them, are 8 registers more: with the gate's constants in flight that is past 128, and spills.
    float bv[16];
    unsigned bt[8];
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[r] = -INFINITY;
#pragma unroll
    for (int r = 0; r < 8; ++r) bt[r] = 0u;

    for (int c0 = 0; c0 < n2; c0 += GM_COLS) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * 512;
            const int col = e >> 4, q = e & 15;
            const int gc = min(c0 + col, n2 - 1);
            const float4 v = *reinterpret_cast<const float4*>(Bm + (size_t)gc * 64 + 4 * q);
            *reinterpret_cast<float4*>(Dl + col * GM_DS + 4 * q) = v;
        }
        if (tid < GM_COLS) Cl[tid] = colc[(size_t)p * N2 + min(c0 + tid, n2 - 1)];
        __syncthreads();
#pragma unroll 1
        for (int ct = 0; ct < GM_COLS / 32; ++ct) {
            const int cbase = c0 + ct * 32;
            if (cbase >= n2) break;
            const float4* bp = reinterpret_cast<const float4*>(Dl + (ct * 32 + l31) * GM_DS + 32 * half);
            gm_f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int hq = 0; hq < 2; ++hq) {
                float bf[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = bp[hq * 4 + q];
                    bf[4 * q + 0] = v.x; bf[4 * q + 1] = v.y; bf[4 * q + 2] = v.z; bf[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[hq * 16 + s], bf[s], acc, 0, 0, 0);
            }
            // D[i=row][j=col]: this lane holds column cbase+l31, rows (r&3)+8*(r>>2)+4*half of the wave's 32.
            // The gate: the column's constants sit in the lane that owns the column, the rows' constants are LDS broadcasts (all lanes of a half read one address).
            const float4 cc = Cl[ct * 32 + l31];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                bool pass;
                if (KIND == XFH_GUIDE_FUNDAMENTAL) {
                    const float4 rc = Rl[ri];
                    const float e = (rc.x * cc.x + rc.y * cc.y) + rc.z;
                    pass = e * e <= rc.w + cc.z;
                } else {
                    const float2 rc = *reinterpret_cast<const float2*>(&Rl[ri]);
                    const float du = rc.x - cc.x, dv = rc.y - cc.y;
                    pass = du * du + dv * dv <= thr2;
                }
                acc[r] = pass ? acc[r] : -INFINITY;
                __builtin_amdgcn_sched_barrier(0);      // one row's constants in flight at a time: hoisted together they are 64 VGPRs, and the kernel spills
            }
            // from here on: mnn_sim_kernel's epilogue (the row maxima remember their tile, not their column).  No validity masks: rows >= n1 and columns >= n2 are copies of the last valid row / column, descriptor and
            // key-point constants alike, so they tie with it and lose every first-index tie-break.
            const unsigned tt = (unsigned)(cbase >> 5) * 0x10001u;      // the tile's number in both halves
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[r];
                if (v > bv[r]) {
                    bv[r] = v;
                    bt[r >> 1] = (r & 1) ? ((bt[r >> 1] & 0x0000ffffu) | (tt & 0xffff0000u)) : ((bt[r >> 1] & 0xffff0000u) | (tt & 0x0000ffffu));
                }
            }
            float cm = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) cm = fmaxf(cm, acc[r]);
            int crow = 0x7fffffff;
#pragma unroll
            for (int r = 15; r >= 0; --r)
                if (acc[r] == cm) crow = wrow0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            unsigned long long best = ((unsigned long long)float_ord(cm) << 32) | (0xffffffffu - (unsigned)crow);
            best = u64_max(best, xhalf_u64(best));
            if (half == 0) colbest[wave][ct * 32 + l31] = best;
        }
        __syncthreads();
        if (tid < GM_COLS) {
            const int col = c0 + tid;
            if (col < n2) {
                unsigned long long k = colbest[0][tid];
#pragma unroll
                for (int w = 1; w < 8; ++w) k = u64_max(k, colbest[w][tid]);
                atomicMax(&colbest_g[(size_t)p * N2 + col], k);
            }
        }
    }

    // row arg-max: reduce the per-lane running maxima over the 32 lanes that share the rows (a row nothing passed in keeps -inf: the finalize rejects it)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned bc = ((bt[r >> 1] >> (16 * (r & 1))) & 0xffffu) * 32u + (unsigned)l31;
        unsigned long long key = ((unsigned long long)float_ord(bv[r]) << 32) | (0xffffffffu - bc);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) key = u64_max(key, shfl_xor_u64(key, o));
        const int row = wrow0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (l31 == 0 && row < n1) rowkey[(size_t)p * N1 + row] = key;
    }
}
// ---- guided kernels end

void launch_match_guided(const GuidedWs& ws, const float* d1, size_t ps1, const float* d2, size_t ps2, const float* k1, size_t ks1, const float* k2, size_t ks2,
                         const int32_t* n1, const int32_t* n2, int n_stride, int n_off2, int P, int N1, int N2, const double* models, int kind, double thr,
                         float min_cossim, int64_t* idx0, int64_t* idx1, int32_t* n_matches, hipStream_t st) {
    const int nrb = ceil_div(N1, GM_ROWS);
    (void)hipMemsetAsync(ws.zeroed, 0, ws.zeroed_bytes, st);   // keys: 0 = below everything
    const int nb = ceil_div(N1 > N2 ? N1 : N2, GM_PREP);
    guided_prep_kernel<<<P * nb, GM_PREP, 0, st>>>(k1, ks1, k2, ks2, n1, n2, n_stride, n_off2, N1, N2, nb, models, kind, thr * thr, ws.rowc, ws.colc);
    const float thr2 = (float)(thr * thr);
    if (kind == XFH_GUIDE_FUNDAMENTAL)
        mnn_guided_kernel<XFH_GUIDE_FUNDAMENTAL><<<xcd_grid_size(nrb, P), 512, 0, st>>>(d1, ps1, d2, ps2, n1, n2, n_stride, n_off2, N1, N2, nrb, P, ws.rowc, ws.colc,
                                                                                        thr2, ws.rowkey, ws.colkey);
    else
        mnn_guided_kernel<XFH_GUIDE_HOMOGRAPHY><<<xcd_grid_size(nrb, P), 512, 0, st>>>(d1, ps1, d2, ps2, n1, n2, n_stride, n_off2, N1, N2, nrb, P, ws.rowc, ws.colc,
                                                                                       thr2, ws.rowkey, ws.colkey);
    launch_match_finalize(ws.rowkey, ws.colkey, n1, n2, n_stride, n_off2, P, N1, N2, min_cossim, idx0, idx1, n_matches, st);
}

}  // namespace xfh
