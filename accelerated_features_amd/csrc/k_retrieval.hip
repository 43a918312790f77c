// Image retrieval: VLAD global descriptors over a k-means codebook of the local descriptors, top-k shortlists from the inner
// products of the global vectors, pair lists from the shortlists.  tests/retrieval_reference.py restates every kernel operation by operation and
// tests/test_retrieval_emulated.py compiles the slice below for the host (tests/emu/retrieval_emu.cpp).  Only + - * / sqrt in fp32 (the k-means
// objective in fp64), fp contraction off, every sum in one order that the shapes fix; no floating-point atomic (the only atomics are integer
// counters and bit sets in LDS), and no order depends on scheduling or on the launch shape: two calls give the same bytes.
// The inner products run on the vector ALUs, not on v_mfma_f32_32x32x2_f32: a score is then a chain of individually rounded fp32 operations that
// numpy repeats bit for bit, where the matrix core's own rounding of a two-product step would have to be modelled.
//
// dot64(x, c) = (((0 + x0 c0) + x1 c1) + ...) + x63 c63: every product rounded, then added.  Depth 64.
// retr_assign_kernel: row i of group g is VALID iff i < clamp(counts[g], 0, Kcap) and its 64 components are finite.  assign = the c with the
//   largest dot64(row, codebook[c]) among the FINITE scores, the lowest c among equals; -1 for a row that is not valid or has no finite score.
//   w_score = the winning score (NaN: none); w_state = 0 beyond the count, 1 valid, 2 below the count but not finite.
// retr_sums_kernel: the rows of a group are cut into chunks of rt::CHUNK = 1024 consecutive rows (the cut depends on the row index alone).
//   partial[chunk, c] = ((0 + t_i0) + t_i1) + ... over the rows of the chunk with assign == c ascending, t_i = row_i (k-means) or
//   row_i - codebook[c] (VLAD; the difference rounded first), per component; count[chunk, c] likewise.
//   objective partial of a chunk (fp64): lane t of 256 adds the winning scores of rows 4 t .. 4 t + 3 of the chunk ascending onto 0 (a row
//   without a cluster adds 0); then p[t] = p[t] + p[t + h] for h = 128, 64, ..., 1.
// retr_vlad_finish_kernel / retr_kmeans_finish_kernel: sum[c] = ((0 + partial[0, c]) + partial[1, c]) + ... over the chunks ascending.
//   n2 of a 64-block: the lane partials and the 16-lane butterfly of k_map.hip.  ok = n2 finite and >= FLT_MIN.
//   VLAD: block = ok ? sum * (1 / sqrt(n2)) : 0; m = the number of ok blocks; vlad = block * (1 / sqrt((float)m)); m = 0: all zero, info[3] = 1.
//     info: valid rows, rows below the count that are not finite, m, m == 0.
//   k-means: codebook_out[c] = ok ? sum * (1 / sqrt(n2)) : codebook[c]; objective = ((0 + o_0) + o_1) + ... over the chunks' partials (fp64).
//     info: valid rows, rows below the count that are not finite, clusters that kept their centroid, 0.  The G Kcap rows are ONE sequence here.
// retr_score_kernel: score(q, d) over D = 64 B components: b_i = dot64 of block i; s_j = ((0 + b_16j) + b_16j+1) + ... over the (up to) 16
//   blocks of segment j; score = ((0 + s_0) + s_1) + ...  Depth 64 + 16 + 16 = 96.
// retr_topk_kernel: among the rows i < clamp(n_db, 0, N) with a finite score (i != the query's index with exclude_self): score descending, then
//   index ascending (-0 counts as +0); the first k.  Entries past the number found: idx -1, score NaN.
// retr_pairs_kernel: the undirected union of the edges (v, idx[v, j]) with v, idx < clamp(n_views, 0, V), idx >= 0, idx != v as pairs a < b in
//   ascending (a, b) order, then (-1, -1).
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace xfh {

// ---- retrieval begin (host-compilable with tests/emu/emu.hpp: tests/test_retrieval_emulated.py slices it out) ----
namespace rt {
constexpr int CHUNK = 1024;                                // rows of one partial sum
constexpr int SEG = 16;                                    // 64-blocks of one segment of a score
constexpr int TILE = 64;                                   // queries and database rows of one workgroup of retr_score_kernel
constexpr int LDS_STRIDE = 68;                             // floats between two rows of a tile in LDS (16-byte aligned, 4 banks apart)
constexpr int MAX_K = 128, MAX_D = 16384, MAX_VIEWS = 32, MAX_C = 256;
constexpr float NORM_MIN = 1.17549435e-38f;                // FLT_MIN
constexpr unsigned NAN_BITS = 0x7fc00000u;
}  // namespace rt

__device__ inline bool rt_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ inline int rt_clamp(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

struct RetrAssignArgs {
    const float* desc;               // (G, K, 64)
    const int32_t* counts;           // (G,) or null: K
    const float* codebook;           // (C, 64)
    int K, C;
    long long total;                 // G K
    int32_t* assign;                 // (G, K)
    float* w_score;                  // (G, K) or null
    unsigned char* w_state;          // (G, K)
};

__global__ __launch_bounds__(256) void retr_assign_kernel(RetrAssignArgs a) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.total) return;
    const int g = (int)(r / a.K), i = (int)(r - (long long)g * a.K);
    const int n = rt_clamp(a.counts ? a.counts[g] : a.K, a.K);
    float x[64];
    bool fin = i < n;
    if (i < n) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float4 d = *reinterpret_cast<const float4*>(a.desc + (size_t)r * 64 + u * 4);
            x[4 * u] = d.x; x[4 * u + 1] = d.y; x[4 * u + 2] = d.z; x[4 * u + 3] = d.w;
            fin = fin && rt_finite(d.x) && rt_finite(d.y) && rt_finite(d.z) && rt_finite(d.w);
        }
    }
    int best = -1;
    float bs = 0.f;
    if (fin) {
        for (int c = 0; c < a.C; ++c) {
            const float* cb = a.codebook + (size_t)c * 64;  // (the same address in every lane)
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 64; ++j) s = s + x[j] * cb[j];
            if (rt_finite(s) && (best < 0 || s > bs)) { best = c; bs = s; }
        }
    }
    a.assign[r] = best;
    if (a.w_score) a.w_score[r] = best >= 0 ? bs : __uint_as_float(rt::NAN_BITS);
    a.w_state[r] = (unsigned char)(i >= n ? 0 : (fin ? 1 : 2));
}

struct RetrSumArgs {
    const float* desc;               // (groups, rows, 64)
    const int32_t* assign;           // (groups, rows)
    const float* codebook;           // (C, 64)
    const float* w_score;            // (groups, rows); read when w_obj is set
    int rows, nchunks, C, residual;
    float* w_part;                   // (groups, nchunks, C, 64)
    int32_t* w_cnt;                  // (groups, nchunks, C)
    double* w_obj;                   // (groups, nchunks) or null
};

__global__ __launch_bounds__(256) void retr_sums_kernel(RetrSumArgs a) {
    __shared__ int s_assign[rt::CHUNK];
    __shared__ double s_obj[256];
    const int tid = threadIdx.x, sub = tid & 15;
    const int cgroups = a.C / 16;
    const int cg = blockIdx.x % cgroups, gc = blockIdx.x / cgroups;      // gc = group * nchunks + chunk
    const int chunk = gc % a.nchunks, g = gc / a.nchunks;
    const int c = cg * 16 + (tid >> 4);
    const size_t row0 = (size_t)g * a.rows + (size_t)chunk * rt::CHUNK;
    const int left = a.rows - chunk * rt::CHUNK, n = left < rt::CHUNK ? left : rt::CHUNK;
    for (int i = tid; i < rt::CHUNK; i += 256) s_assign[i] = i < n ? a.assign[row0 + i] : -1;
    __syncthreads();
    float4 cb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.residual) cb = *reinterpret_cast<const float4*>(a.codebook + (size_t)c * 64 + sub * 4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        if (s_assign[i] != c) continue;
        const float4 d = *reinterpret_cast<const float4*>(a.desc + (row0 + i) * 64 + sub * 4);
        acc.x = acc.x + (d.x - cb.x); acc.y = acc.y + (d.y - cb.y); acc.z = acc.z + (d.z - cb.z); acc.w = acc.w + (d.w - cb.w);
        ++cnt;
    }
    const size_t at = (size_t)gc * a.C + c;
    *reinterpret_cast<float4*>(a.w_part + at * 64 + sub * 4) = acc;
    if (sub == 0) a.w_cnt[at] = cnt;
    if (a.w_obj && cg == 0) {                              // (the same for the whole workgroup: the barriers below are met by all)
        double p = 0.0;
        for (int u = 0; u < 4; ++u) {
            const int i = tid * 4 + u;
            p = p + (i < n && s_assign[i] >= 0 ? (double)a.w_score[row0 + i] : 0.0);
        }
        s_obj[tid] = p;
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if (tid < h) s_obj[tid] = s_obj[tid] + s_obj[tid + h];
            __syncthreads();
        }
        if (tid == 0) a.w_obj[gc] = s_obj[0];
    }
}

// |v|^2 over the 16 lanes of a 64-block: the xor butterfly of map_gather_kernel (k_map.hip)
__device__ inline float rt_norm2(float4 v) {
    float n2 = ((v.x * v.x + v.y * v.y) + v.z * v.z) + v.w * v.w;
#define XFH_RT_DPP_ADD(ctrl) n2 = n2 + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(n2), ctrl, 0xf, 0xf, true))
    XFH_RT_DPP_ADD(0xb1);
    XFH_RT_DPP_ADD(0x4e);
    XFH_RT_DPP_ADD(0x141);
    XFH_RT_DPP_ADD(0x140);
#undef XFH_RT_DPP_ADD
    return n2;
}

struct RetrFinishArgs {
    const float* w_part;             // (groups, nchunks, C, 64)
    const int32_t* w_cnt;            // (groups, nchunks, C)
    const unsigned char* w_state;    // (groups, rows)
    const double* w_obj;             // (nchunks) (k-means)
    const float* codebook;           // (C, 64) (k-means)
    int rows, nchunks, C;
    float* out;                      // vlad (groups, C 64) / codebook_out (C, 64)
    int32_t* n_assigned;             // (groups, C)
    double* objective;               // one value (k-means)
    int32_t* info;                   // (groups, 4)
};

// sum of the chunk partials of cluster c of group g (one float4 per lane of 16), and the rows behind it
__device__ inline float4 rt_chunk_sum(const RetrFinishArgs& a, int g, int c, int sub, int& cnt) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    cnt = 0;
    for (int ch = 0; ch < a.nchunks; ++ch) {
        const size_t at = ((size_t)g * a.nchunks + ch) * a.C + c;
        const float4 p = *reinterpret_cast<const float4*>(a.w_part + at * 64 + sub * 4);
        acc.x = acc.x + p.x; acc.y = acc.y + p.y; acc.z = acc.z + p.z; acc.w = acc.w + p.w;
        cnt += a.w_cnt[at];
    }
    return acc;
}

// the states of the rows of group g into s_n[0] (valid) and s_n[1] (below the count, not finite)
__device__ inline void rt_count_rows(const RetrFinishArgs& a, int g, int tid, int* s_n) {
    int v = 0, bad = 0;
    for (int i = tid; i < a.rows; i += 256) {
        const int st = a.w_state[(size_t)g * a.rows + i];
        v += st == 1; bad += st == 2;
    }
    if (v) atomicAdd(&s_n[0], v);
    if (bad) atomicAdd(&s_n[1], bad);
}

__global__ __launch_bounds__(256) void retr_vlad_finish_kernel(RetrFinishArgs a) {
    __shared__ int s_n[4];
    const int g = blockIdx.x, tid = threadIdx.x, sub = tid & 15;
    if (tid < 4) s_n[tid] = 0;
    __syncthreads();
    rt_count_rows(a, g, tid, s_n);
    int mine = 0;
    for (int c0 = 0; c0 < a.C; c0 += 16) {                 // (C is a multiple of 16: no lane of a row of 16 is missing from the butterfly)
        const int c = c0 + (tid >> 4);
        int cnt;
        const float4 acc = rt_chunk_sum(a, g, c, sub, cnt);
        const float n2 = rt_norm2(acc);
        const bool ok = rt_finite(n2) && n2 >= rt::NORM_MIN;
        const float inv = ok ? 1.f / sqrtf(n2) : 0.f;
        const size_t to = ((size_t)g * a.C + c) * 64 + sub * 4;
        *reinterpret_cast<float4*>(a.out + to) = ok ? make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (sub == 0) {
            a.n_assigned[(size_t)g * a.C + c] = cnt;
            mine += ok;
        }
    }
    if (mine) atomicAdd(&s_n[2], mine);
    __syncthreads();
    const int m = s_n[2];
    if (m > 0) {
        const float scale = 1.f / sqrtf((float)m);
        for (int c0 = 0; c0 < a.C; c0 += 16) {             // (every lane scales the four values it wrote itself)
            const size_t to = ((size_t)g * a.C + c0 + (tid >> 4)) * 64 + sub * 4;
            const float4 v = *reinterpret_cast<const float4*>(a.out + to);
            *reinterpret_cast<float4*>(a.out + to) = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
        }
    }
    if (tid == 0) {
        int32_t* info = a.info + (size_t)g * 4;
        info[0] = s_n[0]; info[1] = s_n[1]; info[2] = m; info[3] = m == 0;
    }
}

__global__ __launch_bounds__(256) void retr_kmeans_finish_kernel(RetrFinishArgs a) {
    __shared__ int s_n[4];
    const int tid = threadIdx.x, sub = tid & 15;
    if (tid < 4) s_n[tid] = 0;
    __syncthreads();
    rt_count_rows(a, 0, tid, s_n);
    int mine = 0;
    for (int c0 = 0; c0 < a.C; c0 += 16) {
        const int c = c0 + (tid >> 4);
        int cnt;
        const float4 acc = rt_chunk_sum(a, 0, c, sub, cnt);
        const float n2 = rt_norm2(acc);
        const bool ok = rt_finite(n2) && n2 >= rt::NORM_MIN;   // (an empty cluster: n2 = 0)
        const float inv = ok ? 1.f / sqrtf(n2) : 0.f;
        const float4 old = *reinterpret_cast<const float4*>(a.codebook + (size_t)c * 64 + sub * 4);
        *reinterpret_cast<float4*>(a.out + (size_t)c * 64 + sub * 4) = ok ? make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv) : old;
        if (sub == 0) {
            a.n_assigned[c] = cnt;
            mine += !ok;
        }
    }
    if (mine) atomicAdd(&s_n[2], mine);
    __syncthreads();
    if (tid == 0) {
        double o = 0.0;
        for (int ch = 0; ch < a.nchunks; ++ch) o = o + a.w_obj[ch];
        a.objective[0] = o;
        a.info[0] = s_n[0]; a.info[1] = s_n[1]; a.info[2] = s_n[2]; a.info[3] = 0;
    }
}

struct RetrScoreArgs {
    const float* q;                  // (G, Q, D)
    const float* db;                 // (G, N, D)
    int Q, N, D, tq, tn;             // tq, tn: tiles of 64 queries / database rows
    float* w_score;                  // (G, Q, N)
};

// 256 lanes = 16 x 16; lane (tx, ty) holds the scores of the queries ty + 16 a and the database rows tx + 16 b of the tile, a, b < 4
__global__ __launch_bounds__(256) void retr_score_kernel(RetrScoreArgs a) {
    __shared__ float lq[rt::TILE * rt::LDS_STRIDE];
    __shared__ float ld[rt::TILE * rt::LDS_STRIDE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int tn_i = blockIdx.x % a.tn, rest = blockIdx.x / a.tn, tq_i = rest % a.tq, g = rest / a.tq;
    const int q0 = tq_i * rt::TILE, n0 = tn_i * rt::TILE, nblk = a.D / 64;
    float tot[4][4], seg[4][4], blk[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) tot[x][y] = 0.f;
    for (int b0 = 0; b0 < nblk; b0 += rt::SEG) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) seg[x][y] = 0.f;
        const int b1 = b0 + rt::SEG < nblk ? b0 + rt::SEG : nblk;
        for (int bb = b0; bb < b1; ++bb) {
            __syncthreads();                               // the last block's reads are done
#pragma unroll
            for (int i = 0; i < 4; ++i) {                  // 16 lanes = the 64 floats of one row (rows past the end: zeros)
                const int row = ty + 16 * i;
                float4 vq = make_float4(0.f, 0.f, 0.f, 0.f), vd = vq;
                if (q0 + row < a.Q) vq = *reinterpret_cast<const float4*>(a.q + ((size_t)g * a.Q + q0 + row) * a.D + (size_t)bb * 64 + tx * 4);
                if (n0 + row < a.N) vd = *reinterpret_cast<const float4*>(a.db + ((size_t)g * a.N + n0 + row) * a.D + (size_t)bb * 64 + tx * 4);
                *reinterpret_cast<float4*>(&lq[row * rt::LDS_STRIDE + tx * 4]) = vq;
                *reinterpret_cast<float4*>(&ld[row * rt::LDS_STRIDE + tx * 4]) = vd;
            }
            __syncthreads();
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) blk[x][y] = 0.f;
#pragma unroll 4
            for (int j4 = 0; j4 < 16; ++j4) {
                float4 vq[4], vd[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    vq[x] = *reinterpret_cast<const float4*>(&lq[(ty + 16 * x) * rt::LDS_STRIDE + j4 * 4]);
                    vd[x] = *reinterpret_cast<const float4*>(&ld[(tx + 16 * x) * rt::LDS_STRIDE + j4 * 4]);
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) {
                        float s = blk[x][y];
                        s = s + vq[x].x * vd[y].x;
                        s = s + vq[x].y * vd[y].y;
                        s = s + vq[x].z * vd[y].z;
                        s = s + vq[x].w * vd[y].w;
                        blk[x][y] = s;
                    }
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) seg[x][y] = seg[x][y] + blk[x][y];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) tot[x][y] = tot[x][y] + seg[x][y];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int qi = q0 + ty + 16 * x, ni = n0 + tx + 16 * y;
            if (qi < a.Q && ni < a.N) a.w_score[((size_t)g * a.Q + qi) * a.N + ni] = tot[x][y];
        }
}

struct RetrTopkArgs {
    const float* w_score;            // (G, Q, N)
    const int32_t* n_db;             // (G,) or null: N
    int Q, N, k, exclude_self;
    int32_t* idx;                    // (G, Q, k)
    float* score;                    // (G, Q, k)
};

// larger key = earlier in the output: the score's order-preserving integer above the complement of the index; 0: never returned
__device__ inline unsigned long long rt_key(float s, int i) {
    if (!rt_finite(s)) return 0ull;
    const unsigned u = s == 0.f ? 0u : __float_as_uint(s);
    const unsigned ord = (u >> 31) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ord << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
}

__global__ __launch_bounds__(256) void retr_topk_kernel(RetrTopkArgs a) {
    __shared__ unsigned long long s_key[256];
    const int tid = threadIdx.x;
    const int g = blockIdx.x / a.Q, j = blockIdx.x % a.Q;
    const int n = rt_clamp(a.n_db ? a.n_db[g] : a.N, a.N);
    const float* s = a.w_score + (size_t)blockIdx.x * a.N;
    const size_t out = (size_t)blockIdx.x * a.k;
    unsigned long long prev = ~0ull;
    int r = 0;
    for (; r < a.k; ++r) {                                 // round r: the largest key below the last one
        unsigned long long best = 0ull;
        for (int i = tid; i < n; i += 256) {
            const unsigned long long key = rt_key(s[i], i);
            if ((!a.exclude_self || i != j) && key < prev && key > best) best = key;
        }
        s_key[tid] = best;
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if (tid < h && s_key[tid + h] > s_key[tid]) s_key[tid] = s_key[tid + h];
            __syncthreads();
        }
        const unsigned long long top = s_key[0];
        __syncthreads();                                   // (everyone has read s_key[0] before the next round writes it)
        if (top == 0ull) break;                            // (the same for every lane)
        if (tid == 0) {
            const int i = (int)(0xffffffffu - (unsigned)(top & 0xffffffffull));
            a.idx[out + r] = i;
            a.score[out + r] = s[i];
        }
        prev = top;
    }
    for (int e = r + tid; e < a.k; e += 256) {
        a.idx[out + e] = -1;
        a.score[out + e] = __uint_as_float(rt::NAN_BITS);
    }
}

struct RetrPairArgs {
    const int32_t* idx;              // (S, V, k)
    const int32_t* n_views;          // (S,) or null: V
    int V, k, pcap;
    int32_t* view_pairs;             // (S, pcap, 2)
    int32_t* n_pairs;                // (S,)
};

__global__ __launch_bounds__(64) void retr_pairs_kernel(RetrPairArgs a) {
    __shared__ int adj[rt::MAX_VIEWS];                     // bit b of adj[a]: the pair (a, b), a < b
    const int s = blockIdx.x, tid = threadIdx.x;
    const int nv = rt_clamp(a.n_views ? a.n_views[s] : a.V, a.V);
    if (tid < rt::MAX_VIEWS) adj[tid] = 0;
    __syncthreads();
    for (int e = tid; e < a.V * a.k; e += 64) {
        const int v = e / a.k, w = a.idx[(size_t)s * a.V * a.k + e];
        if (v < nv && w >= 0 && w < nv && w != v) atomicOr(&adj[v < w ? v : w], (int)(1u << (v < w ? w : v)));
    }
    __syncthreads();
    int total = 0, before = 0;
    for (int x = 0; x < rt::MAX_VIEWS; ++x) {
        const int c = (int)__popcll((unsigned long long)(unsigned)adj[x]);
        total += c;
        if (x < tid) before += c;
    }
    int32_t* out = a.view_pairs + (size_t)s * a.pcap * 2;
    if (tid < rt::MAX_VIEWS) {
        const unsigned bits = (unsigned)adj[tid];
        for (int b = tid + 1; b < rt::MAX_VIEWS; ++b)
            if ((bits >> b) & 1u) {
                if (before < a.pcap) { out[2 * before] = tid; out[2 * before + 1] = b; }
                ++before;
            }
    }
    for (int p = total + tid; p < a.pcap; p += 64) { out[2 * p] = -1; out[2 * p + 1] = -1; }
    if (tid == 0) a.n_pairs[s] = total;
}
// ---- retrieval end ----

static size_t rt_align(size_t x) { return (x + 255) & ~(size_t)255; }
static bool rt_codebook_size(int C) { return C == 32 || C == 64 || C == 128 || C == 256; }

// groups x rows is how the sums see the descriptors: (G, K) for VLAD, (1, G K) for k-means.  Offsets of w_score, w_state, w_part, w_cnt, w_obj.
static size_t rt_layout(long long groups, long long rows, int C, bool kmeans, size_t* off) {
    const size_t n = (size_t)groups * rows, chunks = (size_t)groups * ((rows + rt::CHUNK - 1) / rt::CHUNK);
    const size_t sizes[5] = {kmeans ? n * 4 : 0, n, chunks * C * 256, chunks * C * 4, kmeans ? chunks * 8 : 0};
    size_t at = 0;
    for (int i = 0; i < 5; ++i) {
        if (off) off[i] = at;
        at += rt_align(sizes[i]);
    }
    return at;
}

static bool rt_rows_ok(int G, int K, int C, long long max_rows) {
    return G >= 1 && G <= 65535 && K >= 1 && (long long)G * K <= max_rows && rt_codebook_size(C);
}

size_t vlad_workspace_bytes(int G, int K, int C) { return rt_rows_ok(G, K, C, 1ll << 24) ? rt_layout(G, K, C, false, nullptr) : 0; }
size_t kmeans_workspace_bytes(int G, int K, int C) { return rt_rows_ok(G, K, C, 1ll << 22) ? rt_layout(1, (long long)G * K, C, true, nullptr) : 0; }

// assignment, then the chunk sums over (groups, rows); fills the finishing kernel's arguments.  -1: more than a launch holds
static int rt_assign_and_sum(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, bool kmeans, int32_t* assign, void* ws,
                             RetrFinishArgs& f, hipStream_t st) {
    const long long total = (long long)G * K, groups = kmeans ? 1 : G, rows = kmeans ? total : K;
    const long long nchunks = (rows + rt::CHUNK - 1) / rt::CHUNK, g1 = (total + 255) / 256, g2 = groups * nchunks * (C / 16);
    if (g1 > 0x7fffffffll || g2 > 0x7fffffffll) return -1;
    size_t off[5];
    rt_layout(groups, rows, C, kmeans, off);
    char* w = (char*)ws;
    RetrAssignArgs a = {};
    a.desc = desc; a.counts = counts; a.codebook = codebook; a.K = K; a.C = C; a.total = total; a.assign = assign;
    a.w_score = kmeans ? (float*)(w + off[0]) : nullptr; a.w_state = (unsigned char*)(w + off[1]);
    retr_assign_kernel<<<(unsigned)g1, 256, 0, st>>>(a);
    RetrSumArgs s = {};
    s.desc = desc; s.assign = assign; s.codebook = codebook; s.w_score = a.w_score; s.rows = (int)rows; s.nchunks = (int)nchunks; s.C = C;
    s.residual = kmeans ? 0 : 1; s.w_part = (float*)(w + off[2]); s.w_cnt = (int32_t*)(w + off[3]); s.w_obj = kmeans ? (double*)(w + off[4]) : nullptr;
    retr_sums_kernel<<<(unsigned)g2, 256, 0, st>>>(s);
    f = {};
    f.w_part = s.w_part; f.w_cnt = s.w_cnt; f.w_state = a.w_state; f.w_obj = s.w_obj; f.codebook = codebook; f.rows = (int)rows; f.nchunks = (int)nchunks;
    f.C = C;
    return 0;
}

int launch_vlad(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, float* vlad, int32_t* assign, int32_t* n_assigned,
                int32_t* info, void* ws, hipStream_t st) {
    if (!rt_rows_ok(G, K, C, 1ll << 24)) return -1;
    RetrFinishArgs f;
    if (rt_assign_and_sum(desc, counts, G, K, codebook, C, false, assign, ws, f, st)) return -1;
    f.out = vlad; f.n_assigned = n_assigned; f.info = info;
    retr_vlad_finish_kernel<<<G, 256, 0, st>>>(f);
    return 0;
}

int launch_kmeans_step(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, float* codebook_out, int32_t* assign,
                       int32_t* n_assigned, double* objective, int32_t* info, void* ws, hipStream_t st) {
    if (!rt_rows_ok(G, K, C, 1ll << 22)) return -1;
    RetrFinishArgs f;
    if (rt_assign_and_sum(desc, counts, G, K, codebook, C, true, assign, ws, f, st)) return -1;
    f.out = codebook_out; f.n_assigned = n_assigned; f.objective = objective; f.info = info;
    retr_kmeans_finish_kernel<<<1, 256, 0, st>>>(f);
    return 0;
}

static bool rt_retrieve_ok(int G, int Q, int N) {
    return G >= 1 && G <= 65535 && Q >= 1 && Q <= (1 << 24) && N >= 1 && N <= (1 << 24) && (long long)G * Q <= 0x7fffffffll &&
           (long long)G * Q * (long long)N <= (1ll << 36);
}

size_t retrieve_workspace_bytes(int G, int Q, int N) { return rt_retrieve_ok(G, Q, N) ? rt_align((size_t)G * Q * N * 4) : 0; }

int launch_retrieve_topk(const float* q, const float* db, const int32_t* n_db, int G, int Q, int N, int D, int k, int exclude_self, int32_t* idx,
                         float* score, void* ws, hipStream_t st) {
    if (!rt_retrieve_ok(G, Q, N) || D < 64 || D > rt::MAX_D || D % 64 != 0 || k < 1 || k > rt::MAX_K) return -1;
    const long long tq = (Q + rt::TILE - 1) / rt::TILE, tn = (N + rt::TILE - 1) / rt::TILE;
    if ((long long)G * tq * tn > 0x7fffffffll) return -1;
    RetrScoreArgs a = {};
    a.q = q; a.db = db; a.Q = Q; a.N = N; a.D = D; a.tq = (int)tq; a.tn = (int)tn; a.w_score = (float*)ws;
    retr_score_kernel<<<(unsigned)(G * tq * tn), 256, 0, st>>>(a);
    RetrTopkArgs t = {};
    t.w_score = a.w_score; t.n_db = n_db; t.Q = Q; t.N = N; t.k = k; t.exclude_self = exclude_self; t.idx = idx; t.score = score;
    retr_topk_kernel<<<(unsigned)(G * Q), 256, 0, st>>>(t);
    return 0;
}

int retrieve_pair_capacity(int V, int k) {
    const int all = V * (V - 1) / 2;
    return V * k < all ? V * k : all;
}

int launch_pairs_from_shortlists(const int32_t* idx, const int32_t* n_views, int S, int V, int k, int32_t* view_pairs, int32_t* n_pairs, hipStream_t st) {
    if (S < 1 || S > 65535 || V < 2 || V > rt::MAX_VIEWS || k < 1 || k > rt::MAX_K) return -1;
    RetrPairArgs a = {};
    a.idx = idx; a.n_views = n_views; a.V = V; a.k = k; a.pcap = retrieve_pair_capacity(V, k); a.view_pairs = view_pairs; a.n_pairs = n_pairs;
    retr_pairs_kernel<<<S, 64, 0, st>>>(a);
    return 0;
}

}  // namespace xfh
