// Map rows for localisation: a 3D point with a descriptor for every usable track of a triangulation, and the pixels of the
// rows under a pose.  tests/localization_reference.py restates both operation by operation and tests/test_localization_emulated.py compiles
// the slice below for the host (tests/emu/map_emu.cpp).  Only + - * / sqrt, fp contraction off, every sum in one fixed order; no
// floating-point atomic, and no order depends on scheduling: two calls give the same bytes.
//
// xfh_build_map, per scene: desc (V, Kcap, 64) fp32, tracks (T, V) int32, points3d (T, 3) fp32, status (T) uint8, inlier_views (T) int32.
//   View v CONTRIBUTES to track t iff bit v of inlier_views[t] is set (the word read as unsigned: view 31 is the sign bit),
//   0 <= tracks[t, v] < Kcap, and all 64 components of that row of desc[v] are finite.
//   Track t is SELECTED unless one of the following holds; they are tested in this order and a skipped track counts under the first:
//     1. status[t] != 0;   2. a coordinate of points3d[t] is not finite;   3. fewer than min_views contributing views;
//     4. the squared norm n2 of the sum of the contributing rows is not finite or below FLT_MIN.
//   sum[c] = ((0 + row_v0[c]) + row_v1[c]) + ... in fp32 over the contributing views ascending.
//   n2: component c = 4 l + i belongs to lane l of 16; p_l = ((s0 s0 + s1 s1) + s2 s2) + s3 s3 over the lane's four components, then the
//   balanced tree over the lanes n2 = (((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))) + (((p8 + p9) + (p10 + p11)) + ((p12 + p13) + (p14 + p15)))
//   (an xor butterfly: every addition is of two equal-shaped halves, so all 16 lanes hold the same bits).
//   r = sqrt(n2), inv = 1 / r, desc[c] = sum[c] * inv, desc_f16[c] = fp16 round-to-nearest-even of desc[c] * 256 (what descriptor_kernel of
//   k_detect.hip writes beside its rows), coherence = r / (float)n_obs with n_obs the number of contributing views.
//   The selected tracks go to the rows 0, 1, ... in ascending track id; those from M on are dropped and counted.  Rows n_points .. M - 1: NaN
//   point, zero descriptors, track -1, n_obs 0, coherence 0.  info: T, rows written, skipped by 1, 2, 3, 4, over capacity, 0.
// Launches: map_gather_kernel (16 lanes = one track, one float4 of the row per lane: the sums, the flag and the candidate row into the
// workspace), map_scan_kernel (workgroup = scene: the flags in chunks of 256 ascending by wave ballots -> the destination row of every
// track, the counters) and map_move_kernel (16 lanes = one track / one output row: moves the candidate rows, fills the tail).
//
// xfh_map_project, per query q: X = points[q, j] widened to fp64; x = ((R0 X0 + R1 X1) + R2 X2) + t0 and likewise y, z with the rows of R;
//   (a, b, w) = K (x, y, z) row by row as (K0 x + K1 y) + K2 z; u = a / w, v = b / w, rounded to fp32 once.  Both are NaN when j >= n_points[q],
//   z is not finite or not > 0, u or v is not finite, or an image size is given (width > 0) and u < -margin, u > width + margin, v < -margin
//   or v > height + margin.
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace xfh {

// ---- map begin (host-compilable with tests/emu/emu.hpp: tests/test_localization_emulated.py slices it out) ----
namespace mp {
constexpr int MAX_VIEWS = 32;
constexpr int SELECTED = 0, SKIP_STATUS = 1, SKIP_POINT = 2, SKIP_VIEWS = 3, SKIP_NORM = 4;      // the flag of a track
constexpr float NORM_MIN = 1.17549435e-38f;               // FLT_MIN
constexpr unsigned NAN_BITS = 0x7fc00000u;
}  // namespace mp

struct MapArgs {
    const float* desc;               // (S, V, Kcap, 64)
    const int32_t* tracks;           // (S, T, V)
    const float* points3d;           // (S, T, 3)
    const unsigned char* status;     // (S, T)
    const int32_t* inlier_views;     // (S, T)
    int T, V, Kcap, min_views, M;
    int groups;                      // workgroups per scene of the launch
    float* w_desc;                   // (S, T, 64) candidate rows
    float* w_coh;                    // (S, T)
    int32_t* w_dst;                  // (S, T) the output row of a track or -1
    unsigned char* w_nobs;           // (S, T)
    unsigned char* w_flag;           // (S, T)
    float* points;                   // (S, M, 3)
    float* out_desc;                 // (S, M, 64)
    unsigned short* desc_f16;        // (S, M, 64)
    int32_t* track;                  // (S, M)
    unsigned char* n_obs;            // (S, M)
    float* coherence;                // (S, M)
    int32_t* n_points;               // (S,)
    int32_t* info;                   // (S, 8)
};

__device__ inline bool mp_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool mp_finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(256) void map_gather_kernel(MapArgs a) {
    const int tid = threadIdx.x, sub = tid & 15;
    const int s = blockIdx.x / a.groups, t = (blockIdx.x % a.groups) * 16 + (tid >> 4);
    const bool in = t < a.T;                               // (no lane leaves early: the ballot below is the whole wave's)
    const size_t at = (size_t)s * a.T + (in ? t : 0);
    const float px = a.points3d[at * 3], py = a.points3d[at * 3 + 1], pz = a.points3d[at * 3 + 2];
    const unsigned views = (unsigned)a.inlier_views[at];
    int flag = (!in || a.status[at] != 0) ? mp::SKIP_STATUS : (!(mp_finite(px) && mp_finite(py) && mp_finite(pz)) ? mp::SKIP_POINT : mp::SELECTED);
    const bool live = flag == mp::SELECTED;
    const int shift = tid & 48;                            // the first lane of this track's 16 within its wave
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int n = 0;
    for (int v = 0; v < a.V; ++v) {
        const int row = a.tracks[at * a.V + v];
        const bool cand = live && ((views >> v) & 1u) != 0u && (unsigned)row < (unsigned)a.Kcap;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cand) d = *reinterpret_cast<const float4*>(a.desc + (((size_t)s * a.V + v) * a.Kcap + row) * 64 + sub * 4);
        const unsigned long long fin = __ballot(mp_finite(d.x) && mp_finite(d.y) && mp_finite(d.z) && mp_finite(d.w));
        if (cand && ((fin >> shift) & 0xffffull) == 0xffffull) {
            acc.x = acc.x + d.x; acc.y = acc.y + d.y; acc.z = acc.z + d.z; acc.w = acc.w + d.w;
            ++n;
        }
    }
    // |sum|^2 over the track's 16 lanes: an xor butterfly on DPP operands (quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror)
    float n2 = ((acc.x * acc.x + acc.y * acc.y) + acc.z * acc.z) + acc.w * acc.w;
#define XFH_MAP_DPP_ADD(ctrl) n2 = n2 + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(n2), ctrl, 0xf, 0xf, true))
    XFH_MAP_DPP_ADD(0xb1);
    XFH_MAP_DPP_ADD(0x4e);
    XFH_MAP_DPP_ADD(0x141);
    XFH_MAP_DPP_ADD(0x140);
#undef XFH_MAP_DPP_ADD
    if (flag == mp::SELECTED && n < a.min_views) flag = mp::SKIP_VIEWS;
    if (flag == mp::SELECTED && (!mp_finite(n2) || n2 < mp::NORM_MIN)) flag = mp::SKIP_NORM;
    if (!in) return;
    const bool sel = flag == mp::SELECTED;
    const float r = sel ? sqrtf(n2) : 1.f;
    if (sel) {
        const float inv = 1.f / r;
        *reinterpret_cast<float4*>(a.w_desc + at * 64 + sub * 4) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
    if (sub == 0) {
        a.w_flag[at] = (unsigned char)flag;
        a.w_nobs[at] = (unsigned char)(sel ? n : 0);
        a.w_coh[at] = sel ? r / (float)n : 0.f;
    }
}

__global__ __launch_bounds__(256) void map_scan_kernel(MapArgs a) {
    __shared__ int wave_n[4];
    __shared__ int cnt[4];                                 // skipped by reason 1 .. 4
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)s * a.T;
    if (tid < 4) cnt[tid] = 0;
    int carry = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int b0 = 0; b0 < a.T; b0 += 256) {                 // (the trip count is the same for every thread: the barriers below are met by all)
        const int x = b0 + tid;
        const int flag = x < a.T ? (int)a.w_flag[base + x] : -1;
        c1 += flag == mp::SKIP_STATUS; c2 += flag == mp::SKIP_POINT; c3 += flag == mp::SKIP_VIEWS; c4 += flag == mp::SKIP_NORM;
        const bool keep = flag == mp::SELECTED;
        const unsigned long long m = __ballot(keep);
        __syncthreads();                                   // the last round's wave_n has been read (and cnt is zero)
        if (lane == 0) wave_n[wave] = (int)__popcll(m);
        __syncthreads();
        const int w0 = wave_n[0], w1 = wave_n[1], w2 = wave_n[2], w3 = wave_n[3];
        const int before = wave == 0 ? 0 : (wave == 1 ? w0 : (wave == 2 ? w0 + w1 : (w0 + w1) + w2));
        const int id = (carry + before) + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (x < a.T) a.w_dst[base + x] = keep && id < a.M ? id : -1;
        carry += (w0 + w1) + (w2 + w3);
    }
    if (c1) atomicAdd(&cnt[0], c1);
    if (c2) atomicAdd(&cnt[1], c2);
    if (c3) atomicAdd(&cnt[2], c3);
    if (c4) atomicAdd(&cnt[3], c4);
    __syncthreads();
    if (tid == 0) {
        int32_t* info = a.info + (size_t)s * 8;
        const int kept = carry < a.M ? carry : a.M;
        info[0] = a.T; info[1] = kept; info[2] = cnt[0]; info[3] = cnt[1]; info[4] = cnt[2]; info[5] = cnt[3]; info[6] = carry - kept; info[7] = 0;
        a.n_points[s] = kept;
    }
}

__global__ __launch_bounds__(256) void map_move_kernel(MapArgs a) {
    const int tid = threadIdx.x, sub = tid & 15;
    const int s = blockIdx.x / a.groups, x = (blockIdx.x % a.groups) * 16 + (tid >> 4);
    if (x < a.T) {                                         // track x to its row
        const size_t at = (size_t)s * a.T + x;
        const int dst = a.w_dst[at];
        if (dst >= 0) {
            const size_t to = (size_t)s * a.M + dst;
            const float4 o = *reinterpret_cast<const float4*>(a.w_desc + at * 64 + sub * 4);
            *reinterpret_cast<float4*>(a.out_desc + to * 64 + sub * 4) = o;
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            h4 q;
            q[0] = (_Float16)(o.x * 256.f); q[1] = (_Float16)(o.y * 256.f); q[2] = (_Float16)(o.z * 256.f); q[3] = (_Float16)(o.w * 256.f);
            *reinterpret_cast<ushort4*>(a.desc_f16 + to * 64 + sub * 4) = __builtin_bit_cast(ushort4, q);
            if (sub < 3) a.points[to * 3 + sub] = __uint_as_float(__float_as_uint(a.points3d[at * 3 + sub]));
            if (sub == 3) a.track[to] = x;
            if (sub == 4) a.n_obs[to] = a.w_nobs[at];
            if (sub == 5) a.coherence[to] = a.w_coh[at];
        }
    }
    if (x < a.M && x >= a.info[(size_t)s * 8 + 1]) {        // output row x is past the rows written
        const size_t to = (size_t)s * a.M + x;
        *reinterpret_cast<float4*>(a.out_desc + to * 64 + sub * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<ushort4*>(a.desc_f16 + to * 64 + sub * 4) = make_ushort4(0, 0, 0, 0);
        if (sub < 3) a.points[to * 3 + sub] = __uint_as_float(mp::NAN_BITS);
        if (sub == 3) a.track[to] = -1;
        if (sub == 4) a.n_obs[to] = 0;
        if (sub == 5) a.coherence[to] = 0.f;
    }
}

struct MapProjectArgs {
    const float* points;             // (Q, M, 3)
    const int32_t* n_points;         // (Q,) or null: M
    const double* R;                 // (Q, 9)
    const double* t;                 // (Q, 3)
    const double* K;                 // (Q, 9)
    int M, groups;
    double width, height, margin;    // width <= 0: no image test
    float* uv;                       // (Q, M, 2)
};

__global__ __launch_bounds__(256) void map_project_kernel(MapProjectArgs a) {
    const int q = blockIdx.x / a.groups, j = (blockIdx.x % a.groups) * 256 + threadIdx.x;
    if (j >= a.M) return;
    const size_t at = (size_t)q * a.M + j;
    const double* R = a.R + (size_t)q * 9;
    const double* t = a.t + (size_t)q * 3;
    const double* K = a.K + (size_t)q * 9;
    const double X0 = (double)a.points[at * 3], X1 = (double)a.points[at * 3 + 1], X2 = (double)a.points[at * 3 + 2];
    const double x = ((R[0] * X0 + R[1] * X1) + R[2] * X2) + t[0];
    const double y = ((R[3] * X0 + R[4] * X1) + R[5] * X2) + t[1];
    const double z = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
    const double ha = (K[0] * x + K[1] * y) + K[2] * z;
    const double hb = (K[3] * x + K[4] * y) + K[5] * z;
    const double hw = (K[6] * x + K[7] * y) + K[8] * z;
    const double u = ha / hw, v = hb / hw;
    const int n = a.n_points ? a.n_points[q] : a.M;
    bool ok = j < n && mp_finite64(z) && z > 0.0 && mp_finite64(u) && mp_finite64(v);
    if (a.width > 0.0) ok = ok && !(u < -a.margin) && !(u > a.width + a.margin) && !(v < -a.margin) && !(v > a.height + a.margin);
    const float nan = __uint_as_float(mp::NAN_BITS);
    *reinterpret_cast<float2*>(a.uv + at * 2) = make_float2(ok ? (float)u : nan, ok ? (float)v : nan);
}
// ---- map end ----

static size_t mp_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the offsets of w_desc, w_coh, w_dst, w_nobs, w_flag; returns the size
static size_t mp_layout(int S, int T, size_t* off) {
    const size_t n = (size_t)S * T;
    const size_t sizes[5] = {n * 256, n * 4, n * 4, n, n};
    size_t at = 0;
    for (int i = 0; i < 5; ++i) {
        if (off) off[i] = at;
        at += mp_align(sizes[i]);
    }
    return at;
}

size_t map_workspace_bytes(int S, int T, int V) {
    (void)V;                                               // (the kernels keep nothing per view)
    return mp_layout(S, T, nullptr);
}

int launch_build_map(const float* desc, int kcap, const int32_t* tracks, const float* points3d, const unsigned char* status, const int32_t* inlier_views,
                     int S, int T, int V, int min_views, int M, float* points, float* out_desc, unsigned short* desc_f16, int32_t* track,
                     unsigned char* n_obs, float* coherence, int32_t* n_points, int32_t* info, void* ws, hipStream_t st) {
    if (S < 1 || S > 65535 || T < 1 || T > (1 << 24) || V < 1 || V > mp::MAX_VIEWS || kcap < 1 || kcap > (1 << 24) || M < 1 || M > (1 << 24) ||
        min_views < 1 || min_views > mp::MAX_VIEWS)
        return -1;
    const long long g1 = ceil_div(T, 16), g3 = ceil_div(T > M ? T : M, 16);
    if (g1 * S > 0x7fffffffll || g3 * S > 0x7fffffffll) return -1;
    size_t off[5];
    mp_layout(S, T, off);
    char* w = (char*)ws;
    MapArgs a = {};
    a.desc = desc; a.tracks = tracks; a.points3d = points3d; a.status = status; a.inlier_views = inlier_views;
    a.T = T; a.V = V; a.Kcap = kcap; a.min_views = min_views; a.M = M;
    a.w_desc = (float*)(w + off[0]); a.w_coh = (float*)(w + off[1]); a.w_dst = (int32_t*)(w + off[2]);
    a.w_nobs = (unsigned char*)(w + off[3]); a.w_flag = (unsigned char*)(w + off[4]);
    a.points = points; a.out_desc = out_desc; a.desc_f16 = desc_f16; a.track = track; a.n_obs = n_obs; a.coherence = coherence;
    a.n_points = n_points; a.info = info;
    a.groups = (int)g1;
    map_gather_kernel<<<(unsigned)(g1 * S), 256, 0, st>>>(a);
    map_scan_kernel<<<S, 256, 0, st>>>(a);
    a.groups = (int)g3;
    map_move_kernel<<<(unsigned)(g3 * S), 256, 0, st>>>(a);
    return 0;
}

int launch_map_project(const float* points, const int32_t* n_points, int Q, int M, const double* R, const double* t, const double* K, double width,
                       double height, double margin, float* uv, hipStream_t st) {
    if (Q < 1 || Q > (1 << 20) || M < 1 || M > (1 << 24)) return -1;
    const long long g = ceil_div(M, 256);
    if (g * Q > 0x7fffffffll) return -1;
    MapProjectArgs a = {};
    a.points = points; a.n_points = n_points; a.R = R; a.t = t; a.K = K; a.M = M; a.groups = (int)g;
    a.width = width; a.height = height; a.margin = margin; a.uv = uv;
    map_project_kernel<<<(unsigned)(g * Q), 256, 0, st>>>(a);
    return 0;
}

}  // namespace xfh
