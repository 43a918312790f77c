// Order-preserving compaction of match lists by a mask: what stands between an estimator's inlier mask and the track graph.
// tests/verification_reference.py restates it and tests/test_verification_emulated.py compiles the slice below for the host
// (tests/emu/verify_emu.cpp).  Integers only, no atomic on data, no workspace; no order depends on scheduling: two calls give the same bytes.
//
// xfh_filter_matches, per list l of L: idx_a, idx_b (cap) int64, n = n_matches[l] clamped to [0, cap], mask (cap) uint8, keep[l] uint8 (NULL: 1).
//   Entry i < n is SET iff mask[i] != 0; c = the number of set entries.  The list is EMPTIED when keep[l] == 0 (reason 1) or otherwise when
//   c < min_keep (reason 2).  n_out = 0 when emptied, else c.  The j-th set entry in ascending i goes to slot j < n_out: out_a[j] = idx_a[i],
//   out_b[j] = idx_b[i], src[j] = i; every slot from n_out on is -1 in all three.  info: n, c, the reason (0: none), 0.
// Launch: filter_matches_kernel, one workgroup of 256 per list, the list in chunks of 256 ascending; the rank of an entry is the running base
// plus the set entries of the lower waves (four counts through LDS) plus those of the lower lanes of its wave (a 64-bit ballot): the scan
// of map_scan_kernel (k_map.hip) / tk_number_kernel (k_tracks.hip).
#include "kernels.hpp"

namespace xfh {

// ---- match filter begin (host-compilable with tests/emu/emu.hpp: tests/test_verification_emulated.py slices it out) ----
namespace mf {
constexpr int NONE = 0, BY_KEEP = 1, BY_MIN_KEEP = 2;      // info word 2
}  // namespace mf

struct MfArgs {
    const int64_t* idx_a;            // (L, cap)
    const int64_t* idx_b;
    const int32_t* n_matches;        // (L,)
    const unsigned char* mask;       // (L, cap)
    const unsigned char* keep;       // (L,) or null
    int cap, min_keep;
    int64_t* out_a;                  // (L, cap)
    int64_t* out_b;
    int32_t* src;                    // (L, cap)
    int32_t* n_out;                  // (L,)
    int32_t* info;                   // (L, 4)
};

__global__ __launch_bounds__(256) void filter_matches_kernel(MfArgs a) {
    __shared__ int wave_n[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t l = blockIdx.x, base = l * (size_t)a.cap;
    int n = a.n_matches[l];
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    const bool kept_list = a.keep ? a.keep[l] != 0 : true;
    int carry = 0;
    for (int b0 = 0; b0 < n; b0 += 256) {                   // (the trip count is the same for every thread: the barriers below are met by all)
        const int i = b0 + tid;
        const bool set = i < n && a.mask[base + i] != 0;
        const unsigned long long m = __ballot(set);
        __syncthreads();                                   // the last round's wave_n has been read
        if (lane == 0) wave_n[wave] = (int)__popcll(m);
        __syncthreads();
        const int w0 = wave_n[0], w1 = wave_n[1], w2 = wave_n[2], w3 = wave_n[3];
        const int before = wave == 0 ? 0 : (wave == 1 ? w0 : (wave == 2 ? w0 + w1 : (w0 + w1) + w2));
        const int id = (carry + before) + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (set && kept_list) {                            // id < n <= cap
            a.out_a[base + id] = a.idx_a[base + i];
            a.out_b[base + id] = a.idx_b[base + i];
            a.src[base + id] = i;
        }
        carry += (w0 + w1) + (w2 + w3);
    }
    const int reason = !kept_list ? mf::BY_KEEP : (carry < a.min_keep ? mf::BY_MIN_KEEP : mf::NONE);
    const int count = reason == mf::NONE ? carry : 0;
    __syncthreads();                                       // a list emptied by min_keep: its slots were written above by other threads
    for (int j = count + tid; j < a.cap; j += 256) {
        a.out_a[base + j] = -1;
        a.out_b[base + j] = -1;
        a.src[base + j] = -1;
    }
    if (tid == 0) {
        int32_t* info = a.info + l * 4;
        info[0] = n; info[1] = carry; info[2] = reason; info[3] = 0;
        a.n_out[l] = count;
    }
}
// ---- match filter end ----

int launch_filter_matches(const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches, const unsigned char* mask, const unsigned char* keep,
                          long long L, int cap, int min_keep, int64_t* out_a, int64_t* out_b, int32_t* src, int32_t* n_out, int32_t* info, hipStream_t st) {
    if (L < 1 || L > 0x7fffffffll || cap < 1 || min_keep < 0) return -1;      // the grid is one-dimensional over the lists
    MfArgs a = {};
    a.idx_a = idx_a; a.idx_b = idx_b; a.n_matches = n_matches; a.mask = mask; a.keep = keep; a.cap = cap; a.min_keep = min_keep;
    a.out_a = out_a; a.out_b = out_b; a.src = src; a.n_out = n_out; a.info = info;
    filter_matches_kernel<<<(unsigned)L, 256, 0, st>>>(a);
    return 0;
}

}  // namespace xfh
