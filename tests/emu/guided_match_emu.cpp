// xfh_match_mnn_guided on the host: guided_prep_kernel + mnn_guided_kernel<KIND> (csrc/k_match_guided.hip) and the shared finalize (mutual_keep +
// mnn_finalize_kernel, csrc/k_match.hip), sliced out of the product sources by tests/test_guided_emulated.py into guided_slice.hpp / finalize_slice.hpp and
// run in launch_match_guided's order: keys zeroed, prep, sweep, finalize.
// stdin: {kind, P, N1, N2, n_stride, n_off2} int32, {max_error, min_cossim} float64, ncount int32 and the count array of that length (pair p: rows
// counts[p * n_stride], columns counts[p * n_stride + n_off2]; ncount 0: all rows), d1 (P*N1*64) d2 (P*N2*64) k1 (P*N1*2) k2 (P*N2*2) fp32, models (P*9) fp64;
// stdout: n_matches (P) int32, idx0 (P*N1) int64, idx1 (P*N1) int64.
// What emu.hpp does not have is here: 64-bit atomic max, the 64-bit lane exchanges, the wave sum, the LDS atomic add.
#include "emu.hpp"
#include <cfloat>
#include <cstdio>
#define __global__ inline
#define XFH_GUIDE_FUNDAMENTAL 0
#define XFH_GUIDE_HOMOGRAPHY 1
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
namespace xfh {
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }      // (common.hpp)
inline unsigned float_ord(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
inline float ord_float(unsigned o) { unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; return __uint_as_float(u); }
inline unsigned long long u64_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
inline unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = emu::shfl_xor(lo, o);
    hi = emu::shfl_xor(hi, o);
    return ((unsigned long long)hi << 32) | lo;
}
inline unsigned long long xhalf_u64(unsigned long long v) { return shfl_xor_u64(v, 32); }      // (common.hpp: two v_permlane32_swap)
inline int wave_sum_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v += emu::shfl_xor(v, o);
    return v;
}
#include "guided_slice.hpp"
#include "finalize_slice.hpp"
}  // namespace xfh

template <typename T>
static bool rd(std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

int main() {
    int h[6], ncount;
    double par[2];
    if (fread(h, 4, 6, stdin) != 6 || fread(par, 8, 2, stdin) != 2 || fread(&ncount, 4, 1, stdin) != 1) return 2;
    const int kind = h[0], P = h[1], N1 = h[2], N2 = h[3], n_stride = h[4], n_off2 = h[5];
    std::vector<int32_t> counts(ncount);
    std::vector<float> d1((size_t)P * N1 * 64), d2((size_t)P * N2 * 64), k1((size_t)P * N1 * 2), k2((size_t)P * N2 * 2);
    std::vector<double> models((size_t)P * 9);
    if (!rd(counts) || !rd(d1) || !rd(d2) || !rd(k1) || !rd(k2) || !rd(models)) return 2;
    const int32_t* n1 = ncount ? counts.data() : nullptr;
    std::vector<unsigned long long> rowkey((size_t)P * N1, 0ull), colkey((size_t)P * N2, 0ull);      // (zeroed by launch_match_guided)
    std::vector<float4> rowc((size_t)P * N1, float4{7.f, 7.f, 7.f, 7.f}), colc((size_t)P * N2, float4{7.f, 7.f, 7.f, 7.f});      // (workspace: not initialised)
    const double thr = par[0];
    const int nb = xfh::ceil_div(N1 > N2 ? N1 : N2, xfh::GM_PREP), nrb = xfh::ceil_div(N1, xfh::GM_ROWS);
    emu::launch(P * nb, xfh::GM_PREP, 0, [&] {
        xfh::guided_prep_kernel(k1.data(), (size_t)N1 * 2, k2.data(), (size_t)N2 * 2, n1, n1, n_stride, n_off2, N1, N2, nb, models.data(), kind, thr * thr, rowc.data(),
                                colc.data());
    });
    const size_t lds = sizeof(float) * xfh::GM_COLS * xfh::GM_DS + 8 * 8 * xfh::GM_COLS + 16 * xfh::GM_ROWS + 16 * xfh::GM_COLS;
    const float thr2 = (float)(thr * thr);
    emu::launch(nrb * P, 512, lds, [&] {
        if (kind == XFH_GUIDE_FUNDAMENTAL)
            xfh::mnn_guided_kernel<XFH_GUIDE_FUNDAMENTAL>(d1.data(), (size_t)N1 * 64, d2.data(), (size_t)N2 * 64, n1, n1, n_stride, n_off2, N1, N2, nrb, P, rowc.data(), colc.data(),
                                                          thr2, rowkey.data(), colkey.data());
        else
            xfh::mnn_guided_kernel<XFH_GUIDE_HOMOGRAPHY>(d1.data(), (size_t)N1 * 64, d2.data(), (size_t)N2 * 64, n1, n1, n_stride, n_off2, N1, N2, nrb, P, rowc.data(), colc.data(),
                                                         thr2, rowkey.data(), colkey.data());
    });
    std::vector<int64_t> idx0((size_t)P * N1, -1), idx1((size_t)P * N1, -1);
    std::vector<int32_t> nm(P, -1);
    const int chunks = xfh::ceil_div(N1, 1024);
    emu::launch(P * chunks, 1024, 128, [&] {
        xfh::mnn_finalize_kernel(n1, n1, n_stride, n_off2, N1, N2, chunks, rowkey.data(), colkey.data(), (float)par[1], idx0.data(), idx1.data(), nm.data());
    });
    fwrite(nm.data(), 4, nm.size(), stdout);
    fwrite(idx0.data(), 8, idx0.size(), stdout);
    fwrite(idx1.data(), 8, idx1.size(), stdout);
    return 0;
}
