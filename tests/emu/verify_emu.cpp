// The match-filter slice of csrc/k_matchfilter.hip (filter_matches_kernel) and the match-verify slice of csrc/k_triangulate.hip
// (verify_matches_kernel, behind the solver and views-solver slices of that file and the shared geometry of csrc/twoview_math.hpp; all sliced
// out of the product source by tests/test_verification_emulated.py into verify_slice.hpp) on the host: one thread per work-item, the wave
// ballots and the barriers of emu.hpp, one workgroup of 256 per list / per pair as launch_filter_matches / launch_verify_matches have it.
// stdin: int32 mode.
//   mode 0 (xfh_filter_matches): int32 L, cap, min_keep, has_keep; idx_a, idx_b (L,cap) i64, n_matches (L) i32, mask (L,cap) u8, keep (L) u8 (if
//     has_keep).  stdout: out_a, out_b (L,cap) i64, src (L,cap) i32, n_out (L) i32, info (L,4) i32.
//   mode 1 (xfh_verify_matches): int32 S, P, cap, V, K, has_nv, has_err; f64 max_epipolar_error; kpts (S,V,K,2) f32, view_pairs (S,P,2) i32, idx_a,
//     idx_b (S,P,cap) i64, n_matches (S,P) i32, n_views (S) i32 (if has_nv), Ks (S,V,9), Rs (S,V,9), ts (S,V,3) f64.
//     stdout: mask (S,P,cap) u8, err (S,P,cap) f32 (if has_err), pair_info (S,P,4) i32.
// Every output starts as 0xa5 bytes: whatever the kernels leave unwritten shows.
#include "emu.hpp"
#include <cstdio>
#include <cstdlib>
#define __shared__ static
#define __global__
namespace xfh {
using std::fabs;
using std::floor;
using std::sqrt;
#include "verify_slice.hpp"
}  // namespace xfh
template <typename T> static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <typename T> static void wr(const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), stdout); }
template <typename T> static std::vector<T> junk(size_t n) {
    std::vector<T> v(n);
    std::memset(v.data(), 0xa5, n * sizeof(T));
    return v;
}
static int filter() {
    const auto h = rd<int>(4);
    const int L = h[0], cap = h[1], min_keep = h[2], has_keep = h[3];
    if (L < 1 || cap < 1 || min_keep < 0) return 3;
    const size_t m = (size_t)L * cap;
    auto ia = rd<int64_t>(m), ib = rd<int64_t>(m);
    auto n = rd<int32_t>(L);
    auto mask = rd<unsigned char>(m), keep = rd<unsigned char>(has_keep ? L : 0);
    auto oa = junk<int64_t>(m), ob = junk<int64_t>(m);
    auto src = junk<int32_t>(m), n_out = junk<int32_t>(L), info = junk<int32_t>((size_t)L * 4);
    xfh::MfArgs a = {};
    a.idx_a = ia.data(); a.idx_b = ib.data(); a.n_matches = n.data(); a.mask = mask.data(); a.keep = has_keep ? keep.data() : nullptr;
    a.cap = cap; a.min_keep = min_keep; a.out_a = oa.data(); a.out_b = ob.data(); a.src = src.data(); a.n_out = n_out.data(); a.info = info.data();
    emu::launch(L, 256, 0, [&] { xfh::filter_matches_kernel(a); });
    wr(oa); wr(ob); wr(src); wr(n_out); wr(info);
    return 0;
}
static int verify() {
    const auto h = rd<int>(7);
    const int S = h[0], P = h[1], cap = h[2], V = h[3], K = h[4], has_nv = h[5], has_err = h[6];
    if (S < 1 || P < 1 || cap < 1 || V < 2 || V > xfh::mv::MAX_VIEWS || K < 1) return 3;
    const double max_err = rd<double>(1)[0];
    const size_t pairs = (size_t)S * P, m = pairs * cap, views = (size_t)S * V;
    auto kpts = rd<float>(views * K * 2);
    auto vp = rd<int32_t>(pairs * 2);
    auto ia = rd<int64_t>(m), ib = rd<int64_t>(m);
    auto n = rd<int32_t>(pairs), nv = rd<int32_t>(has_nv ? S : 0);
    auto Ks = rd<double>(views * 9), Rs = rd<double>(views * 9), ts = rd<double>(views * 3);
    auto mask = junk<unsigned char>(m);
    auto err = junk<float>(has_err ? m : 0);
    auto info = junk<int32_t>(pairs * 4);
    xfh::VmArgs a = {};
    a.kpts = kpts.data(); a.view_pairs = vp.data(); a.idx_a = ia.data(); a.idx_b = ib.data(); a.n_matches = n.data(); a.n_views = has_nv ? nv.data() : nullptr;
    a.Ks = Ks.data(); a.Rs = Rs.data(); a.ts = ts.data(); a.P = P; a.cap = cap; a.V = V; a.K = K; a.max_err = max_err;
    a.mask = mask.data(); a.err = has_err ? err.data() : nullptr; a.info = info.data();
    emu::launch((int)pairs, 256, 0, [&] { xfh::verify_matches_kernel(a); });
    wr(mask); wr(err); wr(info);
    return 0;
}
int main() {
    int mode = 0;
    if (fread(&mode, 4, 1, stdin) != 1) return 2;
    return mode == 0 ? filter() : verify();
}
