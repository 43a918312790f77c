// The map slice of csrc/k_map.hip (map_gather_kernel, map_scan_kernel, map_move_kernel, map_project_kernel; sliced out of the product source by
// tests/test_localization_emulated.py into map_slice.hpp) on the host: one thread per work-item, the row-of-16 DPP exchanges and the wave
// ballots of emu.hpp, the three launches of launch_build_map in their order.
// stdin: int32 mode.
//   mode 0 (xfh_build_map): int32 S, V, T, Kcap, min_views, M; desc (S,V,Kcap,64) f32, tracks (S,T,V) i32, points3d (S,T,3) f32, status (S,T) u8,
//     inlier_views (S,T) i32.  stdout: points (S,M,3) f32, desc (S,M,64) f32, desc_f16 (S,M,64) u16, track (S,M) i32, n_obs (S,M) u8,
//     coherence (S,M) f32, n_points (S) i32, info (S,8) i32.  Every output starts as 0xa5 bytes: whatever the kernels leave unwritten shows.
//   mode 1 (xfh_map_project): int32 Q, M, has_n; f64 width, height, margin; points (Q,M,3) f32, n_points (Q) i32 (if has_n), R (Q,9), t (Q,3),
//     K (Q,9) f64.  stdout: uv (Q,M,2) f32.
#include "emu.hpp"
#include <cstdio>
struct ushort4 { unsigned short x, y, z, w; };
inline ushort4 make_ushort4(unsigned short x, unsigned short y, unsigned short z, unsigned short w) { return ushort4{x, y, z, w}; }
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#define __shared__ static
#define __global__
namespace xfh {
#include "map_slice.hpp"
}
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
static int build() {
    const auto h = rd<int>(6);
    const int S = h[0], V = h[1], T = h[2], kcap = h[3], min_views = h[4], M = h[5];
    if (S < 1 || V < 1 || V > xfh::mp::MAX_VIEWS || T < 0 || kcap < 1 || M < 1) return 3;
    const size_t n = (size_t)S * T, m = (size_t)S * M;
    auto desc = rd<float>((size_t)S * V * kcap * 64);
    auto tracks = rd<int32_t>(n * V);
    auto pts = rd<float>(n * 3);
    auto status = rd<unsigned char>(n);
    auto inl = rd<int32_t>(n);
    auto w_desc = junk<float>(n * 64), w_coh = junk<float>(n);
    auto w_dst = junk<int32_t>(n);
    auto w_nobs = junk<unsigned char>(n), w_flag = junk<unsigned char>(n);
    auto points = junk<float>(m * 3), out_desc = junk<float>(m * 64), coh = junk<float>(m);
    auto f16 = junk<unsigned short>(m * 64);
    auto track = junk<int32_t>(m), n_points = junk<int32_t>(S), info = junk<int32_t>((size_t)S * 8);
    auto n_obs = junk<unsigned char>(m);
    xfh::MapArgs a = {};
    a.desc = desc.data(); a.tracks = tracks.data(); a.points3d = pts.data(); a.status = status.data(); a.inlier_views = inl.data();
    a.T = T; a.V = V; a.Kcap = kcap; a.min_views = min_views; a.M = M;
    a.w_desc = w_desc.data(); a.w_coh = w_coh.data(); a.w_dst = w_dst.data(); a.w_nobs = w_nobs.data(); a.w_flag = w_flag.data();
    a.points = points.data(); a.out_desc = out_desc.data(); a.desc_f16 = f16.data(); a.track = track.data(); a.n_obs = n_obs.data();
    a.coherence = coh.data(); a.n_points = n_points.data(); a.info = info.data();
    const int g1 = (T + 15) / 16, g3 = ((T > M ? T : M) + 15) / 16;
    a.groups = g1 ? g1 : 1;
    emu::launch(g1 * S, 256, 0, [&] { xfh::map_gather_kernel(a); });
    emu::launch(S, 256, 0, [&] { xfh::map_scan_kernel(a); });
    a.groups = g3;
    emu::launch(g3 * S, 256, 0, [&] { xfh::map_move_kernel(a); });
    wr(points); wr(out_desc); wr(f16); wr(track); wr(n_obs); wr(coh); wr(n_points); wr(info);
    return 0;
}
static int project() {
    const auto h = rd<int>(3);
    const int Q = h[0], M = h[1], has_n = h[2];
    if (Q < 1 || M < 1) return 3;
    const auto size = rd<double>(3);
    auto pts = rd<float>((size_t)Q * M * 3);
    auto n = rd<int32_t>(has_n ? Q : 0);
    auto R = rd<double>((size_t)Q * 9), t = rd<double>((size_t)Q * 3), K = rd<double>((size_t)Q * 9);
    auto uv = junk<float>((size_t)Q * M * 2);
    xfh::MapProjectArgs a = {};
    a.points = pts.data(); a.n_points = has_n ? n.data() : nullptr; a.R = R.data(); a.t = t.data(); a.K = K.data(); a.M = M; a.groups = (M + 255) / 256;
    a.width = size[0]; a.height = size[1]; a.margin = size[2]; a.uv = uv.data();
    emu::launch(a.groups * Q, 256, 0, [&] { xfh::map_project_kernel(a); });
    wr(uv);
    return 0;
}
int main() {
    int mode = 0;
    if (fread(&mode, 4, 1, stdin) != 1) return 2;
    return mode == 0 ? build() : project();
}
