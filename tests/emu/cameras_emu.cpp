// The cameras slice of csrc/k_cameras.hip (camera_points_kernel, undistort_images_kernel; sliced out of the product source by
// tests/test_cameras_emulated.py into cameras_slice.hpp) on the host: one thread per work-item, the grids of launch_camera_points /
// launch_undistort_images (workgroups of 256; the images' grid y and z are walked here, one emu::launch over x for each).
// stdin: int32 mode.
//   mode 0 (xfh_camera_points): int32 P, K, n_cameras, has_counts, has_other, direction; pts (P,K,2) f32, counts (P) i32 (if has_counts),
//     kind (n_cameras) i32, params (n_cameras,12) f64, k_other (n_cameras,4) f64 (if has_other).  stdout: out (P,K,2) f32, status (P,K) u8.
//   mode 1 (xfh_undistort_images): int32 is_f32, B, C, H, W, n_cameras, has_new, Ho, Wo, has_valid; f64 fill; src (B,C,H,W), kind, params,
//     k_new (n_cameras,4) f64 (if has_new).  stdout: dst (B,C,Ho,Wo), valid (B,Ho,Wo) u8 (if has_valid).
// Every output starts as 0xa5 bytes: whatever the kernels leave unwritten shows.
#include "emu.hpp"
#include <cstdio>
#include <cstdlib>
#define __global__
namespace xfh {
using std::atan;
using std::fabs;
using std::floor;
using std::sqrt;
using std::tan;
#include "cameras_slice.hpp"
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
static int points() {
    const auto h = rd<int>(6);
    const int P = h[0], K = h[1], nc = h[2], has_counts = h[3], has_other = h[4], direction = h[5];
    if (P < 1 || K < 1 || (nc != 1 && nc != P)) return 3;
    const size_t n = (size_t)P * K;
    auto pts = rd<float>(n * 2);
    auto counts = rd<int32_t>(has_counts ? P : 0);
    auto kind = rd<int32_t>(nc);
    auto params = rd<double>((size_t)nc * 12), other = rd<double>(has_other ? (size_t)nc * 4 : 0);
    auto out = junk<float>(n * 2);
    auto status = junk<unsigned char>(n);
    xfh::CamPointsArgs a = {};
    a.pts = pts.data(); a.counts = has_counts ? counts.data() : nullptr; a.kind = kind.data(); a.params = params.data();
    a.k_other = has_other ? other.data() : nullptr; a.total = (long long)n; a.K = K; a.n_cameras = nc; a.direction = direction;
    a.out = out.data(); a.status = status.data();
    emu::launch((int)((n + 255) / 256), 256, 0, [&] { xfh::camera_points_kernel(a); });
    wr(out); wr(status);
    return 0;
}
template <typename T> static int images(const std::vector<int>& h) {
    const int B = h[1], C = h[2], H = h[3], W = h[4], nc = h[5], has_new = h[6], Ho = h[7], Wo = h[8], has_valid = h[9];
    if (B < 1 || C < 1 || C > xfh::cam::MAX_CHANNELS || H < 1 || W < 1 || Ho < 1 || Wo < 1 || (nc != 1 && nc != B)) return 3;
    const double fill = rd<double>(1)[0];
    auto src = rd<T>((size_t)B * C * H * W);
    auto kind = rd<int32_t>(nc);
    auto params = rd<double>((size_t)nc * 12), k_new = rd<double>(has_new ? (size_t)nc * 4 : 0);
    auto dst = junk<T>((size_t)B * C * Ho * Wo);
    auto valid = junk<unsigned char>(has_valid ? (size_t)B * Ho * Wo : 0);
    xfh::CamImagesArgs a = {};
    a.src = src.data(); a.dst = dst.data(); a.valid = has_valid ? valid.data() : nullptr; a.kind = kind.data(); a.params = params.data();
    a.k_new = has_new ? k_new.data() : nullptr; a.C = C; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.n_cameras = nc; a.fill = fill;
    for (int z = 0; z < B; ++z)
        for (int y = 0; y < (Ho + 3) / 4; ++y)
            emu::launch((Wo + 63) / 64, 256, 0, [&] {
                emu::bidx.y = (unsigned)y; emu::bidx.z = (unsigned)z;
                xfh::undistort_images_kernel<T>(a);
            });
    wr(dst); wr(valid);
    return 0;
}
int main() {
    int mode = 0;
    if (fread(&mode, 4, 1, stdin) != 1) return 2;
    if (mode == 0) return points();
    const auto h = rd<int>(10);
    return h[0] ? images<float>(h) : images<unsigned char>(h);
}
