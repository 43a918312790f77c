// fm_solve and fm_fit8 (csrc/k_fundamental.hip: the 7-point solver with the oriented constraint, the 8-point fit with its Jacobi sweeps;
// sliced out of the product source, behind the shared geometry of csrc/twoview_math.hpp, by tests/test_fundamental_emulated.py into
// fundamental_slice.hpp) on the host, with the per-thread
// LDS slice as a plain array (stride 1).
// stdin: mode int32, H int32, then
//   mode 0 (solver): oriented int32, x0 y0 x1 y1 (H, 7) fp64 each, conditioning (H, 6) fp64; stdout: ncand (H) int32, candidates (H, 3, 9)
//   mode 1 (fit8): sums (H, 45) fp64, conditioning (H, 6) fp64; stdout: ok (H) int32, F (H, 9) fp64
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::sqrt;
#include "fundamental_slice.hpp"
}  // namespace xfh
int main() {
    int mode = 0, H = 0;
    if (fread(&mode, 4, 1, stdin) != 1 || fread(&H, 4, 1, stdin) != 1) return 2;
    if (mode == 0) {
        int oriented = 1;
        if (fread(&oriented, 4, 1, stdin) != 1) return 2;
        std::vector<double> in((size_t)H * 28), nt((size_t)H * 6);
        if (fread(in.data(), 8, in.size(), stdin) != in.size() || fread(nt.data(), 8, nt.size(), stdin) != nt.size()) return 2;
        std::vector<int> nc(H);
        std::vector<double> out((size_t)H * 27, 0.0);
        double slice[xfh::fm::SLICE];
        for (int h = 0; h < H; ++h) {
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 7; ++k) slice[xfh::FM_PTS + 7 * c + k] = in[(size_t)c * H * 7 + (size_t)h * 7 + k];
            const double* q = &nt[(size_t)h * 6];
            const xfh::FmNorm t{q[0], q[1], q[2], q[3], q[4], q[5]};
            nc[h] = xfh::fm_solve(xfh::tv::Slice<1>{slice}, t, oriented != 0, &out[(size_t)h * 27]);
        }
        fwrite(nc.data(), 4, H, stdout);
        fwrite(out.data(), 8, out.size(), stdout);
        return 0;
    }
    std::vector<double> sm((size_t)H * 45), nt((size_t)H * 6);
    if (fread(sm.data(), 8, sm.size(), stdin) != sm.size() || fread(nt.data(), 8, nt.size(), stdin) != nt.size()) return 2;
    std::vector<int> ok(H);
    std::vector<double> out((size_t)H * 9, 0.0);
    double A[81], V[81];
    for (int h = 0; h < H; ++h) {
        const double* q = &nt[(size_t)h * 6];
        const xfh::FmNorm t{q[0], q[1], q[2], q[3], q[4], q[5]};
        ok[h] = xfh::fm_fit8(&sm[(size_t)h * 45], A, V, t, &out[(size_t)h * 9]) ? 1 : 0;
    }
    fwrite(ok.data(), 4, H, stdout);
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
