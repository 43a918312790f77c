// relpose_solve (csrc/k_relpose.hip: Nister's five-point solver, decomposition and cheirality; sliced out of the product source, behind
// the shared geometry of csrc/twoview_math.hpp, by tests/test_relpose_emulated.py into relpose_slice.hpp) on the host, with the per-thread LDS slice as a plain array (stride 1).
// The solver's constants (namespace rp: bisection / Newton steps, candidate layout) come with the slice.
// stdin: H int32, then x1 y1 x2 y2 (H, 5) fp64 each; stdout: ncand (H) int32, candidates (H, 10, 12) fp64 (zeros beyond ncand).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::sqrt;
#include "relpose_slice.hpp"
}  // namespace xfh
int main() {
    int H = 0;
    if (fread(&H, 4, 1, stdin) != 1) return 2;
    std::vector<double> in((size_t)H * 20);
    if (fread(in.data(), 8, in.size(), stdin) != in.size()) return 2;
    std::vector<int> nc(H);
    std::vector<double> out((size_t)H * 120, 0.0);
    double slice[280];
    for (int h = 0; h < H; ++h) {
        for (int c = 0; c < 4; ++c)
            for (int k = 0; k < 5; ++k) slice[xfh::RP_PTS + 5 * c + k] = in[(size_t)c * H * 5 + (size_t)h * 5 + k];
        nc[h] = xfh::relpose_solve(xfh::tv::Slice<1>{slice}, &out[(size_t)h * 120]);
    }
    fwrite(nc.data(), 4, H, stdout);
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
