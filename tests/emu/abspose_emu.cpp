// ap_solve (csrc/k_abspose.hip: the P3P quartic, its root isolation, the pose from the two triangle frames; sliced out of the product
// source, behind the shared geometry of csrc/twoview_math.hpp, by tests/test_abspose_emulated.py into abspose_slice.hpp) on the host.
// The solver's constants (namespace ap: bisection / Newton steps, thresholds, candidate layout) come with the slice.
// stdin: H int32, then x (H, 3), y (H, 3), X (H, 3, 3) fp64; stdout: ncand (H) int32, candidates (H, 4, 12) fp64 (zeros beyond ncand).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::floor;
using std::sqrt;
#include "abspose_slice.hpp"
}  // namespace xfh
int main() {
    int H = 0;
    if (fread(&H, 4, 1, stdin) != 1) return 2;
    std::vector<double> in((size_t)H * 15);
    if (fread(in.data(), 8, in.size(), stdin) != in.size()) return 2;
    std::vector<int> nc(H);
    std::vector<double> out((size_t)H * 48, 0.0);
    const double* x = in.data();
    const double* y = x + (size_t)H * 3;
    const double* X = y + (size_t)H * 3;
    for (int h = 0; h < H; ++h) {
        double cand[48];
        nc[h] = xfh::ap_solve(x + (size_t)h * 3, y + (size_t)h * 3, X + (size_t)h * 9, cand);
        for (int k = 0; k < 12 * nc[h]; ++k) out[(size_t)h * 48 + k] = cand[k];
    }
    fwrite(nc.data(), 4, H, stdout);
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
