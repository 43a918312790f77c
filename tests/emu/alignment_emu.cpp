// The solver slice of csrc/k_align.hip (al_solve, al_fit from its centred sums, the residual and its cost; sliced out of the product
// source, behind the shared geometry of csrc/twoview_math.hpp, by tests/test_alignment_emulated.py into alignment_slice.hpp) on the host.
// The slice's constants (namespace al: the Jacobi sweep count, the collinearity threshold, the model's layout) come with it.
// stdin: H, with_scale int32, thr2 fp64, then A (H, 9), B (H, 9), S (H, 10), ca (H, 3), cb (H, 3) fp64.
// stdout: ok_solve (H), ok_fit (H), cost (H) int32, then solved models (H, 13), fitted models (H, 13) (zeros where there is none) and
// r2 (H) fp64: the squared residual of sample h's third correspondence under the model fitted to cloud h (0 where there is none), and
// `cost` its MSAC cost at thr2.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::floor;
using std::sqrt;
#include "alignment_slice.hpp"
}  // namespace xfh
int main() {
    int hdr[2] = {0, 0};
    double thr2 = 0.0;
    if (fread(hdr, 4, 2, stdin) != 2 || fread(&thr2, 8, 1, stdin) != 1) return 2;
    const int H = hdr[0], with_scale = hdr[1];
    std::vector<double> in((size_t)H * 34);
    if (fread(in.data(), 8, in.size(), stdin) != in.size()) return 2;
    const double* A = in.data();
    const double* B = A + (size_t)H * 9;
    const double* S = B + (size_t)H * 9;
    const double* ca = S + (size_t)H * 10;
    const double* cb = ca + (size_t)H * 3;
    std::vector<int> oks(H), okf(H), cost(H, 0);
    std::vector<double> ms((size_t)H * 13, 0.0), mf((size_t)H * 13, 0.0), r2(H, 0.0);
    for (int h = 0; h < H; ++h) {
        double m[13];
        oks[h] = xfh::al_solve(A + (size_t)h * 9, B + (size_t)h * 9, with_scale, m) ? 1 : 0;
        if (oks[h])
            for (int k = 0; k < 13; ++k) ms[(size_t)h * 13 + k] = m[k];
        okf[h] = xfh::al_fit(S + (size_t)h * 10, ca + (size_t)h * 3, cb + (size_t)h * 3, with_scale, m) ? 1 : 0;
        if (okf[h]) {
            for (int k = 0; k < 13; ++k) mf[(size_t)h * 13 + k] = m[k];
            double sR[9];
            xfh::al_scaled_rotation(m, sR);
            const double* a = A + (size_t)h * 9 + 6;
            const double* b = B + (size_t)h * 9 + 6;
            r2[h] = xfh::al_residual2(sR, m + 9, a[0], a[1], a[2], b[0], b[1], b[2]);
            cost[h] = (int)xfh::al_cost(r2[h], thr2);
        }
    }
    fwrite(oks.data(), 4, H, stdout);
    fwrite(okf.data(), 4, H, stdout);
    fwrite(cost.data(), 4, H, stdout);
    fwrite(ms.data(), 8, ms.size(), stdout);
    fwrite(mf.data(), 8, mf.size(), stdout);
    fwrite(r2.data(), 8, r2.size(), stdout);
    return 0;
}
