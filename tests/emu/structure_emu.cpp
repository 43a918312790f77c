// The solver slice of csrc/k_triangulate.hip (tg_point: calibration, Lindstrom's correction, depths, status gates; tg_decompose, tg_vote,
// tg_winner: the four poses of an E and the vote among them; sliced out of the product source, behind the shared geometry of
// csrc/twoview_math.hpp, by tests/test_structure_emulated.py into structure_slice.hpp) on the host.
// stdin: mode int32, H int32, m int32, then fp64 records.
//   mode 0 (triangulate), one correspondence per record: R (9), t (3), cal (8), u0 v0 u1 v1, masked (0 / 1), thr2, cos_min, max_depth = 28
//          stdout per record: status int32, X (3) fp32, err fp32, then all the gates (H, 4) fp64
//   mode 1 (recover pose), m correspondences per record: E (9), cal (8), max_depth, then m x (u0 v0 u1 v1)
//          stdout: per record usable int32, counts (4) int32, winner int32; then per record Ra (9) Rb (9) t (3) En (9) fp64
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::floor;
using std::sqrt;
#include "structure_slice.hpp"
}  // namespace xfh
int main() {
    int hdr[3] = {0, 0, 0};
    if (fread(hdr, 4, 3, stdin) != 3) return 2;
    const int mode = hdr[0], H = hdr[1], m = hdr[2];
    const size_t rec = mode == 0 ? 28 : 18 + 4 * (size_t)m;
    std::vector<double> in((size_t)H * rec);
    if (fread(in.data(), 8, in.size(), stdin) != in.size()) return 2;
    if (mode == 0) {
        std::vector<int32_t> st(H);
        std::vector<float> xe((size_t)H * 4);
        std::vector<double> gate((size_t)H * 4);
        for (int h = 0; h < H; ++h) {
            const double* r = in.data() + (size_t)h * rec;
            double E[9];
            xfh::tg_pose_E(r, r + 9, E);
            float X3[3], err;
            st[h] = xfh::tg_point(r, r + 9, E, xfh::tg_pose_ok(r, r + 9), r + 12, r[20], r[21], r[22], r[23], r[24] != 0.0, r[25], r[26], r[27], X3, err,
                                  gate.data() + (size_t)h * 4);
            for (int k = 0; k < 3; ++k) xe[(size_t)h * 4 + k] = X3[k];
            xe[(size_t)h * 4 + 3] = err;
        }
        fwrite(st.data(), 4, H, stdout);
        fwrite(xe.data(), 4, xe.size(), stdout);
        fwrite(gate.data(), 8, gate.size(), stdout);
        return 0;
    }
    std::vector<int32_t> iv((size_t)H * 6);
    std::vector<double> dv((size_t)H * 30);
    for (int h = 0; h < H; ++h) {
        const double* r = in.data() + (size_t)h * rec;
        double* o = dv.data() + (size_t)h * 30;
        const bool usable = xfh::tg_decompose(r, o, o + 9, o + 18, o + 21);
        int c[4] = {0, 0, 0, 0};
        for (int i = 0; i < m; ++i) {
            const double* p = r + 18 + 4 * i;
            const xfh::TgRays q = xfh::tg_correct(o + 21, r + 9, p[0], p[1], p[2], p[3]);
            double X[3];
            c[0] += xfh::tg_vote<0>(o, o + 9, o + 18, usable, q, r[17], X) == xfh::tg::VALID;
            c[1] += xfh::tg_vote<1>(o, o + 9, o + 18, usable, q, r[17], X) == xfh::tg::VALID;
            c[2] += xfh::tg_vote<2>(o, o + 9, o + 18, usable, q, r[17], X) == xfh::tg::VALID;
            c[3] += xfh::tg_vote<3>(o, o + 9, o + 18, usable, q, r[17], X) == xfh::tg::VALID;
        }
        int32_t* q = iv.data() + (size_t)h * 6;
        q[0] = usable ? 1 : 0;
        for (int k = 0; k < 4; ++k) q[1 + k] = c[k];
        q[5] = xfh::tg_winner(c[0], c[1], c[2], c[3]);
    }
    fwrite(iv.data(), 4, iv.size(), stdout);
    fwrite(dv.data(), 8, dv.size(), stdout);
    return 0;
}
