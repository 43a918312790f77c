// The pose-graph slice of csrc/k_triangulate.hip (pg_keys, pg_tree, pg_rot_weights, pg_rot_assemble, pg_rot_solve, pg_directions,
// pg_pos_weights, pg_pos_assemble, pg_pos_solve, pg_run; sliced out of the product source behind the two-view, the views-solver and the
// bundle-solver slices by tests/test_posegraph_emulated.py into posegraph_slice.hpp) on the host, as one thread of one: every loop of the
// slice strides by the thread count, the sums keep rs::block_sums' order whatever that count is.
// stdin: G int32, then per scene fp64: V, nv, P, iterations, redescend, rot scale, pos scale, min pivot ratio, P x (a, b, R (9), t (3), weight)
// stdout per scene fp64: the stages -- 32 tree edges, the mask, n_r, 32 x 9 rotations after the tree, P x 3 residuals and P factors of round 0,
//        496 + 96 packed Laplacian and right-hand sides, 96 solutions, P x 3 directions, 4371 + 93 packed M and g of round 0, ok, mu, the
//        smallest pivot ratio, 32 x 3 centres after round 0 -- then the whole run: 8 info, the mask, V x 9 Rs, V x 3 ts, P x 2 factors
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
#include "posegraph_slice.hpp"
}  // namespace xfh
using namespace xfh;
struct NoSync {
    void operator()() const {}
};
int main() {
    int G = 0;
    if (fread(&G, 4, 1, stdin) != 1) return 2;
    std::vector<double> out;
    for (int g = 0; g < G; ++g) {
        double hdr[8];
        if (fread(hdr, 8, 8, stdin) != 8) return 2;
        const int V = (int)hdr[0], nv = (int)hdr[1], P = (int)hdr[2];
        if (V < 2 || V > mv::MAX_VIEWS || nv < 0 || nv > V || P < 1) return 3;
        std::vector<double> rec((size_t)P * 15);
        if (fread(rec.data(), 8, rec.size(), stdin) != rec.size()) return 2;
        std::vector<int32_t> pairs((size_t)P * 2), key(P), info(8), reg(1);
        std::vector<double> Rrel((size_t)P * 9), trel((size_t)P * 3), weight(P), Rs((size_t)V * 9), ts((size_t)V * 3), factor((size_t)P * 2);
        std::vector<double> wd((size_t)P * 9), lds(pg::L_END, 0.0);
        std::vector<int> ldi(pg::I_END, 0);
        for (int p = 0; p < P; ++p) {
            const double* r = &rec[(size_t)p * 15];
            pairs[2 * p] = (int32_t)r[0]; pairs[2 * p + 1] = (int32_t)r[1];
            for (int j = 0; j < 9; ++j) Rrel[(size_t)9 * p + j] = r[2 + j];
            for (int j = 0; j < 3; ++j) trel[(size_t)3 * p + j] = r[11 + j];
            weight[p] = r[14];
        }
        PgScene s;
        s.pairs = pairs.data(); s.Rrel = Rrel.data(); s.trel = trel.data(); s.weight = weight.data();
        s.nv = nv; s.P = P; s.V = V; s.iterations = (int)hdr[3]; s.redescend = (int)hdr[4]; s.crot = hdr[5]; s.cpos = hdr[6]; s.min_ratio = hdr[7];
        s.Rs = Rs.data(); s.ts = ts.data(); s.registered = reg.data(); s.factor = factor.data(); s.info = info.data();
        s.key = key.data(); s.wcur = wd.data(); s.res = wd.data() + P; s.dir = wd.data() + (size_t)4 * P; s.ta = wd.data() + (size_t)7 * P;
        s.tb = wd.data() + (size_t)8 * P;
        s.lds = lds.data(); s.ldi = ldi.data();
        const NoSync sync;
        // ---- the stages
        pg_keys(s, 0, 1, sync);
        pg_tree(s, 0, 1, sync);
        for (int i = 0; i < 32; ++i) out.push_back((double)ldi[pg::I_TREE + i]);
        out.push_back((double)(unsigned)ldi[pg::I_REG]);
        const int nr = ldi[pg::I_NR];
        out.push_back((double)nr);
        out.insert(out.end(), lds.begin() + pg::L_ROT, lds.begin() + pg::L_ROT + 288);
        std::vector<double> st((size_t)P * 4 + 592 + 96 + (size_t)P * 3 + pg::TRI + pg::NPOS + 3 + 96, 0.0);
        if (nr > 0) {
            double* d = st.data();
            pg_rot_weights(s, pg_kind(s, 0), 0, 1, sync);
            for (int i = 0; i < 3 * P; ++i) d[i] = s.res[i];
            d += (size_t)3 * P;
            for (int p = 0; p < P; ++p) d[p] = factor[(size_t)2 * p];
            d += P;
            pg_rot_assemble(s, 0, 1, sync);
            for (int i = 0; i < nr * (nr + 1) / 2; ++i) d[i] = lds[pg::L_SYS + pg::R_TRI + i];
            for (int i = 0; i < 96; ++i) d[496 + i] = i % 32 < nr ? lds[pg::L_SYS + pg::R_RHS + i] : 0.0;
            d += 592;
            pg_rot_solve(s, 0, 1, sync);
            for (int i = 0; i < 96; ++i) d[i] = i % 32 < nr ? lds[pg::L_SYS + pg::R_RHS + i] : 0.0;
            d += 96;
            for (int k = 1; k < s.iterations; ++k) {
                pg_rot_weights(s, pg_kind(s, k), 0, 1, sync);
                pg_rot_assemble(s, 0, 1, sync);
                pg_rot_solve(s, 0, 1, sync);
            }
            pg_directions(s, 0, 1, sync);
            for (int i = 0; i < 3 * P; ++i) d[i] = s.dir[i];
            d += (size_t)3 * P;
            pg_pos_weights(s, pg_kind(s, 0), true, 0, 1, sync);
            pg_pos_assemble(s, 0, 1, sync);
            const int n = 3 * nr;
            for (int i = 0; i < n * (n + 1) / 2; ++i) d[i] = lds[pg::L_SYS + i];
            for (int i = 0; i < n; ++i) d[pg::TRI + i] = lds[pg::L_RHS + i];
            d += pg::TRI + pg::NPOS;
            lds[pg::L_SC + 1] = 0.0;
            const bool ok = pg_pos_solve(s, 0, 1, sync);
            d[0] = ok ? 1.0 : 0.0; d[1] = lds[pg::L_SC]; d[2] = lds[pg::L_SC + 1];
            d += 3;
            if (ok) for (int i = 0; i < 96; ++i) d[i] = lds[pg::L_CEN + i];
        }
        out.insert(out.end(), st.begin(), st.end());
        // ---- the whole run
        pg_run(s, 0, 1, sync);
        for (int i = 0; i < 8; ++i) out.push_back((double)info[i]);
        out.push_back((double)(unsigned)reg[0]);
        out.insert(out.end(), Rs.begin(), Rs.end());
        out.insert(out.end(), ts.begin(), ts.end());
        out.insert(out.end(), factor.begin(), factor.end());
    }
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
