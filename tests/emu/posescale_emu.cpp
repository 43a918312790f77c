// The two slices of csrc/posescale_body.hpp (ps_wedge with what it calls; PgRatioTerms under pg_run_with) on the host, behind the slices of
// csrc/k_triangulate.hip that they call into (tests/test_posescale_emulated.py writes them into posescale_slice.hpp), as one thread of one:
// every loop strides by the thread count, the integer "atomics" are plain additions.
// stdin: G int32, then per scene fp64: V, nv, P, K, T, min_common, max_reproj_error, cos_min, max_depth, iterations, redescend, rot scale, pos
//        scale, min pivot ratio, scale_weight, scale_tol, P x (a, b, R (9), t (3), weight), V x 9 intrinsics, V x K x 2 pixels, T x V tracks,
//        V x K track_of
// stdout per scene fp64: P x P ratios, counts, shared views, 8 info; 4371 + 93 packed M and g of round 0 with the ratio terms, ok, mu, the
//        smallest pivot ratio, 32 x 3 centres after round 0; then the whole run: 8 info, the mask, V x 9 Rs, V x 3 ts, P x 2 factors, P x P
//        ratio factors
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::floor;
using std::sqrt;
#include "posescale_slice.hpp"
}  // namespace xfh
using namespace xfh;
struct NoSync {
    void operator()() const {}
};
struct PlainMem {
    int add(int* p, int v) const { const int old = *p; *p += v; return old; }
};
static bool rd(std::vector<double>& v) { return fread(v.data(), 8, v.size(), stdin) == v.size(); }
int main() {
    int G = 0;
    if (fread(&G, 4, 1, stdin) != 1) return 2;
    std::vector<double> out;
    for (int g = 0; g < G; ++g) {
        std::vector<double> hdr(16);
        if (!rd(hdr)) return 2;
        const int V = (int)hdr[0], nv = (int)hdr[1], P = (int)hdr[2], K = (int)hdr[3], T = (int)hdr[4];
        if (V < 2 || V > mv::MAX_VIEWS || nv < 0 || nv > V || P < 1 || P > ps::MAX_PAIRS || K < 1 || K > ps::MAX_K || T < 1) return 3;
        std::vector<double> rec((size_t)P * 15), Ks((size_t)V * 9), px((size_t)V * K * 2), tr((size_t)T * V), tof((size_t)V * K);
        if (!rd(rec) || !rd(Ks) || !rd(px) || !rd(tr) || !rd(tof)) return 2;
        std::vector<int32_t> pairs((size_t)P * 2), key(P), info(8), reg(1), tracks(tr.size()), track_of(tof.size());
        std::vector<float> kpts(px.size());
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
        for (size_t i = 0; i < px.size(); ++i) kpts[i] = (float)px[i];
        for (size_t i = 0; i < tr.size(); ++i) tracks[i] = (int32_t)tr[i];
        for (size_t i = 0; i < tof.size(); ++i) track_of[i] = (int32_t)tof[i];
        const NoSync sync;
        // ---- the ratios
        std::vector<double> ratio((size_t)P * P), vals(ps::MAX_K), stage(2 * ps::STAGE);
        std::vector<int32_t> count((size_t)P * P), shared((size_t)P * P), rinfo(8, 0);
        int cnt[2] = {0, 0};
        PsScene q;
        q.kpts = kpts.data(); q.tracks = tracks.data(); q.track_of = track_of.data(); q.pairs = pairs.data(); q.Rrel = Rrel.data(); q.trel = trel.data();
        q.weight = weight.data(); q.Ks = Ks.data(); q.nv = nv; q.P = P; q.V = V; q.K = K; q.T = T; q.min_common = (int)hdr[5];
        q.thr2 = hdr[6] * hdr[6]; q.cos_min = hdr[7]; q.max_depth = hdr[8]; q.pad = std::numeric_limits<double>::infinity();
        q.ratio = ratio.data(); q.count = count.data(); q.shared = shared.data(); q.info = rinfo.data();
        for (int a = 0; a < P; ++a)
            for (int b = 0; b < P; ++b) ps_wedge(q, a, b, vals.data(), stage.data(), cnt, PlainMem(), 0, 1, sync);
        out.insert(out.end(), ratio.begin(), ratio.end());
        for (int32_t c : count) out.push_back((double)c);
        for (int32_t c : shared) out.push_back((double)c);
        for (int32_t c : rinfo) out.push_back((double)c);
        // ---- the pose graph with them
        PgScene s;
        s.pairs = pairs.data(); s.Rrel = Rrel.data(); s.trel = trel.data(); s.weight = weight.data();
        s.nv = nv; s.P = P; s.V = V; s.iterations = (int)hdr[9]; s.redescend = (int)hdr[10]; s.crot = hdr[11]; s.cpos = hdr[12]; s.min_ratio = hdr[13];
        s.Rs = Rs.data(); s.ts = ts.data(); s.registered = reg.data(); s.factor = factor.data(); s.info = info.data();
        s.key = key.data(); s.wcur = wd.data(); s.res = wd.data() + P; s.dir = wd.data() + (size_t)4 * P; s.ta = wd.data() + (size_t)7 * P;
        s.tb = wd.data() + (size_t)8 * P;
        s.lds = lds.data(); s.ldi = ldi.data();
        const size_t nw = (size_t)P * (P - 1) / 2 + 1;
        std::vector<double> rfac((size_t)P * P), ld(3 * nw);
        std::vector<int32_t> row(P + 1);
        std::vector<long long> list(nw);
        PgRatioTerms x;
        x.ratio = ratio.data(); x.count = count.data(); x.weight = hdr[14]; x.tol = hdr[15]; x.factor = rfac.data(); x.row = row.data();
        x.list = list.data(); x.lr = ld.data(); x.lsr = ld.data() + nw; x.lw = ld.data() + 2 * nw;
        pg_keys(s, 0, 1, sync);
        pg_tree(s, 0, 1, sync);
        x.prepare(s, 0, 1, sync);
        const int nr = ldi[pg::I_NR];
        std::vector<double> st((size_t)pg::TRI + pg::NPOS + 3 + 96, 0.0);
        if (nr > 0) {
            double* d = st.data();
            for (int k = 0; k < s.iterations; ++k) {
                pg_rot_weights(s, pg_kind(s, k), 0, 1, sync);
                pg_rot_assemble(s, 0, 1, sync);
                pg_rot_solve(s, 0, 1, sync);
            }
            pg_directions(s, 0, 1, sync);
            pg_pos_weights(s, pg_kind(s, 0), true, 0, 1, sync);
            x.weights(s, pg_kind(s, 0), true, 0, 1, sync);
            pg_pos_assemble(s, 0, 1, sync);
            x.assemble(s, 0, 1, sync);
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
        pg_run_with(s, x, 0, 1, sync);
        for (int i = 0; i < 8; ++i) out.push_back((double)info[i]);
        out.push_back((double)(unsigned)reg[0]);
        out.insert(out.end(), Rs.begin(), Rs.end());
        out.insert(out.end(), ts.begin(), ts.end());
        out.insert(out.end(), factor.begin(), factor.end());
        out.insert(out.end(), rfac.begin(), rfac.end());
    }
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
