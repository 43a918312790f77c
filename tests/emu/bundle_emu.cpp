// The bundle-solver slice of csrc/k_triangulate.hip (ba_mask, ba_cost, ba_term, ba_point, ba_pair_add, ba_cholesky_solve, ba_pose_update,
// ba_point_step, ba_decide; sliced out of the product source behind the two-view and the views-solver slices by tests/test_bundle_emulated.py
// into bundle_slice.hpp) on the host, driven as the launches drive it: sums over tracks in rs::block_sums' order (thread k % 256 takes its
// tracks in order, 8 segments of 32 threads, a tree), sums over chunks of 256 tracks ascending.
// stdin: G int32, then per scene fp64: V, nv, K, fixed_views, max_iterations, huber, V x (R (9), t (3), K (9)), K x V x (u, v, in range 0 / 1),
//        K x inlier mask, K x X (3)
// stdout per scene fp64: status, free views, iterations, accepted, refined, observations, cost0, cost; K masks; the first round (zeros
//        without one): K x V x 21 terms (du, dv, wt, jp 6, jc 12), K x 10 (V^-1 6, g 3, held), n x n lower triangle, n rhs, ok, n solution,
//        V x 12 candidate poses, K x 3 candidate points, candidate cost, failed; then V x 12 poses, K x 3 points (fp64 state), K x 3 points
//        as the outputs' fp32
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
#include "bundle_slice.hpp"
}  // namespace xfh
using namespace xfh;
struct HostObs {
    const double* p;          // V x (u, v, in range)
    bool operator()(int w, double& u, double& v) const {
        const bool in = p[3 * w + 2] != 0.0;
        u = in ? p[3 * w] : (double)NAN;
        v = in ? p[3 * w + 1] : (double)NAN;
        return in;
    }
};
struct NoSync {
    void operator()() const {}
};
// rs::block_sums over per-thread values acc[256][N]
static void block_sums(const std::vector<double>& acc, int N, double* out) {
    for (int k = 0; k < N; ++k) {
        double q[8];
        for (int j = 0; j < 8; ++j) {
            double t = 0.0;
            for (int i = 0; i < 32; ++i) t += acc[(size_t)(32 * j + i) * N + k];
            q[j] = t;
        }
        out[k] = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7])));
    }
}
static double chunk_sum(const std::vector<double>& per_track) {
    double tot = 0.0;
    const int K = (int)per_track.size();
    for (int a = 0; a < K; a += 256) {
        std::vector<double> acc(256, 0.0);
        for (int k = a; k < K && k < a + 256; ++k) acc[k - a] = per_track[k];
        double s;
        block_sums(acc, 1, &s);
        tot = tot + s;
    }
    return tot;
}
static void stage(const std::vector<double>& pose, const std::vector<double>& cam, int V, std::vector<double>& vd) {
    for (int v = 0; v < V; ++v) mv_stage_pose(&pose[(size_t)v * 12], &pose[(size_t)v * 12 + 9], &cam[(size_t)v * 21 + 12], &vd[(size_t)v * ba::STRIDE]);
}
int main() {
    int G = 0;
    if (fread(&G, 4, 1, stdin) != 1) return 2;
    std::vector<double> out;
    for (int g = 0; g < G; ++g) {
        double hdr[6];
        if (fread(hdr, 8, 6, stdin) != 6) return 2;
        const int V = (int)hdr[0], nv = (int)hdr[1], K = (int)hdr[2], iters_max = (int)hdr[4];
        const unsigned fixed = (unsigned)hdr[3];
        const double c = hdr[5];
        if (V < 2 || V > mv::MAX_VIEWS || nv > V || nv < 0 || K < 0) return 3;
        const int n = 6 * V;
        std::vector<double> cam((size_t)V * 21), obs((size_t)K * V * 3), inl(K), X0((size_t)K * 3);
        if (fread(cam.data(), 8, cam.size(), stdin) != cam.size() || fread(obs.data(), 8, obs.size(), stdin) != obs.size() ||
            fread(inl.data(), 8, inl.size(), stdin) != inl.size() || fread(X0.data(), 8, X0.size(), stdin) != X0.size())
            return 2;
        std::vector<double> pose((size_t)V * 12), cand((size_t)V * 12), vd((size_t)V * ba::STRIDE), vc((size_t)V * ba::STRIDE);
        for (int v = 0; v < V; ++v)
            for (int j = 0; j < 12; ++j) pose[(size_t)v * 12 + j] = cam[(size_t)v * 21 + j];
        stage(pose, cam, V, vd);
        std::vector<double> X = X0, Xc((size_t)K * 3), per(K, 0.0);
        std::vector<unsigned> M(K, 0u);
        std::vector<int> counts(V, 0);
        int nref = 0, nobs = 0;
        for (int k = 0; k < K; ++k) {
            HostObs o{&obs[(size_t)k * V * 3]};
            M[k] = ba_mask(vd.data(), nv, o, (unsigned)inl[k], &X[(size_t)3 * k]);
            bool bad;
            if (M[k]) { per[k] = ba_cost(vd.data(), nv, o, M[k], &X[(size_t)3 * k], c, bad); ++nref; }
            for (int w = 0; w < V; ++w)
                if ((M[k] >> w) & 1u) { ++counts[w]; ++nobs; }
        }
        unsigned fr = 0u;
        for (int v = 0; v < V; ++v)
            if (!((fixed >> v) & 1u) && counts[v] >= ba::MIN_VIEW_OBS) fr |= 1u << v;
        double cost = chunk_sum(per);
        const double cost0 = cost;
        const int status = (fr == 0u || nref == 0) ? ba::ST_NOTHING : (tv::is_finite(cost) ? ba::ST_OK : ba::ST_NOT_FINITE);
        bool done = status != ba::ST_OK;
        double lambda = ba::LAMBDA0;
        int iters = 0, accepted = 0;
        const size_t dump_size = (size_t)K * V * 21 + (size_t)K * 10 + (size_t)n * n + n + 1 + n + (size_t)V * 12 + (size_t)K * 3 + 2;
        std::vector<double> dump(dump_size, 0.0);
        std::vector<double> pv((size_t)K * 9), L((size_t)n * (n + 1) / 2), r(n), piv(n);
        std::vector<unsigned char> held(K, 0);
        for (int it = 0; it < iters_max && !done; ++it) {
            const double opl = 1.0 + lambda;
            double* d = dump.data();
            const bool first = it == 0;
            // ---- point
            for (int k = 0; k < K; ++k) {
                if (!M[k]) continue;
                HostObs o{&obs[(size_t)k * V * 3]};
                held[k] = ba_point(vd.data(), nv, o, M[k], &X[(size_t)3 * k], c, opl, &pv[(size_t)9 * k], &pv[(size_t)9 * k + 6]) ? 0 : 1;
            }
            if (first) {
                for (int k = 0; k < K; ++k)
                    for (int w = 0; w < nv; ++w) {
                        double* q = d + ((size_t)k * V + w) * 21;
                        if (!((M[k] >> w) & 1u)) continue;
                        BaTerm t;
                        ba_term(&vd[(size_t)w * ba::STRIDE], &X[(size_t)3 * k], obs[((size_t)k * V + w) * 3], obs[((size_t)k * V + w) * 3 + 1], c, t);
                        q[0] = t.du; q[1] = t.dv; q[2] = t.wt;
                        for (int j = 0; j < 6; ++j) q[3 + j] = t.jp[j];
                        for (int j = 0; j < 12; ++j) q[9 + j] = t.jc[j];
                    }
                d += (size_t)K * V * 21;
                for (int k = 0; k < K; ++k) {
                    if (M[k]) { for (int j = 0; j < 9; ++j) d[(size_t)k * 10 + j] = pv[(size_t)9 * k + j]; d[(size_t)k * 10 + 9] = held[k]; }
                }
                d += (size_t)K * 10;
            }
            // ---- schur
            for (int w = 0; w < V; ++w)
                for (int v = 0; v <= w; ++v) {
                    double tot[42];
                    const bool diag = v == w;
                    if (!((fr >> v) & 1u) || !((fr >> w) & 1u)) {
                        for (int e = 0; e < 42; ++e) tot[e] = 0.0;
                        if (diag) for (int i = 0; i < 6; ++i) tot[7 * i] = 1.0;
                    } else {
                        const int N = diag ? 42 : 36;
                        std::vector<double> acc((size_t)256 * N, 0.0);
                        const unsigned need = (1u << v) | (1u << w);
                        for (int k = 0; k < K; ++k) {
                            if ((M[k] & need) != need) continue;
                            const double* Xk = &X[(size_t)3 * k];
                            BaTerm tc, tr;
                            ba_term(&vd[(size_t)v * ba::STRIDE], Xk, obs[((size_t)k * V + v) * 3], obs[((size_t)k * V + v) * 3 + 1], c, tc);
                            double* a = &acc[(size_t)(k % 256) * N];
                            if (diag) {
                                ba_pair_add<true>(tc, tc, &pv[(size_t)9 * k], &pv[(size_t)9 * k + 6], held[k] != 0, opl, a);
                            } else {
                                ba_term(&vd[(size_t)w * ba::STRIDE], Xk, obs[((size_t)k * V + w) * 3], obs[((size_t)k * V + w) * 3 + 1], c, tr);
                                ba_pair_add<false>(tr, tc, &pv[(size_t)9 * k], &pv[(size_t)9 * k + 6], held[k] != 0, opl, a);
                            }
                        }
                        block_sums(acc, N, tot);
                    }
                    for (int i = 0; i < 6; ++i)
                        for (int j = 0; j < 6; ++j)
                            if (!diag || j <= i) L[(size_t)(6 * w + i) * (6 * w + i + 1) / 2 + 6 * v + j] = tot[6 * i + j];
                    if (diag) for (int i = 0; i < 6; ++i) r[6 * v + i] = tot[36 + i];
                }
            if (first) {
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j <= i; ++j) d[(size_t)i * n + j] = L[(size_t)i * (i + 1) / 2 + j];
                d += (size_t)n * n;
                for (int i = 0; i < n; ++i) d[i] = r[i];
                d += n;
            }
            // ---- solve
            const bool ok = ba_cholesky_solve(L.data(), r.data(), piv.data(), n, 0, 1, NoSync());
            bool failed = !ok;
            double candcost = 0.0;
            if (first) { d[0] = ok ? 1.0 : 0.0; d += 1; }
            if (ok) {
                for (int v = 0; v < V; ++v) {
                    double Rn[9], tn[3];
                    ba_pose_update(&pose[(size_t)v * 12], &pose[(size_t)v * 12 + 9], &r[(size_t)6 * v], Rn, tn);
                    const bool f = (fr >> v) & 1u;
                    for (int j = 0; j < 9; ++j) cand[(size_t)v * 12 + j] = f ? Rn[j] : pose[(size_t)v * 12 + j];
                    for (int j = 0; j < 3; ++j) cand[(size_t)v * 12 + 9 + j] = f ? tn[j] : pose[(size_t)v * 12 + 9 + j];
                }
                stage(cand, cam, V, vc);
                // ---- update
                bool anybad = false;
                Xc = X;
                for (int k = 0; k < K; ++k) {
                    per[k] = 0.0;
                    if (!M[k]) continue;
                    HostObs o{&obs[(size_t)k * V * 3]};
                    ba_point_step(vd.data(), nv, o, M[k], fr, &X[(size_t)3 * k], c, &pv[(size_t)9 * k], &pv[(size_t)9 * k + 6], held[k] != 0, r.data(), &Xc[(size_t)3 * k]);
                    bool bad;
                    per[k] = ba_cost(vc.data(), nv, o, M[k], &Xc[(size_t)3 * k], c, bad);
                    anybad = anybad || bad;
                }
                failed = anybad;
                if (!failed) candcost = chunk_sum(per);
                if (first) {
                    for (int i = 0; i < n; ++i) d[i] = r[i];
                    d += n;
                    for (size_t i = 0; i < (size_t)V * 12; ++i) d[i] = cand[i];
                    d += (size_t)V * 12;
                    for (size_t i = 0; i < (size_t)K * 3; ++i) d[i] = Xc[i];
                    d += (size_t)K * 3;
                }
            } else if (first) {
                d += n + (size_t)V * 12 + (size_t)K * 3;
            }
            if (first) { d[0] = candcost; d[1] = failed ? 1.0 : 0.0; }
            // ---- decide
            const bool accept = ba_decide(failed, candcost, lambda, cost, done);
            ++iters;
            if (accept) { ++accepted; pose = cand; X = Xc; vd = vc; }
        }
        const bool ran = status == ba::ST_OK;
        int nr = 0;
        for (int k = 0; k < K; ++k) nr += ran && M[k] ? 1 : 0;
        const double head[8] = {(double)status, (double)fr, (double)iters, (double)accepted, (double)nr, (double)nobs, cost0, cost};
        out.insert(out.end(), head, head + 8);
        for (int k = 0; k < K; ++k) out.push_back((double)M[k]);
        out.insert(out.end(), dump.begin(), dump.end());
        out.insert(out.end(), pose.begin(), pose.end());
        out.insert(out.end(), X.begin(), X.end());
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < 3; ++j) out.push_back(ran && M[k] ? (double)(float)X[(size_t)3 * k + j] : X0[(size_t)3 * k + j]);
    }
    fwrite(out.data(), 8, out.size(), stdout);
    return 0;
}
