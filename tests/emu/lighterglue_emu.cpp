// The LighterGlue kernels (csrc/k_lighterglue.hip, and linear_mfma_kernel of csrc/k_linear_mfma.hip for the similarity matrix; sliced out of the product sources by
// tests/test_lighterglue_emulated.py into lighterglue_slice.hpp) on the host.  The grid arithmetic of the launch_lg_* functions is repeated here; the split count and the
// partial sizes come from the sliced lg_attention_splits / lg_attention_partial_floats themselves.  Every buffer is allocated at exactly its capacity (so that an
// AddressSanitizer build sees any read past one) and starts as NaN: what the kernels must not write comes back unchanged and the test checks it.
// stdin: a mode word (int32), then the mode's inputs; stdout: the mode's outputs (see each case below and the test's _run_* helpers).
#include "emu.hpp"
#include <cstdio>
#include <cstdlib>
namespace xfh {
#include "lighterglue_slice.hpp"
}
using namespace xfh;

template <typename T> static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
static int rdi() { return rd<int32_t>(1)[0]; }
static float rdf() { return rd<float>(1)[0]; }
template <typename T> static void wr(const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), stdout); }
static std::vector<float> nanv(size_t n) { return std::vector<float>(n, NAN); }
static std::vector<float> rdnan(size_t n) {      // an input buffer; a zero-sized one still gets a (NaN) element so that its pointer is valid and distinct
    auto v = rd<float>(n);
    if (v.empty()) v.assign(1, NAN);
    return v;
}
// a (gx, gy, gz) grid of workgroups of `nthreads`, one workgroup at a time, on top of emu::launch
template <typename F>
static void launch3(int gx, int gy, int gz, int nthreads, F fn) {
    if (gx <= 0 || gy <= 0 || gz <= 0) return;
    emu::launch(gx * gy * gz, nthreads, 65536, [&] {
        const unsigned b = emu::bidx.x;
        emu::bidx.x = b % gx; emu::bidx.y = (b / gx) % gy; emu::bidx.z = b / (gx * gy);
        emu::gdim.x = gx; emu::gdim.y = gy; emu::gdim.z = gz;
        fn();
        emu::bidx.x = b;
    });
}

int main() {
    const int mode = rdi();
    if (mode == 0) {      // lg_encode_kernel.  in: N, W, H, kpts (N,2), wr (48,2).  out: cs, sn (N,96)
        const int N = rdi(); const float W = rdf(), H = rdf();
        auto kp = rd<float>((size_t)2 * N), wrr = rd<float>(96);
        auto cs = nanv((size_t)N * LG_D), sn = nanv((size_t)N * LG_D);
        launch3(ceil_div(N * 48, 256), 1, 1, 256, [&] { lg_encode_kernel(kp.data(), N, W, H, wrr.data(), cs.data(), sn.data()); });
        wr(cs); wr(sn);
    } else if (mode == 1) {      // lg_linear_kernel.  in: K, N, epi, nsides, wp (N*K, operand order), bias (N), gamma, beta (192); per side: cap, live, ldx, ldy, x (cap,ldx), y (cap,ldy), cs, sn (cap,96).  out: y per side
        const int K = rdi(), N = rdi(), epi = rdi(), nsides = rdi();
        auto wp = rd<float>((size_t)N * K), bias = rd<float>(N), gamma = rd<float>(192), beta = rd<float>(192);
        std::vector<std::vector<float>> x(nsides), y(nsides), cs(nsides), sn(nsides);
        std::vector<int32_t> live(nsides);
        LgLinSide sd[2];
        for (int s = 0; s < nsides; ++s) {
            const int cap = rdi(); live[s] = rdi(); const int ldx = rdi(), ldy = rdi();
            x[s] = rdnan((size_t)cap * ldx); y[s] = rd<float>((size_t)cap * ldy); cs[s] = rdnan((size_t)cap * LG_D); sn[s] = rdnan((size_t)cap * LG_D);
            sd[s] = LgLinSide{x[s].data(), ldx, y[s].data(), ldy, &live[s], cap, cs[s].data(), sn[s].data()};
        }
        // launch_lg_linear
        if (N % 32 || N > 288 || nsides < 1 || nsides > 2 || (epi == LG_EPI_LNGELU && N != 192)) return 3;
        const int cap = max(sd[0].cap, nsides > 1 ? sd[1].cap : 0);
        const LgLinSide a = sd[0], b = sd[nsides - 1];
        auto go = [&](auto fn) { launch3(ceil_div(cap, 32), nsides, 1, N * 2, fn); };
        if (cap <= 0) {}
        else if (K == 64 && epi == LG_EPI_STORE) go([&] { lg_linear_kernel<64, LG_EPI_STORE>(wp.data(), bias.data(), a, b, gamma.data(), beta.data()); });
        else if (K == 96 && epi == LG_EPI_STORE) go([&] { lg_linear_kernel<96, LG_EPI_STORE>(wp.data(), bias.data(), a, b, gamma.data(), beta.data()); });
        else if (K == 96 && epi == LG_EPI_ROTARY) go([&] { lg_linear_kernel<96, LG_EPI_ROTARY>(wp.data(), bias.data(), a, b, gamma.data(), beta.data()); });
        else if (K == 192 && epi == LG_EPI_LNGELU) go([&] { lg_linear_kernel<192, LG_EPI_LNGELU>(wp.data(), bias.data(), a, b, gamma.data(), beta.data()); });
        else if (K == 192 && epi == LG_EPI_RESIDUAL) go([&] { lg_linear_kernel<192, LG_EPI_RESIDUAL>(wp.data(), bias.data(), a, b, gamma.data(), beta.data()); });
        else return 3;
        for (int s = 0; s < nsides; ++s) wr(y[s]);
    } else if (mode == 2) {      // lg_attention_kernel + lg_attention_combine_kernel.  in: nsides, ld, scale; per side: qcap, kcap, nq, nk, Q (qcap,ld), K, V (kcap,ld).  out: per side nsplit (int32), O (qcap,96)
        const int nsides = rdi(), ld = rdi(); const float scale = rdf();
        std::vector<std::vector<float>> Q(nsides), Kb(nsides), Vb(nsides), O(nsides), part(nsides);
        std::vector<int32_t> nq(nsides), nk(nsides);
        LgAttSide sd[2];
        for (int s = 0; s < nsides; ++s) {
            const int qcap = rdi(), kcap = rdi(); nq[s] = rdi(); nk[s] = rdi();
            Q[s] = rdnan((size_t)qcap * ld); Kb[s] = rdnan((size_t)kcap * ld); Vb[s] = rdnan((size_t)kcap * ld);
            O[s] = nanv((size_t)qcap * LG_D);
            sd[s] = LgAttSide{Q[s].data(), Kb[s].data(), Vb[s].data(), O[s].data(), nullptr, &nq[s], &nk[s], qcap, kcap, 1};
        }
        // launch_lg_attention (the partial slices as separate allocations of exactly lg_attention_partial_floats each)
        int qmax = 0, smax = 1;
        for (int s = 0; s < nsides; ++s) {
            sd[s].nsplit = lg_attention_splits(sd[s].qcap, sd[s].kcap);
            part[s] = nanv(lg_attention_partial_floats(sd[s].qcap, sd[s].kcap));
            sd[s].part = part[s].empty() ? nullptr : part[s].data();
            qmax = max(qmax, sd[s].qcap);
            smax = max(smax, sd[s].nsplit);
        }
        const LgAttSide a = sd[0], b = sd[nsides - 1];
        launch3(ceil_div(qmax, 128), smax, nsides, 256, [&] { lg_attention_kernel(a, b, ld, ld, ld, LG_D, scale * 1.44269504088896340736f); });
        if (smax > 1) launch3(ceil_div(qmax, 8), nsides, 1, 256, [&] { lg_attention_combine_kernel(a, b, LG_D); });
        for (int s = 0; s < nsides; ++s) { wr(std::vector<int32_t>{sd[s].nsplit}); wr(O[s]); }
    } else if (mode == 3) {      // lg_dot_kernel, lg_prune_map_kernel, lg_gather_rows_kernel.  in: nsides, thr, min_kpts, w (96), b (1); per side: cap, n, x (cap,192), cs, sn (cap,96), ind (cap).
                                 // out: per side z (cap), map (cap), n_out, xo (cap,192), cso, sno (cap,96), indo (cap)
        const int nsides = rdi(); const float thr = rdf(); const int min_kpts = rdi();
        auto w = rd<float>(96), bb = rd<float>(1);
        const int ld = 192;
        std::vector<std::vector<float>> x(nsides), cs(nsides), sn(nsides), z(nsides), xo(nsides), cso(nsides), sno(nsides);
        std::vector<std::vector<int32_t>> ind(nsides), indo(nsides), map(nsides);
        std::vector<int32_t> n(nsides), n_out(nsides, -7);
        LgRowSide rs[2];
        LgPruneSide ps[2];
        for (int s = 0; s < nsides; ++s) {
            const int cap = rdi(); n[s] = rdi();
            x[s] = rdnan((size_t)cap * ld); cs[s] = rdnan((size_t)cap * LG_D); sn[s] = rdnan((size_t)cap * LG_D); ind[s] = rd<int32_t>(cap);
            z[s] = nanv(cap); xo[s] = nanv((size_t)cap * ld); cso[s] = nanv((size_t)cap * LG_D); sno[s] = nanv((size_t)cap * LG_D);
            indo[s].assign(cap, -7); map[s].assign(cap, -7);
            rs[s] = LgRowSide{x[s].data(), z[s].data(), &n[s], cap};
            ps[s] = LgPruneSide{z[s].data(), &n[s], cap, map[s].data(), &n_out[s], x[s].data(), xo[s].data(), cs[s].data(), cso[s].data(), sn[s].data(), sno[s].data(),
                                ind[s].data(), indo[s].data()};
        }
        const int cap = max(rs[0].cap, rs[nsides - 1].cap);
        if (cap > 0) {
            // launch_lg_dot, launch_lg_prune
            launch3(ceil_div(cap, 8), nsides, 1, 256, [&] { lg_dot_kernel(rs[0], rs[nsides - 1], ld, w.data(), bb.data()); });
            launch3(nsides, 1, 1, 1024, [&] { lg_prune_map_kernel(ps[0], ps[nsides - 1], thr, min_kpts); });
            launch3(ceil_div(cap * 24, 256), nsides, 1, 256, [&] { lg_gather_rows_kernel(ps[0], ps[nsides - 1], ld); });
        }
        for (int s = 0; s < nsides; ++s) { wr(z[s]); wr(map[s]); wr(std::vector<int32_t>{n_out[s]}); wr(xo[s]); wr(cso[s]); wr(sno[s]); wr(indo[s]); }
    } else if (mode == 4) {      // lg_transpose_kernel + linear_mfma_kernel<96, 64, LOAD_ROWMAJOR> (the similarity matrix).  in: cap0, n0, cap1, n1, md0 (cap0,96), md1 (cap1,96).
                                 // out: md1t (96,n1pad), sim (cap0,n1pad)
        const int cap0 = rdi(), n0 = rdi(), cap1 = rdi(), n1 = rdi();
        auto md0 = rdnan((size_t)cap0 * LG_D), md1 = rdnan((size_t)cap1 * LG_D);
        const int npad = (cap1 + 63) / 64 * 64;
        auto md1t = nanv((size_t)LG_D * npad), sim = nanv((size_t)cap0 * npad);
        std::vector<float> zeros(npad, 0.f);
        int32_t nn0 = n0, nn1 = n1;
        launch3(ceil_div(npad, 32), LG_D / 32, 1, 256, [&] { lg_transpose_kernel(md1.data(), LG_D, &nn1, cap1, md1t.data(), npad); });
        LinSrc src{};
        src.x = md0.data(); src.ldx = LG_D;
        if (cap0 > 0) launch3(ceil_div(cap0, 256), ceil_div(npad, 64), 1, 256, [&] { linear_mfma_kernel<96, 64, LOAD_ROWMAJOR>(md1t.data(), zeros.data(), npad, npad, 0, src, cap0, &nn0, sim.data(), npad); });
        wr(md1t); wr(sim);
    } else if (mode == 5) {      // launch_lg_assign's eight kernels.  in: cap0, n0, cap1, n1, thr, sim (cap0,n1pad), z0 (cap0), z1 (n1pad), ind0 (cap0), ind1 (cap1).
                                 // out: z0, z1, rlse (cap0), clse (n1pad), m0 (cap0), m1 (n1pad), best0 (cap0), matches (cap0,2) int64, scores (cap0), n_out
        const int cap0 = rdi(), n0 = rdi(), cap1 = rdi(), n1 = rdi(); const float thr = rdf();
        const int npad = (cap1 + 63) / 64 * 64;
        auto sim = rdnan((size_t)cap0 * npad), z0 = rdnan(cap0), z1 = rdnan(npad);
        auto ind0 = rd<int32_t>(cap0), ind1 = rd<int32_t>(cap1);
        auto rlse = nanv(cap0), clse = nanv(npad), best0 = nanv(cap0), scores = nanv(cap0);
        std::vector<int32_t> m0(cap0, -7), m1(npad, -7);
        std::vector<int64_t> matches((size_t)2 * cap0, -7);
        std::vector<unsigned long long> scratch(lg_assign_scratch_bytes(cap1) / 8, ~0ull);
        int32_t nn0 = n0, nn1 = n1, n_out = -7;
        const int32_t *n0d = &nn0, *n1d = &nn1;
        float2* pf = reinterpret_cast<float2*>(scratch.data());
        unsigned long long* pk = scratch.data();
        launch3(ceil_div(max(cap0, cap1), 256), 2, 1, 256, [&] { lg_logsigmoid_kernel(z0.data(), n0d, cap0, z1.data(), n1d, cap1); });
        launch3(ceil_div(cap0, 4), 1, 1, 256, [&] { lg_row_lse_kernel(sim.data(), npad, n0d, cap0, n1d, cap1, rlse.data()); });
        launch3(npad / 64, LG_RSPLIT, 1, 256, [&] { lg_col_lse_part_kernel(sim.data(), npad, n0d, cap0, n1d, cap1, pf, npad); });
        launch3(ceil_div(cap1, 256), 1, 1, 256, [&] { lg_col_lse_final_kernel(pf, npad, n1d, cap1, clse.data()); });
        launch3(ceil_div(cap0, 4), 1, 1, 256, [&] { lg_row_best_kernel(sim.data(), npad, n0d, cap0, n1d, cap1, rlse.data(), clse.data(), z0.data(), z1.data(), m0.data(), best0.data()); });
        launch3(npad / 64, LG_RSPLIT, 1, 256, [&] { lg_col_best_part_kernel(sim.data(), npad, n0d, cap0, n1d, cap1, rlse.data(), clse.data(), z0.data(), z1.data(), pk, npad); });
        launch3(ceil_div(cap1, 256), 1, 1, 256, [&] { lg_col_best_final_kernel(pk, npad, n1d, cap1, m1.data()); });
        launch3(1, 1, 1, 1024, [&] { lg_mutual_kernel(m0.data(), m1.data(), best0.data(), ind0.data(), ind1.data(), n0d, cap0, thr, matches.data(), scores.data(), &n_out); });
        wr(z0); wr(z1); wr(rlse); wr(clse); wr(m0); wr(m1); wr(best0); wr(matches); wr(scores); wr(std::vector<int32_t>{n_out});
    } else if (mode == 6) {      // lg_mutual_kernel alone.  in: cap0, n0, n1pad, thr, m0 (cap0), m1 (n1pad), best0 (cap0), ind0 (cap0), ind1 (n1pad).  out: matches (cap0,2) int64, scores (cap0), n_out
        const int cap0 = rdi(), n0 = rdi(), npad = rdi(); const float thr = rdf();
        auto m0 = rd<int32_t>(cap0), m1 = rd<int32_t>(npad);
        auto best0 = rd<float>(cap0);
        auto ind0 = rd<int32_t>(cap0), ind1 = rd<int32_t>(npad);
        auto scores = nanv(cap0);
        std::vector<int64_t> matches((size_t)2 * cap0, -7);
        int32_t nn0 = n0, n_out = -7;
        launch3(1, 1, 1, 1024, [&] { lg_mutual_kernel(m0.data(), m1.data(), best0.data(), ind0.data(), ind1.data(), &nn0, cap0, thr, matches.data(), scores.data(), &n_out); });
        wr(matches); wr(scores); wr(std::vector<int32_t>{n_out});
    } else {
        return 3;
    }
    return 0;
}
