// The retrieval slice of csrc/k_retrieval.hip (sliced out of the product source by tests/test_retrieval_emulated.py into retrieval_slice.hpp) on
// the host: one thread per work-item, the row-of-16 DPP exchanges of emu.hpp, the launches of launch_vlad / launch_kmeans_step /
// launch_retrieve_topk / launch_pairs_from_shortlists in their order.  Every output and every workspace starts as 0xa5 bytes: whatever the
// kernels leave unwritten shows.
// stdin: int32 mode.
//   mode 0 (xfh_vlad): int32 G, K, C, has_counts; desc (G,K,64) f32, counts (G) i32 (if has_counts), codebook (C,64) f32.
//     stdout: vlad (G,C*64) f32, assign (G,K) i32, n_assigned (G,C) i32, info (G,4) i32.
//   mode 1 (xfh_kmeans_step): the same input.  stdout: codebook_out (C,64) f32, assign (G,K) i32, n_assigned (C) i32, objective f64, info (4) i32.
//   mode 2 (xfh_retrieve_topk): int32 G, Q, N, D, k, exclude_self, has_n; q (G,Q,D) f32, db (G,N,D) f32, n_db (G) i32 (if has_n).
//     stdout: idx (G,Q,k) i32, score (G,Q,k) f32.
//   mode 3 (xfh_pairs_from_shortlists): int32 S, V, k, has_n; idx (S,V,k) i32, n_views (S) i32 (if has_n).
//     stdout: view_pairs (S,Pcap,2) i32, n_pairs (S) i32.
#include "emu.hpp"
#include <cstdio>
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#define __shared__ static
#define __global__
namespace xfh {
#include "retrieval_slice.hpp"
}
template <typename T> static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
template <typename T> static void wr(const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), stdout); }
template <typename T> static std::vector<T> junk(size_t n) {
    std::vector<T> v(n + 4);                                // (never empty: the kernels' pointers are not null)
    std::memset(v.data(), 0xa5, (n + 4) * sizeof(T));
    v.resize(n);
    return v;
}
static int clusters(int mode) {
    const auto h = rd<int>(4);
    const int G = h[0], K = h[1], C = h[2], has_counts = h[3];
    if (G < 1 || K < 1 || (C != 32 && C != 64 && C != 128 && C != 256)) return 3;
    const bool kmeans = mode == 1;
    const size_t total = (size_t)G * K;
    auto desc = rd<float>(total * 64);
    auto counts = rd<int32_t>(has_counts ? G : 0);
    auto cb = rd<float>((size_t)C * 64);
    const int groups = kmeans ? 1 : G, rows = kmeans ? (int)total : K, nchunks = (rows + xfh::rt::CHUNK - 1) / xfh::rt::CHUNK;
    const size_t parts = (size_t)groups * nchunks * C;
    auto assign = junk<int32_t>(total);
    auto w_score = junk<float>(total), w_part = junk<float>(parts * 64);
    auto w_state = junk<unsigned char>(total);
    auto w_cnt = junk<int32_t>(parts);
    auto w_obj = junk<double>((size_t)groups * nchunks);
    xfh::RetrAssignArgs a = {};
    a.desc = desc.data(); a.counts = has_counts ? counts.data() : nullptr; a.codebook = cb.data(); a.K = K; a.C = C; a.total = (long long)total;
    a.assign = assign.data(); a.w_score = kmeans ? w_score.data() : nullptr; a.w_state = w_state.data();
    emu::launch((int)((total + 255) / 256), 256, 0, [&] { xfh::retr_assign_kernel(a); });
    xfh::RetrSumArgs s = {};
    s.desc = desc.data(); s.assign = assign.data(); s.codebook = cb.data(); s.w_score = a.w_score; s.rows = rows; s.nchunks = nchunks; s.C = C;
    s.residual = kmeans ? 0 : 1; s.w_part = w_part.data(); s.w_cnt = w_cnt.data(); s.w_obj = kmeans ? w_obj.data() : nullptr;
    emu::launch(groups * nchunks * (C / 16), 256, 0, [&] { xfh::retr_sums_kernel(s); });
    xfh::RetrFinishArgs f = {};
    f.w_part = w_part.data(); f.w_cnt = w_cnt.data(); f.w_state = w_state.data(); f.w_obj = s.w_obj; f.codebook = cb.data(); f.rows = rows;
    f.nchunks = nchunks; f.C = C;
    auto out = junk<float>((size_t)groups * C * 64);
    auto n_assigned = junk<int32_t>((size_t)groups * C), info = junk<int32_t>((size_t)groups * 4);
    auto objective = junk<double>(1);
    f.out = out.data(); f.n_assigned = n_assigned.data(); f.info = info.data(); f.objective = objective.data();
    if (kmeans) emu::launch(1, 256, 0, [&] { xfh::retr_kmeans_finish_kernel(f); });
    else emu::launch(G, 256, 0, [&] { xfh::retr_vlad_finish_kernel(f); });
    wr(out); wr(assign); wr(n_assigned);
    if (kmeans) wr(objective);
    wr(info);
    return 0;
}
static int topk() {
    const auto h = rd<int>(7);
    const int G = h[0], Q = h[1], N = h[2], D = h[3], k = h[4], excl = h[5], has_n = h[6];
    if (G < 1 || Q < 1 || N < 1 || D < 64 || D % 64 || D > xfh::rt::MAX_D || k < 1 || k > xfh::rt::MAX_K) return 3;
    auto q = rd<float>((size_t)G * Q * D), db = rd<float>((size_t)G * N * D);
    auto n_db = rd<int32_t>(has_n ? G : 0);
    auto w = junk<float>((size_t)G * Q * N), score = junk<float>((size_t)G * Q * k);
    auto idx = junk<int32_t>((size_t)G * Q * k);
    xfh::RetrScoreArgs a = {};
    a.q = q.data(); a.db = db.data(); a.Q = Q; a.N = N; a.D = D; a.tq = (Q + xfh::rt::TILE - 1) / xfh::rt::TILE; a.tn = (N + xfh::rt::TILE - 1) / xfh::rt::TILE;
    a.w_score = w.data();
    emu::launch(G * a.tq * a.tn, 256, 0, [&] { xfh::retr_score_kernel(a); });
    xfh::RetrTopkArgs t = {};
    t.w_score = w.data(); t.n_db = has_n ? n_db.data() : nullptr; t.Q = Q; t.N = N; t.k = k; t.exclude_self = excl; t.idx = idx.data(); t.score = score.data();
    emu::launch(G * Q, 256, 0, [&] { xfh::retr_topk_kernel(t); });
    wr(idx); wr(score);
    return 0;
}
static int pairs() {
    const auto h = rd<int>(4);
    const int S = h[0], V = h[1], k = h[2], has_n = h[3];
    if (S < 1 || V < 2 || V > xfh::rt::MAX_VIEWS || k < 1 || k > xfh::rt::MAX_K) return 3;
    auto idx = rd<int32_t>((size_t)S * V * k);
    auto n_views = rd<int32_t>(has_n ? S : 0);
    const int all = V * (V - 1) / 2, pcap = V * k < all ? V * k : all;
    auto vp = junk<int32_t>((size_t)S * pcap * 2), n_pairs = junk<int32_t>(S);
    xfh::RetrPairArgs a = {};
    a.idx = idx.data(); a.n_views = has_n ? n_views.data() : nullptr; a.V = V; a.k = k; a.pcap = pcap; a.view_pairs = vp.data(); a.n_pairs = n_pairs.data();
    emu::launch(S, 64, 0, [&] { xfh::retr_pairs_kernel(a); });
    wr(vp); wr(n_pairs);
    return 0;
}
int main() {
    int mode = 0;
    if (fread(&mode, 4, 1, stdin) != 1) return 2;
    return mode <= 1 ? clusters(mode) : (mode == 2 ? topk() : pairs());
}
