// The track-graph slice of csrc/k_tracks.hip (tk_edge, tk_find, tk_union, tk_see, tk_class; sliced out of the product source by
// tests/test_tracks_emulated.py into tracks_slice.hpp) on the host, with a plain minimum and a plain or in the place of the atomics: the
// matches are joined one after the other in the order given, then the steps of tk_flatten_kernel, tk_number_kernel and tk_fill_kernel in
// ascending node order.
// stdin: int64: V, K, P, cap, min_length, max_tracks, then P x (a, b, n), then idx_a (P x cap), idx_b (P x cap)
// stdout: int32: info (8), label (N), mask (N), bad (N), track_of (N), tracks (max_tracks x V)
#include <cstdint>
#include <cstdio>
#include <vector>
#define __device__
namespace xfh {
#include "tracks_slice.hpp"
}  // namespace xfh
struct HostMem {
    int load(const int* p) const { return *p; }
    int fetch_min(int* p, int v) const { const int old = *p; *p = v < old ? v : old; return old; }
    unsigned fetch_or(unsigned* p, unsigned v) const { const unsigned old = *p; *p = old | v; return old; }
};
int main() {
    int64_t h[6];
    if (fread(h, 8, 6, stdin) != 6) return 2;
    const int V = (int)h[0], K = (int)h[1], P = (int)h[2], cap = (int)h[3], min_length = (int)h[4], max_tracks = (int)h[5];
    if (V < 2 || V > xfh::tk::MAX_VIEWS || K < 1 || P < 0 || cap < 0 || max_tracks < 1) return 3;
    const int N = V * K;
    std::vector<int64_t> pr((size_t)P * 3), ia((size_t)P * cap), ib((size_t)P * cap);
    if (fread(pr.data(), 8, pr.size(), stdin) != pr.size() || fread(ia.data(), 8, ia.size(), stdin) != ia.size() ||
        fread(ib.data(), 8, ib.size(), stdin) != ib.size())
        return 2;
    std::vector<int> parent(N), label(N, -1), bad(N, 0), touched(N, 0), track_of(N, -1), tracks((size_t)max_tracks * V, -1), info(8, 0);
    std::vector<unsigned> mask(N, 0u);
    const HostMem mem;
    for (int x = 0; x < N; ++x) parent[x] = x;
    for (int p = 0; p < P; ++p) {
        int64_t n = pr[3 * p + 2];
        n = n > cap ? cap : n;
        for (int64_t i = 0; i < n; ++i) {
            int u, v;
            if (!xfh::tk_edge((int)pr[3 * p], (int)pr[3 * p + 1], ia[(size_t)p * cap + i], ib[(size_t)p * cap + i], V, K, u, v)) continue;
            touched[u] = touched[v] = 1;
            if (!xfh::tk_union(mem, parent.data(), u, v, 2 * N + 1)) info[6] = xfh::tk::ST_BOUND;
        }
    }
    for (int x = 0; x < N; ++x) {
        if (!touched[x]) continue;
        ++info[0];
        const int root = xfh::tk_find(mem, parent.data(), x, N);
        if (root < 0) { info[6] = xfh::tk::ST_BOUND; continue; }
        label[x] = root;
        if (xfh::tk_see(mem, mask.data(), root, x / K)) bad[root] = 1;
    }
    int total = 0;
    std::vector<int> rank(N, -1);
    for (int x = 0; x < N; ++x) {
        if (!touched[x] || label[x] != x) continue;
        ++info[1];
        const int cls = xfh::tk_class(mask[x], bad[x] != 0, min_length);
        info[3] += cls == xfh::tk::INCONSISTENT; info[4] += cls == xfh::tk::SHORT;
        if (cls == xfh::tk::KEPT) { rank[x] = total < max_tracks ? total : -1; ++total; }
    }
    info[2] = total < max_tracks ? total : max_tracks;
    info[5] = total - info[2];
    for (int x = 0; x < N; ++x) {
        const int t = label[x] >= 0 ? rank[label[x]] : -1;
        track_of[x] = t;
        if (t >= 0) tracks[(size_t)t * V + x / K] = x % K;
    }
    fwrite(info.data(), 4, 8, stdout);
    fwrite(label.data(), 4, N, stdout);
    fwrite(mask.data(), 4, N, stdout);
    fwrite(bad.data(), 4, N, stdout);
    fwrite(track_of.data(), 4, N, stdout);
    fwrite(tracks.data(), 4, tracks.size(), stdout);
    return 0;
}
