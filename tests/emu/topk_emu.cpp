// The top-k machinery of csrc/k_detect.hip on the host: cswap .. bitonic_sort_lds, topk_sort_runs_kernel<1>, run_lower_bound and topk_rank_merge_kernel, sliced out of the
// product source by tests/test_topk_emulated.py into topk_slice.hpp (with float_ord and xhalf_u32 of common.hpp).  1024 host threads are one workgroup; the sort's lane
// exchanges are emu.hpp's update_dpp (quad permutes, row_shl / row_shr:4, row_ror:8) and permlane_swap (16, 32), its strides >= 256 and the rank merge go through the LDS buffer.
// The runs do not depend on k, so one input is sorted once and ranked for every k of the list.
// stdin: {B, n, nk} int32, k[nk] int32, vals (B, n) fp32;
// stdout: nsel (B) int32 (for k[0]), runs (B, n) u64, then per k: skeys (B, k) u64 (slots the kernel does not write keep the pattern 0xa5a5...).
#include "emu.hpp"
#include <cstdio>
namespace xfh {
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int xcd_grid_size(int per_group, int n_groups) { return per_group * n_groups; }
struct ScoreSrc { const float* heat; const float* rel; const unsigned* cand; int H, W; };
inline unsigned long long score_key(const ScoreSrc&, int, int, int) { std::abort(); }      // (MODE 0 is not instantiated here: its keys come from the score sampling)
#include "topk_slice.hpp"
}
template <typename T> static std::vector<T> rd(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
int main() {
    using namespace xfh;
    int h[3];
    if (fread(h, 4, 3, stdin) != 3) return 2;
    const int B = h[0], n = h[1], nk = h[2];
    auto ks = rd<int>(nk);
    auto vals = rd<float>((size_t)B * n);
    std::vector<unsigned long long> runs((size_t)B * n, 0xa5a5a5a5a5a5a5a5ull);
    std::vector<int> nsel(B, -1);
    const int qmax = min(ceil_div(n, TK_CH), TK_WG_PER_IMAGE), lds_runs = min(ceil_div(n, TK_CH), TK_LDS_RUNS);      // (run_topk)
    std::vector<std::vector<unsigned long long>> skeys;
    for (int k : ks) skeys.emplace_back((size_t)B * k, 0xa5a5a5a5a5a5a5a5ull);
    // one set of host threads for the 1 + nk launches: workgroups run one after the other, so every workgroup of a launch has finished before the next launch begins
    const int grid = xcd_grid_size(qmax, B);
    emu::launch(grid * (1 + nk), 1024, (size_t)TK_LDS_RUNS * TK_CH * 8, [&] {
        const int launch = blockIdx.x / grid;
        blockIdx.x %= grid;
        if (launch == 0) topk_sort_runs_kernel<1>(ScoreSrc{}, vals.data(), nullptr, n, n, ks[0], qmax, B, runs.data(), nsel.data(), nullptr);
        else topk_rank_merge_kernel(runs.data(), nullptr, n, n, ks[launch - 1], qmax, B, lds_runs, skeys[launch - 1].data());
    });
    fwrite(nsel.data(), 4, nsel.size(), stdout);
    fwrite(runs.data(), 8, runs.size(), stdout);
    for (auto& s : skeys) fwrite(s.data(), 8, s.size(), stdout);
    return 0;
}
