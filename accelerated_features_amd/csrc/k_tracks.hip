// Key-point tracks over an arbitrary graph of view pairs: the connected components of the match graph (DESIGN.md 3.18;
// tests/tracks_reference.py restates it and tests/test_tracks_emulated.py compiles the slice below on the host with a plain minimum in the
// place of the atomic).  A call holds S scenes of V <= 32 views with key-point tables of K rows; node (v, row) has the id v K + row; match i
// of pair p = (a, b) joins the nodes (a, idx_a[i]) and (b, idx_b[i]).  A pair with a == b or a view outside [0, V) and an index outside
// [0, K) are ignored (what track_scatter_kernel of k_triangulate.hip ignores); the same pair may occur more than once.
//   * components: a union-find forest in global memory whose parents never exceed their children.  A union walks both nodes to their roots
//     and hooks the larger root under the smaller by an integer atomicMin; when the larger one has stopped being a root in the meantime the
//     minimum may have replaced its link hi -> old by hi -> lo, and the union goes on with (old, lo), which restores it.  Every step of a
//     union lowers the sum of its two nodes, so 2 V K + 1 steps suffice; a find lowers its node with every step, so V K suffice.  The
//     label of a component is its smallest node id, whatever order the matches arrive in; no floating point is involved;
//   * consistency: the root of a component collects the views of its nodes in a 32-bit mask by atomicOr; a node that finds the bit of its
//     view set marks the component inconsistent (two key-points of one view), which does not depend on the order of arrival either.  A
//     track is a consistent component of at least min_length views; an inconsistent component is dropped whole;
//   * numbering: the rank of the surviving roots in ascending node id within the scene (lowest view first, then row) by one exclusive scan
//     per scene; a track with an id >= max_tracks is dropped and counted;
//   * termination: every loop carries its bound; a thread that reaches it sets status 2 in info word 6 and returns.  No thread waits for
//     another one: no spinning, no flags between workgroups, no cooperative launch.
// Outputs: tracks (S, T, V) int32 (T = max_tracks; a row of the view's table or -1, rows >= n_tracks all -1), track_of (S, V, K) int32 (the
// track of a key-point or -1), n_tracks (S,), info (S, 8): nodes matched, components, tracks kept, dropped inconsistent, dropped short,
// dropped over capacity, status, 0.
//
// Launches per call (workspace: track_graph_workspace_bytes = 14 V K bytes per scene): tk_init_kernel (thread = node: parent = itself),
// tk_hook_kernel (thread = match, grid = (chunks of 256 of cap, P, S)), tk_flatten_kernel (thread = node: its label into an array of its own,
// the view masks), tk_number_kernel (workgroup = scene: the scan over the node ids in chunks of 256 by wave ballots, the counters; the ranks
// go where the parents were) and tk_fill_kernel (thread = node: track_of and its entry of the table).  Every access to the parents while
// unions run is an agent-scope atomic; what one kernel wrote the next one reads with plain loads.
#include "kernels.hpp"

namespace xfh {

// ---- track graph begin (host-compilable: tests/test_tracks_emulated.py slices it out and drops the __device__ qualifiers) ----
namespace tk {
constexpr int MAX_VIEWS = 32;
constexpr int ST_OK = 0, ST_BOUND = 2;      // info word 6
constexpr int KEPT = 0, INCONSISTENT = 1, SHORT = 2;
}  // namespace tk

// the nodes u, v of the match (row ia of view a, row ib of view b); false: the match is ignored
__device__ inline bool tk_edge(int a, int b, long long ia, long long ib, int V, int K, int& u, int& v) {
    const bool ok = a != b && (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned long long)ia < (unsigned long long)K &&
                    (unsigned long long)ib < (unsigned long long)K;               // (a negative index is a huge unsigned one)
    u = ok ? a * K + (int)ia : 0;
    v = ok ? b * K + (int)ib : 0;
    return ok;
}
// The root of x in at most `bound` steps, -1 beyond them.  Mem: load(const int*), fetch_min(int*, int), fetch_or(unsigned*, unsigned).
template <class Mem>
__device__ inline int tk_find(const Mem& mem, const int* parent, int x, int bound) {
    for (int step = 0; step < bound; ++step) {
        const int p = mem.load(parent + x);
        if (p == x) return x;
        x = p;
    }
    return -1;
}
// Joins the components of u and v in at most `bound` steps; false beyond them.  Every step lowers u + v: a step towards a root (a parent
// is smaller than its child), or a hook that found `hi` no root any more (old < hi).
template <class Mem>
__device__ inline bool tk_union(const Mem& mem, int* parent, int u, int v, int bound) {
    for (int step = 0; step < bound; ++step) {
        const int pu = mem.load(parent + u);
        if (pu != u) { u = pu; continue; }
        const int pv = mem.load(parent + v);
        if (pv != v) { v = pv; continue; }
        if (u == v) return true;
        const int hi = u > v ? u : v, lo = u > v ? v : u;
        const int old = mem.fetch_min(parent + hi, lo);
        if (old == hi) return true;                        // hi was a root and hangs under lo now
        u = old; v = lo;                                   // hi had the parent old: min(old, lo) is its parent now, and old and lo are joined next
    }
    return false;
}
// adds the view of a node to the mask of its root; true: the component has a key-point of that view already
template <class Mem>
__device__ inline bool tk_see(const Mem& mem, unsigned* mask, int root, int view) {
    const unsigned bit = 1u << view;
    return (mem.fetch_or(mask + root, bit) & bit) != 0u;
}
// what becomes of a component with the view mask m
__device__ inline int tk_class(unsigned m, bool inconsistent, int min_length) {
    int n = 0;
#pragma unroll
    for (int b = 0; b < tk::MAX_VIEWS; ++b) n += (int)((m >> b) & 1u);
    return inconsistent ? tk::INCONSISTENT : (n < min_length ? tk::SHORT : tk::KEPT);
}
// ---- track graph end ----

struct TkDeviceMem {
    __device__ inline int load(const int* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ inline int fetch_min(int* p, int v) const { return atomicMin(p, v); }
    __device__ inline unsigned fetch_or(unsigned* p, unsigned v) const { return atomicOr(p, v); }
};

struct TkArgs {
    const int32_t* view_pairs;   // (S, P, 2)
    const int64_t* idx_a;        // (S, P, cap)
    const int64_t* idx_b;
    const int32_t* n_matches;    // (S, P)
    int P, cap, V, K, N, min_length, max_tracks;
    int32_t* parent;             // (S, N); tk_number_kernel writes the ranks of the roots here
    int32_t* label;              // (S, N): the root of a matched node, -1 for every other node
    unsigned* mask;              // (S, N): the views of the component, at its root
    unsigned char* touched;      // (S, N): the node has a match
    unsigned char* bad;          // (S, N): the component is inconsistent, at its root
    int32_t* tracks;             // (S, max_tracks, V), pre-filled with -1
    int32_t* track_of;           // (S, N)
    int32_t* n_tracks;           // (S,)
    int32_t* info;               // (S, 8), zeroed before the first launch
};

__global__ __launch_bounds__(256) void tk_init_kernel(TkArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < a.N) a.parent[(size_t)blockIdx.y * a.N + x] = x;
}

__global__ __launch_bounds__(256) void tk_hook_kernel(TkArgs a) {
    const int s = blockIdx.z, p = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t pair = (size_t)s * a.P + p;
    int n = a.n_matches[pair];
    n = n > a.cap ? a.cap : n;
    if (i >= n) return;
    int u, v;
    if (!tk_edge(a.view_pairs[2 * pair], a.view_pairs[2 * pair + 1], (long long)a.idx_a[pair * a.cap + i], (long long)a.idx_b[pair * a.cap + i], a.V, a.K, u, v))
        return;
    const size_t base = (size_t)s * a.N;
    a.touched[base + u] = 1;
    a.touched[base + v] = 1;
    if (!tk_union(TkDeviceMem(), a.parent + base, u, v, 2 * a.N + 1)) a.info[(size_t)s * 8 + 6] = tk::ST_BOUND;
}

__global__ __launch_bounds__(256) void tk_flatten_kernel(TkArgs a) {
    const int s = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const size_t base = (size_t)s * a.N;
    const bool node = x < a.N && a.touched[base + x] != 0;
    if (x < a.N) {
        int root = -1;
        if (node) {
            root = tk_find(TkDeviceMem(), a.parent + base, x, a.N);
            if (root < 0) a.info[(size_t)s * 8 + 6] = tk::ST_BOUND;
            else if (tk_see(TkDeviceMem(), a.mask + base, root, x / a.K)) a.bad[base + root] = 1;
        }
        a.label[base + x] = root;
    }
    const unsigned long long m = __ballot(node);           // nodes matched: one integer atomic per wave
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.info + (size_t)s * 8, (int)__popcll(m));
}

__global__ __launch_bounds__(256) void tk_number_kernel(TkArgs a) {
    __shared__ int wave_n[4];
    __shared__ int cnt[3];                                 // components, inconsistent, short
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)s * a.N;
    if (tid < 3) cnt[tid] = 0;
    int carry = 0, comps = 0, incons = 0, shrt = 0;
    for (int b0 = 0; b0 < a.N; b0 += 256) {                 // (the trip count is the same for every thread: the barriers below are met by all)
        const int x = b0 + tid;
        const bool root = x < a.N && a.touched[base + x] != 0 && a.label[base + x] == x;
        const int cls = root ? tk_class(a.mask[base + x], a.bad[base + x] != 0, a.min_length) : -1;
        comps += root ? 1 : 0; incons += cls == tk::INCONSISTENT ? 1 : 0; shrt += cls == tk::SHORT ? 1 : 0;
        const bool keep = cls == tk::KEPT;
        const unsigned long long m = __ballot(keep);
        __syncthreads();                                   // the last round's wave_n has been read
        if (lane == 0) wave_n[wave] = (int)__popcll(m);
        __syncthreads();
        const int w0 = wave_n[0], w1 = wave_n[1], w2 = wave_n[2], w3 = wave_n[3];
        const int before = wave == 0 ? 0 : (wave == 1 ? w0 : (wave == 2 ? w0 + w1 : (w0 + w1) + w2));
        const int id = (carry + before) + (int)__popcll(m & ((1ull << lane) - 1ull));
        if (x < a.N) a.parent[base + x] = keep && id < a.max_tracks ? id : -1;
        carry += (w0 + w1) + (w2 + w3);
    }
    if (comps) atomicAdd(&cnt[0], comps);
    if (incons) atomicAdd(&cnt[1], incons);
    if (shrt) atomicAdd(&cnt[2], shrt);
    __syncthreads();
    if (tid == 0) {
        int32_t* info = a.info + (size_t)s * 8;            // (word 0 came from tk_flatten_kernel, word 6 is the status)
        const int kept = carry < a.max_tracks ? carry : a.max_tracks;
        info[1] = cnt[0]; info[2] = kept; info[3] = cnt[1]; info[4] = cnt[2]; info[5] = carry - kept; info[7] = 0;
        a.n_tracks[s] = kept;
    }
}

__global__ __launch_bounds__(256) void tk_fill_kernel(TkArgs a) {
    const int s = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.N) return;
    const size_t base = (size_t)s * a.N;
    const int root = a.label[base + x];
    const int t = (unsigned)root < (unsigned)a.N ? a.parent[base + root] : -1;
    a.track_of[base + x] = t;
    if ((unsigned)t < (unsigned)a.max_tracks) a.tracks[((size_t)s * a.max_tracks + t) * a.V + x / a.K] = x % a.K;
}

static size_t tk_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the offsets of parent, label, mask, touched, bad; returns the size
static size_t tk_layout(int S, int V, int K, size_t* off) {
    const size_t n = (size_t)S * V * K;
    const size_t sizes[5] = {n * 4, n * 4, n * 4, n, n};
    size_t at = 0;
    for (int i = 0; i < 5; ++i) {
        if (off) off[i] = at;
        at += tk_align(sizes[i]);
    }
    return at;
}

size_t track_graph_workspace_bytes(int S, int V, int K) { return tk_layout(S, V, K, nullptr); }

int launch_build_tracks_graph(const int32_t* view_pairs, const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches, int S, int P, int cap, int V,
                              int K, int min_length, int max_tracks, int32_t* tracks, int32_t* track_of, int32_t* n_tracks, int32_t* info, void* ws,
                              hipStream_t st) {
    if (S < 1 || S > 65535 || P < 1 || P > 65535 || cap < 1 || V < 2 || V > tk::MAX_VIEWS || K < 1 || K > (1 << 24) || max_tracks < 1 ||
        max_tracks > V * K)
        return -1;
    size_t off[5];
    tk_layout(S, V, K, off);
    char* w = (char*)ws;
    TkArgs a = {};
    a.view_pairs = view_pairs; a.idx_a = idx_a; a.idx_b = idx_b; a.n_matches = n_matches; a.P = P; a.cap = cap; a.V = V; a.K = K; a.N = V * K;
    a.min_length = min_length; a.max_tracks = max_tracks;
    a.parent = (int32_t*)(w + off[0]); a.label = (int32_t*)(w + off[1]); a.mask = (unsigned*)(w + off[2]);
    a.touched = (unsigned char*)(w + off[3]); a.bad = (unsigned char*)(w + off[4]);
    a.tracks = tracks; a.track_of = track_of; a.n_tracks = n_tracks; a.info = info;
    const size_t n = (size_t)S * a.N;
    if (hipMemsetAsync(a.mask, 0, off[4] - off[2] + n, st) != hipSuccess) return -1;                     // mask, touched, bad
    if (hipMemsetAsync(info, 0, (size_t)S * 8 * sizeof(int32_t), st) != hipSuccess) return -1;
    if (hipMemsetAsync(tracks, 0xFF, (size_t)S * max_tracks * V * sizeof(int32_t), st) != hipSuccess) return -1;      // all ones: -1
    const dim3 nodes(ceil_div(a.N, 256), S);
    tk_init_kernel<<<nodes, 256, 0, st>>>(a);
    tk_hook_kernel<<<dim3(ceil_div(cap, 256), P, S), 256, 0, st>>>(a);
    tk_flatten_kernel<<<nodes, 256, 0, st>>>(a);
    tk_number_kernel<<<S, 256, 0, st>>>(a);
    tk_fill_kernel<<<nodes, 256, 0, st>>>(a);
    return 0;
}

}  // namespace xfh
