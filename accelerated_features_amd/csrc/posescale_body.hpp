// Baseline scales from shared tracks; included by k_triangulate.hip behind its pose-graph slice, inside namespace xfh with fp
// contraction off.  tests/posescale_reference.py restates both slices below operation for operation and tests/test_posescale_emulated.py
// compiles them for the host behind the slices of k_triangulate.hip and holds them to that restatement bit for bit.
//
// A relative pose carries its translation up to scale, so the position solve of the pose graph is determined on parallel-rigid graphs only.
// A track seen in the views a, b, c has a depth in the shared view b in units of the baseline of edge (a, b) and another in units of the
// baseline of edge (b, c): their quotient is the ratio of the two baselines.
//   * wedge: edges p < q, both valid and both with a direction (pg_edge_key), whose view sets share exactly one view v (two edges over the same
//     two views are no wedge).  op, oq: the other view of p, of q;
//   * values: every row k of v with t = track_of[v, k] in [0, T) whose track has rows in [0, K) in op and in oq is examined: tg_point under
//     edge p (R_rel_p, t_rel_p / sqrt(n2), the intrinsics of p's views in the edge's order, the pixel of the edge's first view first) and
//     under edge q; its depth in v is gate[0] when v is the edge's first view, else gate[1]; when both statuses are tg::VALID the track's
//     value is z_q / z_p = |baseline p| / |baseline q|;
//   * the wedge's ratio is the lower median of its n values, element (n - 1) / 2 of their ascending order, when n >= min_common, else NaN.
//     A selection averages nothing: the order in which the values arrive does not matter;
//   * outputs (P, P) per scene: ratio, count (n, also below min_common), shared_view (-1: no wedge); entries that are no wedge (p >= q among
//     them) are (NaN, 0, -1).  info: wedges, wedges with a ratio, tracks examined, tracks valid, status 0, 0, 0, 0 (integer sums).
// baseline_ratio_kernel: one workgroup of 256 per (scene, p, q); a candidate without a shared view leaves after four loads.  The poses and
// intrinsics of both edges are staged once (LDS), the threads stride over the K <= 4096 rows of v and append their values to LDS (a row of v
// gives at most one value: n <= K); the selection is a bitonic sort of the next power of two, padded with +inf.

// ---- pose scale begin (host-compilable: tests/test_posescale_emulated.py slices it out behind the pose-graph slice) ----
namespace ps {
constexpr int MAX_PAIRS = 512, MAX_K = 4096;
constexpr int STAGE = 30;                                  // per edge: R (9), unit t (3), E (9), cal (8), usable
}  // namespace ps

struct PsScene {
    const float* kpts;        // (V, K, 2)
    const int32_t* tracks;    // (T, V)
    const int32_t* track_of;  // (V, K)
    const int32_t* pairs;     // (P, 2)
    const double* Rrel;       // (P, 9)
    const double* trel;       // (P, 3)
    const double* weight;     // (P,)
    const double* Ks;         // (V, 9)
    int nv, P, V, K, T, min_common;
    double thr2, cos_min, max_depth, pad;                  // pad: +inf
    double* ratio;            // (P, P)
    int32_t* count;           // (P, P)
    int32_t* shared;          // (P, P)
    int32_t* info;            // (8,), zero before the first wedge
};

// the view that the edges (a0, b0) and (a1, b1) share when they share exactly one, else -1
__device__ inline int ps_shared_view(int a0, int b0, int a1, int b1) {
    const int n = (int)(a0 == a1) + (int)(a0 == b1) + (int)(b0 == a1) + (int)(b0 == b1);
    if (n != 1 || a0 == b0 || a1 == b1) return -1;
    return (a0 == a1 || a0 == b1) ? a0 : b0;
}
// what tg_point needs of edge p
__device__ inline void ps_stage(const PsScene& s, int p, double* st) {
    const int a = s.pairs[2 * p], b = s.pairs[2 * p + 1];
    const double t0 = s.trel[(size_t)3 * p], t1 = s.trel[(size_t)3 * p + 1], t2 = s.trel[(size_t)3 * p + 2];
    const double n = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
    for (int j = 0; j < 9; ++j) st[j] = s.Rrel[(size_t)9 * p + j];
    st[9] = t0 / n; st[10] = t1 / n; st[11] = t2 / n;
    tg_pose_E(st, st + 9, st + 12);
    const double* Ka = s.Ks + 9 * a;
    const double* Kb = s.Ks + 9 * b;
    st[21] = Ka[0]; st[22] = Ka[4]; st[23] = Ka[2]; st[24] = Ka[5];
    st[25] = Kb[0]; st[26] = Kb[4]; st[27] = Kb[2]; st[28] = Kb[5];
    st[29] = tg_pose_ok(st, st + 9) ? 1.0 : 0.0;
}
// the depth in the shared view of the track with the pixels (uv, vv) there and (uo, vo) in the edge's other view; first: the shared view is
// the edge's first view.  false: the status is not tg::VALID
__device__ inline bool ps_depth(const PsScene& s, const double* st, bool first, double uv, double vv, double uo, double vo, double& z) {
    float X3[3], err;
    double gate[4];
    const int status = tg_point(st, st + 9, st + 12, st[29] != 0.0, st + 21, first ? uv : uo, first ? vv : vo, first ? uo : uv, first ? vo : vv, false,
                                s.thr2, s.cos_min, s.max_depth, X3, err, gate);
    z = first ? gate[0] : gate[1];
    return status == tg::VALID;
}
// ascending bitonic sort of x[0 .. m), m a power of two
template <class Sync>
__device__ inline void ps_sort(double* x, int m, int tid, int nt, const Sync& sync) {
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const double lo = x[i], hi = x[l];
                    const bool up = (i & k) == 0;
                    if (up ? lo > hi : lo < hi) { x[i] = hi; x[l] = lo; }
                }
            }
            sync();
        }
}
// Candidate (p, q) of a scene.  vals: ps::MAX_K doubles, stage: 2 ps::STAGE doubles, cnt: 2 ints, all shared by the nt threads;
// Mem: add(int*, int) returns the value before (an integer atomic on the device).
template <class Sync, class Mem>
__device__ inline void ps_wedge(const PsScene& s, int p, int q, double* vals, double* stage, int* cnt, const Mem& mem, int tid, int nt, const Sync& sync) {
    const double zero = s.thr2 - s.thr2, nan = zero / zero;                      // (NaN either way)
    const size_t at = (size_t)p * s.P + q;
    int v = -1;
    if (p < q) {
        v = ps_shared_view(s.pairs[2 * p], s.pairs[2 * p + 1], s.pairs[2 * q], s.pairs[2 * q + 1]);
        if (v >= 0) {
            const int kp = pg_edge_key(s.pairs, s.Rrel, s.trel, s.weight, s.nv, p), kq = pg_edge_key(s.pairs, s.Rrel, s.trel, s.weight, s.nv, q);
            if (kp < 0 || kq < 0 || !(kp & pg::K_DIR) || !(kq & pg::K_DIR)) v = -1;
        }
    }
    if (v < 0) {
        if (tid == 0) { s.ratio[at] = nan; s.count[at] = 0; s.shared[at] = -1; }
        return;
    }
    if (tid == 0) {
        ps_stage(s, p, stage);
        ps_stage(s, q, stage + ps::STAGE);
        cnt[0] = 0; cnt[1] = 0;
    }
    sync();
    const bool fp = s.pairs[2 * p] == v, fq = s.pairs[2 * q] == v;
    const int op = fp ? s.pairs[2 * p + 1] : s.pairs[2 * p], oq = fq ? s.pairs[2 * q + 1] : s.pairs[2 * q];
    for (int k = tid; k < s.K; k += nt) {
        const int t = s.track_of[(size_t)v * s.K + k];
        if (t < 0 || t >= s.T) continue;
        const int rp = s.tracks[(size_t)t * s.V + op], rq = s.tracks[(size_t)t * s.V + oq];
        if (rp < 0 || rp >= s.K || rq < 0 || rq >= s.K) continue;
        mem.add(cnt + 1, 1);
        const float* xv = s.kpts + ((size_t)v * s.K + k) * 2;
        const float* xp = s.kpts + ((size_t)op * s.K + rp) * 2;
        const float* xq = s.kpts + ((size_t)oq * s.K + rq) * 2;
        double zp, zq;
        const bool okp = ps_depth(s, stage, fp, (double)xv[0], (double)xv[1], (double)xp[0], (double)xp[1], zp);
        const bool okq = ps_depth(s, stage + ps::STAGE, fq, (double)xv[0], (double)xv[1], (double)xq[0], (double)xq[1], zq);
        if (okp && okq) vals[mem.add(cnt, 1)] = zq / zp;                         // (a row of v comes by once: fewer than K + 1 values)
    }
    sync();
    const int n = cnt[0];
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = n + tid; i < m; i += nt) vals[i] = s.pad;
    sync();
    ps_sort(vals, m, tid, nt, sync);
    if (tid == 0) {
        const bool has = n >= s.min_common && n > 0;
        s.ratio[at] = has ? vals[(n - 1) / 2] : nan;
        s.count[at] = n; s.shared[at] = v;
        mem.add(s.info, 1);
        if (has) mem.add(s.info + 1, 1);
        mem.add(s.info + 2, cnt[1]);
        mem.add(s.info + 3, n);
    }
}
// ---- pose scale end ----

// The ratio terms of the position rounds (pg_run_with's Terms).  With u_p = d_p . (c_a - c_b) and g_p = (e_a - e_b) (x) d_p a wedge (p, q) with
// the ratio r = |baseline p| / |baseline q| asks for u_p = r u_q: it adds w h h' to M, h = g_p / sqrt(r) - sqrt(r) g_q (the same under a swap
// of p and q with 1 / r), w = (scale_weight count) factor.  The term is homogeneous in the centres: the scale stays in the null space, and
// mu, the gauge and the rigidity test carry over.
//   * taking part: p < q, both edges active with a direction, exactly one shared view, a finite ratio > 0 and a count > 0.  The wedges that take
//     part are compacted into a list in ascending (p, q): a count per row p, an exclusive scan over the rows, a second pass that writes;
//   * factor: 1 in round 0, else pg_factor(rho, scale_tol, kind) with rho = |u_p - r u_q| / (u_p + r u_q) when u_p > 0 and u_q > 0, else 1,
//     at the centres of the round before; after the last round once more: ratio_factor (P, P), 0 where the wedge took no part or the positions
//     failed;
//   * an entry of M adds its edges first (pg_pos_assemble), then its wedges in list order: block (i, j) of the views vi, vj gets
//     (w h_vi[x]) h_vj[y], h_v = c_p (d_p / sqrt(r)) - c_q (sqrt(r) d_q), c = +1 at the edge's first view, -1 at its second, 0 elsewhere; a
//     wedge that does not touch both views is skipped.
// ---- pose graph ratios begin (host-compilable, as above) ----
struct PgRatioTerms {
    const double* ratio;      // (P, P)
    const int32_t* count;     // (P, P)
    double weight, tol;       // scale_weight, scale_tol
    double* factor;           // (P, P): ratio_factor
    int32_t* row;             // workspace (P + 1,): the first list entry of row p; [P]: the length of the list
    long long* list;          // (P (P - 1) / 2,): p | q << 9 | a_p << 18 | b_p << 23 | a_q << 28 | b_q << 33
    double* lr;               // the ratio, its square root, the weight of the round
    double* lsr;
    double* lw;

    __device__ inline bool takes(const PgScene& s, int p, int q) const {
        const int kp = s.key[p], kq = s.key[q], need = pg::K_ACTIVE | pg::K_DIR;
        if (kp < 0 || kq < 0 || (kp & need) != need || (kq & need) != need) return false;
        if (ps_shared_view(kp & 255, (kp >> 8) & 255, kq & 255, (kq >> 8) & 255) < 0) return false;
        const double r = ratio[(size_t)p * s.P + q];
        return tv::is_finite(r) && r > 0.0 && count[(size_t)p * s.P + q] > 0;
    }
    template <class Sync>
    __device__ inline void prepare(const PgScene& s, int tid, int nt, const Sync& sync) const {
        for (size_t i = tid; i < (size_t)s.P * s.P; i += nt) factor[i] = 0.0;
        for (int p = tid; p < s.P; p += nt) {
            int c = 0;
            for (int q = p + 1; q < s.P; ++q) c += takes(s, p, q) ? 1 : 0;
            row[p] = c;
        }
        sync();
        if (tid == 0) {
            int acc = 0;
            for (int p = 0; p < s.P; ++p) { const int c = row[p]; row[p] = acc; acc += c; }
            row[s.P] = acc;
        }
        sync();
        for (int p = tid; p < s.P; p += nt) {
            int at = row[p];
            for (int q = p + 1; q < s.P; ++q) {
                if (!takes(s, p, q)) continue;
                const long long kp = s.key[p], kq = s.key[q];
                list[at] = (long long)p | ((long long)q << 9) | ((kp & 255) << 18) | (((kp >> 8) & 255) << 23) | ((kq & 255) << 28) | (((kq >> 8) & 255) << 33);
                const double r = ratio[(size_t)p * s.P + q];
                lr[at] = r; lsr[at] = sqrt(r); lw[at] = 0.0;
                ++at;
            }
        }
        sync();
    }
    template <class Sync>
    __device__ inline void weights(const PgScene& s, int kind, bool first, int tid, int nt, const Sync& sync) const {
        const double* cen = s.lds + pg::L_CEN;
        const int n = row[s.P];
        for (int i = tid; i < n; i += nt) {
            const long long e = list[i];
            const int p = (int)(e & 511), q = (int)((e >> 9) & 511);
            double f = 1.0;
            if (!first) {
                double u[2];
                for (int h = 0; h < 2; ++h) {
                    const int ed = h ? q : p;
                    const double* ca = cen + 3 * (int)((e >> (h ? 28 : 18)) & 31);
                    const double* cb = cen + 3 * (int)((e >> (h ? 33 : 23)) & 31);
                    const double e0 = ca[0] - cb[0], e1 = ca[1] - cb[1], e2 = ca[2] - cb[2];
                    u[h] = (s.dir[(size_t)3 * ed] * e0 + s.dir[(size_t)3 * ed + 1] * e1) + s.dir[(size_t)3 * ed + 2] * e2;
                }
                const double ru = lr[i] * u[1], d = u[0] - ru;
                const double rho = (u[0] > 0.0 && u[1] > 0.0) ? (d < 0.0 ? -d : d) / (u[0] + ru) : 1.0;
                f = pg_factor(rho, tol, kind);
            }
            factor[(size_t)p * s.P + q] = f;
            lw[i] = (weight * (double)count[(size_t)p * s.P + q]) * f;
        }
        sync();
    }
    template <class Sync>
    __device__ inline void assemble(const PgScene& s, int tid, int nt, const Sync& sync) const {
        const int nr = s.ldi[pg::I_NR], n = row[s.P];
        double* T = s.lds + pg::L_SYS;
        for (int t = tid; t < nr * (nr + 1) / 2; t += nt) {
            int i, j;
            pg_slot(t, i, j);
            const int vi = s.ldi[pg::I_VIEW + i], vj = s.ldi[pg::I_VIEW + j];
            double B[9];
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) B[3 * x + y] = (i != j || y <= x) ? T[(3 * i + x) * (3 * i + x + 1) / 2 + 3 * j + y] : 0.0;
            for (int w = 0; w < n; ++w) {
                const long long e = list[w];
                const int ap = (int)((e >> 18) & 31), bp = (int)((e >> 23) & 31), aq = (int)((e >> 28) & 31), bq = (int)((e >> 33) & 31);
                const int cip = (int)(ap == vi) - (int)(bp == vi), ciq = (int)(aq == vi) - (int)(bq == vi);
                const int cjp = (int)(ap == vj) - (int)(bp == vj), cjq = (int)(aq == vj) - (int)(bq == vj);
                if ((cip == 0 && ciq == 0) || (cjp == 0 && cjq == 0)) continue;
                const int p = (int)(e & 511), q = (int)((e >> 9) & 511);
                const double wt = lw[w], sr = lsr[w];
                double hi[3], hj[3];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    const double gp = s.dir[(size_t)3 * p + x] / sr, gq = sr * s.dir[(size_t)3 * q + x];
                    hi[x] = (double)cip * gp - (double)ciq * gq;
                    hj[x] = (double)cjp * gp - (double)cjq * gq;
                }
#pragma unroll
                for (int x = 0; x < 3; ++x)
#pragma unroll
                    for (int y = 0; y < 3; ++y) B[3 * x + y] = B[3 * x + y] + (wt * hi[x]) * hj[y];
            }
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y)
                    if (i != j || y <= x) T[(3 * i + x) * (3 * i + x + 1) / 2 + 3 * j + y] = B[3 * x + y];
        }
        sync();
    }
    template <class Sync>
    __device__ inline void finish(const PgScene& s, bool pos, int tid, int nt, const Sync& sync) const {
        if (pos) return;
        const int n = row[s.P];
        for (int i = tid; i < n; i += nt) factor[(size_t)(list[i] & 511) * s.P + (size_t)((list[i] >> 9) & 511)] = 0.0;
        sync();
    }
};
// ---- pose graph ratios end ----

struct PsDeviceMem {
    __device__ inline int add(int* p, int v) const { return atomicAdd(p, v); }
};

struct PsArgs {
    const float* kpts;        // (S, V, K, 2)
    const int32_t* tracks;    // (S, T, V)
    const int32_t* track_of;  // (S, V, K)
    const int32_t* pairs;     // (S, P, 2)
    const double* Rrel;
    const double* trel;
    const double* weight;
    const double* Ks;         // (S, V, 9)
    const int32_t* n_views;   // (S,) or NULL
    int P, V, K, T, min_common;
    double thr2, cos_min, max_depth;
    double* ratio;
    int32_t* count;
    int32_t* shared;
    int32_t* info;
};

__global__ __launch_bounds__(256) void baseline_ratio_kernel(PsArgs a) {
    __shared__ double vals[ps::MAX_K];
    __shared__ double stage[2 * ps::STAGE];
    __shared__ int cnt[2];
    const size_t sc = blockIdx.z, P = (size_t)a.P;
    int nv = a.n_views ? a.n_views[sc] : a.V;
    nv = nv < 0 ? 0 : (nv > a.V ? a.V : nv);
    PsScene s;
    s.kpts = a.kpts + sc * a.V * a.K * 2; s.tracks = a.tracks + sc * a.T * a.V; s.track_of = a.track_of + sc * a.V * a.K;
    s.pairs = a.pairs + sc * P * 2; s.Rrel = a.Rrel + sc * P * 9; s.trel = a.trel + sc * P * 3; s.weight = a.weight + sc * P; s.Ks = a.Ks + sc * a.V * 9;
    s.nv = nv; s.P = a.P; s.V = a.V; s.K = a.K; s.T = a.T; s.min_common = a.min_common;
    s.thr2 = a.thr2; s.cos_min = a.cos_min; s.max_depth = a.max_depth; s.pad = __builtin_huge_val();
    s.ratio = a.ratio + sc * P * P; s.count = a.count + sc * P * P; s.shared = a.shared + sc * P * P; s.info = a.info + sc * 8;
    ps_wedge(s, (int)blockIdx.y, (int)blockIdx.x, vals, stage, cnt, PsDeviceMem(), (int)threadIdx.x, 256, BaBarrier());
}

int launch_baseline_ratios(const float* kpts, const int32_t* tracks, const int32_t* track_of, const int32_t* view_pairs, const double* R_rel,
                           const double* t_rel, const double* weight, const double* Ks, const int32_t* n_views, int S, int P, int V, int K, int T,
                           double max_reproj_error, double cos_min, double max_depth, int min_common, double* ratio, int32_t* count,
                           int32_t* shared_view, int32_t* info, hipStream_t st) {
    if (S < 1 || S > 65535 || P < 1 || P > ps::MAX_PAIRS || V < 2 || V > mv::MAX_VIEWS || K < 1 || K > ps::MAX_K || T < 1 || min_common < 1) return -1;
    PsArgs a = {};
    a.kpts = kpts; a.tracks = tracks; a.track_of = track_of; a.pairs = view_pairs; a.Rrel = R_rel; a.trel = t_rel; a.weight = weight; a.Ks = Ks;
    a.n_views = n_views; a.P = P; a.V = V; a.K = K; a.T = T; a.min_common = min_common;
    a.thr2 = max_reproj_error * max_reproj_error; a.cos_min = cos_min; a.max_depth = max_depth;
    a.ratio = ratio; a.count = count; a.shared = shared_view; a.info = info;
    if (hipMemsetAsync(info, 0, (size_t)S * 8 * sizeof(int32_t), st) != hipSuccess) return -1;
    baseline_ratio_kernel<<<dim3(P, P, S), 256, 0, st>>>(a);
    return 0;
}

struct PgRatioArgs {
    const double* ratio;      // (S, P, P)
    const int32_t* count;
    double weight, tol;
    double* factor;           // (S, P, P)
    int32_t* row;             // workspace: (S, P + 1), then (S, NW) lists
    long long* list;
    double* ld;               // (S, 3, NW)
};

__global__ __launch_bounds__(256) void pose_graph_ratio_kernel(PgArgs a, PgRatioArgs r) {
    __shared__ double lds[pg::L_END];
    __shared__ int ldi[pg::I_END];
    const size_t sc = blockIdx.x, P = (size_t)a.P, nw = P * (P - 1) / 2 + 1;
    PgRatioTerms x;
    x.ratio = r.ratio + sc * P * P; x.count = r.count + sc * P * P; x.weight = r.weight; x.tol = r.tol; x.factor = r.factor + sc * P * P;
    x.row = r.row + sc * (P + 1); x.list = r.list + sc * nw;
    x.lr = r.ld + sc * 3 * nw; x.lsr = x.lr + nw; x.lw = x.lsr + nw;
    pg_run_with(pg_scene_of(a, sc, lds, ldi), x, (int)threadIdx.x, 256, BaBarrier());
}

// the workspace behind pose_graph_workspace_bytes' part: the rows, the lists, the lists' doubles
static size_t pgr_layout(int S, int P, size_t* off) {
    const size_t nw = (size_t)P * (P - 1) / 2 + 1;
    const size_t sz[3] = {(size_t)S * (P + 1) * 4, (size_t)S * nw * 8, (size_t)S * nw * 3 * 8};
    size_t at = pg_layout(S, P, nullptr);
    for (int i = 0; i < 3; ++i) { if (off) off[i] = at; at += ba_align(sz[i]); }
    return at;
}
size_t pose_graph_ratios_workspace_bytes(int S, int P, int V) { (void)V; return pgr_layout(S, P, nullptr); }

int launch_average_poses_ratios(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight, const int32_t* n_views,
                                const double* ratio, const int32_t* ratio_count, int S, int P, int V, int iterations, int redescend, double rot_scale_rad,
                                double pos_scale_sin, double min_pivot_ratio, double scale_weight, double scale_tol, double* Rs_out, double* ts_out,
                                int32_t* registered, double* edge_factor, double* ratio_factor, int32_t* info, void* ws, hipStream_t st) {
    if (S < 1 || S > 65535 || P < 1 || P > ps::MAX_PAIRS || V < 2 || V > mv::MAX_VIEWS || iterations < 1 || redescend < 0 || redescend > iterations) return -1;
    const PgArgs a = pg_args(view_pairs, R_rel, t_rel, weight, n_views, S, P, V, iterations, redescend, rot_scale_rad, pos_scale_sin, min_pivot_ratio, Rs_out,
                             ts_out, registered, edge_factor, info, ws);
    size_t off[3];
    pgr_layout(S, P, off);
    char* w = static_cast<char*>(ws);
    PgRatioArgs r = {};
    r.ratio = ratio; r.count = ratio_count; r.weight = scale_weight; r.tol = scale_tol; r.factor = ratio_factor;
    r.row = reinterpret_cast<int32_t*>(w + off[0]); r.list = reinterpret_cast<long long*>(w + off[1]); r.ld = reinterpret_cast<double*>(w + off[2]);
    pose_graph_ratio_kernel<<<S, 256, 0, st>>>(a, r);
    return 0;
}
