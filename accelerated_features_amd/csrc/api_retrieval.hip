// C ABI of image retrieval (include/xfeat_hip.h, k_retrieval.hip): VLAD descriptors, the k-means step behind their codebook, top-k shortlists
// and the pair lists made of them.  No entry takes a handle: each one checks its arguments and launches (kernels.hpp); every check returns
// before any launch.  XFH_ERR_UNSUPPORTED for C, D, k or V beyond the limits, XFH_ERR_ARG for any other bad argument.
#include "api_common.hpp"
#include "kernels.hpp"

using namespace xfh;

constexpr int RT_MAX_C = 256, RT_MAX_D = 16384, RT_MAX_K = 128;
constexpr long long RT_MAX_VLAD_ROWS = 1ll << 24, RT_MAX_KMEANS_ROWS = 1ll << 22;

static int check_codebook_size(const char* who, int C) {
    if (C < 1) return fail(XFH_ERR_ARG, "%s: C %d below 1", who, C);
    if (C != 32 && C != 64 && C != 128 && C != RT_MAX_C) return fail(XFH_ERR_UNSUPPORTED, "%s: C %d is not 32, 64, 128 or 256", who, C);
    return XFH_OK;
}
static int check_shortlist_length(const char* who, int k) {
    if (k < 1) return fail(XFH_ERR_ARG, "%s: k %d below 1", who, k);
    if (k > RT_MAX_K) return fail(XFH_ERR_UNSUPPORTED, "%s: k %d above %d", who, k, RT_MAX_K);
    return XFH_OK;
}
// the descriptor tables of xfh_vlad and xfh_kmeans_step
static int check_tables(const char* who, const float* desc, const float* codebook, int G, int K, int C, long long max_rows) {
    if (G < 1 || G > MAX_BATCH) return fail(XFH_ERR_ARG, "%s: G %d outside [1, %d]", who, G, MAX_BATCH);
    if (K < 1 || (long long)G * K > max_rows) return fail(XFH_ERR_ARG, "%s: bad shape (G %d, K %d: at most %lld rows)", who, G, K, max_rows);
    if (int rc = check_codebook_size(who, C)) return rc;
    if ((((uintptr_t)desc | (uintptr_t)codebook) & 15) != 0) return fail(XFH_ERR_ARG, "%s: desc and codebook must be 16-byte aligned", who);
    return XFH_OK;
}
static int launched(const char* who, int bad) {
    return bad ? fail(XFH_ERR_UNSUPPORTED, "%s: the shape is more than one launch holds", who) : check_launch(who);
}

extern "C" {

size_t xfh_vlad_workspace_bytes(int G, int K, int C) { return xfh::vlad_workspace_bytes(G, K, C); }

int xfh_vlad(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, float* vlad, int32_t* assign, int32_t* n_assigned,
             int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_vlad";
    if (!desc || !codebook || !vlad || !assign || !n_assigned || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_tables(who, desc, codebook, G, K, C, RT_MAX_VLAD_ROWS)) return rc;
    if (((uintptr_t)vlad & 15) != 0) return fail(XFH_ERR_ARG, "%s: vlad must be 16-byte aligned", who);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::vlad_workspace_bytes(G, K, C))) return rc;
    return launched(who, launch_vlad(desc, counts, G, K, codebook, C, vlad, assign, n_assigned, info, workspace, (hipStream_t)stream));
}

size_t xfh_kmeans_workspace_bytes(int G, int K, int C) { return xfh::kmeans_workspace_bytes(G, K, C); }

int xfh_kmeans_step(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, float* codebook_out, int32_t* assign,
                    int32_t* n_assigned, double* objective, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_kmeans_step";
    if (!desc || !codebook || !codebook_out || !assign || !n_assigned || !objective || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_tables(who, desc, codebook, G, K, C, RT_MAX_KMEANS_ROWS)) return rc;
    if (((uintptr_t)codebook_out & 15) != 0) return fail(XFH_ERR_ARG, "%s: codebook_out must be 16-byte aligned", who);
    if (codebook_out == codebook) return fail(XFH_ERR_ARG, "%s: codebook_out must not be codebook", who);
    if (((uintptr_t)objective & 7) != 0) return fail(XFH_ERR_ARG, "%s: objective must be 8-byte aligned", who);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::kmeans_workspace_bytes(G, K, C))) return rc;
    return launched(who, launch_kmeans_step(desc, counts, G, K, codebook, C, codebook_out, assign, n_assigned, objective, info, workspace,
                                            (hipStream_t)stream));
}

size_t xfh_retrieve_workspace_bytes(int G, int Q, int N) { return xfh::retrieve_workspace_bytes(G, Q, N); }

int xfh_retrieve_topk(const float* q, const float* db, const int32_t* n_db, int G, int Q, int N, int D, int k, int exclude_self, int32_t* idx,
                      float* score, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_retrieve_topk";
    if (!q || !db || !idx || !score) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (G < 1 || G > MAX_BATCH || Q < 1 || Q > MAX_ROWS || N < 1 || N > MAX_ROWS) return fail(XFH_ERR_ARG, "%s: bad shape (G %d, Q %d, N %d)", who, G, Q, N);
    if (D < 64 || D % 64 != 0) return fail(XFH_ERR_ARG, "%s: D %d is not a positive multiple of 64", who, D);
    if (D > RT_MAX_D) return fail(XFH_ERR_UNSUPPORTED, "%s: D %d above %d", who, D, RT_MAX_D);
    if (int rc = check_shortlist_length(who, k)) return rc;
    if ((((uintptr_t)q | (uintptr_t)db) & 15) != 0) return fail(XFH_ERR_ARG, "%s: q and db must be 16-byte aligned", who);
    const size_t need = xfh::retrieve_workspace_bytes(G, Q, N);
    if (need == 0) return fail(XFH_ERR_UNSUPPORTED, "%s: G x Q x N = %d x %d x %d scores are more than one call holds", who, G, Q, N);
    if (int rc = check_ws(workspace, workspace_bytes, need)) return rc;
    return launched(who, launch_retrieve_topk(q, db, n_db, G, Q, N, D, k, exclude_self != 0, idx, score, workspace, (hipStream_t)stream));
}

int xfh_pairs_from_shortlists(const int32_t* idx, const int32_t* n_views, int S, int V, int k, int32_t* view_pairs, int32_t* n_pairs, xfh_stream stream) {
    const char* who = "xfh_pairs_from_shortlists";
    if (!idx || !view_pairs || !n_pairs) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (S < 1 || S > MAX_BATCH) return fail(XFH_ERR_ARG, "%s: S %d outside [1, %d]", who, S, MAX_BATCH);
    if (V < 2) return fail(XFH_ERR_ARG, "%s: V %d below 2", who, V);
    if (V > MAX_VIEWS) return fail(XFH_ERR_UNSUPPORTED, "%s: V %d above %d", who, V, MAX_VIEWS);
    if (int rc = check_shortlist_length(who, k)) return rc;
    return launched(who, launch_pairs_from_shortlists(idx, n_views, S, V, k, view_pairs, n_pairs, (hipStream_t)stream));
}

}  // extern "C"
