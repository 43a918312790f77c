// C ABI of the stateless geometry stages behind the matcher (include/xfeat_hip.h): the two-view estimators, two-view structure, tracks, multi-view
// triangulation, bundle adjustment, pose graph, baseline ratios, map and match verification.  No entry takes a handle: each one checks its
// arguments and launches (kernels.hpp); every check returns before any launch.
#include "api_common.hpp"
#include "kernels.hpp"
#include <cmath>

using namespace xfh;

// ---- the checks that several entries share: XFH_OK, or the code of the error they set.  An entry calls them where its own lines stood, so
// which of two violated checks is reported stays what it was (tests/test_argument_contracts_host_api.py).
static int check_scenes(const char* who, int S) { return S < 1 || S > MAX_BATCH ? fail(XFH_ERR_ARG, "%s: S %d outside [1, %d]", who, S, MAX_BATCH) : XFH_OK; }
static int check_views(const char* who, int V) { return V < 2 || V > MAX_VIEWS ? fail(XFH_ERR_ARG, "%s: V %d outside [2, %d]", who, V, MAX_VIEWS) : XFH_OK; }
static int check_max_iters(const char* who, int max_iters) {
    if (max_iters < 1 || max_iters > MAX_RANSAC_ITERS) return fail(XFH_ERR_UNSUPPORTED, "%s: max_iters %d outside [1, %d]", who, max_iters, MAX_RANSAC_ITERS);
    return XFH_OK;
}
// an estimator's lists: P pairs of cap entries into two tables of cap0 and cap1 rows, with a count per pair or one constant count
static int check_lists(const char* who, int P, int cap, int cap0, int cap1, const int32_t* counts, int n_const) {
    if (P <= 0 || P > MAX_BATCH || cap <= 0 || cap > MAX_ROWS || cap0 <= 0 || cap1 <= 0 || (!counts && (n_const < 0 || n_const > cap)))
        return fail(XFH_ERR_ARG, "%s: bad shape (P %d, cap %d, n %d)", who, P, cap, n_const);
    return XFH_OK;
}
// the gates of a triangulation (xfh_baseline_ratios words and orders its own differently)
static int check_gates(const char* who, double max_reproj_error, double max_depth, double cos_min) {
    if (!(max_reproj_error > 0.0) || !std::isfinite(max_reproj_error))
        return fail(XFH_ERR_ARG, "%s: max_reproj_error %g must be positive and finite", who, max_reproj_error);
    if (!(max_depth > 0.0)) return fail(XFH_ERR_ARG, "%s: max_depth %g must be positive (+inf: no limit)", who, max_depth);
    if (!(cos_min >= -1.0 && cos_min <= 1.0)) return fail(XFH_ERR_ARG, "%s: cos_min %g outside [-1, 1]", who, cos_min);
    return XFH_OK;
}
static int check_pose_graph(const char* who, int iterations, int redescend, double rot_scale_rad, double pos_scale_sin, double min_pivot_ratio) {
    if (iterations < 1 || iterations > 1000) return fail(XFH_ERR_ARG, "%s: iterations %d outside [1, 1000]", who, iterations);
    if (redescend < 0 || redescend > iterations) return fail(XFH_ERR_ARG, "%s: redescend %d outside [0, iterations]", who, redescend);
    if (!(rot_scale_rad > 0.0) || !(rot_scale_rad < 4.0)) return fail(XFH_ERR_ARG, "%s: rot_scale_rad %g outside (0, 4)", who, rot_scale_rad);
    if (!(pos_scale_sin > 0.0) || !(pos_scale_sin <= 1.0)) return fail(XFH_ERR_ARG, "%s: pos_scale_sin %g outside (0, 1]", who, pos_scale_sin);
    if (!(min_pivot_ratio >= 0.0) || !(min_pivot_ratio < 1.0)) return fail(XFH_ERR_ARG, "%s: min_pivot_ratio %g outside [0, 1)", who, min_pivot_ratio);
    return XFH_OK;
}
static int launched(const char* who, int bad) { return bad ? fail(XFH_ERR_HIP, "%s: the launch failed", who) : check_launch(who); }      // bad: a launch_*'s answer

extern "C" {

size_t xfh_homography_workspace_bytes(int P, int max_iters) {
    if (P <= 0 || max_iters <= 0) return 0;
    return xfh::homography_workspace_bytes(P, max_iters);
}

static int find_homography_impl(const char* who, const float* pts0, const float* pts1, const int64_t* idx0, const int64_t* idx1, int kcap,
                                const int32_t* counts, int n_const, int P, int cap, double ransac_thr, int max_iters, double confidence,
                                uint64_t seed, double* H, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!pts0 || !pts1 || !H || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_lists(who, P, cap, kcap, kcap, counts, n_const)) return rc;
    if (!(ransac_thr > 0.0) || !(confidence > 0.0 && confidence < 1.0)) return fail(XFH_ERR_ARG, "%s: threshold %g / confidence %g", who, ransac_thr, confidence);
    if (max_iters < 1 || max_iters > 4096) return fail(XFH_ERR_UNSUPPORTED, "%s: max_iters %d outside [1, 4096]", who, max_iters);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::homography_workspace_bytes(P, max_iters))) return rc;
    if (launch_find_homography(pts0, pts1, idx0, idx1, kcap, counts, n_const, P, cap, ransac_thr, max_iters, confidence, seed, H, mask, info, workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: unsupported configuration", who);
    return check_launch(who);
}

int xfh_find_homography(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, double ransac_thr,
                        int max_iters, double confidence, uint64_t seed, double* H, uint8_t* mask, int32_t* info, void* workspace,
                        size_t workspace_bytes, xfh_stream stream) {
    return find_homography_impl("xfh_find_homography", pts0, pts1, nullptr, nullptr, cap, counts, n_const, P, cap, ransac_thr, max_iters, confidence, seed,
                                H, mask, info, workspace, workspace_bytes, stream);
}

int xfh_find_homography_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                const int32_t* n_matches, int P, int cap, double ransac_thr, int max_iters, double confidence, uint64_t seed,
                                double* H, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!idx0 || !idx1 || !n_matches) return fail(XFH_ERR_ARG, "xfh_find_homography_matches: NULL argument");
    return find_homography_impl("xfh_find_homography_matches", kpts0, kpts1, idx0, idx1, kpt_cap, n_matches, 0, P, cap, ransac_thr, max_iters, confidence, seed,
                                H, mask, info, workspace, workspace_bytes, stream);
}

int xfh_homography_tables(double ransac_thr, uint32_t* score_table, double* weight_table, xfh_stream stream) {
    if (!score_table || !weight_table || !(ransac_thr > 0.0)) return fail(XFH_ERR_ARG, "xfh_homography_tables: bad argument");
    launch_homography_tables(ransac_thr, score_table, weight_table, (hipStream_t)stream);
    return check_launch("xfh_homography_tables");
}

size_t xfh_relpose_workspace_bytes(int P, int max_iters) {
    if (P <= 0 || max_iters <= 0) return 0;
    return xfh::relpose_workspace_bytes(P, max_iters);
}

static int estimate_relpose_impl(const char* who, const float* pts0, const float* pts1, const int64_t* idx0, const int64_t* idx1, int kcap,
                                 const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1, double max_epipolar_error,
                                 int min_iters, int max_iters, double success_prob, uint64_t seed, double* R, double* t, double* E, uint8_t* mask,
                                 int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!pts0 || !pts1 || !K0 || !K1 || !R || !t || !E || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_lists(who, P, cap, kcap, kcap, counts, n_const)) return rc;
    if (!(max_epipolar_error > 0.0) || !(success_prob > 0.0 && success_prob < 1.0) || min_iters < 0)
        return fail(XFH_ERR_ARG, "%s: threshold %g / success_prob %g / min_iters %d", who, max_epipolar_error, success_prob, min_iters);
    if (int rc = check_max_iters(who, max_iters)) return rc;
    if (int rc = check_ws(workspace, workspace_bytes, xfh::relpose_workspace_bytes(P, max_iters))) return rc;
    if (launch_estimate_relpose(pts0, pts1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, max_epipolar_error, min_iters, max_iters, success_prob,
                                seed, R, t, E, mask, info, workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: unsupported configuration", who);
    return check_launch(who);
}

int xfh_estimate_relpose(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1,
                         double max_epipolar_error, int min_iters, int max_iters, double success_prob, uint64_t seed, double* R, double* t, double* E,
                         uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    return estimate_relpose_impl("xfh_estimate_relpose", pts0, pts1, nullptr, nullptr, cap, counts, n_const, P, cap, K0, K1, max_epipolar_error,
                                 min_iters, max_iters, success_prob, seed, R, t, E, mask, info, workspace, workspace_bytes, stream);
}

int xfh_estimate_relpose_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                 const int32_t* n_matches, int P, int cap, const double* K0, const double* K1, double max_epipolar_error,
                                 int min_iters, int max_iters, double success_prob, uint64_t seed, double* R, double* t, double* E,
                                 uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!idx0 || !idx1 || !n_matches) return fail(XFH_ERR_ARG, "xfh_estimate_relpose_matches: NULL argument");
    return estimate_relpose_impl("xfh_estimate_relpose_matches", kpts0, kpts1, idx0, idx1, kpt_cap, n_matches, 0, P, cap, K0, K1, max_epipolar_error,
                                 min_iters, max_iters, success_prob, seed, R, t, E, mask, info, workspace, workspace_bytes, stream);
}

size_t xfh_relpose_sweep_workspace_bytes(int P, int max_iters, int T) {
    if (P <= 0 || max_iters <= 0 || T < 1 || T > 16) return 0;
    return xfh::relpose_sweep_workspace_bytes(P, max_iters, T);
}

static int estimate_relpose_sweep_impl(const char* who, const float* pts0, const float* pts1, const int64_t* idx0, const int64_t* idx1, int kcap,
                                       const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1,
                                       const double* max_epipolar_errors, int T, int min_iters, int max_iters, double success_prob, uint64_t seed,
                                       double* R, double* t, double* E, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes,
                                       xfh_stream stream) {
    if (!pts0 || !pts1 || !K0 || !K1 || !max_epipolar_errors || !R || !t || !E || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_lists(who, P, cap, kcap, kcap, counts, n_const)) return rc;
    if (T < 1 || T > 16) return fail(XFH_ERR_ARG, "%s: %d thresholds outside [1, 16]", who, T);
    for (int j = 0; j < T; ++j)
        if (!(max_epipolar_errors[j] > 0.0) || !std::isfinite(max_epipolar_errors[j]))
            return fail(XFH_ERR_ARG, "%s: threshold %d is %g", who, j, max_epipolar_errors[j]);
    if (!(success_prob > 0.0 && success_prob < 1.0) || min_iters < 0)
        return fail(XFH_ERR_ARG, "%s: success_prob %g / min_iters %d", who, success_prob, min_iters);
    if (int rc = check_max_iters(who, max_iters)) return rc;
    if (int rc = check_ws(workspace, workspace_bytes, xfh::relpose_sweep_workspace_bytes(P, max_iters, T))) return rc;
    if (launch_estimate_relpose_sweep(pts0, pts1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, max_epipolar_errors, T, min_iters, max_iters,
                                      success_prob, seed, R, t, E, mask, info, workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: unsupported configuration", who);
    return check_launch(who);
}

int xfh_estimate_relpose_sweep(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, const double* K0,
                               const double* K1, const double* max_epipolar_errors, int T, int min_iters, int max_iters, double success_prob,
                               uint64_t seed, double* R, double* t, double* E, uint8_t* mask, int32_t* info, void* workspace,
                               size_t workspace_bytes, xfh_stream stream) {
    return estimate_relpose_sweep_impl("xfh_estimate_relpose_sweep", pts0, pts1, nullptr, nullptr, cap, counts, n_const, P, cap, K0, K1,
                                       max_epipolar_errors, T, min_iters, max_iters, success_prob, seed, R, t, E, mask, info, workspace,
                                       workspace_bytes, stream);
}

int xfh_estimate_relpose_sweep_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                       const int32_t* n_matches, int P, int cap, const double* K0, const double* K1,
                                       const double* max_epipolar_errors, int T, int min_iters, int max_iters, double success_prob, uint64_t seed,
                                       double* R, double* t, double* E, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes,
                                       xfh_stream stream) {
    if (!idx0 || !idx1 || !n_matches) return fail(XFH_ERR_ARG, "xfh_estimate_relpose_sweep_matches: NULL argument");
    return estimate_relpose_sweep_impl("xfh_estimate_relpose_sweep_matches", kpts0, kpts1, idx0, idx1, kpt_cap, n_matches, 0, P, cap, K0, K1,
                                       max_epipolar_errors, T, min_iters, max_iters, success_prob, seed, R, t, E, mask, info, workspace,
                                       workspace_bytes, stream);
}

size_t xfh_abspose_workspace_bytes(int P, int max_iters) {
    if (P <= 0 || max_iters <= 0) return 0;
    return xfh::abspose_workspace_bytes(P, max_iters);
}

static int estimate_abspose_impl(const char* who, const float* pts2d, const float* pts3d, const int64_t* idx2d, const int64_t* idx3d, int cap2, int cap3,
                                 const int32_t* counts, int n_const, int P, int cap, const double* K, double max_reproj_error, int min_iters,
                                 int max_iters, double success_prob, uint64_t seed, double* R, double* t, uint8_t* mask, int32_t* info,
                                 void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!pts2d || !pts3d || !K || !R || !t || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_lists(who, P, cap, cap2, cap3, counts, n_const)) return rc;
    if (!(max_reproj_error > 0.0) || !(success_prob > 0.0 && success_prob < 1.0) || min_iters < 0)
        return fail(XFH_ERR_ARG, "%s: threshold %g / success_prob %g / min_iters %d", who, max_reproj_error, success_prob, min_iters);
    if (int rc = check_max_iters(who, max_iters)) return rc;
    if (int rc = check_ws(workspace, workspace_bytes, xfh::abspose_workspace_bytes(P, max_iters))) return rc;
    if (launch_estimate_abspose(pts2d, pts3d, idx2d, idx3d, cap2, cap3, counts, n_const, P, cap, K, max_reproj_error, min_iters, max_iters, success_prob,
                                seed, R, t, mask, info, workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: unsupported configuration", who);
    return check_launch(who);
}

int xfh_estimate_abspose(const float* pts2d, const float* pts3d, const int32_t* counts, int n_const, int P, int cap, const double* K,
                         double max_reproj_error, int min_iters, int max_iters, double success_prob, uint64_t seed, double* R, double* t,
                         uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    return estimate_abspose_impl("xfh_estimate_abspose", pts2d, pts3d, nullptr, nullptr, cap, cap, counts, n_const, P, cap, K, max_reproj_error,
                                 min_iters, max_iters, success_prob, seed, R, t, mask, info, workspace, workspace_bytes, stream);
}

int xfh_estimate_abspose_matches(const float* kpts2d, int cap2d, const float* points3d, int cap3d, const int64_t* idx2d, const int64_t* idx3d,
                                 const int32_t* n_matches, int P, int cap, const double* K, double max_reproj_error, int min_iters,
                                 int max_iters, double success_prob, uint64_t seed, double* R, double* t, uint8_t* mask, int32_t* info,
                                 void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!idx2d || !idx3d || !n_matches) return fail(XFH_ERR_ARG, "xfh_estimate_abspose_matches: NULL argument");
    return estimate_abspose_impl("xfh_estimate_abspose_matches", kpts2d, points3d, idx2d, idx3d, cap2d, cap3d, n_matches, 0, P, cap, K,
                                 max_reproj_error, min_iters, max_iters, success_prob, seed, R, t, mask, info, workspace, workspace_bytes, stream);
}

// ---- 3D-3D alignment (k_align.hip)
size_t xfh_align_workspace_bytes(int P, int max_iters) {
    if (P <= 0 || max_iters <= 0) return 0;
    return xfh::align_workspace_bytes(P, max_iters);
}

static int estimate_alignment_impl(const char* who, const float* pts_a, const float* pts_b, const int64_t* idx_a, const int64_t* idx_b, int cap_a, int cap_b,
                                   const int32_t* counts, int n_const, int P, int cap, int with_scale, double max_error, int min_iters, int max_iters,
                                   double success_prob, uint64_t seed, double* R, double* t, double* s, uint8_t* mask, int32_t* info, void* workspace,
                                   size_t workspace_bytes, xfh_stream stream) {
    if (!pts_a || !pts_b || !R || !t || !s || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_lists(who, P, cap, cap_a, cap_b, counts, n_const)) return rc;
    if (!(max_error > 0.0) || !(max_error <= 1.7976931348623157e308) || !(success_prob > 0.0 && success_prob < 1.0) || min_iters < 0)
        return fail(XFH_ERR_ARG, "%s: max_error %g (positive, finite) / success_prob %g / min_iters %d", who, max_error, success_prob, min_iters);
    if (int rc = check_max_iters(who, max_iters)) return rc;
    if (int rc = check_ws(workspace, workspace_bytes, xfh::align_workspace_bytes(P, max_iters))) return rc;
    if (launch_estimate_alignment(pts_a, pts_b, idx_a, idx_b, cap_a, cap_b, counts, n_const, P, cap, with_scale, max_error, min_iters, max_iters,
                                  success_prob, seed, R, t, s, mask, info, workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: unsupported configuration", who);
    return check_launch(who);
}

int xfh_estimate_alignment(const float* pts_a, const float* pts_b, const int32_t* counts, int n_const, int P, int cap, int with_scale, double max_error,
                           int min_iters, int max_iters, double success_prob, uint64_t seed, double* R, double* t, double* s, uint8_t* mask,
                           int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    return estimate_alignment_impl("xfh_estimate_alignment", pts_a, pts_b, nullptr, nullptr, cap, cap, counts, n_const, P, cap, with_scale, max_error,
                                   min_iters, max_iters, success_prob, seed, R, t, s, mask, info, workspace, workspace_bytes, stream);
}

int xfh_estimate_alignment_matches(const float* points_a, int cap_a, const float* points_b, int cap_b, const int64_t* idx_a, const int64_t* idx_b,
                                   const int32_t* n_matches, int P, int cap, int with_scale, double max_error, int min_iters, int max_iters,
                                   double success_prob, uint64_t seed, double* R, double* t, double* s, uint8_t* mask, int32_t* info, void* workspace,
                                   size_t workspace_bytes, xfh_stream stream) {
    if (!idx_a || !idx_b || !n_matches) return fail(XFH_ERR_ARG, "xfh_estimate_alignment_matches: NULL argument");
    return estimate_alignment_impl("xfh_estimate_alignment_matches", points_a, points_b, idx_a, idx_b, cap_a, cap_b, n_matches, 0, P, cap, with_scale,
                                   max_error, min_iters, max_iters, success_prob, seed, R, t, s, mask, info, workspace, workspace_bytes, stream);
}

// ---- two-view structure (k_triangulate.hip): no workspace; every check returns before any launch
static int structure_shape_check(const char* who, const float* pts0, const float* pts1, const double* K0, const double* K1, const int32_t* counts,
                                 int n_const, int P, int cap, int kcap) {
    if (!pts0 || !pts1 || !K0 || !K1) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (P < 1 || P > MAX_BATCH) return fail(XFH_ERR_ARG, "%s: P %d outside [1, 65535]", who, P);
    if (cap < 1 || cap > MAX_ROWS || kcap < 1 || (!counts && (n_const < 0 || n_const > cap)))
        return fail(XFH_ERR_ARG, "%s: bad shape (cap %d, key-point capacity %d, n %d)", who, cap, kcap, n_const);
    return XFH_OK;
}

static int triangulate_impl(const char* who, const float* pts0, const float* pts1, const int64_t* idx0, const int64_t* idx1, int kcap,
                            const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1, const double* R, const double* t,
                            const uint8_t* mask, double max_reproj_error, double cos_min, double max_depth, float* points3d, uint8_t* status,
                            float* reproj_error, int32_t* info, float* points3d_ref, xfh_stream stream) {
    if (!R || !t || !points3d || !status || !reproj_error || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = structure_shape_check(who, pts0, pts1, K0, K1, counts, n_const, P, cap, kcap)) return rc;
    if (int rc = check_gates(who, max_reproj_error, max_depth, cos_min)) return rc;
    return launched(who, launch_triangulate(pts0, pts1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, R, t, mask, max_reproj_error, cos_min, max_depth, points3d,
                           status, reproj_error, info, points3d_ref, (hipStream_t)stream));
}

int xfh_triangulate(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1,
                    const double* R, const double* t, const uint8_t* mask, double max_reproj_error, double cos_min, double max_depth,
                    float* points3d, uint8_t* status, float* reproj_error, int32_t* info, xfh_stream stream) {
    return triangulate_impl("xfh_triangulate", pts0, pts1, nullptr, nullptr, cap, counts, n_const, P, cap, K0, K1, R, t, mask, max_reproj_error,
                            cos_min, max_depth, points3d, status, reproj_error, info, nullptr, stream);
}

int xfh_triangulate_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1, const int32_t* n_matches,
                            int P, int cap, const double* K0, const double* K1, const double* R, const double* t, const uint8_t* mask,
                            double max_reproj_error, double cos_min, double max_depth, float* points3d, uint8_t* status, float* reproj_error,
                            int32_t* info, float* points3d_ref, xfh_stream stream) {
    if (!idx0 || !idx1 || !n_matches) return fail(XFH_ERR_ARG, "xfh_triangulate_matches: NULL argument");
    return triangulate_impl("xfh_triangulate_matches", kpts0, kpts1, idx0, idx1, kpt_cap, n_matches, 0, P, cap, K0, K1, R, t, mask,
                            max_reproj_error, cos_min, max_depth, points3d, status, reproj_error, info, points3d_ref, stream);
}

static int recover_pose_impl(const char* who, const float* pts0, const float* pts1, const int64_t* idx0, const int64_t* idx1, int kcap,
                             const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1, const double* E,
                             const uint8_t* mask_in, double distance_thresh, double* R, double* t, int32_t* good, uint8_t* mask, float* points3d,
                             int32_t* info, xfh_stream stream) {
    if (!E || !R || !t || !good || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = structure_shape_check(who, pts0, pts1, K0, K1, counts, n_const, P, cap, kcap)) return rc;
    if (!(distance_thresh > 0.0)) return fail(XFH_ERR_ARG, "%s: distance_thresh %g must be positive (+inf: no limit)", who, distance_thresh);
    return launched(who, launch_recover_pose(pts0, pts1, idx0, idx1, kcap, counts, n_const, P, cap, K0, K1, E, mask_in, distance_thresh, R, t, good, mask, points3d,
                            info, (hipStream_t)stream));
}

int xfh_recover_pose(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, const double* K0, const double* K1,
                     const double* E, const uint8_t* mask_in, double distance_thresh, double* R, double* t, int32_t* good, uint8_t* mask,
                     float* points3d, int32_t* info, xfh_stream stream) {
    return recover_pose_impl("xfh_recover_pose", pts0, pts1, nullptr, nullptr, cap, counts, n_const, P, cap, K0, K1, E, mask_in, distance_thresh, R, t,
                             good, mask, points3d, info, stream);
}

int xfh_recover_pose_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1, const int32_t* n_matches,
                             int P, int cap, const double* K0, const double* K1, const double* E, const uint8_t* mask_in, double distance_thresh,
                             double* R, double* t, int32_t* good, uint8_t* mask, float* points3d, int32_t* info, xfh_stream stream) {
    if (!idx0 || !idx1 || !n_matches) return fail(XFH_ERR_ARG, "xfh_recover_pose_matches: NULL argument");
    return recover_pose_impl("xfh_recover_pose_matches", kpts0, kpts1, idx0, idx1, kpt_cap, n_matches, 0, P, cap, K0, K1, E, mask_in, distance_thresh,
                             R, t, good, mask, points3d, info, stream);
}

// ---- multi-view triangulation of key-point tracks (k_triangulate.hip): no workspace; every check returns before any launch
int xfh_build_tracks(const int64_t* idx_ref, const int64_t* idx_view, const int32_t* n_matches, int S, int V, int cap, int K, int kpt_cap,
                     int32_t* tracks, xfh_stream stream) {
    const char* who = "xfh_build_tracks";
    if (!tracks || (cap > 0 && (!idx_ref || !idx_view || !n_matches))) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (cap < 0 || cap > MAX_ROWS || K < 1 || K > MAX_ROWS || kpt_cap < 1)
        return fail(XFH_ERR_ARG, "%s: bad shape (cap %d, K %d, key-point capacity %d)", who, cap, K, kpt_cap);
    return launched(who, launch_build_tracks(idx_ref, idx_view, n_matches, S, V, cap, K, kpt_cap, tracks, (hipStream_t)stream));
}

// (first: the anchor of a track is the lowest view that observes it, not view 0)
static int triangulate_views_impl(const char* who, bool first, const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* n_views, int S,
                                  int K, int V, const double* Ks, const double* Rs, const double* ts, double max_reproj_error, double cos_min,
                                  double max_depth, int min_views, float* points3d, uint8_t* status, uint8_t* n_inliers, int32_t* inlier_views,
                                  float* reproj_error, int32_t* info, xfh_stream stream) {
    if (!kpts || !tracks || !Ks || !Rs || !ts || !points3d || !status || !n_inliers || !inlier_views || !reproj_error || !info)
        return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (K < 1 || K > MAX_ROWS || kpt_cap < 1) return fail(XFH_ERR_ARG, "%s: bad shape (K %d, key-point capacity %d)", who, K, kpt_cap);
    if (min_views < 2 || min_views > MAX_VIEWS) return fail(XFH_ERR_ARG, "%s: min_views %d outside [2, 32]", who, min_views);
    if (int rc = check_gates(who, max_reproj_error, max_depth, cos_min)) return rc;
    return launched(who, launch_triangulate_views(kpts, kpt_cap, tracks, n_views, S, K, V, Ks, Rs, ts, max_reproj_error, cos_min, max_depth, min_views, points3d, status,
                                 n_inliers, inlier_views, reproj_error, info, first, (hipStream_t)stream));
}

int xfh_triangulate_views(const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* n_views, int S, int K, int V, const double* Ks,
                          const double* Rs, const double* ts, double max_reproj_error, double cos_min, double max_depth, int min_views,
                          float* points3d, uint8_t* status, uint8_t* n_inliers, int32_t* inlier_views, float* reproj_error, int32_t* info,
                          xfh_stream stream) {
    return triangulate_views_impl("xfh_triangulate_views", false, kpts, kpt_cap, tracks, n_views, S, K, V, Ks, Rs, ts, max_reproj_error, cos_min,
                                  max_depth, min_views, points3d, status, n_inliers, inlier_views, reproj_error, info, stream);
}

int xfh_triangulate_tracks(const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* n_views, int S, int K, int V, const double* Ks,
                           const double* Rs, const double* ts, double max_reproj_error, double cos_min, double max_depth, int min_views,
                           float* points3d, uint8_t* status, uint8_t* n_inliers, int32_t* inlier_views, float* reproj_error, int32_t* info,
                           xfh_stream stream) {
    return triangulate_views_impl("xfh_triangulate_tracks", true, kpts, kpt_cap, tracks, n_views, S, K, V, Ks, Rs, ts, max_reproj_error, cos_min,
                                  max_depth, min_views, points3d, status, n_inliers, inlier_views, reproj_error, info, stream);
}

// ---- key-point tracks over a graph of view pairs (k_tracks.hip): every check returns before any launch
size_t xfh_track_graph_workspace_bytes(int S, int V, int K) {
    if (S <= 0 || S > MAX_BATCH || V < 2 || V > MAX_VIEWS || K <= 0 || K > MAX_ROWS) return 0;
    return xfh::track_graph_workspace_bytes(S, V, K);
}

int xfh_build_tracks_graph(const int32_t* view_pairs, const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches, int S, int P, int cap,
                           int V, int K, int min_length, int max_tracks, int32_t* tracks, int32_t* track_of, int32_t* n_tracks, int32_t* info,
                           void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_build_tracks_graph";
    if (!view_pairs || !idx_a || !idx_b || !n_matches || !tracks || !track_of || !n_tracks || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (P < 1 || P > MAX_BATCH || cap < 1 || cap > MAX_ROWS || K < 1 || K > MAX_ROWS)
        return fail(XFH_ERR_ARG, "%s: bad shape (P %d, cap %d, K %d)", who, P, cap, K);
    if (min_length < 2 || min_length > MAX_VIEWS) return fail(XFH_ERR_ARG, "%s: min_length %d outside [2, 32]", who, min_length);
    if (max_tracks < 1 || max_tracks > V * K) return fail(XFH_ERR_ARG, "%s: max_tracks %d outside [1, V K = %d]", who, max_tracks, V * K);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::track_graph_workspace_bytes(S, V, K))) return rc;
    return launched(who, launch_build_tracks_graph(view_pairs, idx_a, idx_b, n_matches, S, P, cap, V, K, min_length, max_tracks, tracks, track_of, n_tracks, info,
                                  workspace, (hipStream_t)stream));
}

// ---- bundle adjustment of poses and track points (k_triangulate.hip): every check returns before any launch
size_t xfh_bundle_workspace_bytes(int S, int K, int V) {
    if (S <= 0 || S > MAX_BATCH || K <= 0 || K > MAX_ROWS || V < 2 || V > MAX_VIEWS) return 0;
    return xfh::bundle_workspace_bytes(S, K, V);
}

int xfh_bundle_adjust(const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* inlier_views, const float* points3d,
                      const int32_t* n_views, int S, int K, int V, const double* Ks, const double* Rs, const double* ts, uint32_t fixed_views,
                      int max_iterations, double huber_px, double* Rs_out, double* ts_out, float* points3d_out, uint8_t* refined,
                      int32_t* free_views, double* cost, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_bundle_adjust";
    if (!kpts || !tracks || !inlier_views || !points3d || !Ks || !Rs || !ts || !Rs_out || !ts_out || !points3d_out || !refined || !free_views || !cost ||
        !info)
        return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (K < 1 || K > MAX_ROWS || kpt_cap < 1) return fail(XFH_ERR_ARG, "%s: bad shape (K %d, key-point capacity %d)", who, K, kpt_cap);
    if (max_iterations < 0 || max_iterations > 1000) return fail(XFH_ERR_ARG, "%s: max_iterations %d outside [0, 1000]", who, max_iterations);
    if (!(huber_px > 0.0)) return fail(XFH_ERR_ARG, "%s: huber_px %g must be positive (+inf: plain squares)", who, huber_px);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::bundle_workspace_bytes(S, K, V))) return rc;
    return launched(who, launch_bundle_adjust(kpts, kpt_cap, tracks, inlier_views, points3d, n_views, S, K, V, Ks, Rs, ts, fixed_views, max_iterations, huber_px, Rs_out,
                             ts_out, points3d_out, refined, free_views, cost, info, workspace, (hipStream_t)stream));
}

// ---- pose-graph initialisation (k_triangulate.hip): every check returns before any launch
size_t xfh_pose_graph_workspace_bytes(int S, int P, int V) {
    if (S <= 0 || S > MAX_BATCH || P <= 0 || P > (1 << 20) || V < 2 || V > MAX_VIEWS) return 0;
    return xfh::pose_graph_workspace_bytes(S, P, V);
}

int xfh_average_poses(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight, const int32_t* n_views, int S, int P,
                      int V, int iterations, int redescend, double rot_scale_rad, double pos_scale_sin, double min_pivot_ratio, double* Rs_out,
                      double* ts_out, int32_t* registered, double* edge_factor, int32_t* info, void* workspace, size_t workspace_bytes,
                      xfh_stream stream) {
    const char* who = "xfh_average_poses";
    if (!view_pairs || !R_rel || !t_rel || !weight || !Rs_out || !ts_out || !registered || !edge_factor || !info)
        return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (P < 1 || P > (1 << 20)) return fail(XFH_ERR_ARG, "%s: P %d outside [1, 2^20]", who, P);
    if (int rc = check_pose_graph(who, iterations, redescend, rot_scale_rad, pos_scale_sin, min_pivot_ratio)) return rc;
    if (int rc = check_ws(workspace, workspace_bytes, xfh::pose_graph_workspace_bytes(S, P, V))) return rc;
    return launched(who, launch_average_poses(view_pairs, R_rel, t_rel, weight, n_views, S, P, V, iterations, redescend, rot_scale_rad, pos_scale_sin, min_pivot_ratio,
                             Rs_out, ts_out, registered, edge_factor, info, workspace, (hipStream_t)stream));
}

// ---- baseline scales from shared tracks (posescale_body.hpp): every check returns before any launch
size_t xfh_baseline_ratios_workspace_bytes(int S, int P, int V, int K) {
    if (S <= 0 || S > MAX_BATCH || P <= 0 || P > 512 || V < 2 || V > MAX_VIEWS || K <= 0 || K > 4096) return 0;
    return 256;                                            // (the kernel works in LDS; a size of 0 would read as a bad shape)
}

int xfh_baseline_ratios(const float* kpts, const int32_t* tracks, const int32_t* track_of, const int32_t* view_pairs, const double* R_rel,
                        const double* t_rel, const double* weight, const double* Ks, const int32_t* n_views, int S, int P, int V, int K, int T,
                        double max_reproj_error, double cos_min, double max_depth, int min_common, double* ratio, int32_t* count,
                        int32_t* shared_view, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_baseline_ratios";
    if (!kpts || !tracks || !track_of || !view_pairs || !R_rel || !t_rel || !weight || !Ks || !ratio || !count || !shared_view || !info)
        return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (P < 1 || P > 512) return fail(XFH_ERR_ARG, "%s: P %d outside [1, 512]", who, P);
    if (K < 1 || K > 4096) return fail(XFH_ERR_ARG, "%s: K %d outside [1, 4096]", who, K);
    if (T < 1 || T > V * K) return fail(XFH_ERR_ARG, "%s: T %d outside [1, V K = %d]", who, T, V * K);
    if (!(max_reproj_error > 0.0)) return fail(XFH_ERR_ARG, "%s: max_reproj_error %g must be positive", who, max_reproj_error);
    if (!(cos_min >= -1.0 && cos_min <= 1.0)) return fail(XFH_ERR_ARG, "%s: cos_min %g outside [-1, 1]", who, cos_min);
    if (!(max_depth > 0.0)) return fail(XFH_ERR_ARG, "%s: max_depth %g must be positive (+inf: no limit)", who, max_depth);
    if (min_common < 1) return fail(XFH_ERR_ARG, "%s: min_common %d below 1", who, min_common);
    if (int rc = check_ws(workspace, workspace_bytes, 256)) return rc;
    return launched(who, launch_baseline_ratios(kpts, tracks, track_of, view_pairs, R_rel, t_rel, weight, Ks, n_views, S, P, V, K, T, max_reproj_error, cos_min, max_depth,
                               min_common, ratio, count, shared_view, info, (hipStream_t)stream));
}

size_t xfh_pose_graph_ratios_workspace_bytes(int S, int P, int V) {
    if (S <= 0 || S > MAX_BATCH || P <= 0 || P > 512 || V < 2 || V > MAX_VIEWS) return 0;
    return xfh::pose_graph_ratios_workspace_bytes(S, P, V);
}

int xfh_average_poses_ratios(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight, const int32_t* n_views,
                             const double* ratio, const int32_t* ratio_count, int S, int P, int V, int iterations, int redescend, double rot_scale_rad,
                             double pos_scale_sin, double min_pivot_ratio, double scale_weight, double scale_tol, double* Rs_out, double* ts_out,
                             int32_t* registered, double* edge_factor, double* ratio_factor, int32_t* info, void* workspace, size_t workspace_bytes,
                             xfh_stream stream) {
    const char* who = "xfh_average_poses_ratios";
    if (!view_pairs || !R_rel || !t_rel || !weight || !ratio || !ratio_count || !Rs_out || !ts_out || !registered || !edge_factor || !ratio_factor || !info)
        return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (int rc = check_views(who, V)) return rc;
    if (P < 1 || P > 512) return fail(XFH_ERR_ARG, "%s: P %d outside [1, 512]", who, P);
    if (int rc = check_pose_graph(who, iterations, redescend, rot_scale_rad, pos_scale_sin, min_pivot_ratio)) return rc;
    if (!(scale_weight > 0.0) || !(scale_weight < 1e300)) return fail(XFH_ERR_ARG, "%s: scale_weight %g must be positive and finite", who, scale_weight);
    if (!(scale_tol > 0.0) || !(scale_tol <= 1.0)) return fail(XFH_ERR_ARG, "%s: scale_tol %g outside (0, 1]", who, scale_tol);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::pose_graph_ratios_workspace_bytes(S, P, V))) return rc;
    return launched(who, launch_average_poses_ratios(view_pairs, R_rel, t_rel, weight, n_views, ratio, ratio_count, S, P, V, iterations, redescend, rot_scale_rad,
                                    pos_scale_sin, min_pivot_ratio, scale_weight, scale_tol, Rs_out, ts_out, registered, edge_factor, ratio_factor, info,
                                    workspace, (hipStream_t)stream));
}

// ---- map rows for localisation (k_map.hip): every check returns before any launch
size_t xfh_map_workspace_bytes(int S, int T, int V) {
    if (S <= 0 || S > MAX_BATCH || T <= 0 || T > MAX_ROWS || V < 1 || V > MAX_VIEWS) return 0;
    return xfh::map_workspace_bytes(S, T, V);
}

int xfh_build_map(const float* desc, int kpt_cap, const int32_t* tracks, const float* points3d, const uint8_t* status, const int32_t* inlier_views, int S,
                  int T, int V, int min_views, int max_points, float* points, float* map_desc, uint16_t* map_desc_f16, int32_t* track, uint8_t* n_obs,
                  float* coherence, int32_t* n_points, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    const char* who = "xfh_build_map";
    if (!desc || !tracks || !points3d || !status || !inlier_views || !points || !map_desc || !map_desc_f16 || !track || !n_obs || !coherence || !n_points ||
        !info)
        return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (V < 1) return fail(XFH_ERR_ARG, "%s: V %d below 1", who, V);
    if (V > MAX_VIEWS) return fail(XFH_ERR_UNSUPPORTED, "%s: V %d above 32", who, V);
    if (T < 1 || T > MAX_ROWS || kpt_cap < 1 || kpt_cap > MAX_ROWS) return fail(XFH_ERR_ARG, "%s: bad shape (T %d, key-point capacity %d)", who, T, kpt_cap);
    if (min_views < 1 || min_views > MAX_VIEWS) return fail(XFH_ERR_ARG, "%s: min_views %d outside [1, 32]", who, min_views);
    if (max_points < 1 || max_points > MAX_ROWS) return fail(XFH_ERR_ARG, "%s: max_points %d outside [1, 2^24]", who, max_points);
    if ((((uintptr_t)desc | (uintptr_t)map_desc) & 15) != 0 || ((uintptr_t)map_desc_f16 & 7) != 0)
        return fail(XFH_ERR_ARG, "%s: the descriptor tables must be 16-byte aligned (fp16: 8)", who);
    if (int rc = check_ws(workspace, workspace_bytes, xfh::map_workspace_bytes(S, T, V))) return rc;
    if (launch_build_map(desc, kpt_cap, tracks, points3d, status, inlier_views, S, T, V, min_views, max_points, points, map_desc, map_desc_f16, track, n_obs,
                         coherence, n_points, info, workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: S x T = %d x %d is more than one launch holds", who, S, T);
    return check_launch(who);
}

int xfh_map_project(const float* points, const int32_t* n_points, int Q, int M, const double* R, const double* t, const double* K, double width,
                    double height, double margin, float* uv, xfh_stream stream) {
    const char* who = "xfh_map_project";
    if (!points || !R || !t || !K || !uv) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (Q < 1 || Q > (1 << 20) || M < 1 || M > MAX_ROWS) return fail(XFH_ERR_ARG, "%s: bad shape (Q %d, M %d)", who, Q, M);
    if (!(width >= 0.0) || !(height >= 0.0) || !std::isfinite(width) || !std::isfinite(height) || (width > 0.0) != (height > 0.0))
        return fail(XFH_ERR_ARG, "%s: image size %g x %g (both positive and finite, or both 0: none)", who, width, height);
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(XFH_ERR_ARG, "%s: margin %g must be finite and not negative", who, margin);
    if (((uintptr_t)uv & 7) != 0) return fail(XFH_ERR_ARG, "%s: uv must be 8-byte aligned", who);
    if (launch_map_project(points, n_points, Q, M, R, t, K, width, height, margin, uv, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: Q x M = %d x %d is more than one launch holds", who, Q, M);
    return check_launch(who);
}

// ---- verification of match lists (k_matchfilter.hip, k_triangulate.hip): every check returns before any launch
// true: the byte ranges [p, p + np) and [q, q + nq) share a byte
static bool ranges_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && np && nq && a < b + nq && b < a + np;
}

int xfh_filter_matches(const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches, const uint8_t* mask, const uint8_t* keep, int64_t L, int cap,
                       int min_keep, int64_t* out_a, int64_t* out_b, int32_t* src, int32_t* n_out, int32_t* info, xfh_stream stream) {
    const char* who = "xfh_filter_matches";
    if (L < 0 || cap < 0) return fail(XFH_ERR_ARG, "%s: bad shape (L %lld, cap %d)", who, (long long)L, cap);
    if (cap > MAX_ROWS) return fail(XFH_ERR_ARG, "%s: cap %d above 2^24", who, cap);
    if (min_keep < 0) return fail(XFH_ERR_ARG, "%s: min_keep %d is negative", who, min_keep);
    if (L > 0x7fffffffll) return fail(XFH_ERR_UNSUPPORTED, "%s: %lld lists are more than one launch holds", who, (long long)L);
    if (L == 0 || cap == 0) return XFH_OK;                  // nothing to read, nothing to write
    if (!idx_a || !idx_b || !n_matches || !mask || !out_a || !out_b || !src || !n_out || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    const size_t n = (size_t)L, m = n * (size_t)cap;
    const void* in[5] = {idx_a, idx_b, n_matches, mask, keep};
    const size_t in_bytes[5] = {m * 8, m * 8, n * 4, m, n};
    const void* out[5] = {out_a, out_b, src, n_out, info};
    const size_t out_bytes[5] = {m * 8, m * 8, m * 4, n * 4, n * 16};
    for (int o = 0; o < 5; ++o) {
        for (int i = 0; i < 5; ++i)
            if (ranges_overlap(out[o], out_bytes[o], in[i], in_bytes[i]))
                return fail(XFH_ERR_ARG, "%s: output %d overlaps input %d (the call is not in-place)", who, o, i);
        for (int q = 0; q < o; ++q)
            if (ranges_overlap(out[o], out_bytes[o], out[q], out_bytes[q])) return fail(XFH_ERR_ARG, "%s: outputs %d and %d overlap", who, q, o);
    }
    return launched(who, launch_filter_matches(idx_a, idx_b, n_matches, mask, keep, (long long)L, cap, min_keep, out_a, out_b, src, n_out, info, (hipStream_t)stream));
}

int xfh_verify_matches(const float* kpts, const int32_t* view_pairs, const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches,
                       const int32_t* n_views, int S, int P, int cap, int V, int K, const double* Ks, const double* Rs, const double* ts,
                       double max_epipolar_error, uint8_t* mask, float* err, int32_t* pair_info, xfh_stream stream) {
    const char* who = "xfh_verify_matches";
    if (!kpts || !view_pairs || !idx_a || !idx_b || !n_matches || !Ks || !Rs || !ts || !mask || !pair_info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_scenes(who, S)) return rc;
    if (V < 2) return fail(XFH_ERR_ARG, "%s: V %d below 2", who, V);
    if (V > MAX_VIEWS) return fail(XFH_ERR_UNSUPPORTED, "%s: V %d above 32", who, V);
    if (P < 1 || P > MAX_BATCH || cap < 1 || cap > MAX_ROWS || K < 1 || K > MAX_ROWS)
        return fail(XFH_ERR_ARG, "%s: bad shape (P %d, cap %d, K %d)", who, P, cap, K);
    if (!(max_epipolar_error > 0.0) || !std::isfinite(max_epipolar_error))
        return fail(XFH_ERR_ARG, "%s: max_epipolar_error %g must be positive and finite", who, max_epipolar_error);
    if (((uintptr_t)kpts & 7) != 0) return fail(XFH_ERR_ARG, "%s: kpts must be 8-byte aligned", who);
    if (launch_verify_matches(kpts, view_pairs, idx_a, idx_b, n_matches, n_views, S, P, cap, V, K, Ks, Rs, ts, max_epipolar_error, mask, err, pair_info,
                              (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: S x P = %d x %d pairs are more than one launch holds", who, S, P);
    return check_launch(who);
}

size_t xfh_fundamental_workspace_bytes(int P, int max_iters) {
    if (P <= 0 || max_iters <= 0) return 0;
    return xfh::fundamental_workspace_bytes(P, max_iters);
}

static int find_fundamental_impl(const char* who, const float* pts0, const float* pts1, const int64_t* idx0, const int64_t* idx1, int kcap,
                                 const int32_t* counts, int n_const, int P, int cap, int method, double ransac_thr, int max_iters,
                                 double confidence, uint64_t seed, double* F, uint8_t* mask, int32_t* info, void* workspace,
                                 size_t workspace_bytes, xfh_stream stream) {
    if (!pts0 || !pts1 || !F || !mask || !info) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (int rc = check_lists(who, P, cap, kcap, kcap, counts, n_const)) return rc;
    if (method != XFH_FM_7POINT && method != XFH_FM_8POINT && method != XFH_FM_USAC_MAGSAC)
        return fail(XFH_ERR_UNSUPPORTED, "%s: method %d (supported: FM_7POINT 1, FM_8POINT 2, USAC_MAGSAC 38)", who, method);
    if (!(ransac_thr > 0.0) || !(confidence > 0.0 && confidence < 1.0)) return fail(XFH_ERR_ARG, "%s: threshold %g / confidence %g", who, ransac_thr, confidence);
    if (int rc = check_max_iters(who, max_iters)) return rc;
    if (int rc = check_ws(workspace, workspace_bytes, xfh::fundamental_workspace_bytes(P, max_iters))) return rc;
    if (launch_find_fundamental(pts0, pts1, idx0, idx1, kcap, counts, n_const, P, cap, method, ransac_thr, max_iters, confidence, seed, F, mask, info,
                                workspace, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: unsupported configuration", who);
    return check_launch(who);
}

int xfh_find_fundamental(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, int method, double ransac_thr,
                         int max_iters, double confidence, uint64_t seed, double* F, uint8_t* mask, int32_t* info, void* workspace,
                         size_t workspace_bytes, xfh_stream stream) {
    return find_fundamental_impl("xfh_find_fundamental", pts0, pts1, nullptr, nullptr, cap, counts, n_const, P, cap, method, ransac_thr, max_iters,
                                 confidence, seed, F, mask, info, workspace, workspace_bytes, stream);
}

int xfh_find_fundamental_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                 const int32_t* n_matches, int P, int cap, int method, double ransac_thr, int max_iters, double confidence,
                                 uint64_t seed, double* F, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream) {
    if (!idx0 || !idx1 || !n_matches) return fail(XFH_ERR_ARG, "xfh_find_fundamental_matches: NULL argument");
    return find_fundamental_impl("xfh_find_fundamental_matches", kpts0, kpts1, idx0, idx1, kpt_cap, n_matches, 0, P, cap, method, ransac_thr,
                                 max_iters, confidence, seed, F, mask, info, workspace, workspace_bytes, stream);
}

}  // extern "C"
