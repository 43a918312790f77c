// C ABI of the camera models (include/xfeat_hip_cameras.h, k_cameras.hip): key-points through a lens model in both directions and the
// rectification of images.  No entry takes a handle: each one checks its arguments and launches (kernels.hpp); every check returns before
// any launch.  XFH_ERR_UNSUPPORTED for a size beyond one launch and for C > 4, XFH_ERR_ARG for any other bad argument.
#include "../../include/xfeat_hip_cameras.h"
#include "api_common.hpp"
#include "kernels.hpp"

using namespace xfh;

static bool ranges_overlap(const void* p, size_t np, const void* q, size_t nq) {
    if (!p || !q || !np || !nq) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}
// every output against every input and against the outputs before it: XFH_OK, or XFH_ERR_ARG
static int check_not_in_place(const char* who, const void* const* in, const size_t* in_bytes, int n_in, const void* const* out, const size_t* out_bytes, int n_out) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (ranges_overlap(out[o], out_bytes[o], in[i], in_bytes[i]))
                return fail(XFH_ERR_ARG, "%s: output %d overlaps input %d (the call is not in-place)", who, o, i);
        for (int q = 0; q < o; ++q)
            if (ranges_overlap(out[o], out_bytes[o], out[q], out_bytes[q])) return fail(XFH_ERR_ARG, "%s: outputs %d and %d overlap", who, q, o);
    }
    return XFH_OK;
}

extern "C" {

int xfh_camera_points(const float* pts, const int32_t* counts, long long P, int K, const int32_t* kind, const double* params, int n_cameras,
                      const double* K_other, int direction, float* out, uint8_t* status, xfh_stream stream) {
    const char* who = "xfh_camera_points";
    if (P < 0 || K < 0) return fail(XFH_ERR_ARG, "%s: bad shape (P %lld, K %d)", who, P, K);
    if (direction != XFH_CAMERA_UNDISTORT && direction != XFH_CAMERA_DISTORT) return fail(XFH_ERR_ARG, "%s: direction %d is neither 0 nor 1", who, direction);
    if (P == 0 || K == 0) return XFH_OK;                    // nothing to read, nothing to write
    if (n_cameras != 1 && (long long)n_cameras != P) return fail(XFH_ERR_ARG, "%s: n_cameras %d is neither 1 nor P = %lld", who, n_cameras, P);
    if (!pts || !kind || !params || !out || !status) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (P > ((0x7fffffffll * 256) / K)) return fail(XFH_ERR_UNSUPPORTED, "%s: %lld x %d points are more than one launch holds", who, P, K);
    const size_t n = (size_t)P * (size_t)K, nc = (size_t)n_cameras;
    const void* in[5] = {pts, counts, kind, params, K_other};
    const size_t in_bytes[5] = {n * 8, (size_t)P * 4, nc * 4, nc * XFH_CAMERA_PARAMS * 8, nc * 32};
    const void* outs[2] = {out, status};
    const size_t out_bytes[2] = {n * 8, n};
    if (int rc = check_not_in_place(who, in, in_bytes, 5, outs, out_bytes, 2)) return rc;
    if (launch_camera_points(pts, counts, P, K, kind, params, n_cameras, K_other, direction, out, status, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: %lld x %d points are more than one launch holds", who, P, K);
    return check_launch(who);
}

int xfh_undistort_images(const void* src, int dtype, int B, int C, int H, int W, const int32_t* kind, const double* params, int n_cameras,
                         const double* K_new, int Ho, int Wo, double fill, void* dst, uint8_t* valid, xfh_stream stream) {
    const char* who = "xfh_undistort_images";
    if (dtype != XFH_IMAGE_U8 && dtype != XFH_IMAGE_F32) return fail(XFH_ERR_ARG, "%s: dtype %d is neither XFH_IMAGE_U8 nor XFH_IMAGE_F32", who, dtype);
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return fail(XFH_ERR_ARG, "%s: bad shape (B %d, C %d, %d x %d -> %d x %d)", who, B, C, H, W, Ho, Wo);
    if (C > 4) return fail(XFH_ERR_UNSUPPORTED, "%s: C %d above 4", who, C);
    if (n_cameras != 1 && n_cameras != B) return fail(XFH_ERR_ARG, "%s: n_cameras %d is neither 1 nor B = %d", who, n_cameras, B);
    if (!src || !kind || !params || !dst) return fail(XFH_ERR_ARG, "%s: NULL argument", who);
    if (B > MAX_BATCH || (Ho + 3) / 4 > MAX_BATCH || Wo > 0x7fffffff - 63)
        return fail(XFH_ERR_UNSUPPORTED, "%s: B %d, %d x %d are more than one launch holds", who, B, Ho, Wo);
    const size_t e = dtype == XFH_IMAGE_F32 ? 4 : 1, nc = (size_t)n_cameras, planes = (size_t)B * (size_t)C;
    const void* in[4] = {src, kind, params, K_new};
    const size_t in_bytes[4] = {planes * (size_t)H * (size_t)W * e, nc * 4, nc * XFH_CAMERA_PARAMS * 8, nc * 32};
    const void* outs[2] = {dst, valid};
    const size_t out_bytes[2] = {planes * (size_t)Ho * (size_t)Wo * e, (size_t)B * (size_t)Ho * (size_t)Wo};
    if (int rc = check_not_in_place(who, in, in_bytes, 4, outs, out_bytes, 2)) return rc;
    if (launch_undistort_images(src, dtype == XFH_IMAGE_F32, B, C, H, W, kind, params, n_cameras, K_new, Ho, Wo, fill, dst, valid, (hipStream_t)stream))
        return fail(XFH_ERR_UNSUPPORTED, "%s: B %d, %d x %d are more than one launch holds", who, B, Ho, Wo);
    return check_launch(who);
}

}  // extern "C"
