/*
 * xfeat_hip_cameras.h -- camera models of libxfeat_hip.so (DESIGN.md 3.24 / csrc/k_cameras.hip, csrc/api_cameras.hip): key-points
 * through a lens model in both directions, and the rectification of images.  The conventions, xfh_stream and the error codes are
 * those of xfeat_hip.h.  Asynchronous; no host synchronisation inside; no workspace; two calls give the same bytes.  Every argument
 * check returns before any launch: XFH_ERR_UNSUPPORTED for a size beyond one launch and for C > 4, XFH_ERR_ARG otherwise.
 *
 * A camera is a kind (XFH_CAMERA_*) and 12 doubles fx, fy, cx, cy, d0..d7:
 *   XFH_CAMERA_PINHOLE  no distortion             (COLMAP / poselib SIMPLE_PINHOLE, PINHOLE)
 *   XFH_CAMERA_BROWN    d0..d3 = k1, k2, p1, p2   (SIMPLE_RADIAL, RADIAL, OPENCV)
 *   XFH_CAMERA_FISHEYE  d0..d3 = k1, k2, k3, k4   (OPENCV_FISHEYE)
 * and d4..d7 = 0.  kind (n_cameras,) int32 and params (n_cameras,12) fp64 are device arrays; n_cameras is 1 (one camera for every
 * image) or the number of images.  A camera is usable when its 12 doubles are finite, fx > 0, fy > 0 and its kind is one of the
 * three.  The other side of every mapping is an ideal pinhole camera fx, fy, cx, cy: K_other / K_new (n_cameras,4) fp64, or NULL =
 * the camera's own four; usable when finite with fx, fy > 0.  With (u, v) normalised coordinates, x = fx u + cx, y = fy v + cy:
 *   forward  BROWN    r2 = u u + v v; rad = r2 (k1 + k2 r2);
 *                     u' = u + (u rad + (2 p1 u v + p2 (r2 + 2 u u))); v' = v + (v rad + (p1 (r2 + 2 v v) + 2 p2 u v))
 *            FISHEYE  r = sqrt(u u + v v); theta = atan(r); t2 = theta theta;
 *                     theta_d = theta (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))); (u', v') = (u, v) theta_d / r  (r < 1e-8: (u, v))
 *   inverse  BROWN    Newton on the 2x2 system with the analytic Jacobian from (u', v'), at most 32 iterations; an iterate whose
 *                     Jacobian determinant is not above 1e-3 ends with XFH_CAMERA_POINT_FOLD (the radius where a barrel model stops
 *                     being one-to-one); converged when the step satisfies du du + dv dv <= 1e-30 (1 + u u + v v) at the new iterate
 *            FISHEYE  Newton on theta_d(theta) = r' from theta = r', the same limit and step rule, a derivative not above 1e-3 is a
 *                     fold; theta >= 1.5 rad is XFH_CAMERA_POINT_OUTSIDE (no useful pinhole image); else r = tan(theta)
 * All arithmetic is fp64 without contraction, in the order csrc/k_cameras.hip writes it.
 *
 *   xfh_camera_points: the points of P images through their cameras.  pts (P,K,2) fp32 pixels, counts (P,) int32 or
 *     NULL = K (read clamped to [0, K]); direction XFH_CAMERA_UNDISTORT: raw pixels -> pixels of the pinhole camera K_other;
 *     XFH_CAMERA_DISTORT: pixels of the pinhole camera K_other -> raw pixels.  Outputs: out (P,K,2) fp32, the fp64 result rounded
 *     once; status (P,K) uint8, the first that applies of XFH_CAMERA_POINT_ROW (at or beyond the count), _CAMERA (camera or K_other
 *     not usable), _NOT_FINITE (a coordinate), _FOLD, _NOT_CONVERGED, _OUTSIDE; a row whose status is not 0 is NaN, NaN.  P = 0 or
 *     K = 0 return without a launch; more than 2^31 - 1 workgroups of 256 points are XFH_ERR_UNSUPPORTED.  Not in-place: an output
 *     range that overlaps an input range or the other output is XFH_ERR_ARG.
 *   xfh_undistort_images: cv2.undistort for a batch.  src (B,C,H,W) and dst (B,C,Ho,Wo) of dtype XFH_IMAGE_U8 or XFH_IMAGE_F32,
 *     C <= 4; valid (B,Ho,Wo) uint8 or NULL.  Per output pixel (xo, yo), integer coordinates being pixel centres: normalised with
 *     K_new, through the forward model, to the source position (xs, ys); x0 = floor(xs), y0 = floor(ys), wx = xs - x0, wy = ys - y0;
 *     the taps a (x0, y0), b (x0 + 1, y0), c (x0, y0 + 1), d (x0 + 1, y0 + 1), each `fill` when outside the image;
 *     value = (1 - wy) ((1 - wx) a + wx b) + wy ((1 - wx) c + wx d) in fp64, per channel; F32: rounded once; U8: floor(value + 0.5)
 *     clamped to [0, 255] (NaN: 0).  valid = all four taps inside.  A camera or K_new that is not usable, or a source position that
 *     is not finite: `fill` (through the same conversion) and valid 0.  B and ceil(Ho / 4) above 65535 are XFH_ERR_UNSUPPORTED.
 *     Not in-place.
 */
#ifndef XFEAT_HIP_CAMERAS_H
#define XFEAT_HIP_CAMERAS_H

#include "xfeat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XFH_CAMERA_PINHOLE 0
#define XFH_CAMERA_BROWN 1
#define XFH_CAMERA_FISHEYE 2
#define XFH_CAMERA_PARAMS 12
#define XFH_CAMERA_UNDISTORT 0
#define XFH_CAMERA_DISTORT 1
#define XFH_CAMERA_POINT_OK 0
#define XFH_CAMERA_POINT_ROW 1
#define XFH_CAMERA_POINT_NOT_FINITE 2
#define XFH_CAMERA_POINT_FOLD 3
#define XFH_CAMERA_POINT_NOT_CONVERGED 4
#define XFH_CAMERA_POINT_OUTSIDE 5
#define XFH_CAMERA_POINT_CAMERA 6
#define XFH_IMAGE_U8 0
#define XFH_IMAGE_F32 1

int xfh_camera_points(const float* pts, const int32_t* counts, long long P, int K, const int32_t* kind, const double* params,
                      int n_cameras, const double* K_other, int direction, float* out, uint8_t* status, xfh_stream stream);
int xfh_undistort_images(const void* src, int dtype, int B, int C, int H, int W, const int32_t* kind, const double* params,
                         int n_cameras, const double* K_new, int Ho, int Wo, double fill, void* dst, uint8_t* valid,
                         xfh_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* XFEAT_HIP_CAMERAS_H */
