// Camera models: key-points through a lens model in both directions, and the rectification of images (cv2.undistort).
// tests/cameras_reference.py restates both kernels and tests/test_cameras_emulated.py compiles the slice below for the host
// (tests/emu/cameras_emu.cpp).  fp64 throughout, fp contraction off, only + - * / sqrt floor and, in the fisheye branch, atan and tan; every
// expression in the one order written here, which the restatement copies.  No LDS, no atomic, no workspace: two calls give the same bytes.
//
// A camera is a kind (cam::PINHOLE, BROWN, FISHEYE) and 12 doubles fx, fy, cx, cy, d0..d7 (BROWN: d0..d3 = k1, k2, p1, p2; FISHEYE: d0..d3 =
// k1..k4; the rest 0).  USABLE: every one of the 12 is finite, fx > 0, fy > 0, the kind is one of the three.  The other side of a mapping is
// an ideal pinhole camera fx, fy, cx, cy (K_other / K_new; NULL: the camera's own four), usable when finite with fx, fy > 0.
//   forward (u, v) -> (u', v'), normalised coordinates:
//     BROWN    r2 = u u + v v; rad = r2 (k1 + k2 r2); u' = u + (u rad + (2 p1 u v + p2 (r2 + 2 u u))); v' = v + (v rad + (p1 (r2 + 2 v v) + 2 p2 u v))
//     FISHEYE  r = sqrt(u u + v v); th = atan(r); t2 = th th; thd = th (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))); s = r < 1e-8 ? 1 : thd / r; (u s, v s)
//   inverse (u', v') -> (u, v), at most 32 Newton iterations:
//     BROWN    from (u, v) = (u', v'): e = forward(u, v) - (u', v'), J the analytic Jacobian; det = j00 j11 - j01 j10, not > 1e-3: FOLD;
//              du = (j11 eu - j01 ev) / det, dv = (j00 ev - j10 eu) / det; u -= du, v -= dv; du du + dv dv <= 1e-30 (1 + (u u + v v)): done
//     FISHEYE  rd = sqrt(u' u' + v' v'); from th = rd: e = th poly(th) - rd, d = 1 + t2 (3 k1 + t2 (5 k2 + t2 (7 k3 + t2 9 k4))), not > 1e-3: FOLD;
//              dt = e / d; th -= dt; dt dt <= 1e-30 (1 + th th): done.  th not < 1.5: OUTSIDE.  s = rd < 1e-8 ? 1 : tan(th) / rd; (u' s, v' s)
//     32 iterations without `done`: NOT_CONVERGED.
// camera_points_kernel, one thread per point: status (first match) ROW 1 at or beyond the count, CAMERA 6, POINT 2 a coordinate not finite,
//   FOLD 3, NOT_CONVERGED 4, OUTSIDE 5; 0: out = the fp64 result rounded once to fp32; otherwise out = NaN, NaN.
//   direction 0: (x, y) raw -> u' = (x - cx) / fx, v' = (y - cy) / fy -> inverse -> ofx u + ocx, ofy v + ocy.
//   direction 1: (x, y) ideal -> u = (x - ocx) / ofx, v = (y - ocy) / ofy -> forward -> fx u' + cx, fy v' + cy.
// undistort_images_kernel, one thread per output pixel, 64 lanes along x, 4 rows per workgroup, the batch in grid z: (xo, yo) -> u = (xo - ncx) / nfx,
//   v = (yo - ncy) / nfy -> forward -> xs = fx u' + cx, ys = fy v' + cy.  Camera not usable or xs, ys not finite: fill, valid 0.  x0 = floor(xs),
//   wx = xs - x0 (y alike); the taps (x0, y0) a, (x0 + 1, y0) b, (x0, y0 + 1) c, (x0 + 1, y0 + 1) d, each `fill` when outside the image;
//   value = (1 - wy) ((1 - wx) a + wx b) + wy ((1 - wx) c + wx d) per channel; fp32: rounded once; uint8: floor(value + 0.5), below 0 or NaN -> 0,
//   above 255 -> 255 (`fill` itself goes through the same conversion).  valid = all four taps inside.
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace xfh {

// ---- cameras begin (host-compilable with tests/emu/emu.hpp: tests/test_cameras_emulated.py slices it out) ----
namespace cam {
constexpr int PINHOLE = 0, BROWN = 1, FISHEYE = 2;
constexpr int OK = 0, ROW = 1, POINT = 2, FOLD = 3, NOT_CONVERGED = 4, OUTSIDE = 5, CAMERA = 6;      // the status of a point
constexpr int MAX_ITERS = 32, N_PARAMS = 12, MAX_CHANNELS = 4;
constexpr double MIN_DET = 1e-3, STEP_TOL = 1e-30, SMALL_R = 1e-8, MAX_THETA = 1.5;
constexpr unsigned NAN_BITS = 0x7fc00000u;

struct Model {
    int kind;
    double fx, fy, cx, cy, d0, d1, d2, d3;
};

__device__ inline bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)

// the camera at `params`; false: not usable
__device__ inline bool load(int kind, const double* params, Model& m) {
    bool ok = kind == PINHOLE || kind == BROWN || kind == FISHEYE;
    for (int i = 0; i < N_PARAMS; ++i) ok = ok && finite(params[i]);
    m.kind = kind;
    m.fx = params[0]; m.fy = params[1]; m.cx = params[2]; m.cy = params[3];
    m.d0 = params[4]; m.d1 = params[5]; m.d2 = params[6]; m.d3 = params[7];
    return ok && m.fx > 0.0 && m.fy > 0.0;
}

// the ideal side: fx, fy, cx, cy at `k4`, or the camera's own (k4 null); false: not usable
__device__ inline bool load_pinhole(const double* k4, const Model& m, double& fx, double& fy, double& cx, double& cy) {
    if (!k4) { fx = m.fx; fy = m.fy; cx = m.cx; cy = m.cy; return true; }
    fx = k4[0]; fy = k4[1]; cx = k4[2]; cy = k4[3];
    return finite(fx) && finite(fy) && finite(cx) && finite(cy) && fx > 0.0 && fy > 0.0;
}

__device__ inline void brown_forward(const Model& m, double u, double v, double& ud, double& vd) {
    const double r2 = u * u + v * v;
    const double rad = r2 * (m.d0 + m.d1 * r2);
    ud = u + (u * rad + (2.0 * m.d2 * u * v + m.d3 * (r2 + 2.0 * u * u)));
    vd = v + (v * rad + (m.d2 * (r2 + 2.0 * v * v) + 2.0 * m.d3 * u * v));
}

__device__ inline double fisheye_poly(const Model& m, double t2) { return 1.0 + t2 * (m.d0 + t2 * (m.d1 + t2 * (m.d2 + t2 * m.d3))); }

__device__ inline void forward(const Model& m, double u, double v, double& ud, double& vd) {
    if (m.kind == BROWN) {
        brown_forward(m, u, v, ud, vd);
    } else if (m.kind == FISHEYE) {
        const double r = sqrt(u * u + v * v);
        const double th = atan(r);
        const double thd = th * fisheye_poly(m, th * th);
        const double s = r < SMALL_R ? 1.0 : thd / r;
        ud = u * s; vd = v * s;
    } else {
        ud = u; vd = v;
    }
}

// -> OK, FOLD, NOT_CONVERGED or OUTSIDE; (u, v) holds the result only with OK
__device__ inline int inverse(const Model& m, double ud, double vd, double& u, double& v) {
    if (m.kind == BROWN) {
        u = ud; v = vd;
        for (int it = 0; it < MAX_ITERS; ++it) {
            double fu, fv;
            brown_forward(m, u, v, fu, fv);
            const double eu = fu - ud, ev = fv - vd;
            const double r2 = u * u + v * v;
            const double rad = r2 * (m.d0 + m.d1 * r2);
            const double g = m.d0 + 2.0 * m.d1 * r2;
            const double j00 = (1.0 + rad) + (2.0 * u * u * g + (2.0 * m.d2 * v + 6.0 * m.d3 * u));
            const double j11 = (1.0 + rad) + (2.0 * v * v * g + (6.0 * m.d2 * v + 2.0 * m.d3 * u));
            const double j01 = 2.0 * u * v * g + (2.0 * m.d2 * u + 2.0 * m.d3 * v);
            const double j10 = j01;
            const double det = j00 * j11 - j01 * j10;
            if (!(det > MIN_DET)) return FOLD;
            const double du = (j11 * eu - j01 * ev) / det;
            const double dv = (j00 * ev - j10 * eu) / det;
            u = u - du; v = v - dv;
            if (du * du + dv * dv <= STEP_TOL * (1.0 + (u * u + v * v))) return OK;
        }
        return NOT_CONVERGED;
    }
    if (m.kind == FISHEYE) {
        const double rd = sqrt(ud * ud + vd * vd);
        double th = rd;
        bool done = false;
        for (int it = 0; it < MAX_ITERS && !done; ++it) {
            const double t2 = th * th;
            const double e = th * fisheye_poly(m, t2) - rd;
            const double d = 1.0 + t2 * (3.0 * m.d0 + t2 * (5.0 * m.d1 + t2 * (7.0 * m.d2 + t2 * (9.0 * m.d3))));
            if (!(d > MIN_DET)) return FOLD;
            const double dt = e / d;
            th = th - dt;
            done = dt * dt <= STEP_TOL * (1.0 + th * th);
        }
        if (!done) return NOT_CONVERGED;
        if (!(th < MAX_THETA)) return OUTSIDE;
        const double s = rd < SMALL_R ? 1.0 : tan(th) / rd;
        u = ud * s; v = vd * s;
        return OK;
    }
    u = ud; v = vd;
    return OK;
}

__device__ inline float nan32() {
    const unsigned b = NAN_BITS;
    float f;
    memcpy(&f, &b, 4);
    return f;
}
}  // namespace cam

struct CamPointsArgs {
    const float* pts;                // (P, K, 2)
    const int32_t* counts;           // (P,) or null
    const int32_t* kind;             // (n_cameras,)
    const double* params;            // (n_cameras, 12)
    const double* k_other;           // (n_cameras, 4) or null
    long long total;                 // P K
    int K, n_cameras, direction;
    float* out;                      // (P, K, 2)
    unsigned char* status;           // (P, K)
};

__global__ __launch_bounds__(256) void camera_points_kernel(CamPointsArgs a) {
    const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (i >= a.total) return;
    const long long p = i / a.K;
    const int row = (int)(i - p * a.K);
    const long long c = a.n_cameras == 1 ? 0 : p;
    int n = a.K;
    if (a.counts) {
        n = a.counts[p];
        n = n < 0 ? 0 : (n > a.K ? a.K : n);
    }
    int st = cam::OK;
    double ox = 0.0, oy = 0.0;
    if (row >= n) {
        st = cam::ROW;
    } else {
        cam::Model m;
        double ofx, ofy, ocx, ocy;
        bool usable = cam::load(a.kind[c], a.params + c * cam::N_PARAMS, m);
        usable = cam::load_pinhole(a.k_other ? a.k_other + c * 4 : nullptr, m, ofx, ofy, ocx, ocy) && usable;
        const double x = (double)a.pts[2 * i], y = (double)a.pts[2 * i + 1];
        if (!usable) {
            st = cam::CAMERA;
        } else if (!(cam::finite(x) && cam::finite(y))) {
            st = cam::POINT;
        } else if (a.direction == 0) {
            double u, v;
            st = cam::inverse(m, (x - m.cx) / m.fx, (y - m.cy) / m.fy, u, v);
            if (st == cam::OK) { ox = ofx * u + ocx; oy = ofy * v + ocy; }
        } else {
            double ud, vd;
            cam::forward(m, (x - ocx) / ofx, (y - ocy) / ofy, ud, vd);
            ox = m.fx * ud + m.cx; oy = m.fy * vd + m.cy;
        }
    }
    a.out[2 * i] = st == cam::OK ? (float)ox : cam::nan32();
    a.out[2 * i + 1] = st == cam::OK ? (float)oy : cam::nan32();
    a.status[i] = (unsigned char)st;
}

struct CamImagesArgs {
    const void* src;                 // (B, C, H, W) uint8 or fp32
    void* dst;                       // (B, C, Ho, Wo)
    unsigned char* valid;            // (B, Ho, Wo) or null
    const int32_t* kind;
    const double* params;
    const double* k_new;             // (n_cameras, 4) or null
    int C, H, W, Ho, Wo, n_cameras;
    double fill;
};

__device__ inline double cam_tap(const float* s, size_t i) { return (double)s[i]; }
__device__ inline double cam_tap(const unsigned char* s, size_t i) { return (double)s[i]; }
__device__ inline void cam_put(float* d, size_t i, double v) { d[i] = (float)v; }
__device__ inline void cam_put(unsigned char* d, size_t i, double v) {
    double r = floor(v + 0.5);
    r = r >= 0.0 ? r : 0.0;          // (NaN -> 0)
    r = r <= 255.0 ? r : 255.0;
    d[i] = (unsigned char)(int)r;
}

template <typename T>
__global__ __launch_bounds__(256) void undistort_images_kernel(CamImagesArgs a) {
    const int xo = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), yo = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    const size_t b = blockIdx.z;
    if (xo >= a.Wo || yo >= a.Ho) return;
    const size_t c = a.n_cameras == 1 ? 0 : b;
    const T* src = static_cast<const T*>(a.src) + b * (size_t)a.C * (size_t)a.H * (size_t)a.W;
    T* dst = static_cast<T*>(a.dst) + b * (size_t)a.C * (size_t)a.Ho * (size_t)a.Wo;
    const size_t plane = (size_t)a.H * (size_t)a.W, oplane = (size_t)a.Ho * (size_t)a.Wo, o = (size_t)yo * (size_t)a.Wo + (size_t)xo;
    cam::Model m;
    double nfx, nfy, ncx, ncy;
    bool usable = cam::load(a.kind[c], a.params + c * cam::N_PARAMS, m);
    usable = cam::load_pinhole(a.k_new ? a.k_new + c * 4 : nullptr, m, nfx, nfy, ncx, ncy) && usable;
    double xs = 0.0, ys = 0.0;
    if (usable) {
        double ud, vd;
        cam::forward(m, ((double)xo - ncx) / nfx, ((double)yo - ncy) / nfy, ud, vd);
        xs = m.fx * ud + m.cx; ys = m.fy * vd + m.cy;
        usable = cam::finite(xs) && cam::finite(ys);
    }
    if (!usable) {
        for (int ch = 0; ch < a.C; ++ch) cam_put(dst, ch * oplane + o, a.fill);
        if (a.valid) a.valid[b * oplane + o] = 0;
        return;
    }
    const double x0 = floor(xs), y0 = floor(ys);
    const double wx = xs - x0, wy = ys - y0;
    const bool near = x0 >= -1.0 && x0 <= (double)a.W && y0 >= -1.0 && y0 <= (double)a.H;      // else no tap is inside (and x0 may not fit an int)
    const int ix = near ? (int)x0 : -2, iy = near ? (int)y0 : -2;
    const bool in_x0 = ix >= 0 && ix < a.W, in_x1 = ix + 1 >= 0 && ix + 1 < a.W, in_y0 = iy >= 0 && iy < a.H, in_y1 = iy + 1 >= 0 && iy + 1 < a.H;
    const bool in_a = in_x0 && in_y0, in_b = in_x1 && in_y0, in_c = in_x0 && in_y1, in_d = in_x1 && in_y1;
    const size_t at = (size_t)(in_y0 ? iy : 0) * (size_t)a.W + (size_t)(in_x0 ? ix : 0);         // of tap a when it is inside; the others by offset
    for (int ch = 0; ch < a.C; ++ch) {
        const T* s = src + ch * plane;
        const double ta = in_a ? cam_tap(s, at) : a.fill;
        const double tb = in_b ? cam_tap(s, (size_t)iy * (size_t)a.W + (size_t)(ix + 1)) : a.fill;
        const double tc = in_c ? cam_tap(s, (size_t)(iy + 1) * (size_t)a.W + (size_t)ix) : a.fill;
        const double td = in_d ? cam_tap(s, (size_t)(iy + 1) * (size_t)a.W + (size_t)(ix + 1)) : a.fill;
        cam_put(dst, ch * oplane + o, (1.0 - wy) * ((1.0 - wx) * ta + wx * tb) + wy * ((1.0 - wx) * tc + wx * td));
    }
    if (a.valid) a.valid[b * oplane + o] = (in_a && in_b && in_c && in_d) ? 1 : 0;
}
// ---- cameras end ----

int launch_camera_points(const float* pts, const int32_t* counts, long long P, int K, const int32_t* kind, const double* params, int n_cameras,
                         const double* k_other, int direction, float* out, unsigned char* status, hipStream_t st) {
    if (P < 1 || K < 1 || P > 0x7fffffffffffffffll / K) return -1;
    const long long total = P * K, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffll) return -1;                  // the grid is one-dimensional over the points
    CamPointsArgs a = {};
    a.pts = pts; a.counts = counts; a.kind = kind; a.params = params; a.k_other = k_other; a.total = total; a.K = K; a.n_cameras = n_cameras;
    a.direction = direction; a.out = out; a.status = status;
    camera_points_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
    return 0;
}

int launch_undistort_images(const void* src, int is_f32, int B, int C, int H, int W, const int32_t* kind, const double* params, int n_cameras,
                            const double* k_new, int Ho, int Wo, double fill, void* dst, unsigned char* valid, hipStream_t st) {
    if (B < 1 || B > 65535 || Ho < 1 || (Ho + 3) / 4 > 65535 || Wo < 1 || Wo > 0x7fffffff - 63 || C < 1 || C > cam::MAX_CHANNELS || H < 1 || W < 1) return -1;
    CamImagesArgs a = {};
    a.src = src; a.dst = dst; a.valid = valid; a.kind = kind; a.params = params; a.k_new = k_new;
    a.C = C; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.n_cameras = n_cameras; a.fill = fill;
    const dim3 grid((unsigned)((Wo + 63) / 64), (unsigned)((Ho + 3) / 4), (unsigned)B);
    if (is_f32) undistort_images_kernel<float><<<grid, 256, 0, st>>>(a);
    else undistort_images_kernel<unsigned char><<<grid, 256, 0, st>>>(a);
    return 0;
}

}  // namespace xfh
