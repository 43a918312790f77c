"""numpy float64 restatement of csrc/k_cameras.hip: the camera models, camera_points_kernel and undistort_images_kernel with
their status precedence, every expression in the kernel's order (numpy evaluates a * b * c left to right, as C does; nothing is contracted).
Vectorised over the points: a row that has ended (fold, converged) keeps its values while the others iterate, so each row sees exactly the
sequence of operations its thread runs.

No camera library is available to test against (cv2, poselib and pycolmap are not installed), so tests/test_cameras_reference.py pins this
file to the published formulas and to closed forms."""
import numpy as np

PINHOLE, BROWN, FISHEYE = 0, 1, 2
OK, ROW, POINT, FOLD, NOT_CONVERGED, OUTSIDE, CAMERA = 0, 1, 2, 3, 4, 5, 6
MAX_ITERS, MIN_DET, STEP_TOL, SMALL_R, MAX_THETA = 32, 1e-3, 1e-30, 1e-8, 1.5
MODELS = {"SIMPLE_PINHOLE": (PINHOLE, (0, 2, 3)), "PINHOLE": (PINHOLE, (0, 1, 2, 3)), "SIMPLE_RADIAL": (BROWN, (0, 2, 3, 4)),
          "RADIAL": (BROWN, (0, 2, 3, 4, 5)), "OPENCV": (BROWN, tuple(range(8))), "OPENCV_FISHEYE": (FISHEYE, tuple(range(8)))}


def pack(cam):
    """(kind, the 12 doubles) of a camera dict."""
    kind, slots = MODELS[cam["model"]]
    p = np.zeros(12)
    assert len(cam["params"]) == len(slots)
    p[list(slots)] = cam["params"]
    if slots[1] != 1:
        p[1] = p[0]
    return kind, p


def usable(kind, params):
    return bool(kind in (PINHOLE, BROWN, FISHEYE) and np.isfinite(params).all() and params[0] > 0 and params[1] > 0)


def pinhole_side(k4, params):
    """(fx, fy, cx, cy, usable) of the ideal side: k4, or the camera's own."""
    if k4 is None:
        return params[0], params[1], params[2], params[3], True
    k4 = np.asarray(k4, np.float64)
    return k4[0], k4[1], k4[2], k4[3], bool(np.isfinite(k4).all() and k4[0] > 0 and k4[1] > 0)


def brown_forward(d, u, v):
    k1, k2, p1, p2 = d[:4]
    r2 = u * u + v * v
    rad = r2 * (k1 + k2 * r2)
    ud = u + (u * rad + (2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u)))
    vd = v + (v * rad + (p1 * (r2 + 2.0 * v * v) + 2.0 * p2 * u * v))
    return ud, vd


def brown_jacobian(d, u, v):
    """j00, j01, j10, j11 of brown_forward at (u, v)."""
    k1, k2, p1, p2 = d[:4]
    r2 = u * u + v * v
    rad = r2 * (k1 + k2 * r2)
    g = k1 + 2.0 * k2 * r2
    j00 = (1.0 + rad) + (2.0 * u * u * g + (2.0 * p1 * v + 6.0 * p2 * u))
    j11 = (1.0 + rad) + (2.0 * v * v * g + (6.0 * p1 * v + 2.0 * p2 * u))
    j01 = 2.0 * u * v * g + (2.0 * p1 * u + 2.0 * p2 * v)
    return j00, j01, j01, j11


def fisheye_poly(d, t2):
    return 1.0 + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3])))


def forward(kind, d, u, v):
    """Normalised ideal -> normalised distorted coordinates (arrays)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        if kind == BROWN:
            return brown_forward(d, u, v)
        if kind == FISHEYE:
            r = np.sqrt(u * u + v * v)
            th = np.arctan(r)
            thd = th * fisheye_poly(d, th * th)
            s = np.where(r < SMALL_R, 1.0, thd / np.where(r < SMALL_R, 1.0, r))
            return u * s, v * s
        return u.copy(), v.copy()


def inverse(kind, d, ud, vd, return_iters=False):
    """Normalised distorted -> normalised ideal coordinates: (u, v, status) arrays; u, v are meaningful where status is OK."""
    ud, vd = np.atleast_1d(np.asarray(ud, np.float64)), np.atleast_1d(np.asarray(vd, np.float64))
    st = np.full(ud.shape, NOT_CONVERGED, np.int32)
    iters = np.zeros(ud.shape, np.int32)
    with np.errstate(all="ignore"):
        if kind == BROWN:
            u, v = ud.copy(), vd.copy()
            live = np.ones(ud.shape, bool)
            for _ in range(MAX_ITERS):
                fu, fv = brown_forward(d, u, v)
                eu, ev = fu - ud, fv - vd
                j00, j01, j10, j11 = brown_jacobian(d, u, v)
                det = j00 * j11 - j01 * j10
                fold = live & ~(det > MIN_DET)
                st[fold] = FOLD
                live &= ~fold
                du = (j11 * eu - j01 * ev) / det
                dv = (j00 * ev - j10 * eu) / det
                u = np.where(live, u - du, u)
                v = np.where(live, v - dv, v)
                iters += live
                done = live & (du * du + dv * dv <= STEP_TOL * (1.0 + (u * u + v * v)))
                st[done] = OK
                live &= ~done
                if not live.any():
                    break
        elif kind == FISHEYE:
            rd = np.sqrt(ud * ud + vd * vd)
            th = rd.copy()
            live = np.ones(ud.shape, bool)
            for _ in range(MAX_ITERS):
                t2 = th * th
                e = th * fisheye_poly(d, t2) - rd
                dd = 1.0 + t2 * (3.0 * d[0] + t2 * (5.0 * d[1] + t2 * (7.0 * d[2] + t2 * (9.0 * d[3]))))
                fold = live & ~(dd > MIN_DET)
                st[fold] = FOLD
                live &= ~fold
                dt = e / dd
                th = np.where(live, th - dt, th)
                iters += live
                done = live & (dt * dt <= STEP_TOL * (1.0 + th * th))
                st[done] = OK
                live &= ~done
                if not live.any():
                    break
            st[(st == OK) & ~(th < MAX_THETA)] = OUTSIDE
            s = np.where(rd < SMALL_R, 1.0, np.tan(th) / np.where(rd < SMALL_R, 1.0, rd))
            u, v = ud * s, vd * s
        else:
            u, v = ud.copy(), vd.copy()
            st[:] = OK
    return (u, v, st, iters) if return_iters else (u, v, st)


def camera_points(pts, counts, kind, params, k_other, direction):
    """xfh_camera_points: pts (P,K,2) float32, counts (P,) or None, kind (C,), params (C,12), k_other (C,4) or None, C in {1, P}.
    -> out (P,K,2) float32, status (P,K) uint8, and the unrounded fp64 result (P,K,2)."""
    pts = np.asarray(pts, np.float32)
    P, K = pts.shape[:2]
    out = np.full((P, K, 2), np.nan, np.float32)
    exact = np.full((P, K, 2), np.nan, np.float64)
    status = np.zeros((P, K), np.uint8)
    for p in range(P):
        c = 0 if len(kind) == 1 else p
        n = K if counts is None else min(max(int(counts[p]), 0), K)
        status[p, n:] = ROW
        if n == 0:
            continue
        par = np.asarray(params[c], np.float64)
        ofx, ofy, ocx, ocy, ok_other = pinhole_side(None if k_other is None else k_other[c], par)
        if not (usable(int(kind[c]), par) and ok_other):
            status[p, :n] = CAMERA
            continue
        fx, fy, cx, cy, d = par[0], par[1], par[2], par[3], par[4:8]
        x, y = pts[p, :n, 0].astype(np.float64), pts[p, :n, 1].astype(np.float64)
        fin = np.isfinite(x) & np.isfinite(y)
        xs, ys = np.where(fin, x, 0.0), np.where(fin, y, 0.0)
        with np.errstate(all="ignore"):
            if direction == 0:
                u, v, st = inverse(int(kind[c]), d, (xs - cx) / fx, (ys - cy) / fy)
                ox, oy = ofx * u + ocx, ofy * v + ocy
            else:
                ud, vd = forward(int(kind[c]), d, (xs - ocx) / ofx, (ys - ocy) / ofy)
                ox, oy = fx * ud + cx, fy * vd + cy
                st = np.zeros(n, np.int32)
            st = np.where(fin, st, POINT)
            good = st == OK
            status[p, :n] = st
            exact[p, :n, 0], exact[p, :n, 1] = np.where(good, ox, np.nan), np.where(good, oy, np.nan)
            out[p, :n, 0], out[p, :n, 1] = np.where(good, ox, np.nan).astype(np.float32), np.where(good, oy, np.nan).astype(np.float32)
    return out, status, exact


def to_u8(v):
    """floor(v + 0.5), below 0 or NaN -> 0, above 255 -> 255."""
    with np.errstate(all="ignore"):
        r = np.floor(np.asarray(v, np.float64) + 0.5)
        r = np.where(r >= 0.0, r, 0.0)
        r = np.where(r <= 255.0, r, 255.0)
    return r.astype(np.uint8)


def source_coordinates(kind, par, k_new, Ho, Wo):
    """(xs, ys) (Ho, Wo) float64 of every output pixel, and whether the cameras are usable."""
    nfx, nfy, ncx, ncy, ok_new = pinhole_side(k_new, par)
    if not (usable(kind, par) and ok_new):
        return None, None, False
    xo, yo = np.meshgrid(np.arange(Wo, dtype=np.float64), np.arange(Ho, dtype=np.float64))
    with np.errstate(all="ignore"):
        ud, vd = forward(kind, par[4:8], (xo - ncx) / nfx, (yo - ncy) / nfy)
        return par[0] * ud + par[2], par[1] * vd + par[3], True


def undistort_images(src, kind, params, k_new, Ho, Wo, fill):
    """xfh_undistort_images: src (B,C,H,W) uint8 or float32 -> dst (B,C,Ho,Wo) of that type, valid (B,Ho,Wo) uint8, the unrounded values."""
    src = np.asarray(src)
    B, C, H, W = src.shape
    put = to_u8 if src.dtype == np.uint8 else (lambda v: np.asarray(v, np.float64).astype(np.float32))
    dst = np.zeros((B, C, Ho, Wo), src.dtype)
    exact = np.zeros((B, C, Ho, Wo), np.float64)
    valid = np.zeros((B, Ho, Wo), np.uint8)
    fill = float(fill)
    for b in range(B):
        c = 0 if len(kind) == 1 else b
        xs, ys, ok = source_coordinates(int(kind[c]), np.asarray(params[c], np.float64), None if k_new is None else k_new[c], Ho, Wo)
        if not ok:
            dst[b], exact[b] = put(fill), fill
            continue
        with np.errstate(all="ignore"):
            fin = np.isfinite(xs) & np.isfinite(ys)
            xs, ys = np.where(fin, xs, -10.0), np.where(fin, ys, -10.0)
            x0, y0 = np.floor(xs), np.floor(ys)
            wx, wy = xs - x0, ys - y0
            near = (x0 >= -1.0) & (x0 <= W) & (y0 >= -1.0) & (y0 <= H)
            ix, iy = np.where(near, x0, -2.0).astype(np.int64), np.where(near, y0, -2.0).astype(np.int64)

            def tap(img, jy, jx):
                inside = (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H)
                return np.where(inside, img[np.clip(jy, 0, H - 1), np.clip(jx, 0, W - 1)].astype(np.float64), fill), inside

            for ch in range(C):
                (ta, ia), (tb, ib), (tc, ic), (td, idd) = (tap(src[b, ch], iy, ix), tap(src[b, ch], iy, ix + 1), tap(src[b, ch], iy + 1, ix),
                                                          tap(src[b, ch], iy + 1, ix + 1))
                val = (1.0 - wy) * ((1.0 - wx) * ta + wx * tb) + wy * ((1.0 - wx) * tc + wx * td)
                val = np.where(fin, val, fill)
                exact[b, ch] = val
                dst[b, ch] = put(val)
            valid[b] = (fin & ia & ib & ic & idd).astype(np.uint8)
    return dst, valid, exact
