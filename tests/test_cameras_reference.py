"""tests/cameras_reference.py pinned to the published formulas and to closed forms.  No camera library is available to compare with (cv2,
poselib and pycolmap are not installed), so the models are held to: their own round trips, the real root of the radial polynomial from
numpy.roots, central differences for the Jacobian, the fold radius of a barrel model in closed form, the equidistant fisheye r_d = atan(r),
every status by a constructed case, bilinear taps worked out by hand."""
import numpy as np
import pytest

import cameras_reference as CR
import cameras_support as CS

F = 500.0


def _grid(step=8):
    """Normalised coordinates of a 640 x 480 pixel grid at f = 500 about the image centre."""
    x, y = np.meshgrid(np.arange(0, CS.WIDTH + 1, step, dtype=np.float64), np.arange(0, CS.HEIGHT + 1, step, dtype=np.float64))
    return ((x - CS.WIDTH / 2) / F).reshape(-1), ((y - CS.HEIGHT / 2) / F).reshape(-1)


@pytest.mark.parametrize("d", CS.BROWN_SETS)
def test_brown_round_trips_below_1e_12_px(d):
    d = np.array(d)
    ud, vd = _grid()                                                    # the raw image: every pixel has an ideal one
    u, v, st, iters = CR.inverse(CR.BROWN, d, ud, vd, return_iters=True)
    assert (st == CR.OK).all() and iters.max() <= 8
    bu, bv = CR.forward(CR.BROWN, d, u, v)
    assert F * np.hypot(bu - ud, bv - vd).max() < 1e-12
    u0, v0 = _grid()                                                    # the ideal image: forward, then back
    fu, fv = CR.forward(CR.BROWN, d, u0, v0)
    u, v, st = CR.inverse(CR.BROWN, d, fu, fv)
    assert (st == CR.OK).all() and F * np.hypot(u - u0, v - v0).max() < 1e-12
    assert min(np.min(j[0] * j[3] - j[1] * j[2]) for j in [CR.brown_jacobian(d, u0, v0)]) > 0.4


def test_fisheye_round_trips_below_1e_12_px():
    d = np.array(CS.FISHEYE_SET)
    f = 320.0
    x, y = np.meshgrid(np.arange(0, CS.WIDTH + 1, 8.0), np.arange(0, CS.HEIGHT + 1, 8.0))
    ud, vd = ((x - CS.WIDTH / 2) / f).reshape(-1), ((y - CS.HEIGHT / 2) / f).reshape(-1)
    u, v, st, iters = CR.inverse(CR.FISHEYE, d, ud, vd, return_iters=True)
    assert (st == CR.OK).all() and iters.max() <= 8
    bu, bv = CR.forward(CR.FISHEYE, d, u, v)
    assert f * np.hypot(bu - ud, bv - vd).max() < 1e-12


@pytest.mark.parametrize("d", [s for s in CS.BROWN_SETS if s[2] == 0.0 and s[3] == 0.0])
def test_radial_inverse_is_the_real_root_of_the_radial_polynomial(d):
    k1, k2 = d[:2]
    for rd in (0.05, 0.3, 0.55, 0.8):
        roots = np.roots([k2, 0.0, k1, 0.0, 1.0, -rd] if k2 else [k1, 0.0, 1.0, -rd])
        real = roots[(np.abs(roots.imag) < 1e-12) & (roots.real > 0)].real
        r = real.min()                                                  # the branch through the origin
        for a in (0.0, 0.7, 2.5):
            u, v, st = CR.inverse(CR.BROWN, np.array(d), np.array([rd * np.cos(a)]), np.array([rd * np.sin(a)]))
            assert st[0] == CR.OK and abs(np.hypot(u[0], v[0]) - r) < 1e-12
            assert abs(np.arctan2(v[0], u[0]) - np.arctan2(np.sin(a), np.cos(a))) < 1e-12


@pytest.mark.parametrize("d", CS.BROWN_SETS)
def test_brown_jacobian_against_central_differences(d):
    d = np.array(d)
    rng = np.random.default_rng(3)
    u, v = rng.uniform(-0.7, 0.7, 50), rng.uniform(-0.5, 0.5, 50)
    h = 1e-6
    j00, j01, j10, j11 = CR.brown_jacobian(d, u, v)
    (ap, bp), (am, bm) = CR.brown_forward(d, u + h, v), CR.brown_forward(d, u - h, v)
    (cp, dp), (cm, dm) = CR.brown_forward(d, u, v + h), CR.brown_forward(d, u, v - h)
    for got, want in ((j00, (ap - am) / (2 * h)), (j10, (bp - bm) / (2 * h)), (j01, (cp - cm) / (2 * h)), (j11, (dp - dm) / (2 * h))):
        assert np.abs(got - want).max() < 1e-9


def test_the_fold_of_a_barrel_model_just_inside_and_just_outside():
    d = np.array(CS.BROWN_SETS[0])                                      # k1 = -0.12: d r_d / d r = 1 - 0.36 r^2 = 0 at r = 1 / 0.6
    r_fold = 1.0 / 0.6
    rd_fold = r_fold * (1.0 - 0.12 * r_fold ** 2)
    u, v, st = CR.inverse(CR.BROWN, d, np.array([0.99 * rd_fold, 1.01 * rd_fold, 0.0]), np.array([0.0, 0.0, -1.01 * rd_fold]))
    assert st.tolist() == [CR.OK, CR.FOLD, CR.FOLD]
    assert abs(CR.forward(CR.BROWN, d, u[:1], v[:1])[0][0] - 0.99 * rd_fold) < 1e-14 and u[0] < r_fold
    # the determinant limit, not the iteration limit, ends a row beyond the fold; a row far inside never sees a small determinant
    j = CR.brown_jacobian(d, np.array([r_fold * 0.999]), np.array([0.0]))
    assert 0 < j[0][0] * j[3][0] - j[1][0] * j[2][0] < 3e-3


def test_equidistant_fisheye_is_r_d_equals_atan_r():
    d = np.zeros(4)
    r = np.array([1e-9, 0.01, 0.5, 1.0, 3.0, 10.0])
    for a in (0.3, 2.0):
        ud, vd = CR.forward(CR.FISHEYE, d, r * np.cos(a), r * np.sin(a))
        want = np.where(r < 1e-8, r, np.arctan(r))
        assert np.abs(np.hypot(ud, vd) - want).max() < 1e-15
        u, v, st = CR.inverse(CR.FISHEYE, d, ud, vd)
        assert (st == CR.OK).all() and (np.abs(np.hypot(u, v) - r) <= 1e-13 * (1 + r * r)).all()
    # theta = r_d: a ray at 1.5 rad and beyond has no useful pinhole image; just below it has
    u, v, st = CR.inverse(CR.FISHEYE, d, np.array([1.4999, 1.5001, 0.0, 4.0]), np.array([0.0, 0.0, 1.6, 0.0]))
    assert st.tolist() == [CR.OK, CR.OUTSIDE, CR.OUTSIDE, CR.OUTSIDE] and abs(u[0] - np.tan(1.4999)) < 1e-9
    # a polynomial that turns over: the derivative's floor is a fold
    u, v, st = CR.inverse(CR.FISHEYE, np.array([-0.5, 0.0, 0.0, 0.0]), np.array([0.9]), np.array([0.0]))
    assert st[0] == CR.FOLD


def test_every_status_and_their_precedence():
    kind, params = CS.packed([CS.brown_camera(0), CS.fisheye_camera(), CS.pinhole_camera()])
    fold_x = params[0, 2] + params[0, 0] * 1.2                          # beyond the fold radius of k1 = -0.12 (r_d = 1.11)
    out_x = params[1, 2] + params[1, 0] * 1.6
    pts = np.zeros((3, 4, 2), np.float32)
    pts[0] = [[100, 100], [fold_x, params[0, 3]], [np.nan, 5], [7, 7]]
    pts[1] = [[300, 200], [out_x, params[1, 3]], [5, np.inf], [9, 9]]
    pts[2] = [[10, 20], [30, 40], [np.nan, np.nan], [1, 1]]
    counts = np.array([3, 3, 3], np.int32)
    out, st, _ = CR.camera_points(pts, counts, kind, params, None, 0)
    assert st.tolist() == [[CR.OK, CR.FOLD, CR.POINT, CR.ROW], [CR.OK, CR.OUTSIDE, CR.POINT, CR.ROW], [CR.OK, CR.OK, CR.POINT, CR.ROW]]
    assert np.array_equal(np.isnan(out[..., 0]), st != 0) and np.array_equal(np.isnan(out[..., 1]), st != 0)
    assert np.array_equal(out[2, :2], pts[2, :2])                       # a pinhole camera onto itself
    # a camera that is not usable comes before the point, the count before the camera
    for bad in ((0, 0, 0.0), (1, 1, -3.0), (2, 9, np.nan), (0, 11, np.inf)):
        p2 = params.copy()
        p2[bad[0], bad[1]] = bad[2]
        st2 = CR.camera_points(pts, counts, kind, p2, None, 0)[1]
        assert st2[bad[0]].tolist() == [CR.CAMERA] * 3 + [CR.ROW]
        assert np.array_equal(np.delete(st2, bad[0], 0), np.delete(st, bad[0], 0))
    k2 = kind.copy()
    k2[1] = 3
    assert CR.camera_points(pts, counts, k2, params, None, 1)[1][1].tolist() == [CR.CAMERA] * 3 + [CR.ROW]
    other = np.tile(np.array([400.0, 400.0, 320.0, 240.0]), (3, 1))
    other[2, 0] = np.nan
    assert CR.camera_points(pts, counts, kind, params, other, 0)[1][2].tolist() == [CR.CAMERA] * 3 + [CR.ROW]
    # counts are read clamped; a row that Newton cannot finish is NOT_CONVERGED
    assert (CR.camera_points(pts, np.array([-4, 9, 0], np.int32), kind, params, None, 1)[1] == [[1] * 4, [0, 0, 2, 0], [1] * 4]).all()
    u, v, st3 = CR.inverse(CR.BROWN, np.zeros(4), np.array([0.3]), np.array([0.1]))
    assert st3[0] == CR.OK and u[0] == 0.3                              # no distortion: the first step is zero
    for kind_, d, rd in CS.NOT_CONVERGING:                              # models far from any lens, on which Newton wanders for 32 iterations
        assert CR.inverse(kind_, np.array(d), np.array([rd]), np.array([0.0]))[2][0] == CR.NOT_CONVERGED
    # distort and undistort are each other's inverse through K_other
    good = np.array([[[100, 100], [320, 240], [600, 50], [20, 460]]] * 3, np.float32)
    ideal = np.tile([400.0, 405.0, 320.0, 240.0], (3, 1))
    und, s0, exact = CR.camera_points(good, None, kind, params, ideal, 0)
    assert (s0 == 0).all()
    back = CR.camera_points(exact.astype(np.float32), None, kind, params, ideal, 1)[0]
    assert np.abs(back - good).max() < 2e-4                             # the fp32 rounding of the ideal pixels, magnified by the model


def test_bilinear_taps_on_a_2x2_image_by_hand():
    src = np.array([[[[10.0, 20.0], [30.0, 50.0]]]], np.float32)        # a b / c d
    kind, params = CS.packed([{"model": "PINHOLE", "width": 2, "height": 2, "params": [1.0, 1.0, 0.0, 0.0]}])
    # K_new shifts the output grid: output pixel (0, 0) reads the source at (0.25, 0.5)
    dst, valid, exact = CR.undistort_images(src, kind, params, np.array([[1.0, 1.0, -0.25, -0.5]]), 2, 3, -7.0)
    assert exact[0, 0, 0, 0] == 0.5 * (0.75 * 10 + 0.25 * 20) + 0.5 * (0.75 * 30 + 0.25 * 50) and valid[0, 0, 0] == 1
    # (1.25, 0.5): taps b, d inside, the two beyond the right border are `fill`
    assert exact[0, 0, 0, 1] == 0.5 * (0.75 * 20 + 0.25 * -7) + 0.5 * (0.75 * 50 + 0.25 * -7) and valid[0, 0, 1] == 0
    # (2.25, 0.5) and the row below (y = 1.5: the lower taps outside)
    assert exact[0, 0, 0, 2] == -7.0 and valid[0, 0, 2] == 0
    assert exact[0, 0, 1, 0] == 0.5 * (0.75 * 30 + 0.25 * 50) + 0.5 * -7.0 and valid[0, 1, 0] == 0
    assert dst.dtype == np.float32 and np.array_equal(dst, exact.astype(np.float32))
    # integer coordinates are pixel centres: the identity reproduces the image, and its last row and column are not `valid` (their taps
    # x0 + 1 / y0 + 1 lie outside, with weight zero)
    dst, valid, _ = CR.undistort_images(src, kind, params, None, 2, 2, 99.0)
    assert np.array_equal(dst, src) and valid[0].tolist() == [[1, 0], [0, 0]]
    # left of and above the image: x0 = -1 takes `fill` for tap a
    dst, valid, exact = CR.undistort_images(src, kind, params, np.array([[1.0, 1.0, 0.5, 0.0]]), 1, 1, 4.0)
    assert exact[0, 0, 0, 0] == 0.5 * 4.0 + 0.5 * 10.0 and valid[0, 0, 0] == 0
    # far outside, a camera that is not usable and a source coordinate that is not finite: `fill`, not valid
    dst, valid, _ = CR.undistort_images(src, kind, params, np.array([[1.0, 1.0, -1e6, 3e9]]), 2, 2, 4.5)
    assert (dst == 4.5).all() and not valid.any()
    bad = params.copy()
    bad[0, 0] = -1.0
    dst, valid, _ = CR.undistort_images(src, kind, bad, None, 2, 2, 4.5)
    assert (dst == 4.5).all() and not valid.any()
    big = params.copy()
    big[0, 0] = 1e308
    dst, valid, _ = CR.undistort_images(src, kind, big, np.array([[1e-300, 1.0, 0.0, 0.0]]), 1, 2, 4.5)
    assert dst[0, 0, 0].tolist() == [10.0, 4.5] and valid[0, 0].tolist() == [1, 0]


def test_uint8_rounds_half_up_and_clamps():
    assert CR.to_u8(np.array([0.49999, 0.5, 1.5, 2.5, 254.5, 255.4, 255.5, 300.0, -0.5, -0.51, -40.0, np.nan, np.inf, -np.inf])).tolist() == \
        [0, 1, 2, 3, 255, 255, 255, 255, 0, 0, 0, 0, 255, 0]
    src = np.array([[[[1, 2], [4, 7]]]], np.uint8)
    kind, params = CS.packed([{"model": "SIMPLE_PINHOLE", "width": 2, "height": 2, "params": [1.0, 0.0, 0.0]}])
    # (0.5, 0): (1 + 2) / 2 = 1.5 -> 2; (0.5, 0.5): 14 / 4 = 3.5 -> 4; (0, 0.5): 2.5 -> 3
    for k_new, want in (([1.0, 1.0, -0.5, 0.0], 2), ([1.0, 1.0, -0.5, -0.5], 4), ([1.0, 1.0, 0.0, -0.5], 3)):
        dst, valid, exact = CR.undistort_images(src, kind, params, np.array([k_new]), 1, 1, 0.0)
        assert dst.dtype == np.uint8 and dst[0, 0, 0, 0] == want and valid[0, 0, 0] == 1
    dst, _, _ = CR.undistort_images(src, kind, params, np.array([[1.0, 1.0, 5.0, 5.0]]), 1, 1, 300.0)
    assert dst[0, 0, 0, 0] == 255                                       # `fill` goes through the same conversion


def test_pack_follows_colmap_and_poselib():
    assert CR.pack({"model": "SIMPLE_PINHOLE", "params": [5.0, 1.0, 2.0]})[1][:5].tolist() == [5.0, 5.0, 1.0, 2.0, 0.0]
    assert CR.pack({"model": "SIMPLE_RADIAL", "params": [5.0, 1.0, 2.0, 0.1]})[1][:6].tolist() == [5.0, 5.0, 1.0, 2.0, 0.1, 0.0]
    assert CR.pack({"model": "RADIAL", "params": [5.0, 1.0, 2.0, 0.1, 0.2]})[1][:7].tolist() == [5.0, 5.0, 1.0, 2.0, 0.1, 0.2, 0.0]
    k, p = CR.pack({"model": "OPENCV", "params": [5.0, 6.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4]})
    assert k == CR.BROWN and p.tolist() == [5.0, 6.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4, 0, 0, 0, 0]
    k, p = CR.pack({"model": "OPENCV_FISHEYE", "params": [5.0, 6.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4]})
    assert k == CR.FISHEYE and p[:8].tolist() == [5.0, 6.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4]
    # the three polynomial models share one formula
    u, v = np.array([0.3, -0.2]), np.array([0.1, 0.4])
    a = CR.forward(*[(k, p[4:8]) for k, p in [CR.pack({"model": "SIMPLE_RADIAL", "params": [1.0, 0, 0, -0.2]})]][0], u, v)
    b = CR.forward(*[(k, p[4:8]) for k, p in [CR.pack({"model": "OPENCV", "params": [1.0, 1.0, 0, 0, -0.2, 0, 0, 0]})]][0], u, v)
    r2 = u * u + v * v
    assert np.array_equal(a[0], b[0]) and np.abs(a[0] - u * (1 - 0.2 * r2)).max() < 1e-16
