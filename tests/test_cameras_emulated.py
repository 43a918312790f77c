"""The cameras slice of csrc/k_cameras.hip compiled for the host with tests/emu (tests/emu/cameras_emu.cpp: one thread per work-item, fp
contraction off) against the numpy restatement tests/cameras_reference.py: pinhole and Brown outputs bit for bit, fisheye points within one
fp32 spacing with equal status (tests/cameras_support.py has the rules).  The same program also runs under AddressSanitizer and UBSan as a
stand-alone program."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cameras_reference as CR
import cameras_support as CS
import twoview_support as TS

BEGIN, END = "// ---- cameras begin", "// ---- cameras end"


def _slice():
    text, src = TS._between("k_cameras.hip", BEGIN, END)
    assert text.index("#pragma clang fp contract(off)") < text.index(BEGIN)
    for word in ("asm", "atomic", "__shared__", "__syncthreads", "rsqrt", "fma(", "__frcp", "__fdividef", "sin(", "cos(", "exp(", "log(", "pow(",
                 "workspace", "__builtin_amdgcn"):
        assert word not in src, word
    assert src.count("atan(") == 1 and src.count(" tan(") == 1            # the fisheye branch alone
    return src.replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("cameras_slice.hpp", "cameras_emu", _slice())


def _reference(c, direction):
    return CR.camera_points(c["pts"], c["counts"], c["kind"], c["params"], c["k_other"], direction)


def _distort_case(c):
    """The same batch with points that lie in the ideal image: the undistorted ones of the case, where they exist."""
    und = _reference(c, 0)[0]
    pts = np.where(np.isnan(und), c["pts"], und).astype(np.float32)
    pts[np.isnan(c["pts"]) | np.isinf(c["pts"])] = c["pts"][np.isnan(c["pts"]) | np.isinf(c["pts"])]
    return dict(c, pts=pts)


@pytest.mark.parametrize("family", ["pinhole", "brown", "fisheye"])
@pytest.mark.parametrize("K", CS.KS)
@pytest.mark.parametrize("P", [1, 3])
def test_points_slice_against_the_restatement(emu_bin, P, K, family):
    seen = set()
    for shared in ((True, False) if P > 1 else (True,)):
        c = CS.points_case(100 * P + K + (7 if shared else 0), P, K, family, shared, other=not shared)
        want = _reference(c, 0)
        CS.check_points(CS.run_points(emu_bin, c, 0), want, family == "fisheye")
        seen |= set(want[1].reshape(-1).tolist())
        d = _distort_case(c)
        CS.check_points(CS.run_points(emu_bin, d, 1), _reference(d, 1), family == "fisheye")
    if P == 3 and K >= 63:
        assert {CR.OK, CR.ROW, CR.POINT} <= seen
        bad = CS.points_case(K, P, K, family, False, bad_camera=True)
        want = _reference(bad, 0)
        assert (want[1][-1] == CR.CAMERA).all() and (want[1][1] == CR.OK).sum() > 0
        CS.check_points(CS.run_points(emu_bin, bad, 0), want, family == "fisheye")
        bad = dict(CS.points_case(K + 1, P, K, family, True, other=True))
        bad["k_other"][0, 1] = -1.0                                      # the ideal side is not usable: every read row
        want = _reference(bad, 1)
        assert set(want[1].reshape(-1).tolist()) == {CR.ROW, CR.CAMERA}
        CS.check_points(CS.run_points(emu_bin, bad, 1), want, family == "fisheye")


def test_points_beyond_the_fold_and_the_field_of_view(emu_bin):
    """Rows that end with FOLD (a barrel model beyond its fold radius) and OUTSIDE (a fisheye ray at 1.6 rad), beside rows that are fine."""
    cam = CS.brown_camera(0)                                            # k1 = -0.12: folds at r = 1 / sqrt(0.36)
    kind, params = CS.packed([cam])
    f, cx, cy = cam["params"][0], cam["params"][2], cam["params"][3]
    r_fold = 1.0 / np.sqrt(0.36)
    rd_fold = r_fold * (1 - 0.12 * r_fold ** 2)
    pts = np.array([[[cx + f * rd_fold * 1.01, cy], [cx + f * rd_fold * 0.99, cy], [cx + 10.0, cy + 20.0], [cx + f * 5.0, cy]]], np.float32)
    c = dict(pts=pts, counts=None, kind=kind, params=params, k_other=None)
    want = _reference(c, 0)
    assert want[1][0].tolist() == [CR.FOLD, CR.OK, CR.OK, CR.FOLD]
    CS.check_points(CS.run_points(emu_bin, c, 0), want, False)
    cam = CS.fisheye_camera()
    kind, params = CS.packed([cam])
    f, cx, cy = cam["params"][0], cam["params"][2], cam["params"][3]
    thd = 1.6 * CR.fisheye_poly(np.array(CS.FISHEYE_SET), 1.6 ** 2)
    pts = np.array([[[cx + f * thd, cy], [cx + 100.0, cy - 50.0], [cx, cy], [cx - f * thd * 0.7, cy]]], np.float32)
    c = dict(pts=pts, counts=None, kind=kind, params=params, k_other=None)
    want = _reference(c, 0)
    assert want[1][0].tolist() == [CR.OUTSIDE, CR.OK, CR.OK, CR.OK]
    CS.check_points(CS.run_points(emu_bin, c, 0), want, True)
    c = CS.not_converging_case()
    want = _reference(c, 0)
    assert want[1].tolist() == [[CR.NOT_CONVERGED, CR.OK]] * 2
    CS.check_points(CS.run_points(emu_bin, c, 0), want, False)          # (its fisheye rows: the centre and a row that ends in the loop)


def _check_images(emu_bin, c, k_new, Ho, Wo, fill, with_valid, fisheye):
    dst, valid = CS.run_images(emu_bin, c, k_new, Ho, Wo, fill, with_valid)
    w_dst, w_valid, exact = CR.undistort_images(c["src"], c["kind"], c["params"], k_new, Ho, Wo, fill)
    if with_valid:
        assert CS.same_bits(valid, w_valid)
        assert 0 < w_valid.sum() or c["src"].shape[2] == 1
    else:
        assert valid is None
    if not fisheye:
        assert CS.same_bits(dst, w_dst)
    elif dst.dtype == np.float32:
        CS.check_fisheye_f32(dst, exact, c["src"], fill)
    else:
        CS.check_fisheye_u8(dst, w_dst, exact)
    return w_valid


@pytest.mark.parametrize("family", ["pinhole", "brown", "fisheye"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("C", [1, 3])
def test_images_slice_against_the_restatement(emu_bin, C, dtype, family):
    c = CS.image_case(10 * C + (1 if dtype == np.uint8 else 2), 2, C, 37, 53, dtype, family)
    _check_images(emu_bin, c, None, 29, 41, 0.0, False, family == "fisheye")
    v = _check_images(emu_bin, c, CS.new_k(c, 0.5), 29, 41, 7.25 if dtype == np.uint8 else 0.25, True, family == "fisheye")
    assert v.min() == 0 and v.max() == 1                                # a wider view than the source: pixels inside and outside
    one = CS.image_case(3, 2, C, 1, 1, dtype, family, shared=True)
    _check_images(emu_bin, one, None, 1, 1, 3.0 if dtype == np.uint8 else 0.5, True, family == "fisheye")
    if C == 3 and family == "brown":                                    # an unusable camera in the batch: `fill`, valid 0
        bad = dict(c, params=c["params"].copy())
        bad["params"][1, 0] = 0.0
        v = _check_images(emu_bin, bad, None, 29, 41, 200.5, True, False)
        assert not v[1].any() and v[0].any()


def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers():
    """AddressSanitizer and UBSan on the host build of the slice, as a program of its own (nothing is loaded into Python)."""
    if not os.path.exists(TS.CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, "cameras_slice.hpp"), "w").write(_slice())
    exe = os.path.join(td, "cameras_emu_san")
    subprocess.run([TS.CLANG, "-O1", "-g", "-w", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", td, "-I", TS.EMU, os.path.join(TS.EMU, "cameras_emu.cpp"), "-o", exe], check=True)
    for family in ("brown", "fisheye"):
        c = CS.points_case(5, 3, 65, family, False, other=True)
        CS.check_points(CS.run_points(exe, c, 0), _reference(c, 0), family == "fisheye")
        CS.check_points(CS.run_points(exe, c, 1), _reference(c, 1), family == "fisheye")
        for dtype in (np.uint8, np.float32):
            img = CS.image_case(6, 2, 3, 37, 53, dtype, family)
            _check_images(exe, img, CS.new_k(img, 0.5), 29, 41, 0.5 if dtype == np.float32 else 300.0, True, family == "fisheye")
