"""Host-side checks of the camera entries of the C ABI (include/xfeat_hip_cameras.h) and of accelerated_features_amd.cameras: the header as
strict C99 and C++11 on its own, the exported symbols, the argument checks (which return before any launch: the pointers below are never
dereferenced), ``pack_cameras`` on every model and on bad dicts, the shapes that need no library call and the loud failure without a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cameras_reference as CR
import cameras_support as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xfeat_hip_cameras.h")
ARG, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, cameras
    build.build(verbose=False)
    return cameras.load()


def test_the_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib, build, cameras
    import accelerated_features_amd as pkg
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(xfh_[a-z_0-9]+)\s*\(", hdr[hdr.index("#ifndef"):]))
    assert declared == set(cameras.SIGNATURES) == {"xfh_camera_points", "xfh_undistort_images"}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name) and re.search(r"\bint %s\(" % name, hdr) and name not in _lib.SIGNATURES, name
    assert len(cameras.SIGNATURES["xfh_camera_points"][1]) == 12 and len(cameras.SIGNATURES["xfh_undistort_images"][1]) == 16
    assert cameras.load() is _lib.load() and lib.xfh_camera_points.argtypes[2] is C.c_longlong
    main = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    assert lib.xfh_version() == 303 and "#define XFH_VERSION 303 " in main and "camera_points" not in main       # added entry points only
    assert HEADER in build._deps()
    for name in ("pack_cameras", "camera_matrix", "undistort_keypoints", "distort_keypoints", "undistort_images"):
        assert getattr(pkg, name) is getattr(cameras, name)
    p = inspect.signature(cameras.undistort_keypoints).parameters
    assert list(p) == ["kpts", "cameras", "counts", "K_new"] and p["counts"].default is None and p["K_new"].default is None
    assert list(inspect.signature(cameras.distort_keypoints).parameters) == ["kpts", "cameras", "counts", "K_src"]
    p = inspect.signature(cameras.undistort_images).parameters
    assert list(p) == ["images", "cameras", "K_new", "out_size", "fill", "return_valid"] and p["fill"].default == 0.0
    p = inspect.signature(cameras.estimate_relative_pose).parameters
    assert list(p) == ["kpts0", "kpts1", "camera0", "camera1", "ransac_opt", "bundle_opt", "seed"] and p["seed"].kind is p["seed"].KEYWORD_ONLY
    assert list(inspect.signature(cameras.estimate_absolute_pose).parameters) == ["points2D", "points3D", "camera", "ransac_opt", "bundle_opt", "seed"]
    assert len(cameras.STATUS) == 7 and (cameras.PINHOLE, cameras.BROWN, cameras.FISHEYE) == (CR.PINHOLE, CR.BROWN, CR.FISHEYE)
    for name, value in (("PINHOLE", 0), ("BROWN", 1), ("FISHEYE", 2), ("POINT_ROW", 1), ("POINT_NOT_FINITE", 2), ("POINT_FOLD", 3), ("POINT_NOT_CONVERGED", 4),
                        ("POINT_OUTSIDE", 5), ("POINT_CAMERA", 6), ("PARAMS", 12)):
        assert re.search(r"#define XFH_CAMERA_%s %d\n" % (name, value), hdr), name
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "k_cameras.hip")).read()
    assert "camera_points_kernel<<<(unsigned)blocks, 256, 0, st>>>" in src and "undistort_images_kernel<float><<<grid, 256, 0, st>>>" in src
    assert "Triton" not in src and "#pragma clang fp contract(off)" in src


USE = ('#include "xfeat_hip_cameras.h"\nint main(void) {\n'
       'int (*f)(const float*, const int32_t*, long long, int, const int32_t*, const double*, int, const double*, int, float*, uint8_t*, xfh_stream) = '
       'xfh_camera_points;\n'
       'int (*g)(const void*, int, int, int, int, int, const int32_t*, const double*, int, const double*, int, int, double, void*, uint8_t*, xfh_stream) = '
       'xfh_undistort_images;\n'
       'return (f == 0) + (g == 0) + XFH_CAMERA_FISHEYE + XFH_CAMERA_POINT_CAMERA + XFH_IMAGE_F32 + XFH_CAMERA_DISTORT + XFH_ERR_UNSUPPORTED; }\n')


@pytest.mark.parametrize("lang", ["c99", "c++11"])
def test_the_header_compiles_on_its_own_as_strict_c99_and_cxx11(tmp_path, lang):
    cc = "/opt/rocm/lib/llvm/bin/clang" + ("++" if lang == "c++11" else "")
    if not os.path.exists(cc):
        pytest.skip("no host clang")
    src = tmp_path / ("use.c" if lang == "c99" else "use.cpp")
    src.write_text(USE)
    subprocess.run([cc, "-std=" + lang, "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_camera_points_argument_errors_return_before_any_launch(lib):
    P, K = 3, 100
    base = {"pts": 1 << 20, "counts": 2 << 20, "kind": 3 << 20, "params": 4 << 20, "other": 5 << 20, "out": 6 << 20, "status": 7 << 20}
    size = {"pts": P * K * 8, "counts": P * 4, "kind": P * 4, "params": P * 96, "other": P * 32, "out": P * K * 8, "status": P * K}

    def cp(P=P, K=K, nc=P, direction=0, **kw):
        p = {k: (C.c_void_p(v) if v is not None else None) for k, v in dict(base, **kw).items()}
        return lib.xfh_camera_points(p["pts"], p["counts"], P, K, p["kind"], p["params"], nc, p["other"], direction, p["out"], p["status"], None)

    for k in ("pts", "kind", "params", "out", "status"):
        assert cp(**{k: None}) == ARG and b"NULL" in lib.xfh_last_error(), k
    assert cp(P=-1) == ARG and cp(K=-1) == ARG
    for nc in (0, 2, 4, -1):
        assert cp(nc=nc) == ARG and b"n_cameras" in lib.xfh_last_error(), nc
    for d in (-1, 2):
        assert cp(direction=d) == ARG and b"direction" in lib.xfh_last_error()
    # more than 2^31 - 1 workgroups of 256 points: the grid
    assert cp(P=1 << 33, K=1 << 20, nc=1) == UNSUPPORTED and b"more than one launch holds" in lib.xfh_last_error()
    assert cp(P=((1 << 31) - 1) * 256 + 1, K=1, nc=1) == UNSUPPORTED
    # no image or no row: nothing to do, whatever the pointers
    assert cp(P=0) == 0 and cp(K=0) == 0 and cp(P=0, pts=None, out=None, nc=7) == 0
    # the call is not in-place: every output against every input, at the first and at the last byte, and against the other output
    for o in ("out", "status"):
        for i in ("pts", "counts", "kind", "params", "other"):
            assert cp(**{o: base[i]}) == ARG and b"overlaps input" in lib.xfh_last_error(), (o, i)
            assert cp(**{o: base[i] + size[i] - 1}) == ARG, (o, i)
            assert cp(**{o: base[i] - size[o] + 1}) == ARG, (o, i)
    assert cp(status=base["out"] + size["out"] - 1) == ARG and b"outputs 0 and 1 overlap" in lib.xfh_last_error()
    assert cp(out=base["pts"], counts=None, other=None) == ARG


def test_undistort_images_argument_errors_return_before_any_launch(lib):
    B, Ch, H, W, Ho, Wo = 2, 3, 37, 53, 29, 41
    base = {"src": 1 << 20, "kind": 2 << 20, "params": 3 << 20, "new": 4 << 20, "dst": 5 << 20, "valid": 6 << 20}
    size = {"src": B * Ch * H * W * 4, "kind": B * 4, "params": B * 96, "new": B * 32, "dst": B * Ch * Ho * Wo * 4, "valid": B * Ho * Wo}

    def ui(dtype=1, B=B, Ch=Ch, H=H, W=W, nc=B, Ho=Ho, Wo=Wo, **kw):
        p = {k: (C.c_void_p(v) if v is not None else None) for k, v in dict(base, **kw).items()}
        return lib.xfh_undistort_images(p["src"], dtype, B, Ch, H, W, p["kind"], p["params"], nc, p["new"], Ho, Wo, 0.0, p["dst"], p["valid"], None)

    for k in ("src", "kind", "params", "dst"):
        assert ui(**{k: None}) == ARG and b"NULL" in lib.xfh_last_error(), k
    for dtype in (-1, 2):
        assert ui(dtype=dtype) == ARG and b"dtype" in lib.xfh_last_error()
    for kw in (dict(B=0), dict(Ch=0), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0), dict(B=-1), dict(Wo=-5)):
        assert ui(**kw) == ARG and b"bad shape" in lib.xfh_last_error(), kw
    for nc in (0, 3, -1):
        assert ui(nc=nc) == ARG and b"n_cameras" in lib.xfh_last_error(), nc
    assert ui(Ch=5) == UNSUPPORTED and b"C 5 above 4" in lib.xfh_last_error()
    assert ui(B=65536, nc=1) == UNSUPPORTED and b"more than one launch holds" in lib.xfh_last_error()          # grid z
    assert ui(Ho=4 * 65535 + 1) == UNSUPPORTED                                                                # grid y
    for i in ("src", "kind", "params", "new"):
        assert ui(dst=base[i]) == ARG and b"overlaps input" in lib.xfh_last_error(), i
        assert ui(dst=base[i] + size[i] - 1) == ARG and ui(dst=base[i] - size["dst"] + 1) == ARG, i
        assert ui(valid=base[i] + size[i] - 1) == ARG, i
    assert ui(valid=base["dst"] + size["dst"] - 1) == ARG and b"outputs 0 and 1 overlap" in lib.xfh_last_error()
    assert ui(dtype=0, dst=base["src"] + B * Ch * H * W - 1) == ARG                                            # the uint8 extent


def test_pack_cameras_on_every_model_and_on_bad_dicts():
    from accelerated_features_amd import _lib, cameras
    cams = [{"model": "SIMPLE_PINHOLE", "width": 4, "height": 3, "params": [5.0, 1.0, 2.0]},
            {"model": "PINHOLE", "width": 4, "height": 3, "params": [5.0, 6.0, 1.0, 2.0]},
            {"model": "SIMPLE_RADIAL", "width": 4, "height": 3, "params": [5.0, 1.0, 2.0, 0.1]},
            {"model": "RADIAL", "width": 4, "height": 3, "params": [5.0, 1.0, 2.0, 0.1, 0.2]},
            {"model": "OPENCV", "width": 4, "height": 3, "params": [5.0, 6.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4]},
            {"model": "OPENCV_FISHEYE", "width": 4, "height": 3, "params": [5.0, 6.0, 1.0, 2.0, 0.1, 0.2, 0.3, 0.4]}]
    kind, params = cameras.pack_cameras(cams)
    assert kind.dtype == np.int32 and params.dtype == np.float64 and params.shape == (6, 12)
    assert kind.tolist() == [0, 0, 1, 1, 1, 2] and set(cameras.MODELS) == set(CR.MODELS)
    for c, cam in enumerate(cams):                                       # the restatement's packing, written separately
        k, p = CR.pack(cam)
        assert k == kind[c] and np.array_equal(p, params[c]), cam["model"]
    assert params[3].tolist() == [5.0, 5.0, 1.0, 2.0, 0.1, 0.2] + [0.0] * 6
    k1, p1 = cameras.pack_cameras(cams[4])                               # one dict
    assert k1.shape == (1,) and np.array_equal(p1[0], params[4])
    K = cameras.camera_matrix(cams)
    assert K.dtype == torch.float64 and K.shape == (6, 3, 3) and K[4].tolist() == [[5.0, 0.0, 1.0], [0.0, 6.0, 2.0], [0.0, 0.0, 1.0]]
    assert K[0].tolist() == [[5.0, 0.0, 1.0], [0.0, 5.0, 2.0], [0.0, 0.0, 1.0]]
    with pytest.raises(_lib.XFeatHipError, match="FULL_OPENCV"):
        cameras.pack_cameras({"model": "FULL_OPENCV", "width": 1, "height": 1, "params": [1.0] * 12})
    with pytest.raises(_lib.XFeatHipError, match="model RADIAL takes 5 parameters, got 4"):
        cameras.pack_cameras([cams[0], {"model": "RADIAL", "width": 1, "height": 1, "params": [1.0] * 4}])
    with pytest.raises(_lib.XFeatHipError, match="model OPENCV takes 8"):
        cameras.pack_cameras({"model": "OPENCV", "params": [1.0] * 4})
    for bad in ({"params": [1.0] * 4}, {"model": "PINHOLE"}, "PINHOLE", None):
        with pytest.raises(_lib.XFeatHipError, match="camera 0"):
            cameras.pack_cameras([bad])
    # the poselib-shaped wrappers of pose / absolute_pose keep refusing anything but PINHOLE: the camera-aware forms live in cameras
    from accelerated_features_amd import absolute_pose, pose
    for mod in (pose, absolute_pose):
        with pytest.raises(_lib.XFeatHipError):
            mod._camera_K(cams[4])


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, cameras
    cam = CS.brown_camera(2)
    with pytest.raises(RuntimeError, match=r"expected kpts \(K,2\) or \(P,K,2\)"):
        cameras.undistort_keypoints(np.zeros((4, 3)), cam)
    with pytest.raises(RuntimeError, match="expected kpts"):
        cameras.distort_keypoints(np.zeros((2, 2, 4, 2)), cam)
    with pytest.raises(_lib.XFeatHipError, match="2 cameras for 3 images"):
        cameras.undistort_keypoints(np.zeros((3, 4, 2)), [cam, cam])
    with pytest.raises(RuntimeError, match="counts must have one entry per image"):
        cameras.undistort_keypoints(np.zeros((3, 4, 2)), cam, counts=[1, 2])
    with pytest.raises(_lib.XFeatHipError, match="NO_SUCH"):
        cameras.undistort_keypoints(np.zeros((3, 4, 2)), dict(cam, model="NO_SUCH"))
    with pytest.raises(RuntimeError, match="tensors expected"):
        cameras.undistort_images(np.zeros((1, 1, 4, 4), np.float32), cam)
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        cameras.undistort_images(torch.zeros((1, 1, 4, 4), dtype=torch.float64), cam)
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        cameras.undistort_images(torch.zeros((1, 4, 4)), cam)
    with pytest.raises(_lib.XFeatHipError, match="5 channels"):
        cameras.undistort_images(torch.zeros((1, 5, 4, 4)), cam)
    with pytest.raises(_lib.XFeatHipError, match="3 cameras for 2 images"):
        cameras.undistort_images(torch.zeros((2, 1, 4, 4)), [cam] * 3)
    with pytest.raises(_lib.XFeatHipError, match="camera dict expected"):
        cameras.estimate_relative_pose(np.zeros((8, 2)), np.zeros((8, 2)), [cam], cam)


def test_empty_shapes_are_written_without_a_library_call(monkeypatch):
    from accelerated_features_amd import cameras
    monkeypatch.setattr(cameras, "load", lambda: pytest.fail("an empty shape reached the library"))
    cam = CS.brown_camera(3)
    for shape in ((0, 2), (0, 5, 2), (3, 0, 2)):
        for fn in (cameras.undistort_keypoints, cameras.distort_keypoints):
            r = fn(torch.zeros(shape), cam, K_new=np.eye(3)) if fn is cameras.undistort_keypoints else fn(torch.zeros(shape), cam)
            assert r["kpts"].shape == shape and r["kpts"].dtype == torch.float32 and r["status"].shape == shape[:-1] and r["status"].dtype == torch.uint8
            assert r["K"].shape == (1, 3, 3)
    assert cameras.undistort_keypoints(torch.zeros((0, 2)), cam)["K"][0].tolist() == cameras.camera_matrix(cam)[0].tolist()
    for shape, out_size in (((0, 3, 4, 5), None), ((2, 0, 4, 5), None), ((2, 3, 4, 5), (0, 7)), ((2, 3, 4, 5), (7, 0))):
        for dt in (torch.uint8, torch.float32):
            dst, valid = cameras.undistort_images(torch.zeros(shape, dtype=dt), cam, out_size=out_size, return_valid=True)
            ho, wo = out_size or shape[2:]
            assert dst.shape == (shape[0], shape[1], ho, wo) and dst.dtype == dt and valid.shape == (shape[0], ho, wo) and valid.dtype == torch.uint8
    # no source pixel: everything is outside
    dst, valid = cameras.undistort_images(torch.zeros((2, 3, 0, 5), dtype=torch.uint8), cam, out_size=(2, 2), fill=7.5, return_valid=True)
    assert (dst == 8).all() and not valid.any()
    dst = cameras.undistort_images(torch.zeros((1, 1, 4, 0)), cam, out_size=(2, 2), fill=-1.25)
    assert (dst == -1.25).all() and dst.shape == (1, 1, 2, 2)


def test_everything_that_would_launch_raises_without_a_gpu():
    from accelerated_features_amd import _lib, cameras
    if torch.cuda.is_available():
        return                                             # (a GPU is present: tests/test_gpu_cameras.py runs the functions)
    cam, fish = CS.brown_camera(2), CS.fisheye_camera()
    pts = np.random.default_rng(0).uniform(0, 400, (12, 2)).astype(np.float32)
    for fn in (cameras.undistort_keypoints, cameras.distort_keypoints):
        with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
            fn(pts, cam)
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        cameras.undistort_images(torch.zeros((1, 1, 8, 8)), cam)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        cameras.estimate_relative_pose(pts, pts, cam, fish)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        cameras.estimate_absolute_pose(pts, np.ones((12, 3)), fish)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):      # PINHOLE goes to the existing wrapper, which raises alike
        cameras.estimate_relative_pose(pts, pts, CS.pinhole_camera(), CS.pinhole_camera())
