"""Host-side checks of the bundle adjustment entry of the C ABI and of its Python wrappers: the exported symbols and the argument checks (which
return before any launch: the pointers below are never dereferenced).  S = 0 and K = 0 are errors of the C entry (checked here) and results
without a library call of the wrappers, which live on the device (tests/test_gpu_bundle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, ret in (("xfh_bundle_adjust", "int"), ("xfh_bundle_workspace_bytes", "size_t")):
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\b%s %s\(" % (ret, name), hdr), name
        assert getattr(lib, name).argtypes is not None
    for d, v in (("XFH_BA_OK", 0), ("XFH_BA_NOTHING", 1), ("XFH_BA_NOT_FINITE", 2)):
        assert re.search(r"#define %s %d\b" % (d, v), hdr)
    for name in ("bundle_adjust_batch", "refine_views_batch"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(pkg.multiview, name)
    assert len(pkg.multiview.BA_STATUS) == 3 and len(pkg.multiview.BA_INFO_FIELDS) == 8 and pkg.multiview.MIN_VIEW_OBS == 6
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "k_triangulate.hip")).read()
    assert re.search(r"MIN_VIEW_OBS = 6;", src)


def test_the_workspace_grows_with_the_call_and_is_zero_for_a_bad_shape(lib):
    f = lib.xfh_bundle_workspace_bytes
    assert f(0, 16, 3) == 0 and f(65536, 16, 3) == 0 and f(1, 0, 3) == 0 and f(1, 16, 1) == 0 and f(1, 16, 33) == 0
    a, b, c, d = f(1, 256, 3), f(2, 256, 3), f(1, 4096, 3), f(1, 256, 32)
    assert 0 < a < b and a < c and a < d and a % 256 == 0
    assert d >= (192 * 193 // 2 + 192) * 8 and c >= 4096 * (2 * 24 + 72 + 4 + 1)
    assert f(64, 4096, 32) < (512 << 20)


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def ba(kpts=x, tab=x, inl=x, pts=x, Ks=x, Rs=x, Ro=x, Xo=x, refined=x, free=x, cost=x, info=x, S=1, K=16, V=3, kcap=16, iters=10, huber=1.0, ws=x,
           nbytes=1 << 30):
        return lib.xfh_bundle_adjust(kpts, kcap, tab, inl, pts, None, S, K, V, Ks, Rs, x, 1, iters, huber, Ro, x, Xo, refined, free, cost, info, ws, nbytes,
                                     None)

    for kw in (dict(kpts=None), dict(tab=None), dict(inl=None), dict(pts=None), dict(Ks=None), dict(Rs=None), dict(Ro=None), dict(Xo=None), dict(refined=None),
               dict(free=None), dict(cost=None), dict(info=None), dict(S=0), dict(S=-1), dict(S=65536), dict(K=0), dict(K=-1), dict(K=(1 << 24) + 1),
               dict(V=1), dict(V=33), dict(kcap=0), dict(iters=-1), dict(iters=1001), dict(huber=0.0), dict(huber=-1.0), dict(huber=NAN), dict(ws=None),
               dict(ws=C.c_void_p(264)), dict(nbytes=1024)):
        assert ba(**kw) != 0, kw
        assert lib.xfh_last_error()
    ba(V=33)
    assert b"V 33 outside [2, 32]" in lib.xfh_last_error()
    ba(huber=0.0)
    assert b"huber_px" in lib.xfh_last_error()
    ba(nbytes=1024)
    assert b"workspace too small" in lib.xfh_last_error()


def _scene(S=2, V=3, K=5, kcap=5):
    return [np.zeros((S, V, kcap, 2), np.float32), np.zeros((S, K, V), np.int32), np.zeros((S, K), np.int32), np.zeros((S, K, 3), np.float32), None,
            np.tile(np.eye(3), (S, V, 1, 1)), np.tile(np.eye(3), (S, V, 1, 1)), np.zeros((S, V, 3))]


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, multiview
    for kw in (dict(fixed_views=-1), dict(fixed_views=1 << 32), dict(fixed_views=1.0), dict(fixed_views=True), dict(max_iterations=-1),
               dict(max_iterations=1001), dict(huber_px=0.0), dict(huber_px=-2.0), dict(huber_px=NAN)):
        with pytest.raises(_lib.XFeatHipError):
            multiview.bundle_adjust_batch(*_scene(), **kw)
        a = _scene()
        with pytest.raises(_lib.XFeatHipError):
            multiview.refine_views_batch(a[0], a[1], None, a[5], a[6], a[7], **kw)
    a = _scene()
    for kw in (dict(min_views=1), dict(max_reproj_error=0.0), dict(max_depth=NAN)):
        with pytest.raises(_lib.XFeatHipError):
            multiview.refine_views_batch(a[0], a[1], None, a[5], a[6], a[7], **kw)
    with pytest.raises(_lib.XFeatHipError, match="V 33"):
        multiview.bundle_adjust_batch(*_scene(V=33))
    for i, bad, what in ((0, np.zeros((2, 3, 5, 3), np.float32), "expected kpts"), (1, np.zeros((2, 5, 4), np.int32), "expected kpts"),
                         (2, np.zeros((2, 6), np.int32), "expected inlier_views"), (3, np.zeros((2, 5, 2), np.float32), "expected inlier_views"),
                         (4, np.zeros(3, np.int32), "n_views"), (5, np.zeros((2, 3, 3, 2)), "Ks"), (7, np.zeros((2, 3, 4)), "ts")):
        b = _scene()
        b[i] = bad
        if torch.cuda.is_available() or i < 4:
            with pytest.raises(RuntimeError, match=what):
                multiview.bundle_adjust_batch(*b)
    if torch.cuda.is_available():
        return                                             # (the rest is covered on the device by tests/test_gpu_bundle.py)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        multiview.bundle_adjust_batch(*_scene())
