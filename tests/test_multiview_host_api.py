"""Host-side checks of the multi-view entries of the C ABI and of their Python wrappers: the two exported symbols and their argument checks
(which return before any launch: the pointers below are never dereferenced).  S = 0 and K = 0 are errors of the C entries (checked here) and
empty results of the wrappers, which live on the device (tests/test_gpu_multiview.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xfh_build_tracks", "xfh_triangulate_views")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_two_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"#define XFH_MV_UNOBSERVED 1\b", hdr) and re.search(r"#define XFH_MV_MAX_VIEWS 32\b", hdr)
    for name in ("build_tracks", "triangulate_views_batch", "triangulate_views_matches"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(pkg.multiview, name)
    assert len(pkg.multiview.STATUS) == 7 and len(pkg.multiview.INFO_FIELDS) == 8 and pkg.multiview.MAX_VIEWS == 32
    assert pkg.multiview.STATUS[0] == "valid" and pkg.multiview.INFO_FIELDS[0] == "n"


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def tracks(idx=x, nm=x, out=x, S=1, V=3, cap=8, K=16, kcap=16):
        return lib.xfh_build_tracks(idx, x, nm, S, V, cap, K, kcap, out, None)

    def views(kpts=x, tab=x, Ks=x, Rs=x, out=x, ninl=x, info=x, S=1, K=16, V=3, kcap=16, thr=4.0, cosm=0.9998, depth=INF, mv=2):
        return lib.xfh_triangulate_views(kpts, kcap, tab, None, S, K, V, Ks, Rs, x, thr, cosm, depth, mv, out, x, ninl, x, x, info, None)

    for kw in (dict(idx=None), dict(nm=None), dict(out=None), dict(S=0), dict(S=-1), dict(S=65536), dict(V=1), dict(V=0), dict(V=33), dict(cap=-1),
               dict(cap=(1 << 24) + 1), dict(K=0), dict(K=-4), dict(kcap=0)):
        assert tracks(**kw) != 0, kw
        assert lib.xfh_last_error()
    for kw in (dict(kpts=None), dict(tab=None), dict(Ks=None), dict(Rs=None), dict(out=None), dict(ninl=None), dict(info=None), dict(S=0), dict(S=65536),
               dict(K=0), dict(K=-1), dict(V=1), dict(V=33), dict(V=64), dict(kcap=0), dict(mv=1), dict(mv=0), dict(mv=-2), dict(mv=33), dict(thr=0.0),
               dict(thr=-1.0), dict(thr=NAN), dict(thr=INF), dict(depth=0.0), dict(depth=-2.0), dict(depth=NAN), dict(cosm=1.0001), dict(cosm=-1.5),
               dict(cosm=NAN)):
        assert views(**kw) != 0, kw
        assert lib.xfh_last_error()
    views(V=33)
    assert b"V 33 outside [2, 32]" in lib.xfh_last_error()
    views(mv=1)
    assert b"min_views 1" in lib.xfh_last_error()


def _scene(S=2, V=3, K=5, kcap=5):
    return (np.zeros((S, V, kcap, 2), np.float32), np.zeros((S, K, V), np.int32), None, np.tile(np.eye(3), (S, V, 1, 1)), np.tile(np.eye(3), (S, V, 1, 1)),
            np.zeros((S, V, 3)))


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, multiview
    for kw in (dict(min_views=1), dict(min_views=0), dict(min_views=33), dict(max_reproj_error=0.0), dict(max_reproj_error=-1.0), dict(max_reproj_error=INF),
               dict(max_reproj_error=NAN), dict(max_depth=0.0), dict(max_depth=NAN), dict(min_parallax_deg=-1.0), dict(min_parallax_deg=200.0)):
        with pytest.raises(_lib.XFeatHipError):
            multiview.triangulate_views_batch(*_scene(), **kw)
        with pytest.raises(_lib.XFeatHipError):
            multiview.triangulate_views_matches(torch.zeros((1, 3, 4, 2)), None, None, None, None, None, None, None, **kw)
    with pytest.raises(_lib.XFeatHipError, match="V 33"):
        multiview.triangulate_views_batch(*_scene(V=33))
    with pytest.raises(_lib.XFeatHipError, match="V 1 "):
        multiview.triangulate_views_batch(*_scene(V=1))
    # shape mismatches
    a = _scene()
    for i, bad in ((0, np.zeros((2, 3, 5, 3), np.float32)), (0, np.zeros((2, 3, 5), np.float32)), (1, np.zeros((2, 5, 4), np.int32)), (1, np.zeros((3, 5, 3), np.int32)),
                   (1, np.zeros((2, 5), np.int32))):
        b = list(a)
        b[i] = bad
        with pytest.raises(RuntimeError, match="expected kpts"):
            multiview.triangulate_views_batch(*b)
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)      # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    for args in ((i64(2, 2, 8), i64(2, 2, 7), i32(2, 2)), (i64(2, 2, 8), i64(2, 2, 8), i32(2, 3)), (i64(2, 8), i64(2, 8), i32(2)), (i64(2, 2, 8), i64(2, 3, 8), i32(2, 2))):
        with pytest.raises(RuntimeError, match="expected idx_ref"):
            multiview.build_tracks(*args, 16)
    with pytest.raises(RuntimeError, match="tensors expected"):
        multiview.build_tracks(np.zeros((1, 2, 8), np.int64), i64(1, 2, 8), i32(1, 2), 16)
    with pytest.raises(_lib.XFeatHipError, match="V 34"):
        multiview.build_tracks(i64(1, 33, 8), i64(1, 33, 8), i32(1, 33), 16)
    with pytest.raises(RuntimeError, match="negative"):
        multiview.build_tracks(i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), -1)
    with pytest.raises(RuntimeError, match="expected idx_ref"):
        multiview.triangulate_views_matches(torch.zeros((1, 3, 4, 2)), i64(1, 3, 8), i64(1, 3, 8), i32(1, 3), None, None, None, None)
    if torch.cuda.is_available():
        return                                             # (the rest is covered on the device by tests/test_gpu_multiview.py)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        multiview.triangulate_views_batch(*_scene())
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        multiview.build_tracks(i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 16)
