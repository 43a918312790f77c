"""Host-side checks of the two-view structure entries of the C ABI: the four exported symbols and their argument checks (which return
before any launch: the pointers below are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xfh_triangulate", "xfh_triangulate_matches", "xfh_recover_pose", "xfh_recover_pose_matches")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_four_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None
    assert int(re.search(r"#define XFH_VERSION (\d+)", hdr).group(1)) == 303 == lib.xfh_version()
    for code, word in enumerate(("VALID", "MASKED", "NOT_FINITE", "BEHIND", "FAR", "REPROJ", "PARALLAX")):
        assert re.search(r"#define XFH_TRI_%s %d\b" % (word, code), hdr)
    for name in ("triangulate_batch", "triangulate_matches", "recover_pose_batch", "recover_pose_matches", "recover_pose", "essential_from_fundamental"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(pkg.structure, name)
    assert len(pkg.structure.STATUS) == 7 and len(pkg.structure.INFO_FIELDS) == 8


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def tri(p0=x, K0=x, R=x, out=x, info=x, P=1, cap=8, n=8, thr=4.0, cosm=0.9998, depth=INF):
        return lib.xfh_triangulate(p0, x, None, n, P, cap, K0, x, R, x, None, thr, cosm, depth, out, x, x, info, None)

    def tri_m(idx0=x, nm=x, kcap=16, P=1, cap=8, thr=4.0, cosm=0.9998, depth=INF, R=x):
        return lib.xfh_triangulate_matches(x, x, kcap, idx0, x, nm, P, cap, x, x, R, x, None, thr, cosm, depth, x, x, x, x, None, None)

    def rec(p0=x, E=x, R=x, good=x, P=1, cap=8, n=8, thr=50.0):
        return lib.xfh_recover_pose(p0, x, None, n, P, cap, x, x, E, None, thr, R, x, good, x, None, x, None)

    def rec_m(idx1=x, nm=x, kcap=16, P=1, cap=8, thr=50.0, E=x):
        return lib.xfh_recover_pose_matches(x, x, kcap, x, idx1, nm, P, cap, x, x, E, None, thr, x, x, x, x, None, x, None)

    bad_tri = (dict(p0=None), dict(K0=None), dict(R=None), dict(out=None), dict(info=None), dict(P=0), dict(P=-1), dict(P=65536), dict(cap=0), dict(cap=-3),
               dict(n=9), dict(n=-1), dict(thr=0.0), dict(thr=-1.0), dict(thr=NAN), dict(thr=INF), dict(depth=0.0), dict(depth=-2.0), dict(depth=NAN),
               dict(cosm=1.0001), dict(cosm=-1.5), dict(cosm=NAN))
    for kw in bad_tri:
        assert tri(**kw) != 0, kw
        assert lib.xfh_last_error()
    for kw in (dict(idx0=None), dict(nm=None), dict(kcap=0), dict(P=0), dict(P=70000), dict(cap=0), dict(thr=INF), dict(thr=0.0), dict(depth=-1.0), dict(depth=NAN),
               dict(cosm=2.0), dict(cosm=NAN), dict(R=None)):
        assert tri_m(**kw) != 0, kw
        assert lib.xfh_last_error()
    for kw in (dict(p0=None), dict(E=None), dict(R=None), dict(good=None), dict(P=0), dict(P=65536), dict(cap=0), dict(n=9), dict(thr=0.0), dict(thr=-50.0), dict(thr=NAN)):
        assert rec(**kw) != 0, kw
        assert lib.xfh_last_error()
    for kw in (dict(idx1=None), dict(nm=None), dict(kcap=0), dict(P=0), dict(P=65536), dict(cap=0), dict(thr=0.0), dict(thr=NAN), dict(E=None)):
        assert rec_m(**kw) != 0, kw
        assert lib.xfh_last_error()


def test_python_argument_errors_raise_without_a_device():
    """The thresholds are checked before anything touches the device; without one the entry then raises like the other estimators."""
    import numpy as np
    import torch
    from accelerated_features_amd import _lib, structure
    if torch.cuda.is_available():
        return                                             # (covered on the device by tests/test_gpu_structure.py)
    p = np.zeros((1, 4, 2), np.float32)
    with pytest.raises(_lib.XFeatHipError):
        structure.triangulate_batch(p, p, None, np.eye(3), np.eye(3), np.eye(3), np.ones(3))
    with pytest.raises(_lib.XFeatHipError):
        structure.recover_pose(np.eye(3), p[0], p[0])
