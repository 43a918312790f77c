"""Host-side checks of the localisation entries of the C ABI and of their Python wrappers: the exported symbols, the argument checks (which
return before any launch: the pointers below are never dereferenced), the header as strict C, the wrappers' errors, the shapes that need no
library call and the loud failure without a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
NAMES = (("xfh_build_map", "int"), ("xfh_map_workspace_bytes", "size_t"), ("xfh_map_project", "int"))


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    from accelerated_features_amd import localization as loc
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, ret in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b%s %s\(" % (ret, name), hdr), name
    assert len(_lib.SIGNATURES["xfh_build_map"][1]) == 22 and len(_lib.SIGNATURES["xfh_map_project"][1]) == 12
    for name in ("build_map_batch", "localize_map_batch", "resect_views_batch", "project_map"):
        assert getattr(pkg, name) is getattr(loc, name)
    p = inspect.signature(loc.build_map_batch).parameters
    assert list(p) == ["desc", "tracks", "points3d", "status", "inlier_views", "min_views", "max_points"]
    assert p["min_views"].default == 2 and p["max_points"].default is None
    p = inspect.signature(loc.localize_map_batch).parameters
    assert list(p)[:10] == ["kpts_q", "desc_q", "n_q", "map", "K", "scene_of", "min_cossim", "guided", "guide_thr", "image_size"]
    assert [p[k].default for k in ("scene_of", "min_cossim", "guided", "guide_thr", "image_size")] == [None, 0.82, False, None, None]
    assert p["ransac"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(loc.resect_views_batch).parameters) == ["kpts", "track_of", "points3d", "Ks", "ransac"]
    assert len(loc.MAP_INFO_FIELDS) == 8 and loc.WORKSPACE_LIMIT == 512 << 20
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "k_map.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "Triton" not in src


def test_the_header_still_compiles_as_strict_c(tmp_path):
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        pytest.skip("no host clang")
    src = tmp_path / "use.c"
    src.write_text('#include "xfeat_hip.h"\nint main(void) { int (*f)(void) = (int (*)(void))0; size_t n = f ? xfh_map_workspace_bytes(1, 1, 2) : 0;\n'
                   'int (*g)(const float*, const int32_t*, int, int, const double*, const double*, const double*, double, double, double, float*, xfh_stream) '
                   '= xfh_map_project; return (int)n + (g == 0) + (&xfh_build_map == 0); }\n')
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_the_workspace_grows_with_the_call_and_is_zero_for_a_bad_shape(lib):
    f = lib.xfh_map_workspace_bytes
    assert f(0, 16, 3) == 0 and f(65536, 16, 3) == 0 and f(1, 0, 3) == 0 and f(1, (1 << 24) + 1, 3) == 0 and f(1, 16, 0) == 0 and f(1, 16, 33) == 0
    a, b, c = f(1, 256, 3), f(2, 256, 3), f(1, 512, 3)
    assert 0 < a < b and a < c and a % 256 == 0 and a >= 256 * (256 + 10)
    assert f(64, 16384, 8) < (512 << 20)                   # the batch of tools/localize_time.py fits one call


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def bm(desc=x, tracks=x, pts=x, status=x, inl=x, out=x, d=x, d16=x, trk=x, nobs=x, coh=x, npts=x, info=x, kcap=64, S=1, T=96, V=3, mv=2, M=96, ws=x,
           nbytes=1 << 30):
        return lib.xfh_build_map(desc, kcap, tracks, pts, status, inl, S, T, V, mv, M, out, d, d16, trk, nobs, coh, npts, info, ws, nbytes, None)

    for kw in (dict(desc=None), dict(tracks=None), dict(pts=None), dict(status=None), dict(inl=None), dict(out=None), dict(d=None), dict(d16=None),
               dict(trk=None), dict(nobs=None), dict(coh=None), dict(npts=None), dict(info=None), dict(kcap=0), dict(S=0), dict(S=65536), dict(T=0),
               dict(T=(1 << 24) + 1), dict(V=0), dict(V=33), dict(mv=0), dict(mv=33), dict(M=0), dict(M=(1 << 24) + 1), dict(desc=C.c_void_p(260)),
               dict(d=C.c_void_p(264)), dict(d16=C.c_void_p(260)), dict(ws=None), dict(ws=C.c_void_p(264)), dict(nbytes=64)):
        assert bm(**kw) != 0, kw
        assert lib.xfh_last_error()
    assert bm(V=33) == -4 and b"V 33 above 32" in lib.xfh_last_error()       # XFH_ERR_UNSUPPORTED: more views than this build holds
    assert bm(mv=0) == -1 and b"min_views 0 outside [1, 32]" in lib.xfh_last_error()
    assert bm(nbytes=64) == -3 and b"workspace too small" in lib.xfh_last_error()

    def pr(pts=x, R=x, t=x, K=x, uv=x, Q=2, M=64, W=640.0, H=480.0, margin=3.0):
        return lib.xfh_map_project(pts, None, Q, M, R, t, K, W, H, margin, uv, None)

    for kw in (dict(pts=None), dict(R=None), dict(t=None), dict(K=None), dict(uv=None), dict(Q=0), dict(Q=(1 << 20) + 1), dict(M=0), dict(M=(1 << 24) + 1),
               dict(W=-1.0), dict(W=NAN), dict(H=float("inf")), dict(W=0.0), dict(H=0.0), dict(margin=-1.0), dict(margin=NAN), dict(margin=float("inf")),
               dict(uv=C.c_void_p(260))):
        assert pr(**kw) == -1, kw
    assert b"margin" in lib.xfh_last_error() or b"uv" in lib.xfh_last_error()


def _map_args(S=2, V=3, K=8, T=12):
    return [torch.zeros((S, V, K, 64)), torch.full((S, T, V), -1, dtype=torch.int32), torch.zeros((S, T, 3)), torch.zeros((S, T), dtype=torch.uint8),
            torch.zeros((S, T), dtype=torch.int32)]


def _map(S=2, M=6, dev="cpu"):
    return {"points": torch.zeros((S, M, 3), device=dev), "desc": torch.zeros((S, M, 64), device=dev),
            "desc_f16": torch.zeros((S, M, 64), dtype=torch.float16, device=dev), "track": torch.zeros((S, M), dtype=torch.int32, device=dev),
            "n_points": torch.zeros((S,), dtype=torch.int32, device=dev)}


def _query(Q=2, Kq=5, dev="cpu"):
    return [torch.zeros((Q, Kq, 2), device=dev), torch.zeros((Q, Kq, 64), device=dev), torch.zeros((Q,), dtype=torch.int32, device=dev)]


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, localization as loc
    for i, bad, what in ((0, torch.zeros((2, 3, 8, 63)), "expected desc"), (1, torch.zeros((2, 12, 4), dtype=torch.int32), "expected tracks"),
                         (1, torch.zeros((3, 12, 3), dtype=torch.int32), "expected tracks"), (2, torch.zeros((2, 12, 2)), "expected points3d"),
                         (3, torch.zeros((2, 11), dtype=torch.uint8), "expected points3d"), (4, torch.zeros((2, 12, 1), dtype=torch.int32), "expected points3d")):
        a = _map_args()
        a[i] = bad
        with pytest.raises(RuntimeError, match=what):
            loc.build_map_batch(*a)
    for kw in (dict(min_views=0), dict(min_views=33), dict(min_views=True), dict(max_points=0), dict(max_points=-3)):
        with pytest.raises(_lib.XFeatHipError):
            loc.build_map_batch(*_map_args(), **kw)
    with pytest.raises(_lib.XFeatHipError, match="V 33"):
        loc.build_map_batch(*_map_args(V=33))
    K = np.eye(3)
    with pytest.raises(RuntimeError, match="dict of build_map_batch"):
        loc.localize_map_batch(*_query(), {"points": torch.zeros(2, 6, 3)}, K)
    with pytest.raises(RuntimeError, match="tensors expected"):
        loc.localize_map_batch(np.zeros((2, 5, 2), np.float32), *_query()[1:], _map(), K)
    with pytest.raises(RuntimeError, match="expected kpts_q"):
        loc.localize_map_batch(torch.zeros(2, 4, 2), *_query()[1:], _map(), K)
    with pytest.raises(RuntimeError, match="expected map points"):
        loc.localize_map_batch(*_query(), dict(_map(), track=torch.zeros((2, 7), dtype=torch.int32)), K)
    with pytest.raises(RuntimeError, match="need scene_of"):
        loc.localize_map_batch(*_query(Q=3), _map(S=2), K)
    with pytest.raises(RuntimeError, match="scene_of must be"):
        loc.localize_map_batch(*_query(Q=3), _map(S=2), K, scene_of=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="desc_q_f16"):
        loc.localize_map_batch(*_query(), _map(), K, desc_q_f16=torch.zeros((2, 5, 64)))
    for kw in (dict(guided=True, guide_thr=0.0), dict(guided=True, guide_thr=NAN), dict(guided=True, max_reproj_error=float("inf")),
               dict(image_size=(0, 480)), dict(image_size=(640, NAN))):
        with pytest.raises(_lib.XFeatHipError):
            loc.localize_map_batch(*_query(), _map(), K, **kw)
    with pytest.raises(RuntimeError, match="expected kpts"):
        loc.resect_views_batch(torch.zeros(2, 3, 8, 3), torch.zeros((2, 3, 8), dtype=torch.int32), torch.zeros(2, 12, 3), np.zeros((2, 3, 3, 3)))
    with pytest.raises(RuntimeError, match="expected track_of"):
        loc.resect_views_batch(torch.zeros(2, 3, 8, 2), torch.zeros((2, 3, 9), dtype=torch.int32), torch.zeros(2, 12, 3), np.zeros((2, 3, 3, 3)))
    with pytest.raises(RuntimeError, match="Ks must be"):
        loc.resect_views_batch(torch.zeros(2, 3, 8, 2), torch.zeros((2, 3, 8), dtype=torch.int32), torch.zeros(2, 12, 3), np.zeros((2, 3, 3)))
    with pytest.raises(RuntimeError, match="expected points"):
        loc.project_map(torch.zeros(2, 6, 2), None, np.zeros((2, 3, 3)), np.zeros((2, 3)), K)
    for kw in (dict(image_size=(0, 1)), dict(margin=-1.0), dict(margin=NAN)):
        with pytest.raises(_lib.XFeatHipError):
            loc.project_map(torch.zeros(2, 6, 3), None, np.zeros((2, 3, 3)), np.zeros((2, 3)), K, **kw)


def test_loud_failure_without_a_gpu():
    from accelerated_features_amd import _lib, localization as loc
    if torch.cuda.is_available():
        return                                             # (a GPU is present: tests/test_gpu_localization.py runs the functions)
    K = np.eye(3)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        loc.build_map_batch(*_map_args())
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        loc.localize_map_batch(*_query(), _map(), K)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        loc.resect_views_batch(torch.zeros(2, 3, 8, 2), torch.zeros((2, 3, 8), dtype=torch.int32), torch.zeros(2, 12, 3), np.tile(np.eye(3), (2, 3, 1, 1)))
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        loc.project_map(torch.zeros(2, 6, 3), None, np.zeros((2, 3, 3)), np.zeros((2, 3)), K)


def test_the_empty_shapes_are_written_without_a_library_call():
    from accelerated_features_amd import localization as loc
    for kw in (dict(S=0), dict(T=0), dict(K=0)):
        a = _map_args(**kw)
        S, T = a[1].shape[:2]
        M = 4
        if kw == dict(K=0):
            a[3][:, 1] = 5                                 # a status, a bad point: counted in the kernel's order
            a[2][:, 1:3, 0] = NAN
        out = loc.build_map_batch(*a, max_points=M)
        assert out["points"].shape == (S, M, 3) and bool(torch.isnan(out["points"]).all()), kw
        assert out["desc"].shape == (S, M, 64) and not out["desc"].any() and out["desc_f16"].dtype == torch.float16 and not out["desc_f16"].any(), kw
        assert out["track"].dtype == torch.int32 and bool((out["track"] == -1).all()) and out["n_obs"].dtype == torch.uint8 and not out["n_obs"].any(), kw
        assert not out["coherence"].any() and out["n_points"].shape == (S,) and not out["n_points"].any(), kw
        want = [T, 0, 1, 1, T - 2, 0, 0, 0] if kw == dict(K=0) else [0] * 8
        assert out["info"].shape == (S, 8) and all(row == want for row in out["info"].tolist()), (kw, out["info"].tolist())
    assert loc.build_map_batch(*_map_args(T=0))["points"].shape == (2, 0, 3)          # max_points None = T
