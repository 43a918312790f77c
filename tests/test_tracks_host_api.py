"""Host-side checks of the track-graph entries of the C ABI and of their Python wrappers: the three exported symbols, their
argument checks (which return before any launch: the pointers below are never dereferenced) and the wrappers' shape, dtype and `anchor`
errors.  The results live on the device (tests/test_gpu_tracks.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xfh_build_tracks_graph", "xfh_triangulate_tracks", "xfh_track_graph_workspace_bytes")
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
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None
    assert _lib.SIGNATURES["xfh_triangulate_tracks"] == _lib.SIGNATURES["xfh_triangulate_views"]      # one argument list
    assert re.search(r"#define XFH_TRACKS_BOUND 2\b", hdr) and re.search(r"#define XFH_VERSION 303\b", hdr) and lib.xfh_version() == 303
    for name in ("build_tracks_graph", "triangulate_graph_matches", "view_points"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(pkg.multiview, name)
    assert len(pkg.multiview.TRACK_INFO_FIELDS) == 8 and pkg.multiview.TRACK_STATUS[2] == "bound_reached"
    for f in (pkg.triangulate_views_batch, pkg.refine_views_batch):
        assert inspect.signature(f).parameters["anchor"].default == "reference"
    sig = inspect.signature(pkg.build_tracks_graph).parameters
    assert sig["min_length"].default == 2 and sig["max_tracks"].default is None


def test_workspace_planning_is_host_only(lib):
    w = lib.xfh_track_graph_workspace_bytes
    assert w(1, 2, 1) > 0 and w(1, 2, 1) % 256 == 0
    assert 14 * 64 * 32 * 4096 <= w(64, 32, 4096) <= 14 * 64 * 32 * 4096 + 5 * 256
    for bad in ((0, 3, 8), (65536, 3, 8), (1, 1, 8), (1, 33, 8), (1, 3, 0), (1, 3, (1 << 24) + 1), (-1, 3, 8)):
        assert w(*bad) == 0, bad


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def graph(pairs=x, idx=x, nm=x, out=x, of=x, nt=x, info=x, S=1, P=2, cap=8, V=3, K=16, ml=2, T=24, ws=x, nb=1 << 20):
        return lib.xfh_build_tracks_graph(pairs, idx, x, nm, S, P, cap, V, K, ml, T, out, of, nt, info, ws, nb, None)

    def tracks(kpts=x, tab=x, Ks=x, Rs=x, out=x, ninl=x, info=x, S=1, K=16, V=3, kcap=16, thr=4.0, cosm=0.9998, depth=INF, mv=2):
        return lib.xfh_triangulate_tracks(kpts, kcap, tab, None, S, K, V, Ks, Rs, x, thr, cosm, depth, mv, out, x, ninl, x, x, info, None)

    for kw in (dict(pairs=None), dict(idx=None), dict(nm=None), dict(out=None), dict(of=None), dict(nt=None), dict(info=None), dict(S=0), dict(S=-1),
               dict(S=65536), dict(P=0), dict(P=65536), dict(cap=0), dict(cap=-1), dict(cap=(1 << 24) + 1), dict(V=1), dict(V=33), dict(K=0), dict(K=-4),
               dict(ml=1), dict(ml=33), dict(T=0), dict(T=49), dict(T=-1), dict(ws=None), dict(nb=16), dict(ws=C.c_void_p(260))):
        assert graph(**kw) != 0, kw
        assert lib.xfh_last_error()
    graph(V=33)
    assert b"V 33 outside [2, 32]" in lib.xfh_last_error()
    graph(T=49)
    assert b"max_tracks 49" in lib.xfh_last_error()
    for kw in (dict(kpts=None), dict(tab=None), dict(Ks=None), dict(Rs=None), dict(out=None), dict(ninl=None), dict(info=None), dict(S=0), dict(S=65536),
               dict(K=0), dict(K=-1), dict(V=1), dict(V=33), dict(V=64), dict(kcap=0), dict(mv=1), dict(mv=0), dict(mv=-2), dict(mv=33), dict(thr=0.0),
               dict(thr=-1.0), dict(thr=NAN), dict(thr=INF), dict(depth=0.0), dict(depth=-2.0), dict(depth=NAN), dict(cosm=1.0001), dict(cosm=-1.5),
               dict(cosm=NAN)):
        assert tracks(**kw) != 0, kw
        assert lib.xfh_last_error()
    tracks(mv=1)
    assert b"xfh_triangulate_tracks: min_views 1" in lib.xfh_last_error()


def _scene(S=2, V=3, K=5, kcap=5):
    return (np.zeros((S, V, kcap, 2), np.float32), np.zeros((S, K, V), np.int32), None, np.tile(np.eye(3), (S, V, 1, 1)), np.tile(np.eye(3), (S, V, 1, 1)),
            np.zeros((S, V, 3)))


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, multiview
    for anchor in ("last", "", None, 0, "First"):
        with pytest.raises(_lib.XFeatHipError, match="anchor"):
            multiview.triangulate_views_batch(*_scene(), anchor=anchor)
        with pytest.raises(_lib.XFeatHipError, match="anchor"):
            multiview.refine_views_batch(*_scene(), anchor=anchor)
    with pytest.raises(_lib.XFeatHipError, match="min_views"):
        multiview.triangulate_views_batch(*_scene(), min_views=1, anchor="first")
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)      # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    g = multiview.build_tracks_graph
    for args in ((i32(2, 2), i64(3, 2, 8), i64(3, 2, 7), i32(3, 2)), (i32(2, 2), i64(3, 2, 8), i64(3, 2, 8), i32(3, 3)), (i32(2, 2), i64(2, 8), i64(2, 8), i32(2)),
                 (i32(2, 2), i64(3, 2, 8), i64(3, 3, 8), i32(3, 2))):
        with pytest.raises(RuntimeError, match="expected idx_a"):
            g(*args, 3, 16)
    for pairs in (i32(3, 2), i32(2, 3), i32(2, 2, 2), i32(4)):
        with pytest.raises(RuntimeError, match="expected view_pairs"):
            g(pairs, i64(3, 2, 8), i64(3, 2, 8), i32(3, 2), 3, 16)
    with pytest.raises(RuntimeError, match="tensors expected"):
        g(np.zeros((2, 2), np.int32), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 3, 16)
    with pytest.raises(_lib.XFeatHipError, match="V 33"):
        g(i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 33, 16)
    with pytest.raises(_lib.XFeatHipError, match="V 1 "):
        g(i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 1, 16)
    with pytest.raises(RuntimeError, match="negative"):
        g(i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 3, -1)
    for ml in (1, 0, 33):
        with pytest.raises(_lib.XFeatHipError, match="min_length"):
            g(i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 3, 16, min_length=ml)
    for T in (0, -1, 49):
        with pytest.raises(_lib.XFeatHipError, match="max_tracks"):
            g(i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 3, 16, max_tracks=T)
    with pytest.raises(RuntimeError, match="expected kpts"):
        multiview.triangulate_graph_matches(torch.zeros((1, 3, 4)), i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), None, None, None, None)
    with pytest.raises(RuntimeError, match="expected idx_a"):
        multiview.triangulate_graph_matches(torch.zeros((1, 3, 4, 2)), i32(2, 2), i64(2, 2, 8), i64(2, 2, 8), i32(2, 2), None, None, None, None)
    with pytest.raises(_lib.XFeatHipError, match="max_reproj_error"):
        multiview.triangulate_graph_matches(torch.zeros((1, 3, 4, 2)), None, None, None, None, None, None, None, None, max_reproj_error=0.0)
    # view_points is plain indexing and works wherever its tensors live
    X = torch.arange(12.0).reshape(1, 4, 3)
    of = torch.tensor([[[0, -1, 3], [2, 5, -1]]], dtype=torch.int32)
    got = multiview.view_points(X, of, 1)
    assert got.shape == (1, 3, 3) and got.dtype == torch.float32 and torch.equal(got[0, 0], X[0, 2]) and torch.isnan(got[0, 1:]).all()
    assert torch.equal(multiview.view_points(X, of, 0)[0, 2], X[0, 3]) and multiview.view_points(X[:, :0], of, 0).isnan().all()
    for view in (-1, 2):
        with pytest.raises(RuntimeError, match="view"):
            multiview.view_points(X, of, view)
    with pytest.raises(RuntimeError, match="expected points3d"):
        multiview.view_points(X[0], of, 0)
    if torch.cuda.is_available():
        return                                             # (the rest is covered on the device by tests/test_gpu_tracks.py)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        multiview.triangulate_views_batch(*_scene(), anchor="first")
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        g(i32(2, 2), i64(1, 2, 8), i64(1, 2, 8), i32(1, 2), 3, 16)
