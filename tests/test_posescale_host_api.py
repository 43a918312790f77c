"""Host-side checks of the baseline-scale entries of the C ABI and of their Python wrappers: the exported symbols, the argument checks (which
return before any launch: the pointers below are never dereferenced), the header as strict C, the wrappers' errors and the shapes that need
no library call."""
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
NAMES = (("xfh_baseline_ratios", "int"), ("xfh_baseline_ratios_workspace_bytes", "size_t"), ("xfh_average_poses_ratios", "int"),
         ("xfh_pose_graph_ratios_workspace_bytes", "size_t"))


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    from accelerated_features_amd import multiview as mv
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, ret in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b%s %s\(" % (ret, name), hdr), name
    assert len(_lib.SIGNATURES["xfh_baseline_ratios"][1]) == 25 and len(_lib.SIGNATURES["xfh_average_poses_ratios"][1]) == 26
    assert re.search(r"#define XFH_PS_OK 0\b", hdr) and re.search(r"#define XFH_VERSION 303\b", hdr) and lib.xfh_version() == 303
    assert callable(pkg.baseline_ratios_batch)
    p = inspect.signature(mv.baseline_ratios_batch).parameters
    assert list(p) == ["kpts", "tracks", "track_of", "view_pairs", "R_rel", "t_rel", "weight", "Ks", "n_views", "max_reproj_error", "min_parallax_deg",
                       "max_depth", "min_common"]
    assert [p[k].default for k in ("n_views", "max_reproj_error", "min_parallax_deg", "max_depth", "min_common")] == [None, 4.0, 1.0, float("inf"), 8]
    p = inspect.signature(mv.average_poses_batch).parameters
    assert [p[k].default for k in ("ratio", "ratio_count", "scale_weight", "scale_tol")] == [None, None, 1.0, mv.SCALE_TOL] and mv.SCALE_TOL == 0.1
    p = inspect.signature(mv.reconstruct_graph_matches).parameters
    assert p["track_scales"].default is False and p["min_common"].default == 8
    assert mv.MAX_RATIO_PAIRS == 512 and mv.MAX_RATIO_KPTS == 4096 and len(mv.PS_INFO_FIELDS) == 8
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "posescale_body.hpp")).read()
    assert re.search(r"MAX_PAIRS = 512, MAX_K = 4096;", src)


def test_the_header_still_compiles_as_strict_c(tmp_path):
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        pytest.skip("no host clang")
    src = tmp_path / "use.c"
    src.write_text('#include "xfeat_hip.h"\nint main(void) { int (*f)(void) = (int (*)(void))0; size_t n = f ? xfh_pose_graph_ratios_workspace_bytes(1, 1, 2) + '
                   'xfh_baseline_ratios_workspace_bytes(1, 1, 2, 1) : 0; return (int)n + XFH_PS_OK; }\n')
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_the_workspaces_grow_with_the_call_and_are_zero_for_a_bad_shape(lib):
    f, g, h = lib.xfh_pose_graph_ratios_workspace_bytes, lib.xfh_baseline_ratios_workspace_bytes, lib.xfh_pose_graph_workspace_bytes
    assert f(0, 16, 3) == 0 and f(65536, 16, 3) == 0 and f(1, 0, 3) == 0 and f(1, 513, 3) == 0 and f(1, 16, 1) == 0 and f(1, 16, 33) == 0
    a, b, c = f(1, 256, 3), f(2, 256, 3), f(1, 512, 3)
    assert 0 < a < b and a < c and a % 256 == 0 and a > h(1, 256, 3)
    assert c >= 512 * 511 // 2 * 32 and f(64, 496, 32) < (512 << 20)
    assert g(0, 16, 3, 8) == 0 and g(1, 513, 3, 8) == 0 and g(1, 16, 3, 4097) == 0 and g(1, 16, 33, 8) == 0 and g(1, 16, 3, 0) == 0
    assert g(1, 512, 32, 4096) > 0 and g(1, 512, 32, 4096) % 256 == 0


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def br(kpts=x, tracks=x, tof=x, pairs=x, R=x, t=x, w=x, Ks=x, ratio=x, count=x, sh=x, info=x, S=1, P=16, V=3, K=64, T=96, thr=4.0, cm=0.99, md=1e9,
           mc=8, ws=x, nbytes=1 << 20):
        return lib.xfh_baseline_ratios(kpts, tracks, tof, pairs, R, t, w, Ks, None, S, P, V, K, T, thr, cm, md, mc, ratio, count, sh, info, ws, nbytes, None)

    for kw in (dict(kpts=None), dict(tracks=None), dict(tof=None), dict(pairs=None), dict(R=None), dict(t=None), dict(w=None), dict(Ks=None), dict(ratio=None),
               dict(count=None), dict(sh=None), dict(info=None), dict(S=0), dict(S=65536), dict(P=0), dict(P=513), dict(V=1), dict(V=33), dict(K=0),
               dict(K=4097), dict(T=0), dict(T=3 * 64 + 1), dict(thr=0.0), dict(thr=NAN), dict(cm=1.5), dict(cm=NAN), dict(md=0.0), dict(md=NAN), dict(mc=0),
               dict(ws=None), dict(ws=C.c_void_p(264)), dict(nbytes=64)):
        assert br(**kw) != 0, kw
        assert lib.xfh_last_error()
    br(P=513)
    assert b"P 513 outside [1, 512]" in lib.xfh_last_error()
    br(K=4097)
    assert b"K 4097 outside [1, 4096]" in lib.xfh_last_error()

    def ap(pairs=x, R=x, t=x, w=x, ratio=x, count=x, Ro=x, to=x, reg=x, fac=x, rfac=x, info=x, S=1, P=16, V=3, it=30, rd=10, rot=0.03, pos=0.03, piv=1e-8, sw=1.0,
           tol=0.1, ws=x, nbytes=1 << 30):
        return lib.xfh_average_poses_ratios(pairs, R, t, w, None, ratio, count, S, P, V, it, rd, rot, pos, piv, sw, tol, Ro, to, reg, fac, rfac, info, ws, nbytes,
                                            None)

    for kw in (dict(pairs=None), dict(R=None), dict(t=None), dict(w=None), dict(ratio=None), dict(count=None), dict(Ro=None), dict(to=None), dict(reg=None),
               dict(fac=None), dict(rfac=None), dict(info=None), dict(S=0), dict(S=65536), dict(P=0), dict(P=513), dict(V=1), dict(V=33), dict(it=0),
               dict(it=1001), dict(rd=-1), dict(rd=31), dict(rot=0.0), dict(rot=NAN), dict(pos=1.5), dict(piv=1.0), dict(sw=0.0), dict(sw=-1.0), dict(sw=NAN),
               dict(sw=float("inf")), dict(tol=0.0), dict(tol=1.5), dict(tol=NAN), dict(ws=None), dict(ws=C.c_void_p(264)), dict(nbytes=64)):
        assert ap(**kw) != 0, kw
        assert lib.xfh_last_error()
    ap(P=513)
    assert b"P 513 outside [1, 512]" in lib.xfh_last_error()
    ap(tol=1.5)
    assert b"scale_tol" in lib.xfh_last_error()
    ap(nbytes=64)
    assert b"workspace too small" in lib.xfh_last_error()


def _args(S=2, V=3, K=8, T=12, P=2):
    return [torch.zeros((S, V, K, 2)), torch.full((S, T, V), -1, dtype=torch.int32), torch.full((S, V, K), -1, dtype=torch.int32),
            np.zeros((S, P, 2), np.int32), np.tile(np.eye(3), (S, P, 1, 1)), np.ones((S, P, 3)), np.ones((S, P)), np.tile(np.eye(3), (S, V, 1, 1))]


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, multiview as mv
    with pytest.raises(_lib.XFeatHipError, match="513 pairs"):
        mv.baseline_ratios_batch(*_args(P=513))
    with pytest.raises(_lib.XFeatHipError, match="4097 key-points"):
        mv.baseline_ratios_batch(*_args(K=4097))
    for kw in (dict(max_reproj_error=0.0), dict(min_parallax_deg=181.0), dict(max_depth=0.0), dict(min_common=0)):
        with pytest.raises(_lib.XFeatHipError):
            mv.baseline_ratios_batch(*_args(), **kw)
    for i, bad, what in ((0, torch.zeros((2, 3, 8, 3)), "expected kpts"), (1, torch.zeros((2, 12, 4), dtype=torch.int32), "expected tracks"),
                         (2, torch.zeros((2, 3, 9), dtype=torch.int32), "expected tracks"), (3, np.zeros((2, 3, 2), np.int32), "view_pairs"),
                         (4, np.zeros((2, 2, 3, 2)), "R_rel"), (5, np.zeros((2, 2, 2)), "t_rel"), (6, np.zeros((2, 3)), "t_rel"), (7, np.zeros((2, 3, 3, 2)), "Ks"),
                         (0, torch.zeros((2, 3, 8, 2), dtype=torch.float64), "kpts must be"), (1, torch.zeros((2, 12, 3), dtype=torch.int64), "tracks must be"),
                         (2, torch.zeros((2, 3, 8), dtype=torch.int64), "track_of must be"), (0, np.zeros((2, 3, 8, 2), np.float32), "tensors expected")):
        a = _args()
        a[i] = bad
        with pytest.raises(RuntimeError, match=what):
            mv.baseline_ratios_batch(*a)
    with pytest.raises(RuntimeError, match="one entry per scene"):
        mv.baseline_ratios_batch(*_args(), n_views=torch.zeros(3, dtype=torch.int32))
    # the pose graph's new keywords
    e = [np.zeros((2, 4, 2), np.int32), np.tile(np.eye(3), (2, 4, 1, 1)), np.ones((2, 4, 3)), np.ones((2, 4)), 3]
    r, c = np.ones((2, 4, 4)), np.ones((2, 4, 4), np.int32)
    with pytest.raises(RuntimeError, match="come together"):
        mv.average_poses_batch(*e, ratio=r)
    for kw in (dict(scale_weight=0.0), dict(scale_weight=NAN), dict(scale_tol=0.0), dict(scale_tol=1.5), dict(scale_tol=NAN)):
        with pytest.raises(_lib.XFeatHipError):
            mv.average_poses_batch(*e, ratio=r, ratio_count=c, **kw)
    if torch.cuda.is_available():
        return                                             # (the rest is covered on the device by tests/test_gpu_posescale.py)
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        mv.baseline_ratios_batch(*_args())
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        mv.average_poses_batch(*e, ratio=r, ratio_count=c)


def test_the_empty_shapes_are_written_without_a_library_call():
    from accelerated_features_amd import multiview as mv
    for kw in (dict(S=0), dict(P=0), dict(K=0), dict(T=0)):
        a = _args(**kw)
        S, P = a[4].shape[:2]
        out = mv.baseline_ratios_batch(*a)
        assert out["ratio"].shape == (S, P, P) and out["ratio"].dtype == torch.float64 and bool(torch.isnan(out["ratio"]).all()), kw
        assert out["count"].shape == (S, P, P) and out["count"].dtype == torch.int32 and not out["count"].any(), kw
        assert out["shared_view"].shape == (S, P, P) and bool((out["shared_view"] == -1).all()), kw
        assert out["info"].shape == (S, 8) and not out["info"].any(), kw
