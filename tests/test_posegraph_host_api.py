"""Host-side checks of the pose-graph entry of the C ABI and of its Python wrappers: the exported symbols and the argument checks (which
return before any launch: the pointers below are never dereferenced), the wrappers' errors and the shapes that need no library call.
S = 0 and P = 0 are errors of the C entry (checked here) and results without a library call of the wrapper (on the device:
tests/test_gpu_posegraph.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


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
    for name, ret in (("xfh_average_poses", "int"), ("xfh_pose_graph_workspace_bytes", "size_t")):
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\b%s %s\(" % (ret, name), hdr), name
        assert getattr(lib, name).argtypes is not None
    assert len(_lib.SIGNATURES["xfh_average_poses"][1]) == 21
    for d, v in (("XFH_PG_OK", 0), ("XFH_PG_NOTHING", 1), ("XFH_PG_ROTATIONS_ONLY", 2), ("XFH_PG_NOT_FINITE", 3)):
        assert re.search(r"#define %s %d\b" % (d, v), hdr)
    assert re.search(r"#define XFH_VERSION 303\b", hdr) and lib.xfh_version() == 303
    for name in ("average_poses_batch", "relative_poses_graph_matches", "reconstruct_graph_matches"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(pkg.multiview, name)
    mv = pkg.multiview
    assert len(mv.PG_STATUS) == 4 and len(mv.PG_INFO_FIELDS) == 8 and 0.0 < mv.MIN_PIVOT_RATIO < 1e-3
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "k_triangulate.hip")).read()
    assert re.search(r"ST_OK = 0, ST_NOTHING = 1, ST_ROTATIONS_ONLY = 2, ST_NOT_FINITE = 3;", src)


def test_the_header_still_compiles_as_strict_c(tmp_path):
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        pytest.skip("no host clang")
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "xfeat_hip.h"\nint main(void) { int (*f)(void) = (int (*)(void))0; size_t n = f ? xfh_pose_graph_workspace_bytes(1, 1, 2) : 0; return (int)n + XFH_PG_ROTATIONS_ONLY - 2; }\n')
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_the_workspace_grows_with_the_call_and_is_zero_for_a_bad_shape(lib):
    f = lib.xfh_pose_graph_workspace_bytes
    assert f(0, 16, 3) == 0 and f(65536, 16, 3) == 0 and f(1, 0, 3) == 0 and f(1, 16, 1) == 0 and f(1, 16, 33) == 0 and f(1, (1 << 20) + 1, 3) == 0
    a, b, c = f(1, 256, 3), f(2, 256, 3), f(1, 4096, 3)
    assert 0 < a < b and a < c and a % 256 == 0
    assert c >= 4096 * (4 + 9 * 8) and f(64, 496, 32) < (4 << 20)


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def ap(pairs=x, R=x, t=x, w=x, Ro=x, to=x, reg=x, fac=x, info=x, S=1, P=16, V=3, it=30, rd=10, rot=0.03, pos=0.03, piv=1e-8, ws=x, nbytes=1 << 30):
        return lib.xfh_average_poses(pairs, R, t, w, None, S, P, V, it, rd, rot, pos, piv, Ro, to, reg, fac, info, ws, nbytes, None)

    for kw in (dict(pairs=None), dict(R=None), dict(t=None), dict(w=None), dict(Ro=None), dict(to=None), dict(reg=None), dict(fac=None), dict(info=None),
               dict(S=0), dict(S=-1), dict(S=65536), dict(P=0), dict(P=-1), dict(P=(1 << 20) + 1), dict(V=1), dict(V=33), dict(it=0), dict(it=1001),
               dict(rd=-1), dict(rd=31), dict(rot=0.0), dict(rot=-1.0), dict(rot=NAN), dict(rot=4.0), dict(pos=0.0), dict(pos=1.5), dict(pos=NAN),
               dict(piv=-1e-9), dict(piv=1.0), dict(piv=NAN), dict(ws=None), dict(ws=C.c_void_p(264)), dict(nbytes=64)):
        assert ap(**kw) != 0, kw
        assert lib.xfh_last_error()
    ap(V=33)
    assert b"V 33 outside [2, 32]" in lib.xfh_last_error()
    ap(rd=31)
    assert b"redescend" in lib.xfh_last_error()
    ap(nbytes=64)
    assert b"workspace too small" in lib.xfh_last_error()


def _edges(S=2, P=4):
    return [np.zeros((S, P, 2), np.int32), np.tile(np.eye(3), (S, P, 1, 1)), np.ones((S, P, 3)), np.ones((S, P)), 3]


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, multiview
    for kw in (dict(iterations=0), dict(iterations=1001), dict(redescend=-1), dict(redescend=31), dict(rot_scale_deg=0.0), dict(rot_scale_deg=NAN),
               dict(rot_scale_deg=181.0), dict(pos_scale_deg=0.0), dict(pos_scale_deg=91.0), dict(pos_scale_deg=NAN), dict(min_pivot_ratio=-1.0),
               dict(min_pivot_ratio=1.0), dict(min_pivot_ratio=NAN)):
        with pytest.raises(_lib.XFeatHipError):
            multiview.average_poses_batch(*_edges(), **kw)
    for i, bad, what in ((0, np.zeros((2, 5, 2), np.int32), "view_pairs"), (1, np.zeros((2, 4, 3, 2)), "R_rel"), (2, np.zeros((2, 4, 2)), "t_rel"),
                         (3, np.zeros((2, 5)), "t_rel"), (4, torch.zeros(3, dtype=torch.int32), "keyword V")):
        a = _edges()
        a[i] = bad
        with pytest.raises(RuntimeError, match=what):
            multiview.average_poses_batch(*a)
    a = _edges()
    a[4] = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="one entry per scene"):
        multiview.average_poses_batch(*a, V=3)
    for V in (1, 33):
        a = _edges()
        a[4] = V
        with pytest.raises(_lib.XFeatHipError, match="V %d" % V):
            multiview.average_poses_batch(*a)
    # the graph wrappers: tensors, shapes, settings
    k, vp = torch.zeros((2, 3, 8, 2)), torch.zeros((4, 2), dtype=torch.int32)
    ia, nm, Ks = torch.zeros((2, 4, 5), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32), np.tile(np.eye(3), (2, 3, 1, 1))
    with pytest.raises(RuntimeError, match="tensors expected"):
        multiview.relative_poses_graph_matches(k.numpy(), vp, ia, ia, nm, Ks)
    with pytest.raises(RuntimeError, match="expected kpts"):
        multiview.relative_poses_graph_matches(k[..., :1], vp, ia, ia, nm, Ks)
    with pytest.raises(RuntimeError, match="expected idx_a"):
        multiview.relative_poses_graph_matches(k, vp, ia, ia[:, :3], nm, Ks)
    with pytest.raises(RuntimeError, match="expected view_pairs"):
        multiview.relative_poses_graph_matches(k, vp[:3], ia, ia, nm, Ks)
    with pytest.raises(_lib.XFeatHipError, match="min_inliers"):
        multiview.relative_poses_graph_matches(k, vp, ia, ia, nm, Ks, min_inliers=-1)
    for kw in (dict(iterations=0), dict(redescend=31), dict(min_pivot_ratio=2.0), dict(max_reproj_error=0.0), dict(min_views=1), dict(fixed_views=-1),
               dict(huber_px=0.0), dict(max_iterations=-1)):
        with pytest.raises(_lib.XFeatHipError):
            multiview.reconstruct_graph_matches(k, vp, ia, ia, nm, None, Ks, **kw)
    if torch.cuda.is_available():
        return                                             # (the rest is covered on the device by tests/test_gpu_posegraph.py)
    with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
        multiview.average_poses_batch(*_edges())
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        multiview.relative_poses_graph_matches(k, vp, ia, ia, nm, Ks)


def test_the_defaults_are_the_measured_ones():
    import inspect
    from accelerated_features_amd import multiview
    p = inspect.signature(multiview.average_poses_batch).parameters
    assert [p[k].default for k in ("iterations", "redescend", "rot_scale_deg", "pos_scale_deg")] == [30, 10, 2.0, 2.0]
    assert p["min_pivot_ratio"].default == multiview.MIN_PIVOT_RATIO
    # the geometric mean of the two noise-free figures
    assert math.isclose(multiview.MIN_PIVOT_RATIO, math.sqrt(2.4e-2 * 1.8e-15), rel_tol=0.05)
