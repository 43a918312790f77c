"""Host-side checks of the 3D-3D alignment entries: the three exported symbols and their argument checks (which return before any
launch: the pointers below are never dereferenced), the workspace size without a device, the Python wrappers' shape checks and
apply_alignment."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xfh_align_workspace_bytes", "xfh_estimate_alignment", "xfh_estimate_alignment_matches")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_three_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\b(int|size_t) %s\(" % name, hdr), name
    for name in ("estimate_alignment_batch", "estimate_alignment_matches", "estimate_relative_pose_rgbd_matches", "apply_alignment"):
        assert callable(getattr(pkg, name)) and getattr(pkg, name) is getattr(pkg.alignment, name)
    assert len(pkg.alignment.INFO_FIELDS) == 8 and pkg.alignment.MAX_ITERATIONS == 16384


def test_workspace_size_is_host_only(lib):
    one = lib.xfh_align_workspace_bytes(1, 1000)
    assert one >= 1024 * (13 * 8 + 8 + 4 + 4)                        # 1000 hypotheses padded to 1024: the model, a cost, a count, a flag
    assert lib.xfh_align_workspace_bytes(1, 1024) == one < lib.xfh_align_workspace_bytes(1, 1025)
    assert lib.xfh_align_workspace_bytes(1500, 1000) > 1499 * (one - 2048)
    assert lib.xfh_align_workspace_bytes(0, 1000) == 0 and lib.xfh_align_workspace_bytes(4, 0) == 0 and lib.xfh_align_workspace_bytes(-1, 8) == 0
    assert one < lib.xfh_abspose_workspace_bytes(1, 1000)             # one candidate per hypothesis instead of four


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first
    big = 1 << 40

    def est(a=x, b=x, R=x, t=x, s=x, mask=x, info=x, P=1, cap=8, n=8, thr=0.1, lo=20, hi=1000, prob=0.9999, ws=x, wsb=big):
        return lib.xfh_estimate_alignment(a, b, None, n, P, cap, 1, thr, lo, hi, prob, 0, R, t, s, mask, info, ws, wsb, None)

    def est_m(a=x, b=x, ia=x, ib=x, nm=x, ka=16, kb=24, s=x, P=1, cap=8, thr=0.1, lo=20, hi=1000, prob=0.9999, ws=x, wsb=big):
        return lib.xfh_estimate_alignment_matches(a, ka, b, kb, ia, ib, nm, P, cap, 0, thr, lo, hi, prob, 0, x, x, s, x, x, ws, wsb, None)

    bad = (dict(a=None), dict(b=None), dict(R=None), dict(t=None), dict(s=None), dict(mask=None), dict(info=None), dict(P=0), dict(P=-1), dict(P=65536),
           dict(cap=0), dict(cap=-3), dict(n=9), dict(n=-1), dict(thr=0.0), dict(thr=-1.0), dict(thr=NAN), dict(thr=INF), dict(lo=-1), dict(hi=0),
           dict(hi=16385), dict(prob=0.0), dict(prob=1.0), dict(prob=NAN), dict(ws=None), dict(wsb=1024))
    for kw in bad:
        assert est(**kw) != 0, kw
        assert lib.xfh_last_error()
    for kw in (dict(a=None), dict(b=None), dict(ia=None), dict(ib=None), dict(nm=None), dict(ka=0), dict(kb=-1), dict(s=None), dict(P=0), dict(P=70000),
               dict(cap=0), dict(thr=0.0), dict(thr=NAN), dict(thr=INF), dict(lo=-1), dict(hi=0), dict(hi=20000), dict(prob=1.5), dict(ws=None), dict(wsb=0)):
        assert est_m(**kw) != 0, kw
        assert lib.xfh_last_error()
    assert b"max_iters" in (est(hi=16385), lib.xfh_last_error())[1]


def test_python_wrappers_refuse_mismatched_shapes():
    from accelerated_features_amd import alignment as al
    a = np.zeros((2, 5, 3), np.float32)
    for pa, pb, counts in ((a, a[:, :4], None), (a, a[:1], None), (a[..., :2], a[..., :2], None), (a[0], a[0], None), (a, a, [5]), (a, a, [[5, 5]])):
        with pytest.raises(RuntimeError, match="expected|counts"):
            al.estimate_alignment_batch(pa, pb, counts, 0.1)
    ta, tb = torch.zeros(2, 7, 3), torch.zeros(2, 9, 3)
    ia, nm = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    for args in ((ta, tb, ia, ia[:, :3], nm), (ta, tb[:1], ia, ia, nm), (ta, tb, ia, ia, nm[:1]), (ta[..., :2], tb, ia, ia, nm), (ta, tb, ia[0], ia[0], nm),
                 (ta, tb, ia.int(), ia, nm), (ta.double(), tb, ia, ia, nm), (ta, tb, ia, ia, nm.long()), (ta, tb.transpose(1, 2), ia, ia, nm)):
        with pytest.raises(RuntimeError, match="expected"):
            al.estimate_alignment_matches(*args, 0.1)
    with pytest.raises(RuntimeError):
        al.apply_alignment(torch.zeros(2, 5, 3), torch.ones(3), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError):
        al.apply_alignment(torch.zeros(5, 2), 1.0, torch.eye(3), torch.zeros(3))


def test_no_device_means_loud_failure_and_bad_parameters_raise():
    from accelerated_features_amd import _lib, alignment as al
    a = np.zeros((1, 4, 3), np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.XFeatHipError):
            al.estimate_alignment_batch(a, a, None, 0.1)
        ta, ia, nm = torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
        with pytest.raises(_lib.XFeatHipError):
            al.estimate_alignment_matches(ta, ta, ia, ia, nm, 0.1)
    else:                                                      # (with a device the parameter checks are reached)
        for kw in (dict(max_error=0.0), dict(max_error=NAN), dict(max_error=INF), dict(max_error=0.1, max_iterations=0), dict(max_error=0.1, max_iterations=16385)):
            with pytest.raises(_lib.XFeatHipError):
                al.estimate_alignment_batch(a, a, None, **kw)


def test_apply_alignment_keeps_nan_rows():
    from accelerated_features_amd import apply_alignment
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])         # a quarter turn about z
    pts = torch.tensor([[[1.0, 0.0, 0.0], [NAN, NAN, NAN], [0.0, 2.0, 1.0], [1.0, NAN, 3.0]],
                        [[NAN, NAN, NAN], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [-1.0, 0.5, 2.0]]])
    out = apply_alignment(pts, [2.0, 1.0], np.stack([R, np.eye(3)]), [[10.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    assert out.dtype == torch.float32 and out.shape == pts.shape
    want = torch.tensor([[[10.0, 2.0, 0.0], [NAN, NAN, NAN], [6.0, 0.0, 2.0], [NAN, NAN, NAN]],
                         [[NAN, NAN, NAN], [1.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.5, 1.0]]])
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.equal(torch.nan_to_num(out), torch.nan_to_num(want))
    one = apply_alignment(pts[0].double(), 2.0, R, [10.0, 0.0, 0.0])
    assert one.dtype == torch.float64 and torch.equal(torch.nan_to_num(one), torch.nan_to_num(want[0].double()))
