"""Host-side checks of the match-verification entries of the C ABI and of their Python wrappers: the exported symbols, the argument checks
(which return before any launch: the pointers below are never dereferenced), the overlap check of the filter, the header as strict C, the
wrappers' errors, the shapes that need no library call and the loud failure without a GPU."""
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
NAMES = (("xfh_filter_matches", "int"), ("xfh_verify_matches", "int"))


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    from accelerated_features_amd import multiview as mv, verification as ver
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, ret in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b%s %s\(" % (ret, name), hdr), name
    assert len(_lib.SIGNATURES["xfh_filter_matches"][1]) == 14 and len(_lib.SIGNATURES["xfh_verify_matches"][1]) == 19
    assert lib.xfh_version() == 303 and "#define XFH_VERSION 303 " in hdr           # added entry points only
    for name in ("filter_matches_batch", "verify_matches_graph"):
        assert getattr(pkg, name) is getattr(ver, name)
    p = inspect.signature(ver.filter_matches_batch).parameters
    assert list(p) == ["idx_a", "idx_b", "n_matches", "mask", "keep", "min_keep"] and p["keep"].default is None and p["min_keep"].default == 0
    p = inspect.signature(ver.verify_matches_graph).parameters
    assert list(p) == ["kpts", "view_pairs", "idx_a", "idx_b", "n_matches", "n_views", "Ks", "Rs", "ts", "max_epipolar_error"]
    assert p["max_epipolar_error"].default == 1.0
    p = inspect.signature(mv.reconstruct_graph_matches).parameters
    assert p["verified"].default is False and list(p)[-1] == "verified"             # every earlier keyword and default stays where it was
    assert len(ver.FILTER_INFO_FIELDS) == 4 and len(ver.VERIFY_INFO_FIELDS) == 4 and len(ver.VERIFY_STATUS) == 4 and len(ver.EMPTIED) == 3
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "k_matchfilter.hip")).read()
    assert "filter_matches_kernel<<<(unsigned)L, 256, 0, st>>>" in src and "Triton" not in src


def test_the_header_still_compiles_as_strict_c(tmp_path):
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        pytest.skip("no host clang")
    src = tmp_path / "use.c"
    src.write_text('#include "xfeat_hip.h"\nint main(void) {\n'
                   'int (*f)(const int64_t*, const int64_t*, const int32_t*, const uint8_t*, const uint8_t*, int64_t, int, int, int64_t*, int64_t*, int32_t*, '
                   'int32_t*, int32_t*, xfh_stream) = xfh_filter_matches;\n'
                   'return (f == 0) + (&xfh_verify_matches == 0) + XFH_FILTER_BY_MIN_KEEP + XFH_VERIFY_BASELINE; }\n')
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_filter_argument_errors_return_before_any_launch(lib):
    L, cap = 4, 100
    # distinct, never dereferenced ranges: every call below fails its argument checks first
    base = {"ia": 1 << 20, "ib": 2 << 20, "n": 3 << 20, "mask": 4 << 20, "keep": 5 << 20, "oa": 6 << 20, "ob": 7 << 20, "src": 8 << 20, "no": 9 << 20,
            "info": 10 << 20}
    size = {"ia": L * cap * 8, "ib": L * cap * 8, "n": L * 4, "mask": L * cap, "keep": L, "oa": L * cap * 8, "ob": L * cap * 8, "src": L * cap * 4,
            "no": L * 4, "info": L * 16}

    def fm(L=L, cap=cap, min_keep=0, **kw):
        p = {k: (C.c_void_p(v) if v is not None else None) for k, v in dict(base, **kw).items()}
        return lib.xfh_filter_matches(p["ia"], p["ib"], p["n"], p["mask"], p["keep"], L, cap, min_keep, p["oa"], p["ob"], p["src"], p["no"], p["info"], None)

    for k in ("ia", "ib", "n", "mask", "oa", "ob", "src", "no", "info"):
        assert fm(**{k: None}) == -1 and b"NULL" in lib.xfh_last_error(), k
    assert fm(L=-1) == -1 and fm(cap=-1) == -1 and fm(cap=(1 << 24) + 1) == -1 and fm(min_keep=-1) == -1
    assert b"min_keep -1" in lib.xfh_last_error()
    assert fm(L=1 << 31) == -4 and b"more than one launch holds" in lib.xfh_last_error()          # XFH_ERR_UNSUPPORTED: the grid
    # no list or no slot: nothing to do, whatever the pointers
    assert fm(L=0) == 0 and fm(cap=0) == 0 and fm(L=0, ia=None, oa=None) == 0
    # the call is not in-place: every output against every input, at the first and at the last byte, and the outputs against each other
    for o in ("oa", "ob", "src", "no", "info"):
        for i in ("ia", "ib", "n", "mask", "keep"):
            assert fm(**{o: base[i]}) == -1 and b"overlaps input" in lib.xfh_last_error(), (o, i)
            assert fm(**{o: base[i] + size[i] - 1}) == -1, (o, i)
            assert fm(**{o: base[i] - size[o] + 1}) == -1, (o, i)
        for q in ("oa", "ob", "src", "no", "info"):
            if q != o:
                assert fm(**{o: base[q] + size[q] - 1}) == -1 and b"overlap" in lib.xfh_last_error(), (o, q)
    assert fm(oa=base["ia"], keep=None) == -1


def test_verify_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced

    def vm(kpts=x, vp=x, ia=x, ib=x, n=x, nv=None, Ks=x, Rs=x, ts=x, mask=x, err=None, info=x, S=1, P=3, cap=64, V=3, K=64, thr=1.0):
        return lib.xfh_verify_matches(kpts, vp, ia, ib, n, nv, S, P, cap, V, K, Ks, Rs, ts, thr, mask, err, info, None)

    for kw in (dict(kpts=None), dict(vp=None), dict(ia=None), dict(ib=None), dict(n=None), dict(Ks=None), dict(Rs=None), dict(ts=None), dict(mask=None),
               dict(info=None), dict(S=0), dict(S=65536), dict(P=0), dict(P=65536), dict(cap=0), dict(cap=(1 << 24) + 1), dict(V=1), dict(K=0),
               dict(K=(1 << 24) + 1), dict(thr=0.0), dict(thr=-1.0), dict(thr=NAN), dict(thr=float("inf")), dict(kpts=C.c_void_p(260))):
        assert vm(**kw) == -1, kw
        assert lib.xfh_last_error()
    assert vm(V=33) == -4 and b"V 33 above 32" in lib.xfh_last_error()
    assert vm(thr=NAN) == -1 and b"max_epipolar_error" in lib.xfh_last_error()
    assert vm(S=65535, P=65535) == -4 and b"more than one launch holds" in lib.xfh_last_error()   # S P >= 2^31: the grid


def _lists(S=2, P=3, cap=5, dev="cpu", lead3=True):
    shape = (S, P) if lead3 else (P,)
    return [torch.zeros(shape + (cap,), dtype=torch.int64, device=dev), torch.zeros(shape + (cap,), dtype=torch.int64, device=dev),
            torch.zeros(shape, dtype=torch.int32, device=dev), torch.ones(shape + (cap,), dtype=torch.uint8, device=dev)]


def _graph(S=2, V=3, K=8, P=3, cap=5):
    ia, ib, n, _ = _lists(S, P, cap)
    return [torch.zeros((S, V, K, 2)), torch.zeros((P, 2), dtype=torch.int32), ia, ib, n, None, np.zeros((S, V, 3, 3)), np.zeros((S, V, 3, 3)),
            np.zeros((S, V, 3))]


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, verification as ver
    with pytest.raises(RuntimeError, match="tensors expected"):
        ver.filter_matches_batch(np.zeros((3, 5), np.int64), *_lists()[1:])
    for i, bad in ((1, torch.zeros((2, 3, 6), dtype=torch.int64)), (2, torch.zeros((2, 4), dtype=torch.int32)), (3, torch.ones((2, 3, 4), dtype=torch.uint8)),
                   (0, torch.zeros((5,), dtype=torch.int64))):
        a = _lists()
        a[i] = bad
        with pytest.raises(RuntimeError, match="expected idx_a"):
            ver.filter_matches_batch(*a)
    with pytest.raises(RuntimeError, match="one entry per list"):
        ver.filter_matches_batch(*_lists(), keep=torch.ones((2, 4), dtype=torch.uint8))
    for mk in (-1, 1.5, True):
        with pytest.raises(_lib.XFeatHipError, match="min_keep"):
            ver.filter_matches_batch(*_lists(), min_keep=mk)
    for i, bad in ((0, torch.zeros((2, 3, 5), dtype=torch.int32)), (2, torch.zeros((2, 3), dtype=torch.int64)), (3, torch.ones((2, 3, 5)))):
        a = _lists(cap=0)                                  # (dtypes are checked before the empty shape returns)
        a[i] = bad[..., :0] if bad.dim() == 3 else bad
        with pytest.raises(RuntimeError, match="must be a"):
            ver.filter_matches_batch(*a)
    with pytest.raises(RuntimeError, match="expected kpts"):
        ver.verify_matches_graph(torch.zeros((2, 3, 8, 3)), *_graph()[1:])
    with pytest.raises(_lib.XFeatHipError, match="V 33"):
        ver.verify_matches_graph(*_graph(V=33))
    with pytest.raises(_lib.XFeatHipError, match="V 1 "):
        ver.verify_matches_graph(*_graph(V=1))
    a = _graph()
    a[3] = torch.zeros((2, 3, 6), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="expected idx_a"):
        ver.verify_matches_graph(*a)
    a = _graph()
    a[1] = torch.zeros((4, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="expected view_pairs"):
        ver.verify_matches_graph(*a)
    for thr in (0.0, -1.0, NAN, float("inf")):
        with pytest.raises(_lib.XFeatHipError, match="max_epipolar_error"):
            ver.verify_matches_graph(*_graph(), max_epipolar_error=thr)
    a = _graph(cap=0)
    a[6] = np.zeros((2, 3, 3))
    with pytest.raises(RuntimeError, match="Ks must be"):
        ver.verify_matches_graph(*a)
    a = _graph(cap=0)
    a[5] = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="n_views must have"):
        ver.verify_matches_graph(*a)


def test_loud_failure_without_a_gpu():
    from accelerated_features_amd import _lib, verification as ver
    if torch.cuda.is_available():
        return                                             # (a GPU is present: tests/test_gpu_verification.py runs the functions)
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        ver.filter_matches_batch(*_lists())
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        ver.filter_matches_batch(*_lists(lead3=False))
    with pytest.raises(_lib.XFeatHipError, match="device-resident"):
        ver.verify_matches_graph(*_graph())


def test_the_empty_shapes_are_written_without_a_library_call():
    from accelerated_features_amd import verification as ver
    for kw in (dict(S=0), dict(P=0), dict(cap=0)):
        a = _lists(**kw)
        a[2] += 7                                          # counts are read clamped to [0, cap]
        shape = a[2].shape
        keep = torch.ones(shape, dtype=torch.uint8)
        if keep.numel():
            keep.view(-1)[0] = 0
        for mk in (0, 1):
            oa, ob, n, src, info = ver.filter_matches_batch(*a, keep=keep, min_keep=mk)
            assert oa.shape == a[0].shape and ob.shape == a[0].shape and src.shape == a[0].shape and src.dtype == torch.int32 and oa.dtype == torch.int64
            assert n.shape == shape and n.dtype == torch.int32 and not n.any() and info.shape == shape + (4,)
            if info.numel():                               # cap = 0: nothing read, nothing set; keep empties first, then min_keep
                want = torch.full(shape, 2 if mk else 0, dtype=torch.int32)
                want.view(-1)[0] = 1
                assert not info[..., 0].any() and not info[..., 1].any() and torch.equal(info[..., 2], want) and not info[..., 3].any()
    for kw in (dict(S=0), dict(P=0), dict(cap=0), dict(K=0)):
        a = _graph(**kw)
        a[4] += 9
        mask, err, info = ver.verify_matches_graph(*a)
        S, P, cap = a[2].shape
        assert mask.shape == (S, P, cap) and mask.dtype == torch.uint8 and not mask.any()
        assert err.shape == (S, P, cap) and err.dtype == torch.float32 and bool(torch.isnan(err).all())
        assert info.shape == (S, P, 4) and info.dtype == torch.int32 and not info[..., 0].any() and not info[..., 2:].any()
        assert bool((info[..., 1] == min(9, cap)).all())
