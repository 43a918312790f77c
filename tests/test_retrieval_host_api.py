"""Host-side checks of the retrieval entries of the C ABI and of their Python wrappers: the exported symbols, the argument checks (which return
before any launch: the pointers below are never dereferenced), the header as strict C, the workspace functions, the wrappers' errors, the
shapes that need no library call and the loud failure without a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("xfh_vlad_workspace_bytes", "size_t"), ("xfh_vlad", "int"), ("xfh_kmeans_workspace_bytes", "size_t"), ("xfh_kmeans_step", "int"),
         ("xfh_retrieve_workspace_bytes", "size_t"), ("xfh_retrieve_topk", "int"), ("xfh_pairs_from_shortlists", "int"))
ARG, WORKSPACE, UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_the_entries_are_exported_bound_and_declared(lib):
    from accelerated_features_amd import _lib
    import accelerated_features_amd as pkg
    from accelerated_features_amd import retrieval as rt
    hdr = open(os.path.join(ROOT, "include", "xfeat_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, ret in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b%s %s\(" % (ret, name), hdr), name
    assert [len(_lib.SIGNATURES[n][1]) for n, _ in NAMES] == [3, 13, 3, 14, 3, 14, 8]
    assert lib.xfh_version() == 303                        # (entries were added, nothing changed)
    for name in ("train_codebook", "global_descriptors_batch", "retrieve_topk", "select_pairs"):
        assert getattr(pkg, name) is getattr(rt, name)
    p = inspect.signature(rt.train_codebook).parameters
    assert list(p) == ["desc", "counts", "n_centroids", "iterations", "init"]
    assert [p[k].default for k in ("counts", "n_centroids", "iterations", "init")] == [None, 64, 10, None]
    assert list(inspect.signature(rt.global_descriptors_batch).parameters) == ["desc", "counts", "codebook"]
    p = inspect.signature(rt.retrieve_topk).parameters
    assert list(p) == ["query", "database", "k", "n_database", "exclude_self"] and p["n_database"].default is None and p["exclude_self"].default is False
    p = inspect.signature(rt.select_pairs).parameters
    assert list(p) == ["vlad", "n_views", "k"] and p["k"].default == 4
    assert rt.WORKSPACE_LIMIT == 512 << 20 and rt.CODEBOOK_SIZES == (32, 64, 128, 256)
    src = open(os.path.join(ROOT, "accelerated_features_amd", "csrc", "k_retrieval.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "Triton" not in src and "atomicAdd(a." not in src


def test_the_header_still_compiles_as_strict_c(tmp_path):
    cc = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(cc):
        pytest.skip("no host clang")
    src = tmp_path / "use.c"
    src.write_text('#include "xfeat_hip.h"\nint main(void) { int (*f)(void) = (int (*)(void))0;\n'
                   'size_t n = f ? xfh_vlad_workspace_bytes(1, 1, 32) + xfh_kmeans_workspace_bytes(1, 1, 32) + xfh_retrieve_workspace_bytes(1, 1, 1) : 0;\n'
                   'int (*g)(const int32_t*, const int32_t*, int, int, int, int32_t*, int32_t*, xfh_stream) = xfh_pairs_from_shortlists;\n'
                   'return (int)n + (g == 0) + (&xfh_vlad == 0) + (&xfh_kmeans_step == 0) + (&xfh_retrieve_topk == 0); }\n')
    subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_the_workspaces_grow_with_the_call_and_are_zero_for_a_bad_shape(lib):
    for f, rows in ((lib.xfh_vlad_workspace_bytes, 1 << 24), (lib.xfh_kmeans_workspace_bytes, 1 << 22)):
        assert f(0, 16, 32) == 0 and f(65536, 16, 32) == 0 and f(1, 0, 32) == 0 and f(1, rows + 1, 32) == 0 and f(2, rows // 2 + 1, 32) == 0
        assert f(1, 16, 0) == 0 and f(1, 16, 33) == 0 and f(1, 16, 512) == 0 and f(1, 16, 16) == 0
        a, b, c, d = f(1, 1024, 32), f(2, 1024, 32), f(1, 2048, 32), f(1, 1024, 64)
        assert 0 < a < b and a < c and a < d and a % 256 == 0 and a >= 32 * 256 + 1024
        assert f(1, rows, 256) > 0
    assert lib.xfh_vlad_workspace_bytes(64, 4096, 64) < (512 << 20)      # the batch of tools/retrieve_time.py fits one call
    f = lib.xfh_retrieve_workspace_bytes
    assert f(0, 1, 1) == 0 and f(65536, 1, 1) == 0 and f(1, 0, 1) == 0 and f(1, 1, 0) == 0 and f(1, 1, (1 << 24) + 1) == 0 and f(1, (1 << 24) + 1, 1) == 0
    assert f(1, 1 << 20, 1 << 20) == 0                      # more scores than one call holds
    assert f(1, 64, 65536) == 64 * 65536 * 4 and 0 < f(1, 3, 5) < f(2, 30, 50) < f(2, 30, 100) and f(1, 3, 5) % 256 == 0


def test_argument_errors_return_before_any_launch(lib):
    x = C.c_void_p(256)                                             # never dereferenced: every call below fails its argument checks first

    def clusters(fn, extra):
        def call(desc=x, cb=x, out=C.c_void_p(512), assign=x, n=x, info=x, G=2, K=100, C_=32, ws=x, nbytes=1 << 30, **kw):
            more = [kw.get(k, x) for k in extra]
            return fn(desc, None, G, K, cb, C_, out, assign, n, *more, info, ws, nbytes, None)
        return call

    for call, rows, extra in ((clusters(lib.xfh_vlad, ()), 1 << 24, ()), (clusters(lib.xfh_kmeans_step, ("objective",)), 1 << 22, ("objective",))):
        for kw in (dict(desc=None), dict(cb=None), dict(out=None), dict(assign=None), dict(n=None), dict(info=None), dict(G=0), dict(G=65536), dict(K=0),
                   dict(G=1, K=rows + 1), dict(C_=0), dict(C_=-32), dict(desc=C.c_void_p(260)), dict(cb=C.c_void_p(264)), dict(out=C.c_void_p(260))) + \
                tuple(dict({k: None}) for k in extra):
            assert call(**kw) == ARG, kw
            assert lib.xfh_last_error()
        for c in (16, 33, 48, 512):
            assert call(C_=c) == UNSUPPORTED and b"is not 32, 64, 128 or 256" in lib.xfh_last_error()
        for kw in (dict(ws=None), dict(ws=C.c_void_p(264)), dict(nbytes=64)):
            assert call(**kw) == WORKSPACE, kw
    km = clusters(lib.xfh_kmeans_step, ("objective",))
    assert km(out=x, cb=x) == ARG and b"must not be codebook" in lib.xfh_last_error()      # (x is both)
    assert km(objective=C.c_void_p(260), out=C.c_void_p(512)) == ARG and b"objective" in lib.xfh_last_error()

    def topk(q=x, db=x, idx=x, score=x, G=1, Q=4, N=100, D=2048, k=8, ws=x, nbytes=1 << 30):
        return lib.xfh_retrieve_topk(q, db, None, G, Q, N, D, k, 0, idx, score, ws, nbytes, None)

    for kw in (dict(q=None), dict(db=None), dict(idx=None), dict(score=None), dict(G=0), dict(G=65536), dict(Q=0), dict(N=0), dict(N=(1 << 24) + 1), dict(D=0),
               dict(D=63), dict(D=100), dict(D=-64), dict(k=0), dict(k=-1), dict(q=C.c_void_p(260)), dict(db=C.c_void_p(264))):
        assert topk(**kw) == ARG, kw
    assert topk(D=16384 + 64) == UNSUPPORTED and b"D 16448 above 16384" in lib.xfh_last_error()
    assert topk(k=129) == UNSUPPORTED and b"k 129 above 128" in lib.xfh_last_error()
    assert topk(Q=1 << 20, N=1 << 20) == UNSUPPORTED
    for kw in (dict(ws=None), dict(ws=C.c_void_p(264)), dict(nbytes=64)):
        assert topk(**kw) == WORKSPACE, kw
    assert b"workspace too small" in lib.xfh_last_error()

    def pairs(idx=x, vp=x, n=x, S=1, V=8, k=3):
        return lib.xfh_pairs_from_shortlists(idx, None, S, V, k, vp, n, None)

    for kw in (dict(idx=None), dict(vp=None), dict(n=None), dict(S=0), dict(S=65536), dict(V=1), dict(V=0), dict(k=0)):
        assert pairs(**kw) == ARG, kw
    assert pairs(V=33) == UNSUPPORTED and b"V 33 above 32" in lib.xfh_last_error()
    assert pairs(k=129) == UNSUPPORTED


def test_python_argument_errors_raise_before_the_device_is_asked_for():
    from accelerated_features_amd import _lib, retrieval as rt
    d, cb = torch.zeros((2, 10, 64)), torch.zeros((32, 64))
    for fn in (lambda x: rt.train_codebook(x), lambda x: rt.global_descriptors_batch(x, None, cb)):
        for bad in (torch.zeros((2, 10, 63)), torch.zeros((2, 10, 64, 1)), torch.zeros(64)):
            with pytest.raises(RuntimeError, match="expected desc"):
                fn(bad)
    with pytest.raises(RuntimeError, match="one entry per group"):
        rt.train_codebook(d, counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="one entry per group"):
        rt.global_descriptors_batch(d, torch.zeros(3, dtype=torch.int32), cb)
    for kw in (dict(n_centroids=16), dict(n_centroids=100), dict(n_centroids=True), dict(iterations=0), dict(iterations=1001)):
        with pytest.raises(_lib.XFeatHipError):
            rt.train_codebook(d, **kw)
    with pytest.raises(RuntimeError, match="init must be"):
        rt.train_codebook(d, n_centroids=32, init=torch.zeros((64, 64)))
    with pytest.raises(_lib.XFeatHipError, match="no descriptor rows"):
        rt.train_codebook(torch.zeros((0, 10, 64)))
    with pytest.raises(_lib.XFeatHipError, match="training set"):
        rt.train_codebook(torch.zeros((1, 1, 64)).expand(1, (1 << 22) + 1, 64))
    with pytest.raises(RuntimeError, match="expected codebook"):
        rt.global_descriptors_batch(d, None, torch.zeros((32, 63)))
    with pytest.raises(_lib.XFeatHipError, match="codebook sizes"):
        rt.global_descriptors_batch(d, None, torch.zeros((48, 64)))
    q, db = torch.zeros((2, 3, 128)), torch.zeros((2, 5, 128))
    for a, b in ((q, torch.zeros((3, 5, 128))), (q, torch.zeros((2, 5, 64))), (torch.zeros(128), db), (q, torch.zeros((5, 128)))):
        with pytest.raises(RuntimeError, match="expected query"):
            rt.retrieve_topk(a, b, 2)
    with pytest.raises(RuntimeError, match="one entry per group"):
        rt.retrieve_topk(q, db, 2, n_database=torch.zeros(3, dtype=torch.int32))
    for k in (0, 129, True):
        with pytest.raises(_lib.XFeatHipError, match="outside"):
            rt.retrieve_topk(q, db, k)
    for D in (32, 100, 16384 + 64):
        with pytest.raises(_lib.XFeatHipError, match="multiple of 64"):
            rt.retrieve_topk(torch.zeros((1, D)), torch.zeros((1, D)), 1)
    with pytest.raises(RuntimeError, match="expected vlad"):
        rt.select_pairs(torch.zeros((4, 128)))
    for V in (1, 33):
        with pytest.raises(_lib.XFeatHipError, match="V %d" % V):
            rt.select_pairs(torch.zeros((2, V, 128)))
    with pytest.raises(_lib.XFeatHipError, match="outside"):
        rt.select_pairs(torch.zeros((2, 4, 128)), k=0)
    with pytest.raises(RuntimeError, match="one entry per scene"):
        rt.select_pairs(torch.zeros((2, 4, 128)), n_views=torch.zeros(3))
    with pytest.raises(RuntimeError, match="expected idx"):
        rt.pairs_from_shortlists(torch.zeros((4, 3), dtype=torch.int32))


def test_loud_failure_without_a_gpu():
    from accelerated_features_amd import _lib, retrieval as rt
    if torch.cuda.is_available():
        return                                             # (a GPU is present: tests/test_gpu_retrieval.py runs the functions)
    d, cb = torch.zeros((2, 10, 64)), torch.zeros((32, 64))
    for call in (lambda: rt.train_codebook(d, n_centroids=32), lambda: rt.global_descriptors_batch(d, None, cb), lambda: rt.kmeans_step(d, None, cb),
                 lambda: rt.retrieve_topk(torch.zeros((3, 128)), torch.zeros((5, 128)), 2), lambda: rt.select_pairs(torch.zeros((2, 4, 128))),
                 lambda: rt.pairs_from_shortlists(torch.zeros((2, 4, 3), dtype=torch.int32))):
        with pytest.raises(_lib.XFeatHipError, match="no CPU fallback"):
            call()


def test_the_empty_shapes_are_written_without_a_library_call():
    from accelerated_features_amd import retrieval as rt
    cb = torch.zeros((32, 64))
    for shape in ((0, 10, 64), (3, 0, 64)):
        out = rt.global_descriptors_batch(torch.zeros(shape), None, cb)
        G, K = shape[:2]
        assert out["vlad"].shape == (G, 32 * 64) and not out["vlad"].any() and out["assign"].shape == (G, K) and out["assign"].dtype == torch.int32
        assert out["n_assigned"].shape == (G, 32) and not out["n_assigned"].any() and out["info"].tolist() == [[0, 0, 0, 1]] * G
    for qs, ds, want in (((0, 3, 128), (0, 5, 128), (0, 3, 2)), ((2, 0, 128), (2, 5, 128), (2, 0, 2)), ((2, 3, 128), (2, 0, 128), (2, 3, 2))):
        out = rt.retrieve_topk(torch.zeros(qs), torch.zeros(ds), 2)
        assert out["idx"].shape == want and out["idx"].dtype == torch.int32 and bool((out["idx"] == -1).all())
        assert out["score"].shape == want and out["score"].dtype == torch.float32 and bool(torch.isnan(out["score"]).all())
    out = rt.retrieve_topk(torch.zeros((3, 128)), torch.zeros((0, 128)), 4)
    assert out["idx"].shape == (3, 4) and bool((out["idx"] == -1).all())
    out = rt.select_pairs(torch.zeros((0, 8, 128)), k=3)
    assert out["view_pairs"].shape == (0, 24, 2) and out["n_pairs"].shape == (0,) and out["neighbours"].shape == (0, 8, 3) and out["score"].shape == (0, 8, 3)
    assert rt.select_pairs(torch.zeros((0, 4, 128)), k=3)["view_pairs"].shape == (0, 6, 2)      # Pcap = min(V k, V (V - 1) / 2)
