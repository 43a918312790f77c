"""The retrieval slice of csrc/k_retrieval.hip compiled for the host with tests/emu (tests/emu/retrieval_emu.cpp: one thread per work-item, the
row-of-16 DPP exchanges of emu.hpp, fp contraction off) against the numpy restatement tests/retrieval_reference.py: every output of xfh_vlad,
xfh_kmeans_step, xfh_retrieve_topk and xfh_pairs_from_shortlists bit for bit.  The same program also runs under AddressSanitizer and UBSan
as a stand-alone program."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import retrieval_reference as RR
import retrieval_support as RS
import twoview_support as TS
from retrieval_support import bits

BEGIN, END = "// ---- retrieval begin", "// ---- retrieval end"


def _slice():
    text, src = TS._between("k_retrieval.hip", BEGIN, END)
    assert "asm" not in src and text.index("#pragma clang fp contract(off)") < text.index(BEGIN)
    for word in ("rsqrt", "fmaf", "__frcp", "__fdividef", "expf", "logf", "powf", "atomicAdd(a.", "atomicAdd(&a.", "unsafeAtomic", "mfma"):
        assert word not in src, word
    return src.replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("retrieval_slice.hpp", "retrieval_emu", _slice())


def _run(binary, blob, spec):
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=900)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-2000:])
    out, o, got = r.stdout, 0, {}
    for name, dt, shape in spec:
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        got[name] = np.frombuffer(out[o:o + n], dt).reshape(shape)
        o += n
    assert o == len(out)
    return got


def run_clusters(binary, mode, desc, counts, cb):
    G, K = desc.shape[:2]
    C = len(cb)
    blob = np.array([mode, G, K, C, int(counts is not None)], np.int32).tobytes() + desc.tobytes() + (counts.tobytes() if counts is not None else b"") + cb.tobytes()
    if mode == 0:
        spec = (("vlad", np.float32, (G, C * 64)), ("assign", np.int32, (G, K)), ("n_assigned", np.int32, (G, C)), ("info", np.int32, (G, 4)))
    else:
        spec = (("codebook", np.float32, (C, 64)), ("assign", np.int32, (G, K)), ("n_assigned", np.int32, (C,)), ("objective", np.float64, ()),
                ("info", np.int32, (4,)))
    return _run(binary, blob, spec)


def run_topk(binary, q, db, n_db, k, exclude_self):
    G, Q, D = q.shape
    N = db.shape[1]
    blob = np.array([2, G, Q, N, D, k, int(exclude_self), int(n_db is not None)], np.int32).tobytes() + q.tobytes() + db.tobytes()
    blob += n_db.tobytes() if n_db is not None else b""
    return _run(binary, blob, (("idx", np.int32, (G, Q, k)), ("score", np.float32, (G, Q, k))))


def run_pairs(binary, idx, n_views):
    S, V, k = idx.shape
    blob = np.array([3, S, V, k, int(n_views is not None)], np.int32).tobytes() + idx.tobytes() + (n_views.tobytes() if n_views is not None else b"")
    return _run(binary, blob, (("view_pairs", np.int32, (S, RR.pair_capacity(V, k), 2)), ("n_pairs", np.int32, (S,))))


def same(got, want, keys):
    for key in keys:
        assert np.array_equal(bits(got[key]), bits(np.ascontiguousarray(want[key], got[key].dtype))), key


COUNTS = (0, 1, 31, 32, 33, 257)


@pytest.mark.parametrize("C", [32, 256])
def test_vlad_slice_equals_the_restatement_bit_for_bit(emu_bin, C):
    """K in {0, 1, 31, 32, 33, 257} valid rows (one group each, in a table of 257 rows), rows that are not finite among them."""
    rng = np.random.default_rng(C)
    desc, _, cb = RS.tables(rng, len(COUNTS), 257, C, ragged=False, bad_rows=0)
    counts = np.array(COUNTS, np.int32)
    desc[5, 7, 3], desc[5, 256, 63], desc[4, 0, 0], desc[2, 40, 1] = np.nan, np.inf, -np.inf, np.nan      # (the last one is beyond its count)
    cb[1] = cb[0]                                           # equal scores: the lower centroid wins
    got = run_clusters(emu_bin, 0, desc, counts, cb)
    want = RR.vlad(desc, counts, cb)
    same(got, want, ("assign", "n_assigned", "info", "vlad"))
    assert list(got["info"][0]) == [0, 0, 0, 1] and not got["vlad"][0].any() and (got["assign"][0] == -1).all()      # m = 0
    assert list(got["info"][5][:2]) == [255, 2] and list(got["info"][4][:2]) == [32, 1] and got["info"][2][1] == 0
    assert (got["assign"] != 1).all() and (got["assign"] == 0).any()
    n = np.linalg.norm(got["vlad"][5].astype(np.float64))
    assert abs(n - 1) < 1e-6
    RR.check_vlad(desc, counts, cb, got)


def test_vlad_over_more_than_one_chunk_and_without_counts(emu_bin):
    rng = np.random.default_rng(5)
    desc, _, cb = RS.tables(rng, 2, 2 * RR.CHUNK + 57, 32, ragged=False, bad_rows=2)
    got = run_clusters(emu_bin, 0, desc, None, cb)
    same(got, RR.vlad(desc, None, cb), ("assign", "n_assigned", "info", "vlad"))


@pytest.mark.parametrize("C", [32, 256])
def test_kmeans_step_slice_equals_the_restatement_bit_for_bit(emu_bin, C):
    rng = np.random.default_rng(10 + C)
    desc, counts, cb = RS.tables(rng, 5, 257, C)             # 1285 rows as one set: two chunks
    cb[3] = -cb[2]
    cb[C - 1] = np.nan                                     # a centroid no row can choose: it stays
    got = run_clusters(emu_bin, 1, desc, counts, cb)
    want = RR.kmeans_step(desc, counts, cb)
    same(got, want, ("assign", "n_assigned", "info", "codebook", "objective"))
    assert got["n_assigned"][C - 1] == 0 and got["info"][2] >= 1 and np.isnan(got["codebook"][C - 1]).all()
    RR.check_kmeans(desc, counts, cb, got)


@pytest.mark.parametrize("D,k,Ns", [(2048, 8, (1, 7, 8, 255, 256, 257)), (2048, 1, (1, 257)), (16384, 128, (127, 128, 257))])
def test_topk_slice_equals_the_restatement_bit_for_bit(emu_bin, D, k, Ns):
    """N in {1, k - 1, k, 255, 256, 257}, k in {1, 8, 128}, D in {2048, 16384}; duplicate rows, a NaN row, n_db below N, exclude_self."""
    rng = np.random.default_rng(D + k)
    for N in Ns:
        q, db = RS.global_vectors(rng, 2, 3, N, D)
        n_db = np.array([N, max(N - 2, 0)], np.int32)
        for excl, counts in ((0, n_db), (1, None)):
            got = run_topk(emu_bin, q, db, counts, k, excl)
            idx, score = RR.retrieve_topk(q, db, counts, k, excl)
            assert np.array_equal(got["idx"], idx) and np.array_equal(bits(got["score"]), bits(score)), (N, excl)
            for g in range(2):
                RR.check_topk(q[g], db[g], None if counts is None else counts[g], k, excl, got["idx"][g], got["score"][g])


def test_topk_with_more_queries_than_a_tile(emu_bin):
    rng = np.random.default_rng(3)
    q, db = RS.global_vectors(rng, 1, 70, 70, 64)
    got = run_topk(emu_bin, q, q.copy(), None, 5, 1)
    idx, score = RR.retrieve_topk(q, q, None, 5, 1)
    assert np.array_equal(got["idx"], idx) and np.array_equal(bits(got["score"]), bits(score))
    assert (got["idx"][0] != np.arange(70)[:, None]).all()


@pytest.mark.parametrize("V,k", [(2, 1), (2, 128), (32, 3), (32, 128)])
def test_pairs_slice_equals_the_restatement(emu_bin, V, k):
    rng = np.random.default_rng(V + k)
    idx, n_views = RS.shortlists(rng, 3, V, k)
    for counts in (n_views, None):
        got = run_pairs(emu_bin, idx, counts)
        for s in range(3):
            vp, n = RR.pairs(idx[s], None if counts is None else counts[s])
            assert got["n_pairs"][s] == n and np.array_equal(got["view_pairs"][s], vp), (s, V, k)


def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers():
    """AddressSanitizer and UBSan on the host build of the slice, as a program of its own (nothing is loaded into Python)."""
    if not os.path.exists(TS.CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, "retrieval_slice.hpp"), "w").write(_slice())
    exe = os.path.join(td, "retrieval_emu_san")
    subprocess.run([TS.CLANG, "-O1", "-g", "-w", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", td, "-I", TS.EMU, os.path.join(TS.EMU, "retrieval_emu.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(11)
    desc, counts, cb = RS.tables(rng, 3, 257, 32)
    same(run_clusters(exe, 0, desc, counts, cb), RR.vlad(desc, counts, cb), ("assign", "n_assigned", "info", "vlad"))
    same(run_clusters(exe, 1, desc, counts, cb), RR.kmeans_step(desc, counts, cb), ("assign", "n_assigned", "info", "codebook", "objective"))
    q, db = RS.global_vectors(rng, 2, 3, 65, 128)
    n_db = np.array([65, 1], np.int32)
    got = run_topk(exe, q, db, n_db, 8, 1)
    idx, score = RR.retrieve_topk(q, db, n_db, 8, 1)
    assert np.array_equal(got["idx"], idx) and np.array_equal(bits(got["score"]), bits(score))
    idx, n_views = RS.shortlists(rng, 2, 32, 128)
    got = run_pairs(exe, idx, n_views)
    for s in range(2):
        vp, n = RR.pairs(idx[s], n_views[s])
        assert got["n_pairs"][s] == n and np.array_equal(got["view_pairs"][s], vp)
