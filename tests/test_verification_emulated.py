"""The match-filter slice of csrc/k_matchfilter.hip and the match-verify slice of csrc/k_triangulate.hip (behind the solver and views-solver
slices of that file and the shared geometry of csrc/twoview_math.hpp) compiled for the host with tests/emu (tests/emu/verify_emu.cpp: one
thread per work-item, the wave ballots and barriers of emu.hpp, fp contraction off) against the numpy restatement
tests/verification_reference.py: every output of xfh_filter_matches and xfh_verify_matches bit for bit.  The same program also runs under
AddressSanitizer and UBSan as a stand-alone program."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import twoview_support as TS
import verification_reference as VR
import verification_support as VS

F_BEGIN, F_END = "// ---- match filter begin", "// ---- match filter end"
V_BEGIN, V_END = "// ---- match verify begin", "// ---- match verify end"


def _slice():
    two = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    _, views = TS._between("k_triangulate.hip", "// ---- views solver begin", "// ---- views solver end")
    text, verify = TS._between("k_triangulate.hip", V_BEGIN, V_END)
    _, filt = TS._between("k_matchfilter.hip", F_BEGIN, F_END)
    assert text.index("#pragma clang fp contract(off)") < text.index(V_BEGIN)
    assert text.index("// ---- pose graph end") < text.index(V_BEGIN)          # a slice of its own behind the pose-graph slice
    for src in (verify, filt):
        for word in ("asm", "atomic", "rsqrt", "fma(", "__frcp", "__fdividef", "sin(", "cos(", "exp(", "log(", "pow(", "unsafeAtomic"):
            assert word not in src, word
    for word in ("float", "double", "workspace"):               # integers only
        assert word not in filt, word
    # the verifier calls the functions of the slices above where they are
    for name in ("mv_stage_pose(", "mv_pair(", "tv::sampson("):
        assert name in verify and "void " + name not in verify and "double " + name.replace("tv::", "") not in verify, name
    return two + (views + verify + filt).replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("verify_slice.hpp", "verify_emu", _slice())


def run_filter(binary, ia, ib, n, mask, keep, min_keep):
    L, cap = ia.shape
    blob = np.array([0, L, cap, min_keep, int(keep is not None)], np.int32).tobytes()
    blob += ia.astype(np.int64).tobytes() + ib.astype(np.int64).tobytes() + n.astype(np.int32).tobytes() + mask.astype(np.uint8).tobytes()
    blob += keep.astype(np.uint8).tobytes() if keep is not None else b""
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-2000:])
    return _unpack(r.stdout, (("idx_a", np.int64, (L, cap)), ("idx_b", np.int64, (L, cap)), ("src", np.int32, (L, cap)), ("n", np.int32, (L,)),
                              ("info", np.int32, (L, 4))))


def run_verify(binary, b, max_err, with_nv=True, with_err=True):
    S, V, K = b["kpts"].shape[:3]
    P, cap = b["idx_a"].shape[1:]
    blob = np.array([1, S, P, cap, V, K, int(with_nv), int(with_err)], np.int32).tobytes() + np.array([max_err], np.float64).tobytes()
    blob += b["kpts"].astype(np.float32).tobytes() + b["view_pairs"].astype(np.int32).tobytes() + b["idx_a"].astype(np.int64).tobytes()
    blob += b["idx_b"].astype(np.int64).tobytes() + b["n_matches"].astype(np.int32).tobytes()
    blob += b["n_views"].astype(np.int32).tobytes() if with_nv else b""
    blob += b["Ks"].astype(np.float64).tobytes() + b["Rs"].astype(np.float64).tobytes() + b["ts"].astype(np.float64).tobytes()
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-2000:])
    return _unpack(r.stdout, (("mask", np.uint8, (S, P, cap)),) + ((("err", np.float32, (S, P, cap)),) if with_err else ()) +
                   (("info", np.int32, (S, P, 4)),))


def _unpack(out, fields):
    o, got = 0, {}
    for name, dt, shape in fields:
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        got[name] = np.frombuffer(out[o:o + nb], dt).reshape(shape)
        o += nb
    assert o == len(out)
    return got


def check_filter(got, want):
    for k in ("idx_a", "idx_b", "src", "n", "info"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def check_verify(got, want):
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["info"], want["info"]), (got["info"].reshape(-1, 4)[:8], want["info"].reshape(-1, 4)[:8])
    if "err" in got:
        assert VS.same_bits(got["err"], want["err"])


@pytest.mark.parametrize("cap", VS.CAPS)
@pytest.mark.parametrize("L", [1, 5])
def test_filter_slice_equals_the_restatement_byte_for_byte(emu_bin, cap, L):
    rng = np.random.default_rng(1000 * L + cap)
    for kind in ("random", "zeros", "ones"):
        ia, ib, n, mask = VS.filter_case(rng, L, cap, kind)
        if L == 1:
            n[0] = cap if kind != "random" else rng.integers(0, cap + 1)
        check_filter(run_filter(emu_bin, ia, ib, n, mask, None, 0), VR.filter_matches(ia, ib, n, mask))
    keep = (rng.random(L) < 0.6).astype(np.uint8)
    keep[L - 1] = 0 if L > 1 else keep[0]                   # (the first list stays: its count sets min_keep below)
    keep[0] = 1 if L > 1 else keep[0]
    count = int(VR.filter_matches(ia[:1], ib[:1], n[:1], mask[:1])["n"][0])
    seen = set()
    for mk in sorted({0, count, count + 1}):                # at the first list's count: kept; one above: emptied
        want = VR.filter_matches(ia, ib, n, mask, keep, mk)
        check_filter(run_filter(emu_bin, ia, ib, n, mask, keep, mk), want)
        seen |= set(want["info"][:, 2].tolist())
    want = VR.filter_matches(ia, ib, n, mask, None, count + 1)
    check_filter(run_filter(emu_bin, ia, ib, n, mask, None, count + 1), want)
    assert want["info"][0, 2] == VR.BY_MIN_KEEP and want["n"][0] == 0 and (want["idx_a"][0] == -1).all()
    assert VR.filter_matches(ia, ib, n, mask, None, count)["info"][0, 2] == VR.NONE
    if L == 5:
        assert seen >= {VR.NONE, VR.BY_KEEP}


@pytest.mark.parametrize("V", [2, 3, 32])
@pytest.mark.parametrize("K", [1, 64])
def test_verify_slice_equals_the_restatement_bit_for_bit(emu_bin, V, K):
    pairs = VS.TS.all_pairs(V) if V <= 3 else VS.TS.chain_pairs(V) + [(0, 31), (31, 0), (5, 17), (30, 2)]
    b = VS.verify_batch(100 * V + K, V, K, pairs)
    want = VS.verify_batch_reference(b, 1.0)
    VS.assert_clear_of_threshold(want["r2"], want["thr2"])
    st = want["info"][..., 0]
    assert {0, 1, 2, 3} <= set(st.reshape(-1).tolist())
    if K == 64:
        assert 0 < want["mask"].sum() < want["info"][..., 1].sum()              # entries kept and entries rejected
        ev = ~np.isnan(want["r2"])
        assert (ev.sum(axis=2)[st == 0] < want["info"][..., 1][st == 0]).any()    # entries not evaluated in an ok pair: rows and pixels
    check_verify(run_verify(emu_bin, b, 1.0), want)
    if (V, K) == (3, 64):                                   # no n_views, no err, another threshold
        nb = dict(b, n_views=np.full(4, V, np.int32))
        want = VS.verify_batch_reference(nb, 3.0)
        VS.assert_clear_of_threshold(want["r2"], want["thr2"])
        got = run_verify(emu_bin, b, 3.0, with_nv=False, with_err=False)
        assert "err" not in got
        check_verify(got, want)


def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers():
    """AddressSanitizer and UBSan on the host build of the slices, as a program of its own (nothing is loaded into Python)."""
    if not os.path.exists(TS.CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, "verify_slice.hpp"), "w").write(_slice())
    exe = os.path.join(td, "verify_emu_san")
    subprocess.run([TS.CLANG, "-O1", "-g", "-w", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", td, "-I", TS.EMU, os.path.join(TS.EMU, "verify_emu.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(5)
    for L, cap in ((3, 257), (1, 1), (4, 64)):
        ia, ib, n, mask = VS.filter_case(rng, L, cap)
        keep = (rng.random(L) < 0.6).astype(np.uint8)
        check_filter(run_filter(exe, ia, ib, n, mask, keep, 2), VR.filter_matches(ia, ib, n, mask, keep, 2))
    for V, K in ((3, 64), (32, 1)):
        b = VS.verify_batch(V + K, V, K, VS.TS.chain_pairs(V))
        check_verify(run_verify(exe, b, 1.0), VS.verify_batch_reference(b, 1.0))
