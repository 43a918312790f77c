"""The map slice of csrc/k_map.hip compiled for the host with tests/emu (tests/emu/map_emu.cpp: one thread per work-item, the row-of-16 DPP
exchanges and the wave ballots of emu.hpp, fp contraction off) against the numpy restatement tests/localization_reference.py: every output of
xfh_build_map and xfh_map_project bit for bit.  The same program also runs under AddressSanitizer and UBSan as a stand-alone program."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import localization_reference as LR
import localization_support as LS
import twoview_support as TS
from localization_support import bits, check_build, check_project

BEGIN, END = "// ---- map begin", "// ---- map end"


def _slice():
    text, src = TS._between("k_map.hip", BEGIN, END)
    assert "asm" not in src and "atomicAdd(&cnt" in src           # (the only atomics are integer counters in LDS)
    assert text.index("#pragma clang fp contract(off)") < text.index(BEGIN)
    for word in ("rsqrt", "fmaf", "__frcp", "__fdividef", "sinf", "cosf", "expf", "logf", "powf", "atomicAdd(a.", "unsafeAtomic"):
        assert word not in src, word
    return src.replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("map_slice.hpp", "map_emu", _slice())


def run_build(binary, scenes, min_views, M):
    """scenes: a list of map_inputs tuples of one shape -> the outputs of the three launches per scene."""
    S = len(scenes)
    V, kcap = scenes[0][0].shape[:2]
    T = scenes[0][1].shape[0]
    blob = np.array([0, S, V, T, kcap, min_views, M], np.int32).tobytes()
    for i, dt in enumerate((np.float32, np.int32, np.float32, np.uint8, np.int32)):
        blob += b"".join(np.ascontiguousarray(sc[i], dt).tobytes() for sc in scenes)
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=900)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-2000:])
    out, o, got = r.stdout, 0, {}
    for name, dt, shape in (("points", np.float32, (S, M, 3)), ("desc", np.float32, (S, M, 64)), ("desc_f16", np.float16, (S, M, 64)),
                            ("track", np.int32, (S, M)), ("n_obs", np.uint8, (S, M)), ("coherence", np.float32, (S, M)), ("n_points", np.int32, (S,)),
                            ("info", np.int32, (S, 8))):
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        got[name] = np.frombuffer(out[o:o + n], dt).reshape(shape)
        o += n
    assert o == len(out)
    return got


@pytest.mark.parametrize("V", [2, 3, 32])
@pytest.mark.parametrize("kcap", [1, 64])
def test_build_map_slice_equals_the_restatement_bit_for_bit(emu_bin, V, kcap):
    rng = np.random.default_rng(100 * V + kcap)
    min_views = 1 if kcap == 1 else 2
    seen = np.zeros(8, np.int64)
    for T in (0, 1, 255, 256, 257, 1000):
        if T == 0:
            e = (np.zeros((V, kcap, 64), np.float32), np.zeros((0, V), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.int32))
            got = run_build(emu_bin, [e], min_views, 1)
            check_build(got, 0, LR.build_map(*e, min_views, 1))
            assert list(got["info"][0]) == [0] * 8 and got["track"][0, 0] == -1
            continue
        sc = LS.map_inputs(rng, V, T, kcap, view31=True)
        full = LR.build_map(*sc, min_views)
        info = full["info"]
        assert info[0] == T and info[1] + info[2:7].sum() == T and info[6] == 0
        if T >= 255:
            assert (info[1:6] > 0).all(), info              # selected tracks and every skip reason
            if V == 32:
                r = full["rows"]
                high = (sc[4] < 0) & (r["flag"] == LR.SELECTED)
                assert high.sum() > 0 and (LR.contributing(sc[0], sc[1], sc[4])[:, 31] & high).sum() > 0      # view 31 contributes somewhere
        for M in sorted({1, max(int(info[1]) - 1, 1), T}):
            got = run_build(emu_bin, [sc], min_views, M)
            want = LR.build_map(*sc, min_views, M)
            check_build(got, 0, want)
            seen += want["info"]
    assert seen[6] > 0                                      # rows dropped over capacity


def test_a_batch_of_scenes_and_the_order_of_the_other_tracks(emu_bin):
    rng = np.random.default_rng(7)
    scenes = [LS.map_inputs(rng, 3, 100, 16) for _ in range(3)]
    got = run_build(emu_bin, scenes, 2, 40)
    for s, sc in enumerate(scenes):
        check_build(got, s, LR.build_map(*sc, 2, 40))
    # the row of a track does not depend on what the other tracks hold: reverse the track order, the rows come out reversed
    sc = scenes[0]
    rev = (sc[0],) + tuple(np.ascontiguousarray(a[::-1]) for a in sc[1:])
    a, b = run_build(emu_bin, [sc], 2, 100), run_build(emu_bin, [rev], 2, 100)
    n = int(a["n_points"][0])
    assert n == int(b["n_points"][0]) and n > 10
    assert np.array_equal(99 - b["track"][0, :n][::-1], a["track"][0, :n])
    for k in ("desc", "desc_f16", "coherence", "points", "n_obs"):
        assert np.array_equal(bits(b[k][0, :n][::-1]), bits(a[k][0, :n])), k


def run_project(binary, pts, n, R, t, K, size):
    Q, M = pts.shape[:2]
    blob = np.array([1, Q, M, int(n is not None)], np.int32).tobytes() + np.array(size, np.float64).tobytes() + pts.tobytes()
    blob += (n.tobytes() if n is not None else b"") + R.tobytes() + t.tobytes() + K.tobytes()
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    return np.frombuffer(r.stdout, np.float32).reshape(Q, M, 2)


@pytest.mark.parametrize("M", [1, 257])
def test_map_project_slice_equals_the_restatement_bit_for_bit(emu_bin, M):
    rng = np.random.default_rng(M)
    pts, n, R, t, K = LS.project_case(rng, 3, M)
    for size, counts in (((0.0, 0.0, 0.0), n), ((640.0, 480.0, 12.0), n), ((640.0, 480.0, 0.0), None)):
        got = run_project(emu_bin, pts, counts, R, t, K, size)
        hit = check_project(got, pts, counts, R, t, K, size)
        assert np.isnan(got[1]).all() and (M == 1 or 0 < hit < 3 * M * 2)


def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers():
    """AddressSanitizer and UBSan on the host build of the slice, as a program of its own (nothing is loaded into Python)."""
    if not os.path.exists(TS.CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, "map_slice.hpp"), "w").write(_slice())
    exe = os.path.join(td, "map_emu_san")
    subprocess.run([TS.CLANG, "-O1", "-g", "-w", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", td, "-I", TS.EMU, os.path.join(TS.EMU, "map_emu.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(11)
    for V, T, kcap, M in ((3, 257, 64, 40), (32, 17, 1, 17), (2, 1, 1, 5)):
        sc = LS.map_inputs(rng, V, T, kcap, view31=True)
        check_build(run_build(exe, [sc, sc], 1, M), 1, LR.build_map(*sc, 1, M))
    pts, n, R, t, K = LS.project_case(rng, 2, 257)
    check_project(run_project(exe, pts, n, R, t, K, (640.0, 480.0, 3.0)), pts, n, R, t, K, (640.0, 480.0, 3.0))
