"""The solver slice of csrc/k_triangulate.hip (on the shared geometry of csrc/twoview_math.hpp) compiled for the HOST
(tests/emu/structure_emu.cpp, fp contraction off) against the numpy restatement tests/structure_reference.py: on noise-free, noisy,
random, degenerate and non-finite samples the points (as float32 bits), the status, the reprojection error, the gate quantities, the
four poses of an E, the counts and the winner must be equal bit for bit."""
import subprocess

import numpy as np
import pytest

import structure_reference as SR
import structure_support as SS
import twoview_support as TS


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("structure_slice.hpp", "structure_emu", TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end"))


def _run(emu_bin, mode, H, m, records):
    blob = np.array([mode, H, m], np.int32).tobytes() + np.ascontiguousarray(records, np.float64).tobytes()
    return subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout


def test_the_slice_is_what_the_issue_asks_of_the_device_code():
    src = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    text = open(TS.CSRC + "/k_triangulate.hip").read()
    assert "#pragma clang fp contract(off)" in text
    for word in ("sin(", "cos(", "acos(", "atan", "pow(", "exp(", "log("):
        assert word not in src, word


def test_triangulation_equals_the_restatement_bit_for_bit(emu_bin):
    rng = np.random.default_rng(2026)
    G, m = 120, 100                                        # 12 000 correspondences: 120 poses of 100
    groups = [SS.mixed_group(rng, g, m) for g in range(G)]
    rec = np.concatenate([SS.records(g) for g in groups])
    H = rec.shape[0]
    assert H == G * m
    out = _run(emu_bin, 0, H, 0, rec)
    st = np.frombuffer(out[:4 * H], np.int32)
    xe = np.frombuffer(out[4 * H:20 * H], np.uint32).reshape(H, 4)
    gate = np.frombuffer(out[20 * H:], np.uint64).reshape(H, 4)
    seen = np.zeros(7, int)
    for k, g in enumerate(groups):
        w = SR.triangulate(g["p0"], g["p1"], g["K0"], g["K1"], g["R"], g["t"], g["thr"], g["deg"], g["max_depth"], g["mask"])
        s = slice(k * m, (k + 1) * m)
        assert np.array_equal(st[s], w["status"]), (k, np.nonzero(st[s] != w["status"])[0][:5])
        assert np.array_equal(xe[s, :3], w["points3d"].view(np.uint32)), k
        assert np.array_equal(xe[s, 3], w["reproj_error"].view(np.uint32)), k
        want_gate = np.stack([w["l0"], w["l1"], w["e2"], w["cos"]], axis=1)
        decided = w["status"] != SR.MASKED                 # (every row computes them; compare them all as bits but NaN payloads)
        a, b = gate[s][decided], want_gate.view(np.uint64)[decided]
        both_nan = np.isnan(a.view(np.float64)) & np.isnan(b.view(np.float64))
        assert np.array_equal(a[~both_nan], b[~both_nan]), k
        seen += np.bincount(w["status"], minlength=7)
    assert (seen > 50).all(), seen                         # every status is exercised
    assert seen[0] > 3000


def test_decomposition_and_vote_equal_the_restatement_bit_for_bit(emu_bin):
    rng = np.random.default_rng(7)
    H, m = 600, 20
    cases = [SS.recover_case(rng, h, m) for h in range(H)]
    rec = np.stack([np.concatenate([c["E"].reshape(9), SR.calibration(c["K0"], c["K1"]), [c["thr"]],
                                    np.c_[c["p0"], c["p1"]].astype(np.float64).reshape(-1)]) for c in cases])
    out = _run(emu_bin, 1, H, m, rec)
    iv = np.frombuffer(out[:24 * H], np.int32).reshape(H, 6)
    dv = np.frombuffer(out[24 * H:], np.uint64).reshape(H, 30)
    n_usable = n_true = 0
    for h, c in enumerate(cases):
        w = SR.recover_pose(c["E"], c["p0"], c["p1"], c["K0"], c["K1"], c["thr"])
        assert bool(iv[h, 0]) == w["usable"], h
        if not w["usable"]:
            assert list(w["good"]) == [0, 0, 0, 0] and not w["found"]
            continue
        n_usable += 1
        Ra, Rb, t = w["poses"]
        assert np.array_equal(dv[h, :9], Ra.view(np.uint64)) and np.array_equal(dv[h, 9:18], Rb.view(np.uint64)), h
        assert np.array_equal(dv[h, 18:21], t.view(np.uint64)), h
        assert list(iv[h, 1:5]) == list(w["good"]), (h, iv[h], w["good"])
        assert iv[h, 5] == SR.winner(list(w["good"])), h
        if c["truth"] is not None and w["found"]:
            n_true += np.abs(w["R"] - c["truth"][0]).max() < 1e-9
    assert n_usable > 0.7 * H and n_true > 0.4 * H
