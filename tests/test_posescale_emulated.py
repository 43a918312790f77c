"""The two slices of csrc/posescale_body.hpp (the baseline ratios of the wedges; the ratio terms of the position rounds) compiled for the HOST
behind the slices of csrc/k_triangulate.hip that they call into (tests/emu/posescale_emu.cpp, fp contraction off) against the numpy
restatement tests/posescale_reference.py: ratios, counts, shared views, info, the first position system with ratio terms, its solve and the
whole runs must be equal bit for bit, for V in {3, 8, 32}, K in {16, 400} and n in {0, 7, 8, 9, 255, 256, 257} common tracks.  The same program
built with AddressSanitizer and UBSan, stand-alone, must run clean."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import posegraph_support as PS
import posescale_reference as QR
import posescale_support as QS
import twoview_support as TS

TRI, NPOS = 4371, 93
GATES = dict(max_reproj_error=4.0, min_parallax_deg=1.0, max_depth=np.inf, min_common=8)


def _slice():
    two = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    parts = [TS._between("k_triangulate.hip", b, e)[1] for b, e in (("// ---- views solver begin", "// ---- views solver end"),
                                                                    ("// ---- bundle solver begin", "// ---- bundle solver end"),
                                                                    ("// ---- pose graph begin", "// ---- pose graph end"))]
    parts += [TS._between("posescale_body.hpp", b, e)[1] for b, e in (("// ---- pose scale begin", "// ---- pose scale end"),
                                                                     ("// ---- pose graph ratios begin", "// ---- pose graph ratios end"))]
    for s in parts:
        assert "__shared__" not in s and "asm" not in s and "__builtin_amdgcn" not in s
    return two + "".join(parts).replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("posescale_slice.hpp", "posescale_emu", _slice())


def test_the_slices_are_what_the_issue_asks_of_the_device_code():
    text = open(TS.CSRC + "/posescale_body.hpp").read()
    tri = open(TS.CSRC + "/k_triangulate.hip").read()
    assert tri.index("#pragma clang fp contract(off)") < tri.index('#include "posescale_body.hpp"') and tri.count('#include "posescale_body.hpp"') == 1
    for b, e in (("// ---- pose scale begin", "// ---- pose scale end"), ("// ---- pose graph ratios begin", "// ---- pose graph ratios end")):
        _, s = TS._between("posescale_body.hpp", b, e)
        for word in ("__shared__", "asm", "builtin", "sin(", "cos(", "acos(", "atan", "tan(", "pow(", "exp(", "log(", "fabs", "atomicAdd", "threadIdx",
                     "__syncthreads"):
            assert word not in s, word
    # called where they are, not copied
    for name in ("tg_point(", "tg_pose_E(", "tg_pose_ok(", "pg_edge_key(", "pg_factor(", "pg_slot("):
        copies = sum(text.count("inline %s %s" % (ty, name)) for ty in ("int", "void", "bool", "double"))
        assert name in text and copies == 0, name
    assert tri.count("int tg_point(") == 1 and tri.count("double pg_factor(") == 1 and tri.count("bool ba_cholesky_solve(") == 1
    # one workgroup of 256 per candidate; the pose graph with ratios one per scene
    assert text.count("baseline_ratio_kernel<<<dim3(P, P, S), 256, 0, st>>>") == 1 and text.count("pose_graph_ratio_kernel<<<S, 256, 0, st>>>") == 1


def common_tracks(sc, n):
    """The scene with exactly n tracks that have a key-point in every view (the first n that do); the others lose theirs in the last view."""
    full = np.nonzero((sc["tracks"] >= 0).all(axis=1))[0]
    assert len(full) >= n, (len(full), n)
    drop = full[n:]
    last = sc["V"] - 1
    sc["track_of"][last, sc["tracks"][drop, last]] = -1
    sc["tracks"][drop, last] = -1
    return sc


def _cases():
    """(name, scene, gates, settings)"""
    base = dict(QS.SETTINGS, **QS.SCALE)
    short = dict(base, iterations=6, redescend=2)
    out = []
    for K, ns in ((16, (0, 7, 8, 9)), (400, (0, 7, 8, 9, 255, 256, 257))):
        for n in ns:
            out.append(("V3 K%d n%d" % (K, n), common_tracks(QS.scene(10 + n, 3, K, PS.chain_pairs(3), 0.0, 0.0, 0.0), n), GATES, base))
    out.append(("V8 K16 chain", QS.scene(1, 8, 16, PS.chain_pairs(8), 0.0, 0.0, 0.0), dict(GATES, min_common=4), base))
    out.append(("V8 K400 chain, noisy", QS.scene(2, 8, 400, PS.chain_pairs(8)), dict(GATES, max_reproj_error=32.0), base))
    out.append(("V8 K400 strip, noisy", QS.scene(3, 8, 400, PS.near_pairs(8)), dict(GATES, max_reproj_error=32.0), dict(base, redescend=0)))
    out.append(("V5 K400 two triangles, noisy", QS.scene(4, 5, 400, PS.TWO_TRIANGLES), dict(GATES, max_reproj_error=32.0), base))
    out.append(("V32 K16 chain", QS.scene(5, 32, 16, PS.chain_pairs(32), 0.0, 0.0, 0.0), dict(GATES, min_common=4), short))
    out.append(("V32 K400 chain", QS.scene(6, 32, 400, PS.chain_pairs(32), 0.0, 0.0, 0.0), GATES, short))
    out.append(("V8 strip, a tight scale_tol", QS.scene(7, 8, 400, PS.near_pairs(8)), dict(GATES, max_reproj_error=32.0), dict(base, scale_tol=0.01)))
    sc = PS.swap_edges(QS.scene(8, 8, 400, PS.near_pairs(8), 0.5, 0.1), [1, 4, 9])
    sc["n_views"] = 7
    sc["Rrel"][3, 1, 1] = np.nan
    sc["trel"][5] = 0.0
    sc["pairs"][11] = (2, 2)
    sc["pairs"][12] = sc["pairs"][0]                          # a duplicate of edge 0: no wedge with it
    sc["Rrel"][12], sc["trel"][12] = sc["Rrel"][0], sc["trel"][0]
    out.append(("V8 ragged, swapped, bad edges, a duplicate", sc, dict(GATES, max_reproj_error=8.0, max_depth=9.0), base))
    return out


def record(sc, gates, kw):
    P, V, K = sc["pairs"].shape[0], sc["V"], sc["K"]
    rec = np.concatenate([sc["pairs"].astype(np.float64), sc["Rrel"].reshape(P, 9), sc["trel"], sc["weight"][:, None]], axis=1)
    head = [V, sc.get("n_views", V), P, K, sc["tracks"].shape[0], gates["min_common"], gates["max_reproj_error"],
            np.cos(np.radians(gates["min_parallax_deg"])), gates["max_depth"], kw["iterations"], kw["redescend"], kw["rot_scale_rad"], kw["pos_scale_sin"],
            kw["min_pivot_ratio"], kw["scale_weight"], kw["scale_tol"]]
    return np.concatenate([np.array(head, np.float64), rec.reshape(-1), sc["Ks"].reshape(-1), sc["kpts"].astype(np.float64).reshape(-1),
                           sc["tracks"].astype(np.float64).reshape(-1), sc["track_of"].astype(np.float64).reshape(-1)])


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64).reshape(-1), np.ascontiguousarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(got) & np.isnan(want)
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)) & ~nan)[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _packed(L):
    n = L.shape[0]
    return np.concatenate([L[i, :i + 1] for i in range(n)]) if n else np.zeros(0)


def blob(cases):
    return np.array([len(cases)], np.int32).tobytes() + b"".join(record(sc, g, kw).tobytes() for _, sc, g, kw in cases)


def test_ratios_stages_and_runs_equal_the_restatement_bit_for_bit(emu_bin):
    cases = _cases()
    out = np.frombuffer(subprocess.run([emu_bin], input=blob(cases), capture_output=True, check=True, timeout=600).stdout, np.float64)
    at = 0
    seen = dict(status0=0, status2=0, no_ratio=0, below=0, ratio=0, flagged=0, took_part=0, n256=0)
    for name, sc, gates, kw in cases:
        V, P = sc["V"], sc["pairs"].shape[0]
        r = QS.ratios(sc, **gates)
        pose = {k: v for k, v in kw.items()}
        w = QR.average_poses(sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc.get("n_views", V), V, ratio=r["ratio"], ratio_count=r["count"], **pose)
        d, nr = w["dump"], len(w["views"])

        def take(m):
            nonlocal at
            at += m
            return out[at - m:at]
        _eq(take(P * P), r["ratio"], name + " ratios")
        assert (take(P * P).astype(int) == r["count"].reshape(-1)).all(), name
        assert (take(P * P).astype(int) == r["shared_view"].reshape(-1)).all(), name
        assert list(take(8).astype(int)) == list(r["info"]), (name, r["info"])
        pos, flags, cen = take(TRI + NPOS), take(3), take(96)
        if nr > 0:
            n = 3 * nr
            _eq(pos[:n * (n + 1) // 2], _packed(d["pos_M"]), name + " position system")
            _eq(pos[TRI:TRI + n], d["pos_g"], name + " position g")
            _eq(flags[1:2], [d["pos_mu"]], name + " mu")
            ok0 = bool(d.get("pos_ok")) and w["ratios"][0] >= kw["min_pivot_ratio"]
            assert bool(flags[0]) == ok0, (name, flags, w["ratios"][:1])
            _eq(flags[2:3], w["ratios"][:1], name + " pivot ratio")
            if ok0:
                _eq(cen, d["pos_cen"], name + " position solve")
        info = take(8).astype(int)
        assert list(info) == list(w["info"]), (name, info, w["info"])
        assert int(take(1)[0]) == w["registered"], name
        _eq(take(V * 9), w["Rs"], name + " Rs")
        _eq(take(V * 3), w["ts"], name + " ts")
        _eq(take(P * 2), w["edge_factor"], name + " factors")
        _eq(take(P * P), w["ratio_factor"], name + " ratio factors")
        wedge = r["shared_view"] >= 0
        seen["status%d" % info[6]] += 1
        seen["no_ratio"] += int((wedge & np.isnan(r["ratio"])).sum())
        seen["below"] += int((wedge & (r["count"] > 0) & (r["count"] < gates["min_common"])).sum())
        seen["ratio"] += int(np.isfinite(r["ratio"]).sum())
        seen["took_part"] += len(w["wedges"][0])
        seen["flagged"] += int((w["ratio_factor"][w["wedges"]] < 0.5).sum()) if info[6] == 0 else 0
        seen["n256"] += int((r["count"] == 256).sum())
    assert at == out.size
    assert all(v > 0 for v in seen.values()), seen


def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers():
    """AddressSanitizer and UBSan on the host build of both slices, as a program of its own (nothing is loaded into Python)."""
    if not os.path.exists(TS.CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, "posescale_slice.hpp"), "w").write(_slice())
    exe = os.path.join(td, "posescale_emu_san")
    subprocess.run([TS.CLANG, "-O1", "-g", "-w", "-std=c++20", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", td, "-I", TS.EMU, os.path.join(TS.EMU, "posescale_emu.cpp"), "-o", exe], check=True)
    cases = [c for c in _cases() if c[0] in ("V3 K16 n0", "V3 K16 n8", "V3 K400 n257", "V8 K400 strip, noisy", "V8 ragged, swapped, bad edges, a duplicate")]
    assert len(cases) == 5
    r = subprocess.run([exe], input=blob(cases), capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
