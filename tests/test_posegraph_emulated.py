"""The pose-graph slice of csrc/k_triangulate.hip (behind the two-view, the views-solver and the bundle-solver slices of the same file and the
shared geometry of csrc/twoview_math.hpp) compiled for the HOST (tests/emu/posegraph_emu.cpp, fp contraction off) against the numpy
restatement tests/posegraph_reference.py: the tree, the residuals, the first Laplacian and the first position system, their Cholesky solves
and the whole runs must be equal bit for bit, for V in {2, 3, 8, 32}, P in {1, 3, 28, 496} and 600 with duplicates, with outliers, an
unregistered view, a failing pivot and a failing pivot ratio."""
import subprocess

import numpy as np
import pytest

import posegraph_reference as PR
import posegraph_support as PS
import twoview_support as TS

BEGIN, END = "// ---- pose graph begin", "// ---- pose graph end"
TRI, NPOS = 4371, 93


def _slice():
    two = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    _, views = TS._between("k_triangulate.hip", "// ---- views solver begin", "// ---- views solver end")
    _, bundle = TS._between("k_triangulate.hip", "// ---- bundle solver begin", "// ---- bundle solver end")
    _, graph = TS._between("k_triangulate.hip", BEGIN, END)
    for s in (views, bundle, graph):
        assert "__shared__" not in s and "asm" not in s and "__builtin_amdgcn" not in s
    return two + (views + bundle + graph).replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("posegraph_slice.hpp", "posegraph_emu", _slice())


def test_the_slice_is_what_the_issue_asks_of_the_device_code():
    text = open(TS.CSRC + "/k_triangulate.hip").read()
    _, graph = TS._between("k_triangulate.hip", BEGIN, END)
    assert "#pragma clang fp contract(off)" in text and text.index("#pragma clang fp contract(off)") < text.index(BEGIN)
    for word in ("__shared__", "asm", "builtin", "sin(", "cos(", "acos(", "atan", "tan(", "pow(", "exp(", "log(", "atomic", "threadIdx", "__syncthreads"):
        assert word not in graph, word
    # the bundle solver's functions are called where they are, not duplicated
    for name in ("ba_cholesky_solve(", "ba_pose_update("):
        assert name in graph and ("bool " + name not in graph) and ("void " + name not in graph), name
    assert text.index("// ---- bundle solver end") < text.index(BEGIN) < text.index(END)
    assert text.count("bool ba_cholesky_solve(") == 1 and text.count("void ba_pose_update(") == 1
    assert text.index("bool ba_cholesky_solve(") < text.index("// ---- bundle solver end")
    # one kernel, one workgroup of 256 per scene
    assert text.count("pose_graph_kernel<<<S, 256, 0, st>>>") == 1 and text.count("void pose_graph_kernel(") == 1


def _record(sc, kw):
    P = sc["pairs"].shape[0]
    rec = np.concatenate([sc["pairs"].astype(np.float64), sc["Rrel"].reshape(P, 9), sc["trel"], sc["weight"][:, None]], axis=1)
    head = [sc["V"], sc.get("n_views", sc["V"]), P, kw["iterations"], kw["redescend"], kw["rot_scale_rad"], kw["pos_scale_sin"], kw["min_pivot_ratio"]]
    return np.concatenate([np.array(head, np.float64), rec.reshape(-1)])


def _cases():
    """(name, scene, settings)"""
    base = dict(PS.DEFAULTS, min_pivot_ratio=1e-8)
    short = dict(base, iterations=6, redescend=2)
    out = [("V2 P1", PS.scene(1, 2, PS.all_pairs(2), 0.5), base), ("V3 P3", PS.scene(2, 3, PS.all_pairs(3), 0.5), base),
           ("V8 P28", PS.scene(3, 8, PS.all_pairs(8), 0.5), base), ("V32 P496", PS.scene(4, 32, PS.all_pairs(32), 0.5), short),
           ("V32 P600 duplicates", PS.repeat_edges(PS.scene(5, 32, PS.all_pairs(32), 0.5), 600), short),
           ("V8 outliers", PS.scene(1, 8, PS.all_pairs(8), 0.5, 0.15), base), ("V32 outliers", PS.scene(1, 32, PS.all_pairs(32), 0.5, 0.15), short),
           ("V8 near", PS.scene(6, 8, PS.near_pairs(8), 0.5), dict(base, redescend=0)), ("V8 chain: failing pivot", PS.scene(7, 8, PS.chain_pairs(8), 0.5), base),
           ("two triangles: failing ratio", PS.scene(2, 5, PS.TWO_TRIANGLES), base)]
    sc = PS.scene(8, 8, PS.all_pairs(8), 0.5)
    sc["weight"][(sc["pairs"] == 5).any(axis=1)] = 0.0
    out.append(("V8 unregistered view 5", sc, base))
    sc = PS.swap_edges(PS.scene(9, 8, PS.all_pairs(8), 0.5), [1, 4, 9])
    sc["n_views"] = 6
    sc["Rrel"][3, 1, 1] = np.nan
    sc["trel"][5] = 0.0
    sc["weight"][7] = np.inf
    sc["pairs"][11] = (2, 2)
    out.append(("V8 ragged, swapped, bad edges", sc, base))
    sc = PS.scene(10, 4, PS.all_pairs(4), 0.5)
    sc["weight"][(sc["pairs"] == 0).any(axis=1)] = -1.0
    out.append(("V4 nothing at view 0", sc, base))
    return out


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64).reshape(-1), np.ascontiguousarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(got) & np.isnan(want)
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)) & ~nan)[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _packed(L):
    n = L.shape[0]
    return np.concatenate([L[i, :i + 1] for i in range(n)]) if n else np.zeros(0)


def test_stages_and_runs_equal_the_restatement_bit_for_bit(emu_bin):
    cases = _cases()
    blob = np.array([len(cases)], np.int32).tobytes() + b"".join(_record(sc, kw).tobytes() for _, sc, kw in cases)
    out = np.frombuffer(subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout, np.float64)
    at = 0
    seen = dict(status0=0, status1=0, status2=0, unregistered=0, rot_flagged=0, pos_flagged=0, failed_pivot=0, failed_ratio=0, cauchy=0)
    for name, sc, kw in cases:
        V, P = sc["V"], sc["pairs"].shape[0]
        w = PR.average_poses(sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"], sc.get("n_views", V), V, **kw)
        d, nr = w["dump"], len(w["views"])

        def take(m):
            nonlocal at
            at += m
            return out[at - m:at]
        tree = take(32).astype(int)
        assert list(tree[:len(w["tree"])]) == w["tree"] and (tree[len(w["tree"]):] == -1).all(), (name, tree, w["tree"])
        assert int(take(1)[0]) == w["registered"] and int(take(1)[0]) == nr, name
        _eq(take(288), d["rot_tree"], name + " tree rotations")
        res, fac, lap, sol, dirs, pos, flags, cen = take(3 * P), take(P), take(592), take(96), take(3 * P), take(TRI + NPOS), take(3), take(96)
        if nr > 0:
            ea, ep = np.nonzero(w["active"])[0], np.nonzero(w["active"] & w["hasdir"])[0]
            want = np.zeros((P, 3)); want[ea] = d["rot_res"]
            _eq(res, want, name + " rotation residuals")
            want = np.zeros(P); want[ea] = d["rot_factor"]
            _eq(fac, want, name + " rotation factors")
            _eq(lap[:nr * (nr + 1) // 2], _packed(d["lap"]), name + " laplacian")
            rhs = np.zeros((3, 32)); rhs[:, :nr] = d["lap_rhs"].T
            _eq(lap[496:], rhs, name + " laplacian rhs")
            assert d["lap_ok"], name
            s3 = np.zeros((3, 32)); s3[:, :nr] = d["lap_sol"].T
            _eq(sol, s3, name + " laplacian solve")
            want = np.zeros((P, 3)); want[ep] = d["pos_dir"]
            _eq(dirs, want, name + " directions")
            n = 3 * nr
            _eq(pos[:n * (n + 1) // 2], _packed(d["pos_M"]), name + " position system")
            _eq(pos[TRI:TRI + n], d["pos_g"], name + " position g")
            _eq(flags[1:2], [d["pos_mu"]], name + " mu")
            ok0 = bool(d.get("pos_ok")) and w["ratios"][0] >= kw["min_pivot_ratio"]
            assert bool(flags[0]) == ok0, (name, flags, w["ratios"][:1])
            _eq(flags[2:3], w["ratios"][:1], name + " pivot ratio")
            if ok0:
                _eq(cen, d["pos_cen"], name + " position solve")
            seen["failed_pivot"] += int(not d.get("pos_ok"))
            seen["failed_ratio"] += int(bool(d.get("pos_ok")) and not ok0)
        info = take(8).astype(int)
        assert list(info) == list(w["info"]), (name, info, w["info"])
        assert int(take(1)[0]) == w["registered"], name
        _eq(take(V * 9), w["Rs"], name + " Rs")
        _eq(take(V * 3), w["ts"], name + " ts")
        _eq(take(P * 2), w["edge_factor"], name + " factors")
        seen["status%d" % info[6]] += 1
        seen["unregistered"] += int(info[1] < sc.get("n_views", V))
        seen["rot_flagged"] += int(info[3]); seen["pos_flagged"] += int(info[4]); seen["cauchy"] += int(kw["redescend"] > 0)
    assert at == out.size
    assert all(v > 0 for v in seen.values()), seen
