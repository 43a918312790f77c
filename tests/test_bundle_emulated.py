"""The bundle-solver slice of csrc/k_triangulate.hip (behind the two-view and the views-solver slices of the same file and the shared geometry
of csrc/twoview_math.hpp) compiled for the HOST (tests/emu/bundle_emu.cpp, fp contraction off; the driver adds in rs::block_sums' order)
against the numpy restatement tests/bundle_reference.py: the observation terms, the point blocks, the pair blocks of the reduced system, the
packed Cholesky solve, the pose and point updates of the first round and the whole runs must be equal bit for bit, for V in {2, 3, 8, 32} and
scenes with holes in the tables, a held view, a singular point block, a failing pivot and both loss settings."""
import subprocess

import numpy as np
import pytest

import bundle_reference as BR
import bundle_support as BS
import twoview_support as TS

BEGIN, END = "// ---- bundle solver begin", "// ---- bundle solver end"


def _slice():
    two = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    _, views = TS._between("k_triangulate.hip", "// ---- views solver begin", "// ---- views solver end")
    _, bundle = TS._between("k_triangulate.hip", BEGIN, END)
    for s in (views, bundle):
        assert "__shared__" not in s and "asm" not in s and "__builtin_amdgcn" not in s
    return two + (views + bundle).replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("bundle_slice.hpp", "bundle_emu", _slice())


def test_the_slice_is_what_the_issue_asks_of_the_device_code():
    text = open(TS.CSRC + "/k_triangulate.hip").read()
    _, bundle = TS._between("k_triangulate.hip", BEGIN, END)
    assert "#pragma clang fp contract(off)" in text and text.index("#pragma clang fp contract(off)") < text.index(BEGIN)
    assert "__shared__" not in bundle
    for word in ("sin(", "cos(", "acos(", "atan", "tan(", "pow(", "exp(", "log(", "atomic"):
        assert word not in bundle, word
    # the views solver's functions are called, not duplicated
    for name in ("mv_reproj(", "mv_step("):
        assert name in bundle and ("double " + name not in bundle) and ("void " + name not in bundle), name
    assert text.index("// ---- views solver end") < text.index(BEGIN) < text.index(END)
    assert text.count("double mv_reproj(") == 1 and text.count("void mv_step(") == 1


def _record(sc, fixed, iters, huber):
    V, K = sc["Rs"].shape[0], sc["tracks"].shape[0]
    cam = np.concatenate([np.concatenate([sc["Rs0"][v].reshape(9), sc["ts0"][v], sc["Ks"][v].reshape(9)]) for v in range(V)])
    t = sc["tracks"]
    kcap = sc["kpts"].shape[1]
    inr = (t >= 0) & (t < kcap)
    px = sc["kpts"].astype(np.float64)[np.arange(V)[None, :], np.where(inr, t, 0)]         # (K, V, 2)
    obs = np.concatenate([np.where(inr[..., None], px, 0.0), inr[..., None].astype(np.float64)], axis=2)
    inl = (sc["inlier_views"].astype(np.int64) & 0xFFFFFFFF).astype(np.float64)
    return np.concatenate([[V, sc["n_views"], K, fixed, iters, huber], cam, obs.reshape(-1), inl, sc["points3d"].astype(np.float64).reshape(-1)])


def _cases():
    """(name, scene, fixed_views, max_iterations, huber_px)"""
    inf = float("inf")
    out = []
    for i, (V, K) in enumerate(((2, 300), (3, 257), (8, 120), (32, 70))):
        fixed = 1 if V == 2 else 3
        out.append((f"plain V{V}", BS.scene(10 + i, V, K, fixed=fixed, holes=0.1 if V > 2 else 0.0), fixed, 6, 1.0 if i % 2 == 0 else inf))
    out.append(("squares V3", BS.scene(20, 3, 600, fixed=3, holes=0.1), 3, 6, inf))
    out.append(("view 0 only", BS.scene(21, 8, 100, fixed=1), 1, 5, 1.0))
    out.append(("fixed 0b101", BS.scene(22, 8, 90, fixed=5, holes=0.05), 5, 5, 1.0))
    out.append(("ragged", BS.scene(23, 8, 90, fixed=3, n_views=5), 3, 5, inf))
    out.append(("starved view", BS.starve_view(BS.scene(24, 8, 80, fixed=3), 4), 3, 5, 1.0))
    out.append(("singular point", BS.axis_scene(25, 60), 3, 5, 1.0))
    out.append(("failing pivot", BS.far_view_scene(26, 3, 80), 3, 4, inf))
    out.append(("every view fixed", BS.scene(27, 3, 50, fixed=7), 7, 3, 1.0))
    return out


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64).reshape(-1), np.ascontiguousarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(got) & np.isnan(want)
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)) & ~nan)[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def test_rounds_and_runs_equal_the_restatement_bit_for_bit(emu_bin):
    cases = _cases()
    blob = np.array([len(cases)], np.int32).tobytes() + b"".join(_record(sc, f, it, h).astype(np.float64).tobytes() for _, sc, f, it, h in cases)
    out = np.frombuffer(subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout, np.float64)
    at = 0
    seen = dict(held_point=0, failed_pivot=0, held_view=0, accepted=0, rejected=0, huber_far=0)
    for name, sc, fixed, iters, huber in cases:
        V, K = sc["Rs"].shape[0], sc["tracks"].shape[0]
        n, nv = 6 * V, sc["n_views"]
        take = lambda m: out[at:at + m]      # noqa: E731
        w = BS.run_reference(sc, fixed_views=fixed, max_iterations=iters, huber_px=huber)
        head = take(8); at += 8
        assert list(head[:6].astype(int)) == [w["info"][5], w["free_views"], w["info"][3], w["info"][4], w["info"][0], w["info"][1]], (name, head, w["info"])
        _eq(head[6:8], w["cost"], name + " cost")
        mask = np.zeros(K, np.int64)
        for v in range(nv):
            mask |= w["mask"][v].astype(np.int64) << v
        assert np.array_equal(take(K).astype(np.int64), mask), name
        at += K
        d = w["dump"]
        sizes = [K * V * 21, K * 10, n * n, n, 1, n, V * 12, K * 3, 2]
        parts = []
        for m in sizes:
            parts.append(take(m)); at += m
        if d is not None:
            terms = np.zeros((K, V, 21))
            for v in range(nv):
                t = d["terms"][v]
                row = np.stack([t["du"], t["dv"], t["wt"]] + t["jp"] + t["jc"], axis=1)
                terms[:, v] = np.where(w["mask"][v][:, None], row, 0.0)
            _eq(parts[0], terms, name + " terms")
            ref = np.any(w["mask"], axis=0)
            pv = np.where(ref[:, None], np.stack(d["Vi"] + d["g"] + [d["held"].astype(np.float64)], axis=1), 0.0)
            _eq(parts[1], pv, name + " point blocks")
            _eq(parts[2], d["S"], name + " pair blocks")
            _eq(parts[3], d["rhs"], name + " rhs")
            assert bool(parts[4][0]) == bool(d["ok"]), name
            if d["ok"]:
                _eq(parts[5], d["dcam"], name + " solve")
                _eq(parts[6], np.concatenate([d["Rn"], d["tn"]], axis=1), name + " pose update")
                _eq(parts[7], np.stack(d["Xn"], axis=1), name + " point update")
            _eq(parts[8][:1], [d["cand"]], name + " candidate cost")
            assert bool(parts[8][1]) == bool(d["failed"]), name
            seen["held_point"] += int((d["held"] & ref).sum())
            seen["failed_pivot"] += int(not d["ok"])
            seen["huber_far"] += int(sum(((d["terms"][v]["wt"] < 1.0) & w["mask"][v]).sum() for v in range(nv)))
        _eq(take(V * 12), np.concatenate([w["Rs"].reshape(V, 9), w["ts"]], axis=1), name + " poses"); at += V * 12
        _eq(take(K * 3), w["X"], name + " points"); at += K * 3
        got = take(K * 3).astype(np.float32); at += K * 3
        nan = np.isnan(got) & np.isnan(w["points3d"].reshape(-1))
        assert np.array_equal(got.view(np.uint32)[~nan], w["points3d"].reshape(-1).view(np.uint32)[~nan]), name
        seen["accepted"] += int(w["info"][4]); seen["rejected"] += int(w["info"][3] - w["info"][4])
        seen["held_view"] += int(any(not (w["free_views"] >> v) & 1 and not (fixed >> v) & 1 and v < nv for v in range(V)))
        # what the run must leave alone
        for v in range(V):
            if not (w["free_views"] >> v) & 1:
                assert np.array_equal(w["Rs"][v], sc["Rs0"][v]) and np.array_equal(w["ts"][v], sc["ts0"][v]), (name, v)
    assert at == out.size
    assert all(v > 0 for v in seen.values()), seen
