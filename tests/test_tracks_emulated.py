"""The two host-compilable slices of DESIGN.md 3.18 against the numpy restatement tests/tracks_reference.py.

The track-graph slice of csrc/k_tracks.hip (tests/emu/tracks_emu.cpp) runs with a plain minimum in the place of the atomic: the matches
forward, reversed and shuffled must give the restatement's labels, view masks, inconsistency flags, counters and tables, for V in {2, 3, 32}
and K in {1, 64, 300}, the zigzag (the deepest parent chain two views can make) included.

The views-solver slice of csrc/k_triangulate.hip anchored at the lowest observing view, mv_track<true> (tests/emu/tracks_anchor_emu.cpp, fp
contraction off; behind the two-view slice of the same file), must equal the restatement bit for bit on tests/multiview_support.mixed_scene's
eight kinds at V in {2, 3, 8, 32} with view 0's column emptied on a third of the tracks, and must equal the reference instantiation
mv_track<false> wherever the anchor is view 0."""
import subprocess

import numpy as np
import pytest

import multiview_reference as MR
import multiview_support as MS
import tracks_reference as TR
import tracks_support as TKS
import twoview_support as TS
from test_multiview_emulated import _record          # the scene record of tests/emu/multiview_emu.cpp, which tracks_anchor_emu.cpp reads too

G_BEGIN, G_END = "// ---- track graph begin", "// ---- track graph end"
V_BEGIN, V_END = "// ---- views solver begin", "// ---- views solver end"


@pytest.fixture(scope="module")
def graph_bin():
    _, src = TS._between("k_tracks.hip", G_BEGIN, G_END)
    assert "__shared__" not in src and "asm" not in src and "__builtin_amdgcn" not in src and "atomic" not in src
    return TS.build_emu("tracks_slice.hpp", "tracks_emu", src.replace("__device__ ", ""))


@pytest.fixture(scope="module")
def anchor_bin():
    two = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    _, views = TS._between("k_triangulate.hip", V_BEGIN, V_END)
    assert "__shared__" not in views and "asm" not in views and "__builtin_amdgcn" not in views
    return TS.build_emu("tracks_anchor_slice.hpp", "tracks_anchor_emu", two + views.replace("__device__ ", ""))


def test_the_slices_are_what_the_issue_asks_of_the_device_code():
    text = open(TS.CSRC + "/k_triangulate.hip").read()
    _, views = TS._between("k_triangulate.hip", V_BEGIN, V_END)
    assert text.index("#pragma clang fp contract(off)") < text.index("// ---- solver end") < text.index(V_BEGIN) < text.index(V_END)
    assert "__shared__" not in views and "asm" not in views and "__builtin_amdgcn" not in views
    for word in ("sin(", "cos(", "acos(", "atan", "pow(", "exp(", "log(", "atomic"):
        assert word not in views, word
    # one per-track function for both anchors: it calls the helpers of the two-view slice and of its own slice, and nothing is written twice
    track = views[views.index("MvResult mv_track("):]
    for name in ("tg_correct(", "tg_depths(", "tg_depth_status(", "mv_pair(", "mv_reproj(", "mv_normal(", "mv_step("):
        assert name in track, name
        for kind in ("inline TgRays ", "void ", "int ", "double "):
            assert kind + name not in track, name
    assert "tg_pose_E(" in views and "void tg_pose_E(" not in views
    for definition in ("double mv_reproj(", "double mv_normal(", "void mv_step(", "void mv_pair(", "void mv_stage_pose(", "void mv_stage_view(",
                       "MvResult mv_track("):
        assert text.count(definition) == 1, definition
    assert "mv_track_anchor" not in text and "mva_stage_view" not in text and "ba_stage_view" not in text
    graph = open(TS.CSRC + "/k_tracks.hip").read()
    _, g = TS._between("k_tracks.hip", G_BEGIN, G_END)
    for name in ("tk_union(", "tk_find(", "tk_see("):
        assert "template <class Mem>" in g and name in g and name in graph[graph.index(G_END):], name      # the kernels call the slice
    assert g.count("for (int step = 0; step < bound; ++step)") == 2 and "while" not in g and "goto" not in g      # every loop carries its bound
    assert "float" not in g and "double" not in g


def _run_graph(binary, lists, V, K, min_length=2, max_tracks=None):
    pairs, ia, ib, n = lists
    P, cap = ia.shape
    T = (V * K) // 2 if max_tracks is None else max_tracks
    head = np.array([V, K, P, cap, min_length, T], np.int64)
    pr = np.concatenate([np.asarray(pairs, np.int64).reshape(P, 2), np.asarray(n, np.int64).reshape(P, 1)], axis=1)
    blob = head.tobytes() + pr.tobytes() + np.ascontiguousarray(ia, np.int64).tobytes() + np.ascontiguousarray(ib, np.int64).tobytes()
    out = np.frombuffer(subprocess.run([binary], input=blob, capture_output=True, check=True, timeout=120).stdout, np.int32)
    N = V * K
    assert len(out) == 8 + 4 * N + T * V
    cut = np.split(out, [8, 8 + N, 8 + 2 * N, 8 + 3 * N, 8 + 4 * N])
    return dict(info=cut[0], label=cut[1], mask=cut[2].view(np.uint32), bad=cut[3].astype(bool), track_of=cut[4].reshape(V, K), tracks=cut[5].reshape(T, V))


def _orders(rng, lists):
    """The lists forward, reversed (pairs and matches) and shuffled (pairs and matches)."""
    pairs, ia, ib, n = lists
    P = len(n)
    yield lists
    ra, rb = ia.copy(), ib.copy()
    sa, sb = ia.copy(), ib.copy()
    for p in range(P):
        m = int(min(max(n[p], 0), ia.shape[1]))
        ra[p, :m], rb[p, :m] = ia[p, :m][::-1], ib[p, :m][::-1]
        o = rng.permutation(m)
        sa[p, :m], sb[p, :m] = ia[p, o], ib[p, o]
    yield pairs[::-1], ra[::-1], rb[::-1], n[::-1]
    o = rng.permutation(P)
    yield pairs[o], sa[o], sb[o], n[o]


def _check_graph(binary, rng, lists, V, K, **kw):
    want = TR.build_tracks_graph(*lists, V, K, **kw)
    for order in _orders(rng, lists):
        got = _run_graph(binary, order, V, K, **kw)
        for k in ("info", "label", "mask", "bad", "track_of", "tracks"):
            assert np.array_equal(got[k], want[k]), (k, V, K)
    return want


@pytest.mark.parametrize("V", [2, 3, 32])
@pytest.mark.parametrize("K", [1, 64, 300])
def test_track_graph_slice_equals_the_restatement_in_any_order(graph_bin, V, K):
    rng = np.random.default_rng(1000 * V + K)
    # a scene's own tracks over the chain and over all pairs, with a few wrong matches that merge tracks (inconsistent components), indices
    # and views out of range and a repeated pair
    for pairs in (TKS.chain_pairs(V), TKS.all_pairs(V)):
        vp, ia, ib, n = TKS.noisy_lists(rng, V, K, pairs, 0.03 if len(pairs) < 100 else 0.0005)
        w = _check_graph(graph_bin, rng, (vp, ia, ib, n), V, K)
        assert w["info"][6] == 0 and (K == 1 or w["info"][2] > 0)
        if K == 300:
            assert w["info"][3] > 0
            _check_graph(graph_bin, rng, (vp, ia, ib, n), V, K, min_length=min(3, V), max_tracks=40)
    # the zigzag between the views 0 and 1
    w = _check_graph(graph_bin, rng, TKS.zigzag(K), V, K)
    assert list(w["info"]) == ([2, 1, 1, 0, 0, 0, 0, 0] if K == 1 else [2 * K, 1, 0, 1, 0, 0, 0, 0])


def _blocks(out, H):
    iv = np.frombuffer(out[:16 * H], np.int32).reshape(H, 4)
    fv = np.frombuffer(out[16 * H:32 * H], np.uint32).reshape(H, 4)
    dv = np.frombuffer(out[32 * H:56 * H], np.uint64).reshape(H, 3)
    return iv, fv, dv


def test_anchored_tracks_equal_the_restatement_bit_for_bit(anchor_bin):
    rng = np.random.default_rng(2027)
    G = 64                                                 # 8 kinds x 4 view counts x 2 rounds
    scenes = []
    for g in range(G):
        V = MS.MIXED_V[g % 4]
        sc = MS.mixed_scene(rng, g, 40 if V == 32 else 90)
        sc["tracks"][g % 3::3, 0] = -1                     # view 0 does not see a third of the tracks
        if g % 7 == 3 and V > 2:
            sc["n_views"] = V - 1
        scenes.append(sc)
    blob = np.array([G], np.int32).tobytes() + b"".join(_record(sc, sc["Rs"].shape[0], sc["tracks"].shape[0]).astype(np.float64).tobytes() for sc in scenes)
    out = subprocess.run([anchor_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    H = sum(sc["tracks"].shape[0] for sc in scenes)
    assert len(out) == 2 * H * 56
    iv, fv, dv = _blocks(out, H)
    riv, rfv, rdv = _blocks(out[56 * H:], H)
    seen, seen_high, zero_n, a = np.zeros(7, int), np.zeros(7, int), 0, 0
    for g, sc in enumerate(scenes):
        m = sc["tracks"].shape[0]
        w = TR.triangulate_views(sc["kpts"], sc["tracks"], sc["n_views"], sc["Ks"], sc["Rs"], sc["ts"], sc["thr"], sc["deg"], sc["max_depth"], sc["min_views"])
        s = slice(a, a + m)
        a += m
        assert np.array_equal(iv[s, 0], w["status"]), (g, np.nonzero(iv[s, 0] != w["status"])[0][:5])
        assert np.array_equal(iv[s, 1], w["n_inliers"]) and np.array_equal(iv[s, 2], w["inlier_views"]), g
        assert np.array_equal(iv[s, 3], w["winner"]), g
        for got, want in ((fv[s, :3], w["points3d"]), (fv[s, 3], w["reproj_error"])):
            nan = np.isnan(got.view(np.float32)) & np.isnan(want)
            assert np.array_equal(got[~nan], want.view(np.uint32)[~nan]), g
        want = np.stack([w["score"], w["cost0"], w["cost1"]], axis=1)
        assert np.array_equal(dv[s], want.view(np.uint64)), (g, np.nonzero(dv[s] != want.view(np.uint64))[0][:5])
        assert (np.isnan(w["points3d"]).all(axis=1) == (w["status"] != 0)).all() and np.isfinite(w["points3d"][w["status"] == 0]).all()
        # wherever the anchor is view 0: the bits of mv_track<false> (NaN payloads included)
        zero = np.zeros(H, bool)
        zero[s] = w["anchor"] == 0
        assert np.array_equal(iv[zero], riv[zero]) and np.array_equal(dv[zero], rdv[zero]), g
        nan = np.isnan(fv[zero].view(np.float32)) & np.isnan(rfv[zero].view(np.float32))
        assert np.array_equal(fv[zero][~nan], rfv[zero][~nan]), g
        # every other track is unobserved for mv_track<false>
        assert (riv[s, 0][w["anchor"] != 0] == MR.UNOBSERVED).all(), g
        zero_n += int(zero.sum())
        seen += np.bincount(w["status"], minlength=7)
        seen_high += np.bincount(w["status"][w["anchor"] > 0], minlength=7)
    assert (seen > 50).all(), seen                         # every status is exercised,
    assert (np.delete(seen_high, MR.NOT_FINITE) > 5).all() and seen_high[0] > 300, seen_high      # also with an anchor above view 0 (but for
    # "not finite": the scenes' zero-baseline pair is (0, V - 1))
    assert zero_n > 2000
