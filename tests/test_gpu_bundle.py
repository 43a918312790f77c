"""xfh_bundle_adjust (csrc/k_triangulate.hip) on the MI355X against the numpy restatement tests/bundle_reference.py on the same inputs: info,
refined and free_views exactly, the poses and the costs to 1e-9 (the family's figure for R and t in tests/test_gpu_abspose.py and
tests/test_gpu_multiview.py), the points within one float32 ulp.  Every compared scene first asserts that no decision of its run (accept or
reject, the FTOL test, a pivot, a determinant, a Huber switch, a depth test) lies within relative 1e-9 of a tie
(bundle_reference.decision_margin), so a last-bit difference could not flip a discrete result."""
import numpy as np
import pytest
import torch

import abspose_reference as AR
import bundle_reference as BR
import bundle_support as BS
import multiview_reference as MR
from twoview_support import check_common

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def mv():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import multiview as m
    return m


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _clear_scene(make, seed, **kw):
    """The first scene of make(seed), make(seed + 1000), ... whose run in the restatement is clear of every tie."""
    for i in range(20):
        sc = make(seed + 1000 * i)
        want = BS.run_reference(sc, **kw)
        if BR.decision_margin(want) > 1e-9:
            return sc, want
    raise AssertionError("no scene clear of its ties in 20 draws")


def _run(mv, scenes, n_views=None, **kw):
    kp, tr, inl, X, Ks, Rs, ts = (np.stack([sc[k] for sc in scenes]) for k in ("kpts", "tracks", "inlier_views", "points3d", "Ks", "Rs0", "ts0"))
    kp, tr, inl, X = _cuda(kp, tr, inl, X)
    nv = None if n_views is None else _cuda(np.asarray(n_views, np.int32))[0]
    got = mv.bundle_adjust_batch(kp, tr, inl, X, nv, Ks, Rs, ts, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _ulp_apart(a, b):
    """float32 arrays: the distance in units of the last place (0 for two NaNs)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-(2 ** 31)) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))      # noqa: E731
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def _check(got, s, want, sc):
    assert BR.decision_margin(want) > 1e-9
    assert list(got["info"][s]) == list(want["info"]), (got["info"][s], want["info"])
    assert got["refined"].dtype == np.bool_ and np.array_equal(got["refined"][s], want["refined"])
    assert int(got["free_views"][s]) == (want["free_views"] if want["free_views"] < 2 ** 31 else want["free_views"] - 2 ** 32)
    assert np.abs(got["Rs"][s] - want["Rs"]).max() <= 1e-9, np.abs(got["Rs"][s] - want["Rs"]).max()
    assert np.abs(got["ts"][s] - want["ts"]).max() <= 1e-9 * max(1.0, np.abs(want["ts"]).max())
    assert np.all(np.abs(got["cost"][s] - want["cost"]) <= 1e-9 * np.maximum(1.0, np.abs(want["cost"]))), (got["cost"][s], want["cost"])
    assert got["points3d"].dtype == np.float32 and _ulp_apart(got["points3d"][s], want["points3d"]).max(initial=0) <= 1
    # held views and unrefined tracks keep the input's bits
    V = sc["Rs0"].shape[0]
    for v in range(V):
        if not (want["free_views"] >> v) & 1:
            assert np.array_equal(got["Rs"][s, v], sc["Rs0"][v]) and np.array_equal(got["ts"][s, v], sc["ts0"][v]), v
    keep = ~want["refined"]
    assert np.array_equal(got["points3d"][s][keep].view(np.uint32), sc["points3d"][keep].view(np.uint32))


@pytest.mark.parametrize("K", [0, 1, 255, 256, 257, 600])
def test_track_counts_around_the_chunk_edge(mv, K):
    """K around the 256 tracks of a chunk (one and two cost partials), and 600: a thread of the pair kernel adds more than one term."""
    kw = dict(fixed_views=3, max_iterations=6, huber_px=1.0)
    sc, want = _clear_scene(lambda seed: _cut(BS.scene(seed, 3, max(K, 8), holes=0.05), K), 300 + K, **kw)
    got = _run(mv, [sc], **kw)
    _check(got, 0, want, sc)
    assert want["info"][5] == (0 if K > 1 else 1)


def _cut(sc, K):
    """The first K tracks of a scene."""
    for k in ("tracks", "inlier_views", "points3d"):
        sc[k] = sc[k][:K]
    return sc


@pytest.mark.parametrize("V,K,fixed,huber,iters", [(2, 300, 1, 1.0, 5), (3, 200, 0b101, INF, 10), (8, 150, 1, INF, 5), (32, 70, 3, 1.0, 3)])
def test_view_counts_fixed_views_and_losses(mv, V, K, fixed, huber, iters):
    """2 and 32 views (the solve's LDS at its smallest and at its 148 KB), every fixed_views of the issue, both losses; at 10 rounds the
    scene ends by FTOL."""
    kw = dict(fixed_views=fixed, max_iterations=iters, huber_px=huber)
    sc, want = _clear_scene(lambda seed: BS.scene(seed, V, K, fixed=fixed, holes=0.05 if V > 2 else 0.0), 400 + V, **kw)
    got = _run(mv, [sc], **kw)
    _check(got, 0, want, sc)
    assert want["info"][4] >= 2 and want["cost"][1] < want["cost"][0]


def test_ragged_batch_a_starved_view_and_two_calls(mv):
    """S = 3 with different n_views; scene 1 has a view under MIN_VIEW_OBS (held, its observations still count); two calls, equal bits."""
    V, nv = 5, [3, 5, 2]
    kw = dict(fixed_views=1, max_iterations=5, huber_px=1.0)
    scenes, wants = [], []
    for s in range(3):
        make = lambda seed: BS.scene(seed, V, 140, fixed=1, n_views=nv[s])      # noqa: E731
        if s == 1:
            make = lambda seed: BS.starve_view(BS.scene(seed, V, 140, fixed=1), 3)      # noqa: E731
        sc, want = _clear_scene(make, 500 + s, **kw)
        scenes.append(sc); wants.append(want)
    got = _run(mv, scenes, n_views=nv, **kw)
    for s in range(3):
        _check(got, s, wants[s], scenes[s])
    assert not (wants[1]["free_views"] >> 3) & 1 and 0 < wants[1]["counts"][3] < BR.MIN_VIEW_OBS and wants[0]["free_views"] == 0b110 and wants[2]["free_views"] == 0b10
    again = _run(mv, scenes, n_views=nv, **kw)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k


def test_degenerate_batches_run_without_a_fault(mv):
    """All tracks unobserved, NaN poses (no view is usable: no observation), every view fixed: status 1, nothing moves, by construction."""
    a, b = BS.scene(600, 3, 100), BS.scene(601, 3, 100)
    a["tracks"] = np.full_like(a["tracks"], -1)
    b["Rs0"] = np.full_like(b["Rs0"], np.nan)
    got = _run(mv, [a, b], fixed_views=1)
    c = BS.scene(602, 3, 100)
    got7 = _run(mv, [c], fixed_views=7)
    for g, scenes in ((got, [a, b]), (got7, [c])):
        for s, sc in enumerate(scenes):
            assert g["info"][s][5] == 1 and g["info"][s][0] == 0 and g["info"][s][3] == 0 and not g["refined"][s].any() and g["free_views"][s] == 0
            assert np.array_equal(g["points3d"][s].view(np.uint32), sc["points3d"].view(np.uint32))
            assert np.array_equal(g["Rs"][s].view(np.uint64), sc["Rs0"].view(np.uint64)) and np.array_equal(g["ts"][s], sc["ts0"])
    assert got7["info"][0][1] > 250 and got["info"][0][1] == 0 and got["info"][1][1] == 0


def test_refine_views_then_localise_a_further_view(mv):
    """refine_views_batch end to end: its adjustment is the restatement's on the first triangulation, its second triangulation is the
    restatement's under the refined poses, the refined poses are nearer the truth, and points3d goes, unchanged, into
    estimate_absolute_pose_matches for a held-out view (the result is abspose_reference's on the same float32 points)."""
    from accelerated_features_amd import absolute_pose
    V, K = 5, 400
    kw = dict(fixed_views=3, max_iterations=10, huber_px=1.0)
    for seed in range(700, 720):
        sc = BS.scene(seed, V, K, fixed=3)
        four = dict(sc, kpts=sc["kpts"][:4], tracks=sc["tracks"][:, :4], Ks=sc["Ks"][:4], Rs=sc["Rs"][:4], ts=sc["ts"][:4], n_views=4)
        BS.triangulated(four, sc["Rs0"][:4], sc["ts0"][:4])
        want = BS.run_reference(four, **kw)
        if BR.decision_margin(want) > 1e-9 and MR.gate_margin(four["tri"]) > 1e-9:
            break
    assert BR.decision_margin(want) > 1e-9 and MR.gate_margin(four["tri"]) > 1e-9
    kp, tr = _cuda(sc["kpts"][None, :4], sc["tracks"][None, :, :4])
    out = mv.refine_views_batch(kp, tr, None, sc["Ks"][None, :4], sc["Rs0"][None, :4], sc["ts0"][None, :4], max_reproj_error=BS.GATE, **kw)
    torch.cuda.synchronize()
    Rs, ts = out["Rs"][0].cpu().numpy(), out["ts"][0].cpu().numpy()
    assert list(out["ba_info"][0].cpu().numpy()) == list(want["info"])
    assert np.abs(Rs - want["Rs"]).max() <= 1e-9 and np.abs(ts - want["ts"]).max() <= 1e-9 * max(1.0, np.abs(want["ts"]).max())
    second = MR.triangulate_views(four["kpts"], four["tracks"], 4, four["Ks"], Rs, ts, max_reproj_error=BS.GATE)
    assert MR.gate_margin(second) > 1e-9
    assert np.array_equal(out["status"][0].cpu().numpy(), second["status"]) and np.array_equal(out["inlier_views"][0].cpu().numpy(), second["inlier_views"])
    X = out["points3d"][0].cpu().numpy()
    assert _ulp_apart(X, second["points3d"]).max() == 0
    r0, c0 = BS.pose_errors(four, four["Rs0"], four["ts0"])
    r1, c1 = BS.pose_errors(four, Rs, ts)
    assert r1 < 0.5 * r0 and c1 < 0.5 * c0, (r0, r1, c0, c1)
    rng = np.random.default_rng(5)
    seen = np.nonzero(sc["tracks"][:, 4] >= 0)[0]
    n = len(seen)
    order = rng.permutation(n)
    idx_ref, idx_q = seen[order].astype(np.int64), sc["tracks"][seen[order], 4].astype(np.int64)
    q, ir, iq, nm = _cuda(sc["kpts"][None, 4], idx_ref[None], idx_q[None], np.array([n], np.int32))
    loc = absolute_pose.estimate_absolute_pose_matches(q, out["points3d"], iq, ir, nm, sc["Ks"][4], 3.0, seed=6)
    torch.cuda.synchronize()
    ref = AR.estimate(sc["kpts"][4][idx_q], X[idx_ref], sc["Ks"][4], 3.0, seed=6)
    check_common(loc, ref, 0, n)
    R, t = loc["R"][0].cpu().numpy(), loc["t"][0].cpu().numpy()
    assert ref["info"][0] == 1 and np.abs(R - ref["R"]).max() <= 1e-9 and np.abs(t - ref["t"]).max() <= 1e-9 * max(1.0, np.abs(ref["t"]).max())
