"""Localisation against the map on the MI355X: xfh_build_map and xfh_map_project against the numpy restatement
tests/localization_reference.py (integers exactly, floats as bits), then the chain map -> matches -> pose end to end against the restatement
chain (brute-force float64 matcher -> tests/abspose_reference.py) and against the truth, the guided second stage, queries that match nothing,
and the resection of a view the triangulation did not use.

The figures of the restatement chain on the end-to-end scene (arc_scene seed 1, V = 5, K = 400, 0.5 px, sigma 0.05, view 4 the query; measured
on the CPU): 389 matches, all true, rotation error 0.00920 degrees, centre error 0.00098 (scene units, depth 7); the device is
asserted at twice them."""
import numpy as np
import pytest
import torch

import abspose_reference as AR
import localization_reference as LR
import localization_support as LS
from localization_support import check_build, check_project

pytestmark = pytest.mark.gpu

ROT_ERR_DEG, CENTRE_ERR = 0.00920, 0.00098                # of the restatement chain (see above)
MAP_KEYS = ("points", "desc", "desc_f16", "track", "n_obs", "coherence", "n_points", "info")


@pytest.fixture(scope="module")
def loc():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import localization as m
    return m


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _build(loc, scenes, **kw):
    return loc.build_map_batch(*_cuda(*(np.stack([sc[i] for sc in scenes]) for i in range(5))), **kw)


@pytest.mark.parametrize("V,T,kcap", [(3, 64, 16), (32, 257, 64)])
def test_build_map_equals_the_restatement(loc, V, T, kcap):
    rng = np.random.default_rng(V + T)
    sc = LS.map_inputs(rng, V, T, kcap, view31=True)
    got = _host(_build(loc, [sc]))
    want = LR.build_map(*sc)
    check_build(got, 0, want)
    assert (want["info"][1:6] > 0).all()
    if V == 32:
        assert (LR.contributing(sc[0], sc[1], sc[4])[:, 31] & (want["rows"]["flag"] == 0)).sum() > 0


def test_a_ragged_batch_with_a_capacity_below_the_count_and_two_calls_byte_identical(loc):
    rng = np.random.default_rng(5)
    scenes = [LS.map_inputs(rng, 8, 300, 32) for _ in range(3)]
    scenes[1][3][::2] = 1                                  # scene 1 keeps half as many tracks
    scenes[2][3][:] = 2                                    # scene 2 keeps none
    first = _build(loc, scenes, min_views=2, max_points=60)
    second = _build(loc, scenes, min_views=2, max_points=60)
    torch.cuda.synchronize()
    for k in MAP_KEYS:
        a, b = first[k], second[k]
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int16) if b.dtype == torch.float16 else b.view(torch.int32) if b.dtype == torch.float32 else b), k
    got = _host(first)
    counts = []
    for s, sc in enumerate(scenes):
        want = LR.build_map(*sc, 2, 60)
        check_build(got, s, want)
        counts.append((int(want["n_points"]), int(want["info"][6])))
    assert counts[0][0] == 60 and counts[0][1] > 0 and 0 < counts[1][0] < 60 and counts[2] == (0, 0)


@pytest.mark.parametrize("M", [1, 257])
def test_map_project_equals_the_restatement(loc, M):
    rng = np.random.default_rng(M)
    pts, n, R, t, K = LS.project_case(rng, 3, M)
    for size, counts in (((0.0, 0.0, 0.0), n), ((640.0, 480.0, 12.0), n), ((640.0, 480.0, 0.0), None)):
        uv = loc.project_map(*_cuda(pts), None if counts is None else torch.from_numpy(counts), R, t, K, None if size[0] == 0 else size[:2], size[2])
        hit = check_project(uv.cpu().numpy(), pts, counts, R, t, K, size)
        assert M == 1 or 0 < hit < 3 * M * 2
    assert (pts[..., 2] <= 0).any()                        # points behind the camera


@pytest.fixture(scope="module")
def scene(loc):
    """The end-to-end scene: views 0-3 triangulated under their true poses into the map (on the device), view 4 the query; the restatement of
    the map from the same triangulation, its float64 matches and their pose."""
    from accelerated_features_amd import multiview as mv
    sc = LS.descriptor_scene(np.random.default_rng(1), 5, 400, 0.5, 0.05)
    kpts, tracks = _cuda(sc["kpts"][None, :4], sc["tracks"][None, :, :4])
    tri = mv.triangulate_views_batch(kpts, tracks, None, sc["Ks"][None, :4], sc["Rs"][None, :4], sc["ts"][None, :4])
    desc, = _cuda(sc["desc"][None, :4])
    m = loc.build_map_batch(desc, tracks, tri["points3d"], tri["status"], tri["inlier_views"])
    th = _host(tri)
    want = LR.build_map(sc["desc"][:4], sc["tracks"][:, :4], th["points3d"][0], th["status"][0], th["inlier_views"][0])
    check_build(_host(m), 0, want)
    n = int(want["n_points"])
    i0, i1, margin = LR.mnn(sc["desc"][4], 400, want["desc"], n, 0.8)
    row = sc["tracks"][want["track"][:n], 4]               # the query's row of every map point, -1: not seen
    cos = (sc["desc"][4][row[row >= 0]].astype(np.float64) * want["desc"][:n][row >= 0].astype(np.float64)).sum(axis=1)
    print(f"map rows {n}, matches {len(i0)}, margin {margin:.4f}, smallest true cosine {cos.min():.4f}")
    assert margin > 1e-3 and cos.min() > 0.8 and np.array_equal(row[i1], i0) and len(i0) == int((row >= 0).sum()) > 300
    est = AR.estimate(sc["kpts"][4][i0], want["points"][i1], sc["Ks"][4])
    q = _cuda(sc["kpts"][None, 4], sc["desc"][None, 4]) + (torch.tensor([400], dtype=torch.int32).cuda(),)
    return dict(sc=sc, map=m, want=want, i0=i0, i1=i1, est=est, query=q, tri=tri)


def _check_pose(r, p, sc):
    er, ec = LS.truth_pose_errors(r["R"][p].cpu().numpy(), r["t"][p].cpu().numpy(), sc["Rs"][4], sc["ts"][4])
    print(f"rotation error {er:.5f} degrees, centre error {ec:.5f}")
    assert er <= 2 * ROT_ERR_DEG and ec <= 2 * CENTRE_ERR, (er, ec)


def test_localize_equals_the_restatement_chain(loc, scene):
    sc, est = scene["sc"], scene["est"]
    r = loc.localize_map_batch(*scene["query"], scene["map"], sc["Ks"][4], min_cossim=0.8)
    n = int(r["n_matches"][0])
    assert n == len(scene["i0"]) and r["idx_query"].shape == (1, 400) and int(r["stage"][0]) == 1
    assert np.array_equal(r["idx_query"][0, :n].cpu().numpy(), scene["i0"]) and np.array_equal(r["idx_map"][0, :n].cpu().numpy(), scene["i1"])
    assert np.array_equal(r["track"][0, :n].cpu().numpy(), scene["want"]["track"][scene["i1"]]) and bool((r["track"][0, n:] == -1).all())
    # the pose against abspose_reference on those lists, to the tolerance of tests/test_gpu_abspose.py
    assert list(r["info"][0].cpu().numpy()) == list(est["info"]) and np.array_equal(r["inliers"][0, :n].cpu().numpy(), est["mask"])
    R, t = r["R"][0].cpu().numpy(), r["t"][0].cpu().numpy()
    assert np.abs(R - est["R"]).max() <= 1e-9 and np.abs(t - est["t"]).max() <= 1e-9 * max(1.0, np.abs(est["t"]).max())
    er, ec = LS.truth_pose_errors(est["R"], est["t"], sc["Rs"][4], sc["ts"][4])
    assert abs(er - ROT_ERR_DEG) < 5e-6 and abs(ec - CENTRE_ERR) < 5e-6, (er, ec)      # the figures above are this chain's
    _check_pose(r, 0, sc)
    # the detector's fp16 copy of the query changes nothing
    h = loc.localize_map_batch(*scene["query"], scene["map"], sc["Ks"][4], min_cossim=0.8,
                               desc_q_f16=(scene["query"][1] * 256.0).to(torch.float16))
    for k in ("R", "t", "info", "inliers", "n_matches", "track"):
        assert torch.equal(h[k], r[k]), k


def test_the_guided_stage(loc, scene):
    sc = scene["sc"]
    one = loc.localize_map_batch(*scene["query"], scene["map"], sc["Ks"][4], min_cossim=0.8)
    two = loc.localize_map_batch(*scene["query"], scene["map"], sc["Ks"][4], min_cossim=0.8, guided=True, image_size=sc["sizes"][4][::-1])
    assert int(two["stage"][0]) == 2 and int(two["info"][0, 0]) == 1 and int(two["info"][0, 3]) >= int(one["info"][0, 3])
    n = int(two["n_matches"][0])
    row = sc["tracks"][two["track"][0, :n].cpu().numpy(), 4]
    assert np.array_equal(row, two["idx_query"][0, :n].cpu().numpy())          # every guided match is a true pair
    _check_pose(two, 0, sc)


def test_queries_that_match_nothing_leave_the_others_alone(loc, scene):
    sc = scene["sc"]
    kq, dq, _ = scene["query"]
    noise, = _cuda(LS.unit_rows(np.random.default_rng(9), 400).astype(np.float32)[None])
    kpts, desc = torch.cat([kq, kq, kq]).contiguous(), torch.cat([dq, noise, dq]).contiguous()
    n_q = torch.tensor([400, 400, 0], dtype=torch.int32).cuda()
    scene_of = torch.zeros(3, dtype=torch.int64)
    for guided in (False, True):
        solo = loc.localize_map_batch(*scene["query"], scene["map"], sc["Ks"][4], min_cossim=0.8, guided=guided)
        r = loc.localize_map_batch(kpts, desc, n_q, scene["map"], sc["Ks"][4], scene_of=scene_of, min_cossim=0.8, guided=guided)
        info = r["info"].cpu().numpy()
        assert info[1, 0] == 0 and info[2, 0] == 0 and r["n_matches"].tolist()[1:] == [0, 0] and bool((r["track"][1:] == -1).all())
        assert not r["R"][1:].any() and not r["t"][1:].any() and not r["inliers"][1:].any() and r["stage"].tolist() == [2 if guided else 1, 1, 1]
        for k in ("R", "t", "info", "inliers", "n_matches", "track", "idx_query", "idx_map"):
            a, b = r[k][0], solo[k][0]
            if k.startswith("idx"):
                a, b = a[:int(solo["n_matches"][0])], b[:int(solo["n_matches"][0])]
            assert torch.equal(a, b), (guided, k)
        assert bool(torch.isfinite(r["R"]).all()) and bool(torch.isfinite(r["t"]).all())


def test_resection_of_a_view_the_triangulation_did_not_use(loc):
    from accelerated_features_amd import multiview as mv
    sc = LS.descriptor_scene(np.random.default_rng(1), 5, 400, 0.5, 0.05)
    Rs, ts = sc["Rs"].copy(), sc["ts"].copy()
    Rs[3], ts[3] = np.nan, np.nan
    kpts, tracks = _cuda(sc["kpts"][None], sc["tracks"][None])
    tri = mv.triangulate_views_batch(kpts, tracks, None, sc["Ks"][None], Rs[None], ts[None], anchor="first")
    track_of = np.full((5, 400), -1, np.int32)
    for v in range(5):
        seen = np.nonzero(sc["tracks"][:, v] >= 0)[0]
        track_of[v, sc["tracks"][seen, v]] = seen
    r = loc.resect_views_batch(kpts, torch.from_numpy(track_of[None]).cuda(), tri["points3d"], sc["Ks"][None])
    assert r["Rs"].shape == (1, 5, 3, 3) and r["ts"].shape == (1, 5, 3) and r["info"].shape == (1, 5, 8) and r["inliers"].shape == (1, 5, 400)
    X = tri["points3d"][0].cpu().numpy()
    assert not (tri["inlier_views"][0].cpu().numpy() >> 3 & 1).any() and (tri["status"][0] == 0).sum() > 300
    rows = np.where(track_of[3][:, None] >= 0, X[np.maximum(track_of[3], 0)], np.nan).astype(np.float32)
    want = AR.estimate(sc["kpts"][3], rows, sc["Ks"][3], pair=3)
    assert list(r["info"][0, 3].cpu().numpy()) == list(want["info"]) and want["info"][0] == 1 and want["info"][3] > 300
    assert np.array_equal(r["inliers"][0, 3].cpu().numpy(), want["mask"])
    R, t = r["Rs"][0, 3].cpu().numpy(), r["ts"][0, 3].cpu().numpy()
    assert np.abs(R - want["R"]).max() <= 1e-9 and np.abs(t - want["t"]).max() <= 1e-9 * max(1.0, np.abs(want["t"]).max())
    for v in range(5):                                      # every view within the bound of its truth, the one that was left out included
        er, ec = LS.truth_pose_errors(r["Rs"][0, v].cpu().numpy(), r["ts"][0, v].cpu().numpy(), sc["Rs"][v], sc["ts"][v])
        print(f"view {v}: rotation error {er:.5f} degrees, centre error {ec:.5f}")
        assert er <= 2 * ROT_ERR_DEG and ec <= 2 * CENTRE_ERR, (v, er, ec)
