"""xfh_baseline_ratios and xfh_average_poses_ratios on the device against the numpy restatement (tests/posescale_reference.py) on the same
inputs: counts, shared views, info and statuses exactly, ratios and factors to 1e-9 relative (the family's figure: the device and numpy round
alike; a decision within 1e-9 of a tie could still flip, so the cases are first checked to have none).  Then ``reconstruct_graph_matches``
on a chain of pairs (v, v + 1) end to end, with and without track_scales."""
import math

import numpy as np
import pytest
import torch

import posegraph_reference as PR
import posegraph_support as PS
import posescale_reference as QR
import posescale_support as QS
import tracks_support as KS

pytestmark = pytest.mark.gpu
TOL = 1e-9
NOISY = dict(max_reproj_error=32.0)


def _mv():
    from accelerated_features_amd import multiview
    return multiview


def _pad(scenes):
    """Scenes padded to one batch: views without key-points, rows and tracks of -1, edges of weight 0."""
    S, V, K = len(scenes), max(sc["V"] for sc in scenes), max(sc["K"] for sc in scenes)
    T, P = max(sc["tracks"].shape[0] for sc in scenes), max(sc["pairs"].shape[0] for sc in scenes)
    b = dict(kpts=np.zeros((S, V, K, 2), np.float32), tracks=np.full((S, T, V), -1, np.int32), track_of=np.full((S, V, K), -1, np.int32),
             pairs=np.zeros((S, P, 2), np.int32), Rrel=np.zeros((S, P, 3, 3)), trel=np.zeros((S, P, 3)), weight=np.zeros((S, P)),
             Ks=np.tile(np.eye(3), (S, V, 1, 1)), nv=np.zeros(S, np.int32))
    for i, sc in enumerate(scenes):
        v, k, t, p = sc["V"], sc["K"], sc["tracks"].shape[0], sc["pairs"].shape[0]
        b["kpts"][i, :v, :k], b["tracks"][i, :t, :v], b["track_of"][i, :v, :k] = sc["kpts"], sc["tracks"], sc["track_of"]
        b["pairs"][i, :p], b["Rrel"][i, :p], b["trel"][i, :p], b["weight"][i, :p] = sc["pairs"], sc["Rrel"], sc["trel"], sc["weight"]
        b["Ks"][i, :v], b["nv"][i] = sc["Ks"], sc.get("n_views", v)
    return b, V


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device_ratios(b, **gates):
    r = _mv().baseline_ratios_batch(*(_cuda(b[k]) for k in ("kpts", "tracks", "track_of", "pairs", "Rrel", "trel", "weight", "Ks", "nv")), **gates)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _reference_ratios(b, i, V, **gates):
    return QR.baseline_ratios(b["kpts"][i], b["tracks"][i], b["track_of"][i], b["pairs"][i], b["Rrel"][i], b["trel"][i], b["weight"][i], b["Ks"][i],
                              b["nv"][i], V, **gates)


def _compare_ratios(name, got, i, want):
    print(f"{name}: info {list(want['info'])}, gate margin {want['margin']:.2e}")
    assert want["margin"] > TOL, (name, want["margin"])                                  # no gate of a track near a tie
    assert list(got["info"][i]) == list(want["info"]), (name, got["info"][i], want["info"])
    assert np.array_equal(got["count"][i], want["count"]) and np.array_equal(got["shared_view"][i], want["shared_view"]), name
    a, w = got["ratio"][i], want["ratio"]
    assert np.array_equal(np.isnan(a), np.isnan(w)), name
    has = np.isfinite(w)
    assert np.all(np.abs(a[has] / w[has] - 1.0) <= TOL), (name, np.abs(a[has] / w[has] - 1.0).max())


def _full(K, n):
    """Three views, one wedge, exactly n of the K tracks in all three views (a 3 degree arc keeps every point in every image)."""
    sc = QS.scene(40, 3, K, PS.chain_pairs(3), 0.0, 0.0, 0.0, step_deg=3.0)
    full = np.nonzero((sc["tracks"] >= 0).all(axis=1))[0]
    assert len(full) == K
    drop = full[n:]
    sc["track_of"][2, sc["tracks"][drop, 2]] = -1
    sc["tracks"][drop, 2] = -1
    return sc


def test_the_ratios_match_the_restatement():
    cases = [("V3 K64, one wedge", QS.scene(41, 3, 64, PS.chain_pairs(3), 0.0, 0.0, 0.0), {}),
             ("V6 K400 chain", QS.scene(42, 6, 400, PS.chain_pairs(6)), NOISY), ("V8 K256 strip", QS.scene(43, 8, 256, PS.near_pairs(8)), NOISY),
             ("K4096, 4095 common", _full(4096, 4095), {}), ("K4096, 4096 common", _full(4096, 4096), {})]
    for name, sc, gates in cases:
        b, V = _pad([sc])
        want = _reference_ratios(b, 0, V, **gates)
        _compare_ratios(name, _device_ratios(b, **gates), 0, want)
        if name.startswith("K4096"):
            assert want["count"][0, 1] == int(name.split()[1]) and want["info"][0] == 1 and np.isfinite(want["ratio"][0, 1])
        if name.startswith("V3"):
            assert want["info"][0] == 1 and want["info"][1] == 1


def _ragged():
    scenes = [QS.scene(44, 6, 200, PS.near_pairs(6)), QS.scene(45, 3, 64, PS.chain_pairs(3), 0.0, 0.0, 0.0), QS.scene(46, 8, 128, PS.chain_pairs(8)),
              QS.scene(47, 5, 100, PS.TWO_TRIANGLES)]
    scenes[0]["n_views"] = 5                                  # the edges at view 5 are not valid
    scenes[2]["Rrel"][2, 0, 0] = np.nan                       # an invalid edge
    scenes[2]["trel"][5] = 0.0                                # an edge without a direction
    scenes[3]["weight"][1] = 0.0
    return scenes


def test_a_ragged_batch_matches_the_restatement_and_two_calls_give_the_same_bytes():
    b, V = _pad(_ragged())
    got, again = _device_ratios(b, **NOISY), _device_ratios(b, **NOISY)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    wedges = []
    for i in range(4):
        want = _reference_ratios(b, i, V, **NOISY)
        _compare_ratios(f"ragged {i}", got, i, want)
        wedges.append(int(want["info"][0]))
    assert wedges[2] == 6 - 2 - 2 and wedges[1] == 1 and all(w > 0 for w in wedges), wedges
    # every entry of every buffer is defined: p >= q is (NaN, 0, -1)
    low = np.tril(np.ones(got["count"].shape[1:], bool))
    assert np.isnan(got["ratio"][:, low]).all() and (got["count"][:, low] == 0).all() and (got["shared_view"][:, low] == -1).all()
    # empty shapes come without a library call
    mv = _mv()
    r = mv.baseline_ratios_batch(torch.zeros((2, 3, 0, 2)).cuda(), torch.zeros((2, 0, 3), dtype=torch.int32).cuda(), torch.zeros((2, 3, 0), dtype=torch.int32).cuda(),
                                 _cuda(b["pairs"][:2]), _cuda(b["Rrel"][:2]), _cuda(b["trel"][:2]), _cuda(b["weight"][:2]), _cuda(b["Ks"][:2, :3]))
    P = b["pairs"].shape[1]
    assert r["ratio"].shape == (2, P, P) and torch.isnan(r["ratio"]).all() and not r["count"].any() and (r["shared_view"] == -1).all() and not r["info"].any()


def _settings(**kw):
    mv = _mv()
    s = dict(iterations=30, redescend=10, rot_scale_deg=2.0, pos_scale_deg=2.0, min_pivot_ratio=mv.MIN_PIVOT_RATIO, scale_weight=1.0, scale_tol=mv.SCALE_TOL)
    s.update(kw)
    return s


def _reference_poses(b, i, V, r, s):
    return QR.average_poses(b["pairs"][i], b["Rrel"][i], b["trel"][i], b["weight"][i], b["nv"][i], V, ratio=r["ratio"], ratio_count=r["count"],
                            scale_weight=s["scale_weight"], scale_tol=s["scale_tol"], iterations=s["iterations"], redescend=s["redescend"],
                            rot_scale_rad=math.radians(s["rot_scale_deg"]), pos_scale_sin=math.sin(math.radians(s["pos_scale_deg"])),
                            min_pivot_ratio=s["min_pivot_ratio"])


def test_the_pose_graph_with_ratios_matches_the_restatement():
    """The chain, the strip and the ragged batch: the ratios of the restatement go to both sides, so the comparison is the pose graph's own."""
    s = _settings()
    for name, scenes in (("chain", [QS.scene(42, 6, 400, PS.chain_pairs(6))]), ("strip", [QS.scene(43, 8, 256, PS.near_pairs(8))]), ("ragged", _ragged())):
        b, V = _pad(scenes)
        S, P = b["pairs"].shape[:2]
        refs = [_reference_ratios(b, i, V, **NOISY) for i in range(S)]
        ratio, count = np.stack([r["ratio"] for r in refs]), np.stack([r["count"] for r in refs])
        mv = _mv()
        call = lambda **kw: mv.average_poses_batch(_cuda(b["pairs"]), _cuda(b["Rrel"]), _cuda(b["trel"]), _cuda(b["weight"]), _cuda(b["nv"]), V=V, **kw)   # noqa: E731
        got = {k: v.cpu().numpy() for k, v in call(ratio=_cuda(ratio), ratio_count=_cuda(count), **s).items()}
        again = {k: v.cpu().numpy() for k, v in call(ratio=_cuda(ratio), ratio_count=_cuda(count), **s).items()}
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (name, k)
        for i, sc in enumerate(scenes):
            want = _reference_poses(b, i, V, refs[i], s)
            m = want["margin"]
            print(f"{name} {i}: info {list(want['info'])}, wedges {len(want['wedges'][0])}, margins {({k: float('%.2e' % v) for k, v in m.items()})}")
            assert all(v > TOL for v in m.values()), (name, i, m)                          # no decision of the run near a tie
            assert list(got["info"][i]) == list(want["info"]) and int(got["registered"][i]) & 0xFFFFFFFF == want["registered"], (name, i)
            for key in ("Rs", "ts"):
                a, w = got[key][i], want[key]
                assert np.array_equal(np.isnan(a), np.isnan(w)) and np.nanmax(np.abs(a - w), initial=0.0) <= TOL, (name, i, key)
            assert np.abs(got["edge_factor"][i] - want["edge_factor"]).max() <= TOL and np.abs(got["ratio_factor"][i] - want["ratio_factor"]).max() <= TOL
            if name in ("chain", "strip"):
                assert want["info"][6] == PR.ST_OK and len(want["wedges"][0]) > 0
        # without the new arguments: today's call, today's bytes, and no ratio_factor
        plain = call(**{k: v for k, v in s.items() if not k.startswith("scale")})
        assert "ratio_factor" not in plain
        if name == "chain":
            assert plain["info"][0, 6].item() == PR.ST_ROTATIONS_ONLY and got["info"][0, 6] == PR.ST_OK


def _truth(sc):
    """The scene's poses in the gauge of view 0, as PS.errors wants them."""
    V = sc["Rs"].shape[0]
    c = np.stack([-sc["Rs"][v].T @ sc["ts"][v] for v in range(V)])
    return dict(V=V, Rs=np.stack([sc["Rs"][v] @ sc["Rs"][0].T for v in range(V)]), cs=(c - c[0]) @ sc["Rs"][0].T)


def test_a_chain_of_pairs_gets_a_map_end_to_end():
    """KS.chain_scene at V = 6, K = 400, 0.5 px, the pairs (v, v + 1), 1000 RANSAC iterations.  Without track_scales: pose-graph status 2 and
    no valid track (what the chain gave before).  With them: status 0, all six views registered, and the errors against the truth (the gauge
    of view 0, one least-squares scale) within twice those of the same chain with the restatement in the place of the two new stages (the
    device's relative poses and tracks -> posescale_reference -> the device's triangulation and adjustment).  Measured on one MI355X
    (DESIGN.md 3.20): initial poses 0.199 deg / 1.39e-2, refined 0.0164 deg / 9.4e-4 for both chains, 400 of 400 tracks valid, the four
    ratios 0.913, 1.029, 1.050, 0.940."""
    mv = _mv()
    V, K = 6, 400
    sc = KS.chain_scene(6, K=K, V=V, noise=0.5)
    vp, ia, ib, nm = sc["lists"]
    dev = lambda x: _cuda(x)[None]                                                         # noqa: E731
    args = (dev(sc["kpts"]), dev(vp), dev(ia), dev(ib), dev(nm))
    Ks = dev(sc["Ks"])
    ransac = dict(max_iterations=1000, seed=3)
    off = mv.reconstruct_graph_matches(*args, None, Ks, ransac=ransac, track_scales=False)
    on = mv.reconstruct_graph_matches(*args, None, Ks, ransac=ransac, track_scales=True)
    torch.cuda.synchronize()
    assert off["pg_info"][0, 6].item() == PR.ST_ROTATIONS_ONLY and int(off["valid"].sum()) == 0 and "ratio" not in off
    assert on["pg_info"][0, 6].item() == PR.ST_OK and on["pg_info"][0, 1].item() == V and on["ba_info"][0, 5].item() == 0
    assert torch.equal(on["R_rel"], off["R_rel"]) and torch.equal(on["tracks"], off["tracks"])
    # the restatement in the place of the two new stages
    rel = {k: on[k][0].cpu().numpy() for k in ("R_rel", "t_rel", "weight")}
    tracks, track_of = on["tracks"][0].cpu().numpy(), on["track_of"][0].cpu().numpy()
    r = QR.baseline_ratios(sc["kpts"], tracks, track_of, vp, rel["R_rel"], rel["t_rel"], rel["weight"], sc["Ks"], V, V)
    s = _settings()
    want = QR.average_poses(vp, rel["R_rel"], rel["t_rel"], rel["weight"], V, V, ratio=r["ratio"], ratio_count=r["count"], scale_weight=s["scale_weight"],
                            scale_tol=s["scale_tol"], rot_scale_rad=math.radians(2.0), pos_scale_sin=math.sin(math.radians(2.0)),
                            min_pivot_ratio=s["min_pivot_ratio"])
    assert want["info"][6] == PR.ST_OK and np.array_equal(on["ratio_count"][0].cpu().numpy(), r["count"])
    Rw, tw = dev(want["Rs"]), dev(want["ts"])
    first = mv.triangulate_views_batch(args[0], on["tracks"], None, Ks, Rw, tw, anchor='first')
    ba = mv.bundle_adjust_batch(args[0], on["tracks"], first["inlier_views"], first["points3d"], None, Ks, Rw, tw)
    truth = _truth(sc)
    num = lambda x: x[0].cpu().numpy()                                                     # noqa: E731
    e_init, e_init_ref = PS.errors(truth, num(on["Rs_init"]), num(on["ts_init"])), PS.errors(truth, want["Rs"], want["ts"])
    e_fin, e_fin_ref = PS.errors(truth, num(on["Rs"]), num(on["ts"])), PS.errors(truth, num(ba["Rs"]), num(ba["ts"]))
    print(f"end to end (rotation deg, centres): initial {e_init} against {e_init_ref}, refined {e_fin} against {e_fin_ref}, "
          f"valid points {int(on['valid'].sum())} of {int(on['n_tracks'][0])} tracks, ratios {r['ratio'][np.isfinite(r['ratio'])]}")
    for a, b in ((e_init, e_init_ref), (e_fin, e_fin_ref)):
        assert a[0] <= 2.0 * b[0] and a[1] <= 2.0 * b[1]
    assert int(on["valid"].sum()) > 0
