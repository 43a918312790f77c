"""xfh_estimate_alignment (csrc/k_align.hip) on the MI355X against the numpy restatement tests/alignment_reference.py: the winner, the
iteration count, the inlier count, the integer cost and the mask exactly; R, t and s to 1e-9 (t relative to max(1, |t|), s to max(1, s)):
the refit's sums are taken in one fixed order on both sides.  Every case stays within P <= 8, n <= 2100, max_iterations <= 1024."""
import numpy as np
import pytest
import torch

import alignment_reference as AL
import alignment_support as AS
import twoview_support as TS
from twoview_support import check_common

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def al():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from accelerated_features_amd import alignment as m
    return m


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _check(got, want, p, n):
    check_common(got, want, p, n)
    R, t, s = got["R"][p].cpu().numpy(), got["t"][p].cpu().numpy(), float(got["s"][p])
    assert np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s)
    assert np.abs(R - want["R"]).max() <= 1e-9, (R, want["R"])
    assert np.abs(t - want["t"]).max() <= 1e-9 * max(1.0, np.abs(want["t"]).max()), (t, want["t"])
    assert abs(s - want["s"]) <= 1e-9 * max(1.0, want["s"]), (s, want["s"])
    if not want["info"][0]:
        assert not R.any() and not t.any() and s == 0.0 and not got["inliers"][p].any()


@pytest.mark.parametrize("with_scale", [True, False], ids=["similarity", "rigid"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, 300])
def test_single_pair_equals_the_restatement(al, n, with_scale):
    sc = AS.scene(max(n, 1), 0.01, 0.3 if n >= 63 else 0.0, 0.1 if n >= 63 else 0.0, seed=n, with_scale=with_scale)
    A, B = sc["A"][:n], sc["B"][:n]
    got = al.estimate_alignment_batch(*_cuda(A[None], B[None]), None, sc["thr"], with_scale, seed=11)
    torch.cuda.synchronize()
    want = AL.estimate(A, B, sc["thr"], with_scale, seed=11)
    _check(got, want, 0, n)
    assert want["info"][0] == (1 if n >= 3 else 0)
    if n >= 63:
        assert want["info"][4] >= 1 and want["info"][3] >= 0.5 * n            # a refit was accepted


def test_more_correspondences_than_the_select_kernels_lds_cache(al):
    """n = 2100 > SEL_CACHE = 2048: the select kernel reads the last 52 correspondences through the tables (rs::for_each_cached's tail)."""
    sc = AS.scene(2100, 0.01, 0.5, 0.1, seed=21)
    sc["B"][2060:2100:3] = sc["B_true"][2060:2100:3].astype(np.float32)      # true correspondences in the tail, NaN rows and outliers among them
    got = al.estimate_alignment_batch(*_cuda(sc["A"][None], sc["B"][None]), None, sc["thr"], seed=2)
    torch.cuda.synchronize()
    want = AL.estimate(sc["A"], sc["B"], sc["thr"], seed=2)
    _check(got, want, 0, 2100)
    assert want["info"][0] == 1 and want["mask"][2048:].sum() >= 10 and not want["mask"][2048:].all()


def test_loop_past_the_first_block_of_hypotheses(al):
    """70 % outliers and min_iterations = 300: the first 256 hypotheses do not end the loop (at 30 % inliers its bound is
    log 1e-4 / log(1 - 0.3^3) = 337), so the second block of hypotheses is solved and scored below the bound kernel's value and the
    stopping rule walks past the first 256 entries of its tile.  (max_iterations <= 1024 keeps the list inside one tile of 2048 entries.)"""
    sc = AS.scene(300, 0.01, 0.7, 0.0, seed=7)
    got = al.estimate_alignment_batch(*_cuda(sc["A"][None], sc["B"][None]), None, sc["thr"], min_iterations=300, max_iterations=1024, seed=3)
    torch.cuda.synchronize()
    want = AL.estimate(sc["A"], sc["B"], sc["thr"], min_iterations=300, max_iterations=1024, seed=3)
    _check(got, want, 0, 300)
    assert 256 < want["info"][2] < 1024 and want["info"][0] == 1


NS = [300, 3, 0, 1200, 57, 2]


@pytest.mark.parametrize("with_scale", [True, False], ids=["similarity", "rigid"])
def test_ragged_batch_equals_the_restatement_pair_by_pair(al, with_scale):
    A, B, thr = AS.ragged(NS, with_scale=with_scale)
    got = al.estimate_alignment_batch(*_cuda(A, B), torch.tensor(NS, dtype=torch.int32), thr, with_scale, seed=5)
    torch.cuda.synchronize()
    for p, n in enumerate(NS):
        want = AL.estimate(A[p, :n], B[p, :n], thr, with_scale, seed=5, pair=p)
        _check(got, want, p, n)
    assert got["info"][:, 0].tolist() == [1, 1, 0, 1, 1, 0]


def test_index_list_entry_equals_gathered_points(al):
    P, cap_a, cap_b, cap = 3, 700, 900, 500
    rng = np.random.default_rng(3)
    ta, tb = np.full((P, cap_a, 3), np.nan, np.float32), np.full((P, cap_b, 3), np.nan, np.float32)
    ia, ib = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64)
    nm = np.array([500, 333, 20], np.int32)
    for p in range(P):
        sc = AS.scene(cap, 0.01, 0.3, 0.1, seed=p, scale=0.5)
        ia[p], ib[p] = rng.permutation(cap_a)[:cap], rng.permutation(cap_b)[:cap]
        ta[p, ia[p]], tb[p, ib[p]], thr = sc["A"], sc["B"], sc["thr"]
    r1 = al.estimate_alignment_matches(*_cuda(ta, tb, ia, ib, nm), thr, seed=9)
    ga, gb = np.take_along_axis(ta, ia[:, :, None], 1), np.take_along_axis(tb, ib[:, :, None], 1)
    r2 = al.estimate_alignment_batch(*_cuda(ga, gb), torch.from_numpy(nm), thr, seed=9)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    assert r1["info"][:, 0].all() and r1["inliers"].shape == (P, cap)
    want = AL.estimate(ga[1, :333], gb[1, :333], thr, seed=9, pair=1)
    _check(r1, want, 1, 333)


def test_chunked_equals_unchunked(al, monkeypatch):
    A, B, thr = AS.ragged(NS)
    a, b = _cuda(A, B)
    counts = torch.tensor(NS, dtype=torch.int32)
    whole = al.estimate_alignment_batch(a, b, counts, thr, seed=5)
    from accelerated_features_amd import _lib
    per_pair = _lib.load().xfh_align_workspace_bytes(1, 1000)
    monkeypatch.setattr(al, "WORKSPACE_LIMIT", 2 * per_pair + 1024)          # 2 pairs per library call: 3 chunks
    assert (2 * per_pair + 1024) // per_pair == 2
    split = al.estimate_alignment_batch(a, b, counts, thr, seed=5)
    torch.cuda.synchronize()
    for k in whole:
        assert torch.equal(whole[k], split[k]), k
    assert whole["info"][:, 0].tolist() == [1, 1, 0, 1, 1, 0]


def test_same_seed_same_bits(al):
    sc = AS.scene(1500, 0.01, 0.5, 0.1, seed=1)
    a, b = _cuda(sc["A"][None], sc["B"][None])
    r1 = al.estimate_alignment_batch(a, b, None, sc["thr"], seed=4)
    r2 = al.estimate_alignment_batch(a, b, None, sc["thr"], seed=4)
    r3 = al.estimate_alignment_batch(a, b, None, sc["thr"], seed=5)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    assert int(r1["info"][0, 0]) == 1 and int(r3["info"][0, 0]) == 1 and int(r1["info"][0, 1]) != int(r3["info"][0, 1])


def test_degenerate_inputs_do_not_fault_or_nan(al):
    cap = 64
    sc = AS.scene(cap, 0.01, 0.0, 0.0, seed=5, scale=1.0)
    A, B = np.repeat(sc["A"][None], 6, 0), np.repeat(sc["B"][None], 6, 0)
    line = (np.array([0.25, -0.5, 3.0]) + np.arange(cap)[:, None] * np.array([0.125, 0.0625, 0.25])).astype(np.float32)
    A[0], B[0] = line, line + np.float32(1.0)               # all collinear
    A[1] = A[1, :1]                                         # all of A coincident
    A[2], B[2] = A[2, :1], B[2, :1]                         # both sides coincident
    A[3, ::3] = np.nan                                      # NaN rows on either side
    B[3, 1::7] = np.nan
    A[4] = np.nan                                           # nothing finite
    B[4] = np.nan
    counts = torch.tensor([cap, cap, cap, cap, cap, 2], dtype=torch.int32)
    a, b = _cuda(A, B)
    thr = sc["thr"]
    for with_scale in (True, False):
        r = al.estimate_alignment_batch(a, b, counts, thr, with_scale, max_iterations=300, seed=1)
        z = al.estimate_alignment_batch(a, b, torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32), thr, with_scale, max_iterations=300, seed=1)
        torch.cuda.synchronize()
        for k in ("R", "t", "s"):
            assert torch.isfinite(r[k]).all() and torch.isfinite(z[k]).all()
        assert (z["info"][:, 0] == 0).all() and not z["inliers"].any() and (z["info"][:, 2] == 0).all()
        assert not z["R"].any() and not z["t"].any() and not z["s"].any()
        assert z["info"][:, 5].tolist() == [0, 1, 2, 0, 1, 2] and (z["info"][:, 1] == -1).all()
        info = r["info"].cpu().numpy()
        for q in range(6):
            n = int(counts[q])
            _check(r, AL.estimate(A[q, :n], B[q, :n], thr, with_scale, max_iterations=300, seed=1, pair=q), q, n)
        assert [int(v) for v in info[:, 0]] == [0, 0, 0, 1, 0, 0]
        bad = np.isnan(A[3]).any(1) | np.isnan(B[3]).any(1)
        assert not r["inliers"][3].cpu().numpy()[bad].any() and int(info[3, 3]) == int((~bad).sum())
    # the list form with indices outside the tables: those correspondences are "no point", nothing is read outside
    ia = np.tile(np.arange(cap, dtype=np.int64), (6, 1))
    ib = ia.copy()
    ia[3, 1], ia[3, 4], ib[3, 8], ib[3, 10], ia[5, 0] = -1, cap, cap + 5, 1 << 40, -(1 << 62)
    m = al.estimate_alignment_matches(a, b, *_cuda(ia, ib), counts.cuda(), thr, max_iterations=300, seed=1)
    A2, B2 = A.copy(), B.copy()
    A2[3, [1, 4]], B2[3, [8, 10]], A2[5, 0] = np.nan, np.nan, np.nan
    g = al.estimate_alignment_batch(*_cuda(A2, B2), counts, thr, max_iterations=300, seed=1)
    torch.cuda.synchronize()
    for k in m:
        assert torch.equal(m[k], g[k]), k
    assert int(m["info"][3, 0]) == 1 and not m["inliers"][3, [1, 4, 8, 10]].any() and torch.isfinite(m["R"]).all()


def test_two_reconstructions_of_one_scene_differ_by_the_baseline_ratio(al):
    """One pair of images triangulated under its pose with |t| = 1 and with |t| = ratio: the two scattered key-point tables (NaN where no
    point was triangulated) differ by a pure scale, which the batch form recovers: R = I and s = ratio to 1e-6, t = 0 to 1e-6 of the scene
    depth.  (The tables are fp32: a coordinate carries a relative rounding of 6e-8, the fit averages it over some hundred points.)"""
    from accelerated_features_amd import structure
    ratios, n, kcap = (2.5, 0.4), 400, 512
    rng = np.random.default_rng(8)
    k0, k1 = np.zeros((2, kcap, 2), np.float32), np.zeros((2, kcap, 2), np.float32)
    idx0, idx1 = np.zeros((2, n), np.int64), np.zeros((2, n), np.int64)
    K0, K1, R, t = np.zeros((2, 3, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3))
    for p, i in enumerate((3, 40)):
        p0, p1, _, K0[p], K1[p], T = TS.scene(i, n, 0.5, 0.2, 100 + i)
        idx0[p], idx1[p] = rng.permutation(kcap)[:n], rng.permutation(kcap)[:n]
        k0[p, idx0[p]], k1[p, idx1[p]] = p0, p1
        R[p], t[p] = T[:3, :3], T[:3, 3] / np.linalg.norm(T[:3, 3])
    nm = torch.full((2,), n, dtype=torch.int32).cuda()
    lists = _cuda(k0, k1, idx0, idx1)
    one = structure.triangulate_matches(*lists, nm, K0, K1, R, t, max_reproj_error=2.0)
    two = structure.triangulate_matches(*lists, nm, K0, K1, R, t * np.array(ratios)[:, None], max_reproj_error=2.0)
    ta, tb = one["points3d_ref"], two["points3d_ref"]
    have = torch.isfinite(ta).all(dim=2)
    assert torch.equal(have, torch.isfinite(tb).all(dim=2)) and (have.sum(dim=1) >= 200).all() and (~have).sum() >= 2 * (kcap - n) + 40
    depth = float(torch.nan_to_num(ta[..., 2]).max())
    r = al.estimate_alignment_batch(ta, tb, None, 1e-3 * depth * min(ratios), seed=1)
    torch.cuda.synchronize()
    assert r["info"][:, 0].tolist() == [1, 1]
    assert torch.equal(r["inliers"].bool(), have)             # every point both reconstructions have, and no NaN row
    for p in range(2):
        assert np.abs(r["R"][p].cpu().numpy() - np.eye(3)).max() <= 1e-6
        assert np.abs(r["t"][p].cpu().numpy()).max() <= 1e-6 * depth * max(1.0, ratios[p])
        assert abs(float(r["s"][p]) / ratios[p] - 1.0) <= 1e-6
    merged = al.apply_alignment(ta, r["s"], r["R"], r["t"])
    assert torch.equal(torch.isfinite(merged).all(dim=2), have)
    assert float((torch.nan_to_num(merged) - torch.nan_to_num(tb)).abs().max()) <= 1e-5 * depth * max(ratios)


def test_rgbd_pose_equals_the_alignment_of_the_lifted_tables(al):
    """Two depth maps rendered from one plane under a known pose X1 = R X0 + t, key-points at integer pixels of both images (image 1's are
    the rounded projections of image 0's, so a pair of lifted points is up to half a pixel's footprint apart on the plane):
    estimate_relative_pose_rgbd_matches equals estimate_alignment_matches (rigid) on the two lifted tables bit for bit, and the pose is
    the true one to the footprint of that rounding."""
    from accelerated_features_amd import absolute_pose
    H, W, N, n = 240, 320, 300, 250
    K = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1]])
    Rt, tt = TS.rotation(np.array([0.03, -0.08, 0.02])), np.array([0.25, -0.05, 0.1])
    nrm, d = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0]), 4.0            # the plane nrm . X0 = d in camera 0
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], axis=-1)
    depth0 = d / (rays @ nrm)
    n1 = Rt @ nrm
    depth1 = (d + n1 @ tt) / (rays @ n1)
    rng = np.random.default_rng(4)
    kp0 = np.c_[rng.integers(30, W - 30, N), rng.integers(30, H - 30, N)].astype(np.float64)
    X0 = np.c_[(kp0[:, 0] - K[0, 2]) / K[0, 0], (kp0[:, 1] - K[1, 2]) / K[1, 1], np.ones(N)] * depth0[kp0[:, 1].astype(int), kp0[:, 0].astype(int)][:, None]
    X1 = X0 @ Rt.T + tt
    kp1 = np.round(np.c_[K[0, 0] * X1[:, 0] / X1[:, 2] + K[0, 2], K[1, 1] * X1[:, 1] / X1[:, 2] + K[1, 2]])
    assert (kp1[:, 0] >= 0).all() and (kp1[:, 0] < W).all() and (kp1[:, 1] >= 0).all() and (kp1[:, 1] < H).all()
    depth0[kp0[5, 1].astype(int), kp0[5, 0].astype(int)] = 0.0                                 # a key-point without depth: "no point"
    rows1 = rng.permutation(N)                                                                 # image 1's key-points in an order of their own
    kp1s = np.zeros_like(kp1)
    kp1s[rows1] = kp1
    idx0 = rng.permutation(N)[:n]
    idx1 = rows1[idx0]
    wrong = np.arange(0, n, 5)                                                                 # a fifth of the matches are wrong
    idx1[wrong] = rows1[rng.integers(0, N, len(wrong))]
    k0, k1, i0, i1 = _cuda(kp0.astype(np.float32)[None], kp1s.astype(np.float32)[None], idx0[None], idx1[None])
    d0, d1 = _cuda(depth0.astype(np.float32)[None], depth1.astype(np.float32)[None])
    nm = torch.tensor([n], dtype=torch.int32).cuda()
    thr = 0.03
    r1 = al.estimate_relative_pose_rgbd_matches(k0, d0, K, k1, d1, K, i0, i1, nm, thr, seed=6)
    L0, v0 = absolute_pose.unproject_keypoints(k0, d0, K)
    L1, _ = absolute_pose.unproject_keypoints(k1, d1, K)
    r2 = al.estimate_alignment_matches(L0, L1, i0, i1, nm, thr, False, seed=6)
    torch.cuda.synchronize()
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    assert int(r1["info"][0, 0]) == 1 and float(r1["s"][0]) == 1.0 and int(r1["info"][0, 3]) >= 0.7 * n and not bool(v0[0, 5])
    R, t = r1["R"][0].cpu().numpy(), r1["t"][0].cpu().numpy()
    ang = np.rad2deg(np.arccos(np.clip((np.trace(Rt.T @ R) - 1.0) / 2.0, -1.0, 1.0)))
    print("rgbd pose: rotation error", ang, "deg, translation error", np.abs(t - tt).max())
    # half a pixel at depth 4 and focal length 300 is 7 mm on the plane: no fit moves further than its points do (0.01), or turns by more
    # than that over the cloud's half extent of 1 (0.43 degrees)
    assert ang <= 0.43 and np.abs(t - tt).max() <= 0.01
    want = AL.estimate(L0[0].cpu().numpy()[idx0], L1[0].cpu().numpy()[idx1], thr, False, seed=6)
    _check(r1, want, 0, n)
