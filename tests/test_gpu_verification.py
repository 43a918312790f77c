"""xfh_filter_matches and xfh_verify_matches on the device against the numpy restatement tests/verification_reference.py: the filter as
bytes, the verifier's mask and pair_info exactly and its errors as bits (the cases are first checked to have no error within 1e-9 relative
of its threshold).  Then ``reconstruct_graph_matches(verified=True)`` end to end on match lists with 20 % wrong matches.

The end-to-end bounds are twice the worst of three seeds of the restatement chain (verification_support.restatement_chain on
verification_support.wrong_scene(seed), seeds 1 - 3, V = 6, K = 400, 0.5 px, all 15 pairs, wrong = 0.2, 1000 iterations):
    seed   tracks   rotation (deg)   centres    median point error / depth
    1      391      0.0593           4.47e-3    4.05e-3
    2      382      0.0176           1.90e-3    7.79e-4
    3      390      0.0891           1.32e-2    1.29e-3"""
import numpy as np
import pytest
import torch

import tracks_reference as KR
import tracks_support as TS
import verification_reference as VR
import verification_support as VS

pytestmark = pytest.mark.gpu
ROT_DEG, CENTRE, POINT = 2 * 0.0892, 2 * 1.33e-2, 2 * 4.06e-3


def _ver():
    from accelerated_features_amd import verification
    return verification


def _mv():
    from accelerated_features_amd import multiview
    return multiview


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _filter(ia, ib, n, mask, keep=None, min_keep=0):
    r = _ver().filter_matches_batch(dev(ia), dev(ib), dev(n), dev(mask), None if keep is None else dev(keep), min_keep)
    torch.cuda.synchronize()
    return dict(zip(("idx_a", "idx_b", "n", "src", "info"), (t.cpu().numpy() for t in r)))


def _same_filter(got, want):
    for k in ("idx_a", "idx_b", "src", "n", "info"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


# ---- the filter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", VS.CAPS)
def test_filter_equals_the_restatement_as_bytes(cap):
    rng = np.random.default_rng(cap)
    L = 5
    for kind in ("random", "zeros", "ones"):                # ragged counts, one of them negative and one above cap
        ia, ib, n, mask = VS.filter_case(rng, L, cap, kind)
        _same_filter(_filter(ia, ib, n, mask), VR.filter_matches(ia, ib, n, mask))
    keep = np.array([1, 0, 1, 1, 0], np.uint8)
    count = int(VR.filter_matches(ia[:1], ib[:1], n[:1], mask[:1])["n"][0])
    for mk in sorted({0, count, count + 1}):                # at the first list's count: kept; one above: emptied
        want = VR.filter_matches(ia, ib, n, mask, keep, mk)
        assert want["info"][0, 2] == (VR.BY_MIN_KEEP if mk > count else VR.NONE) and want["info"][1, 2] == VR.BY_KEEP
        _same_filter(_filter(ia, ib, n, mask, keep, mk), want)
    # lists of shape (S, P, cap) and a bool mask
    ia3, ib3, n3, m3 = ia[:4].reshape(2, 2, cap), ib[:4].reshape(2, 2, cap), n[:4].reshape(2, 2), mask[:4].reshape(2, 2, cap)
    got = _filter(ia3, ib3, n3, m3 != 0, keep[:4].reshape(2, 2) != 0, 1)
    assert got["idx_a"].shape == (2, 2, cap) and got["n"].shape == (2, 2) and got["info"].shape == (2, 2, 4)
    _same_filter(got, VR.filter_matches(ia3, ib3, n3, m3, keep[:4].reshape(2, 2), 1))


def test_filter_over_more_lists_than_a_grid_dimension_and_two_calls():
    rng = np.random.default_rng(65537)
    L, cap = 65537, 3
    ia, ib = rng.integers(0, 1000, (L, cap)), rng.integers(0, 1000, (L, cap))
    n, mask = rng.integers(-1, cap + 2, L).astype(np.int32), rng.integers(0, 2, (L, cap)).astype(np.uint8)
    a, b = _filter(ia, ib, n, mask, None, 1), _filter(ia, ib, n, mask, None, 1)
    _same_filter(a, b)                                      # two calls give the same bytes
    m = np.clip(n, 0, cap)
    live = mask.astype(bool) & (np.arange(cap)[None] < m[:, None])
    c = live.sum(axis=1)
    assert np.array_equal(a["info"][:, 0], m) and np.array_equal(a["info"][:, 1], c) and np.array_equal(a["n"], c)   # (min_keep 1 empties only empty lists)
    assert np.array_equal(a["info"][:, 2], np.where(c < 1, 2, 0))
    order = np.argsort(~live, axis=1, kind="stable")        # the kept positions first, in their order
    want_src = np.where(np.arange(cap)[None] < c[:, None], order, -1)
    assert np.array_equal(a["src"], want_src)
    assert np.array_equal(a["idx_a"], np.where(want_src >= 0, np.take_along_axis(ia, np.maximum(want_src, 0), 1), -1))
    assert np.array_equal(a["idx_b"][-1], VR.filter_list(ia[-1], ib[-1], n[-1], mask[-1], 1, 1)[1])


# ---- the verifier -------------------------------------------------------------------------------------------------------------------------
def _verify(b, thr=1.0, n_views=True):
    mask, err, info = _ver().verify_matches_graph(dev(b["kpts"]), dev(b["view_pairs"]), dev(b["idx_a"]), dev(b["idx_b"]), dev(b["n_matches"]),
                                                  dev(b["n_views"]) if n_views else None, b["Ks"], b["Rs"], b["ts"], thr)
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), err=err.cpu().numpy(), info=info.cpu().numpy())


def _same_verify(got, want):
    VS.assert_clear_of_threshold(want["r2"], want["thr2"])    # no comparison of the case hangs on the last bit
    assert np.array_equal(got["info"], want["info"]), (got["info"].reshape(-1, 4)[:8], want["info"].reshape(-1, 4)[:8])
    assert np.array_equal(got["mask"], want["mask"])
    assert VS.same_bits(got["err"], want["err"])


@pytest.mark.parametrize("V,K,pairs", [(3, 1, "all"), (3, 64, "all"), (3, 300, "all"), (32, 64, "chain"), (32, 64, "all")])
def test_verify_equals_the_restatement(V, K, pairs):
    """Four scenes per case (verification_support.verify_batch): an illegal pair and a view out of range, ragged counts, indices out of
    range; equal poses (a zero baseline); a NaN pose; NaN pixels and a ragged n_views."""
    b = VS.verify_batch(1000 * V + K, V, K, TS.all_pairs(V) if pairs == "all" else TS.chain_pairs(V))
    want = VS.verify_batch_reference(b)
    st = want["info"][..., 0]
    assert {0, 1, 2, 3} <= set(st.reshape(-1).tolist())
    if K > 1:
        assert 0 < want["mask"].sum() < want["info"][..., 1].sum()
    _same_verify(_verify(b), want)
    if (V, K) == (3, 64):                                   # n_views None = V, another threshold; two calls give the same bytes
        nb = dict(b, n_views=np.full(4, V, np.int32))
        got = _verify(nb, 2.5, n_views=False)
        _same_verify(got, VS.verify_batch_reference(nb, 2.5))
        again = _verify(nb, 2.5, n_views=False)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _scene_args(scenes):
    st = lambda k: dev(np.stack([sc[k] for sc in scenes]))           # noqa: E731
    lists = [dev(np.stack([sc["lists"][i] for sc in scenes])) for i in range(4)]
    return (st("kpts"), lists[0], lists[1], lists[2], lists[3], None, st("Ks"))


def test_reconstruction_from_lists_with_wrong_matches_end_to_end():
    mv, ver = _mv(), _ver()
    sc = VS.wrong_scene(1)
    V, K = sc["kpts"].shape[:2]
    args = _scene_args([sc])
    raw = mv.reconstruct_graph_matches(*args)
    got = mv.reconstruct_graph_matches(*args, verified=True)
    rel = mv.relative_poses_graph_matches(*args[:5], args[6])
    torch.cuda.synchronize()
    print(f"raw lists: {int(raw['n_tracks'][0])} tracks; verified: {int(got['n_tracks'][0])} tracks, {int(got['valid'].sum())} valid points")
    assert int(raw["n_tracks"][0]) < 40                                        # 0.1 K (the restatement: 2)
    assert "n_verified" not in raw and torch.equal(raw["R_rel"], got["R_rel"]) and torch.equal(rel["R_rel"], got["R_rel"])
    # the compacted lists are the restatement's filter of the device's own masks
    vp, ia, ib, n = sc["lists"]
    keep = (rel["weight"][0] > 0).cpu().numpy().astype(np.uint8)
    want = VR.filter_matches(ia, ib, n, rel["inliers"][0].cpu().numpy(), keep)
    for key, k in (("idx_a_verified", "idx_a"), ("idx_b_verified", "idx_b"), ("n_verified", "n"), ("match_src", "src"), ("filter_info", "info")):
        g = got[key][0].cpu().numpy()
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), key
    assert keep.all() and int(want["n"].sum()) < int(n.sum())
    # the tables are the track graph's restatement on those lists
    tab = KR.build_tracks_graph(vp, want["idx_a"], want["idx_b"], want["n"], V, K)
    assert np.array_equal(got["tracks"][0].cpu().numpy(), tab["tracks"]) and np.array_equal(got["track_of"][0].cpu().numpy(), tab["track_of"])
    assert list(got["track_info"][0].cpu().numpy()) == list(tab["info"]) and int(got["n_tracks"][0]) == tab["n_tracks"]
    assert tab["n_tracks"] >= 360                                              # 0.9 K (the restatement: 391)
    assert got["pg_info"][0, 6].item() == 0 and got["pg_info"][0, 1].item() == V and got["ba_info"][0, 5].item() == 0
    rot, cen, pt = VS.chain_errors(sc, got["Rs"][0].cpu().numpy(), got["ts"][0].cpu().numpy(), tab["tracks"], got["points3d"][0].cpu().numpy(),
                                   got["valid"][0].cpu().numpy())
    print(f"verified chain: rotation {rot:.4f} deg, centres {cen:.3e}, median point error {pt:.3e} (bounds {ROT_DEG:.4f}, {CENTRE:.3e}, {POINT:.3e})")
    assert rot <= ROT_DEG and cen <= CENTRE and pt <= POINT
    assert int(got["valid"].sum()) >= 0.9 * tab["n_tracks"]

    # composition: the verifier on the raw lists under the refined poses -> the filter -> the track graph
    mask, err, info = ver.verify_matches_graph(*args[:5], None, args[6], got["Rs"], got["ts"])
    fa, fb, fn, src, finfo = ver.filter_matches_batch(args[2], args[3], args[4], mask, min_keep=15)
    tracks, track_of, n_tracks, tinfo = mv.build_tracks_graph(args[1], fa, fb, fn, V, K)
    torch.cuda.synchronize()
    bad = torch.from_numpy(sc["bad"]).cuda()[None]
    live = torch.arange(K, device="cuda")[None, None] < args[4][..., None]
    print(f"composition: {int(n_tracks[0])} tracks, {int(fn.sum())} of {int(args[4].sum())} entries kept, planted wrong entries kept "
          f"{int((mask.bool() & bad & live).sum())} of {int((bad & live).sum())}")
    assert (info[0, :, 0] == 0).all() and torch.equal(info[0, :, 2], fn[0]) and (finfo[0, :, 2] == 0).all()
    assert int(n_tracks[0]) >= 360                                             # (the restatement chain: 394, 388, 392 for the seeds 1 - 3)


def test_a_clean_scene_in_a_batch_gives_the_bytes_it_gives_alone():
    """Scene 0 of the batch has no wrong match, scene 1 has 20 %: scene 0's results are those of the call that holds it alone (its pairs
    keep their numbers, so its RANSAC draws are the same)."""
    mv = _mv()
    clean, noisy = VS.wrong_scene(2, wrong=0.0), VS.wrong_scene(1)
    alone = mv.reconstruct_graph_matches(*_scene_args([clean]), verified=True)
    both = mv.reconstruct_graph_matches(*_scene_args([clean, noisy]), verified=True)
    torch.cuda.synchronize()
    assert set(alone) == set(both) and {"idx_a_verified", "idx_b_verified", "n_verified", "match_src", "filter_info"} <= set(both)
    for k in sorted(alone):
        a, b = alone[k][0].cpu().numpy(), both[k][0].cpu().numpy()
        assert a.dtype == b.dtype and VS.same_bits(a, b), k
    assert int(both["n_tracks"][0]) >= 360 and int(both["n_tracks"][1]) >= 360
    # a clean list loses little: the Sampson error of a true match is the 0.5 px noise of two key-points projected on one normal, sigma 0.5 px,
    # so the 1 px gate is at 2 sigma and keeps 95.4 % in expectation, less what the estimate's own error takes; 0.9 leaves that room
    kept, total = int(both["n_verified"][0].sum()), int(clean["lists"][3].sum())
    print(f"clean scene: {kept} of {total} entries kept")
    assert kept > 0.9 * total
