"""The float64 restatement of the match refinement (tests/refine_reference.py) against the fp32 torch oracle, the reference's golden rows and hand cases; the
generators of tests/refine_support.py.  CPU only."""
import os

import numpy as np
import pytest
import torch

import fixtures
import parity
import refine_reference as RR
import refine_support as RS
from oracle import xfeat_oracle as O

G = fixtures.GOLDEN_DIR


@pytest.fixture(scope="module")
def sd():
    return fixtures.synthetic_state_dict(0)


def _oracle_sets(s, p=None):
    sl = slice(None) if p is None else slice(p, p + 1)
    d0 = {"descriptors": torch.from_numpy(s["desc0"][sl]), "keypoints": torch.from_numpy(s["kp0"][sl]), "scales": torch.from_numpy(s["scale0"][sl])}
    d1 = {"descriptors": torch.from_numpy(s["desc1"][sl]), "keypoints": torch.from_numpy(s["kp1"][sl])}
    return d0, d1


@pytest.mark.parametrize("scale", [1.0, 1e-3, 300.0])
def test_fine_matcher_restatement_against_the_torch_oracle(sd, scale):
    v = torch.from_numpy((np.random.default_rng(3).standard_normal((257, 128)) * scale).astype(np.float32))
    truth = RR.fine_matcher(sd, v)
    got = O.fine_matcher(sd, v).numpy()
    assert truth.dtype == np.float64 and truth.shape == (257, 64)
    e = np.abs(got - truth).max() / np.abs(truth).max()
    print("fp32 oracle against float64, relative to max |logit|:", e)
    assert e <= 5e-6                     # (fp32 sums over 128 and four times 512 terms: ~7e-7 seen)


def test_refine_restatement_against_the_torch_oracle(sd):
    P, N = 3, 300
    s = RS.scene(11, P, N)
    n_matches = [N, 0, 123]
    conf = RR.confidence(RR.live_logits(sd, s["desc0"], s["desc1"], s["idx0"], s["idx1"], n_matches))
    fine_conf, gap = RS.pick_fine_conf(conf)
    assert gap >= 1e-4
    assert RR.confidence_margin(sd, s["desc0"], s["desc1"], s["idx0"], s["idx1"], n_matches, fine_conf) >= 0.5 * gap * (1 - 1e-9)
    rows, n_out, info = RR.refine(sd, s["desc0"], s["desc1"], s["kp0"], s["kp1"], s["scale0"], s["idx0"], s["idx1"], n_matches, fine_conf)
    d0, d1 = _oracle_sets(s)
    assert n_out[1] == 0 and 0 < n_out[0] < N and 0 < n_out[2] < 123          # mixed keep flags
    for p in range(P):
        m = [(torch.from_numpy(s["idx0"][q, :n_matches[q]]), torch.from_numpy(s["idx1"][q, :n_matches[q]])) for q in range(P)]
        r = O.refine_matches(sd, d0, d1, m, p, fine_conf=fine_conf).numpy()
        assert r.shape == rows[p].shape and len(info[p]["kept"]) == n_out[p] and len(info[p]["conf"]) == n_matches[p]
        assert np.array_equal(r[:, 2:], s["kp1"][p][s["idx1"][p, info[p]["kept"]]])          # the kept set, in match order
        assert np.array_equal(rows[p][:, 2:], r[:, 2:].astype(np.float64))
        if len(r):
            assert np.abs(r[:, :2] - rows[p][:, :2]).max() <= 5e-4           # (two ulps of a coordinate near 1600 and the fp32 oracle's own offset error)


def test_refine_restatement_clamps_counts_and_takes_repeated_indices(sd):
    s = RS.scene(5, 4, 40, N1=30, table_draw=RS.repeated_index_lists)
    assert s["idx1"].max() < 30 and s["idx0"].max() < 40 and len(np.unique(s["idx0"][0])) < 40
    rows, n_out, info = RR.refine(sd, s["desc0"], s["desc1"], s["kp0"], s["kp1"], s["scale0"], s["idx0"], s["idx1"], [-3, 900, 40, 7], 0.0)
    assert [len(i["conf"]) for i in info] == [0, 40, 40, 7]                  # fine_conf 0 keeps every live row
    assert n_out.tolist() == [0, 40, 40, 7] and rows[0].shape == (0, 4)
    assert np.array_equal(rows[3][:, 2:], s["kp1"][3][s["idx1"][3, :7]].astype(np.float64))
    assert RR.confidence_margin(sd, s["desc0"], s["desc1"], s["idx0"], s["idx1"], [0, 0, 0, 0], 0.25) == float("inf")


def test_restatement_against_the_reference_golden_rows(sd):
    g = np.load(os.path.join(G, "g4_dense.npz"))
    sa, sb = fixtures.shifted_pair(2, 160, 192, seed=31, shift=(8, 8))
    d0 = O.detect_and_compute_dense(sd, sa, top_k=512)
    d1 = O.detect_and_compute_dense(sd, sb, top_k=512)
    n = d0["keypoints"].shape[1]
    for b in range(2):
        perm = g[f"forced_perm{b}"]
        rows, n_out, _ = RR.refine(sd, d0["descriptors"][b:b + 1], d1["descriptors"][b:b + 1], d0["keypoints"][b:b + 1], d1["keypoints"][b:b + 1],
                                   d0["scales"][b:b + 1], np.arange(n)[None], perm[None], [n], 0.25)
        assert rows[0].shape == g[f"refine{b}"].shape and n_out[0] == len(g[f"refine{b}"])
        parity.assert_close(torch.from_numpy(rows[0]).float(), g[f"refine{b}"], 2e-4, "restatement vs golden")


def test_hand_cases_of_the_soft_argmax():
    for x, y in ((0, 0), (7, 0), (3, 5), (7, 7), (4, 4)):
        o = np.zeros((1, 64))
        o[0, 8 * y + x] = 50.0                       # softmax(3 o): the rest weighs e^-150
        assert np.allclose(RR.offsets(o), [[x - 4, y - 4]], atol=1e-12)
        assert abs(RR.confidence(o)[0] - 1.0) <= 1e-12
    for c in (0.0, -2.5, 1e3):
        o = np.full((2, 64), c)
        assert np.allclose(RR.offsets(o), [[-0.5, -0.5]] * 2, atol=1e-14)
        assert np.allclose(RR.confidence(o), 1.0 / 64, rtol=1e-14)


def test_generators_and_the_gap_helper():
    a, b = RS.scene(9, 2, 50, N1=20), RS.scene(9, 2, 50, N1=20)
    assert all(np.array_equal(a[k], b[k]) for k in a)                        # a seed names one scene
    assert np.allclose(np.linalg.norm(a["desc0"], axis=-1), 1.0, atol=1e-6) and a["desc1"].shape == (2, 20, 64)
    assert a["kp0"].min() >= 0 and a["kp0"].max() <= RS.GRID and np.array_equal(a["kp0"], np.round(a["kp0"]))
    assert all(len({tuple(r) for r in a["kp0"][p].tolist()}) == 50 for p in range(2))
    assert set(np.unique(a["scale0"]).tolist()) <= {np.float32(s) for s in RS.SCALES}
    assert all(sorted(a["idx0"][p].tolist()) == list(range(50)) for p in range(2))
    assert a["idx1"].shape == (2, 50) and a["idx1"].max() < 20 and sorted(a["idx1"][0, :20].tolist()) == list(range(20))
    f, gap = RS.pick_fine_conf([0.1, 0.21, 0.22, 0.28, 0.9])
    assert abs(f - 0.25) < 1e-12 and abs(gap - 0.06) < 1e-12
    f, gap = RS.pick_fine_conf([0.9])
    assert abs(f - 0.25) < 1e-12 and abs(gap - 0.1) < 1e-12


def test_bounds_helper_accepts_and_refuses():
    truth = np.array([[1000.0, 2.0]])
    RR.check_bounds("ok", truth, truth + 1e-6, truth + 3e-6, truth + 5e-6)
    with pytest.raises(AssertionError):
        RR.check_bounds("f32 off", truth, truth + 1e-6, truth + 6e-3, truth)
    with pytest.raises(AssertionError):
        RR.check_bounds("fx off", truth, truth + 1e-6, truth + 3e-6, truth + 2e-3)
    with pytest.raises(AssertionError):
        RR.check_bounds("nan", truth, truth, truth, truth * np.nan)
    # coordinates: two fp32 ulps of the coordinate join the floor (ulp(1000) = 6.1e-5), T is handed in
    RR.check_bounds("coord", truth, truth, truth + np.array([[1.2e-4, 0.0]]), truth, coord=truth, T=1.0)
    with pytest.raises(AssertionError):
        RR.check_bounds("coord small", truth, truth, truth + np.array([[0.0, 1.2e-4]]), truth, coord=truth, T=1.0)
