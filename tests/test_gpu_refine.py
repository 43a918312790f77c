"""The match refinement on the GPU against float64 (tests/refine_reference.py), on both kernel sets of the fine_matcher chain.

xfh_refine_matches = row map (refine_offsets_kernel, refine_rowmap_kernel) -> five fine_matcher layers (fine_chain: the fp16-pair kernels of launch_linear_fx by default, the
f32-MFMA kernels of launch_linear_mfma when option fx lacks FX_FINE, after the range fallback, or when a layer has no fp16-pair image) -> soft-argmax, confidence test and
ordered compaction (refine_rows_kernel, refine_compact_kernel).  xfh_fine_matcher runs the same chain on plain rows.

Every case runs on two models with the same weights: "fx" (default options) and "f32" (fx without FX_FINE).  Which chain a model runs is asserted through xfh_get_option; the
direct observable is the status word after an overflow (cases 6 and 7).  Inputs are synthetic tensors handed to XFeat._refine_device and XFeat.net.fine_matcher, all indices
inside their tables.  Bounds: refine_reference.check_bounds (e_f32 <= max(4 e_ref, 5e-6 T), e_fx <= max(2 e_f32, 1e-6 T), two fp32 ulps more for coordinates); counts, kept
sets and the second image's key-points are exact: every fine_conf is proven clear of a tie in float64 first.

Measured on an MI355X ("Refinement against float64"): worst error / bound 0.41 (f32) and 0.55 (fp16 pair) on the logits, 0.26 and 0.28 on rows with key-points
up to 1600, 0.72 and 0.29 with the key-points at the origin; the f32 chain's error is 1.1-4.8 times the torch oracle's, the pair chain's 0.5-1.1 times the f32 chain's."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import fixtures
import refine_reference as RR
import refine_support as RS
from oracle import xfeat_oracle as O

pytestmark = pytest.mark.gpu
CHAINS = ("f32", "fx")


@pytest.fixture(scope="module")
def sd():
    return fixtures.synthetic_state_dict(0)


def _models(weights):
    from accelerated_features_amd import XFeat
    from accelerated_features_amd.xfeat import DEFAULT_FX, FX_FINE
    fx, f32 = XFeat(weights=weights, top_k=512), XFeat(weights=weights, top_k=512)
    f32.set_option("fx", DEFAULT_FX & ~FX_FINE)
    return {"fx": fx, "f32": f32}


@pytest.fixture(scope="module")
def models(sd):
    return _models(sd)


def _assert_chains(models):
    """The option each handle holds: the default model has FX_FINE, the other one lacks it (and only it)."""
    from accelerated_features_amd import _lib
    from accelerated_features_amd.xfeat import DEFAULT_FX, FX_FINE
    lib, v = _lib.load(), C.c_int(-1)
    for name, want in (("fx", DEFAULT_FX), ("f32", DEFAULT_FX & ~FX_FINE)):
        assert lib.xfh_get_option(models[name].net.handle(), b"fx", C.byref(v)) == 0 and v.value == want, (name, v.value, want)
    assert DEFAULT_FX & FX_FINE


def _logits(m, v):
    return m.net.fine_matcher(torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()).cpu().numpy()


def _device_sets(s, gain=1.0):
    d0 = {"descriptors": torch.from_numpy(s["desc0"] * np.float32(gain)).cuda(), "keypoints": torch.from_numpy(s["kp0"]).cuda(), "scales": torch.from_numpy(s["scale0"]).cuda()}
    d1 = {"descriptors": torch.from_numpy(s["desc1"] * np.float32(gain)).cuda(), "keypoints": torch.from_numpy(s["kp1"]).cuda(), "scales": torch.ones(s["kp1"].shape[:2]).cuda()}
    return d0, d1


def _refine(m, s, n_matches, fine_conf, gain=1.0):
    """XFeat._refine_device on the scene -> (out (P, N, 4), n_out (P)) as numpy; rows at and beyond n_out are unspecified."""
    d0, d1 = _device_sets(s, gain)
    out, n_out = m._refine_device(d0, d1, torch.from_numpy(s["idx0"]).cuda(), torch.from_numpy(s["idx1"]).cuda(),
                                  torch.tensor(list(n_matches), dtype=torch.int32).cuda(), fine_conf)
    P, N = s["idx0"].shape
    assert out.shape == (P, N, 4) and out.dtype == torch.float32 and n_out.shape == (P,) and n_out.dtype == torch.int32
    return out.cpu().numpy(), n_out.cpu().numpy()


def _oracle_rows(sd, s, n_matches, fine_conf):
    """The fp32 torch oracle pair by pair (counts clamped on the host: the reference takes lists)."""
    P, N = s["idx0"].shape
    d0 = {"descriptors": torch.from_numpy(s["desc0"]), "keypoints": torch.from_numpy(s["kp0"]), "scales": torch.from_numpy(s["scale0"])}
    d1 = {"descriptors": torch.from_numpy(s["desc1"]), "keypoints": torch.from_numpy(s["kp1"])}
    n = np.clip(np.asarray(n_matches), 0, N)
    lists = [(torch.from_numpy(s["idx0"][p, :n[p]]), torch.from_numpy(s["idx1"][p, :n[p]])) for p in range(P)]
    return [O.refine_matches(sd, d0, d1, lists, p, fine_conf=fine_conf).numpy() for p in range(P)]


def _gap_conf(sd, s, n_matches):
    conf = RR.confidence(RR.live_logits(sd, s["desc0"], s["desc1"], s["idx0"], s["idx1"], n_matches))
    fine_conf, gap = RS.pick_fine_conf(conf)
    print(f"fine_conf {fine_conf:.6f} gap {gap:.3e} live {len(conf)} kept {(conf > fine_conf).mean() if len(conf) else 0:.3f}")
    assert gap >= 1e-4
    return fine_conf


def _check_rows(tag, sd, models, s, n_matches, fine_conf, chains=CHAINS, results=None):
    """Both chains against the restatement: n_out and the kept set exact (columns 2-3 are kp1[idx1] of the kept rows, bit for bit and in match order; key-points are distinct
    per pair), columns 0-1 inside the bounds."""
    truth, n_truth, info = RR.refine(sd, s["desc0"], s["desc1"], s["kp0"], s["kp1"], s["scale0"], s["idx0"], s["idx1"], n_matches, fine_conf)
    ref = _oracle_rows(sd, s, n_matches, fine_conf)
    got = {}
    for c in chains:
        out, n_out = results[c] if results else _refine(models[c], s, n_matches, fine_conf)
        assert np.array_equal(n_out, n_truth), (tag, c, n_out.tolist(), n_truth.tolist())
        rows = [out[p, :n_truth[p]] for p in range(len(n_truth))]
        for p, r in enumerate(rows):
            assert np.array_equal(r[:, 2:], truth[p][:, 2:].astype(np.float32)), (tag, c, p)
            assert ref[p].shape == r.shape, (tag, "oracle", p)
        got[c] = np.concatenate([r[:, :2] for r in rows])
    xy = np.concatenate([t[:, :2] for t in truth])
    shift = np.concatenate([i["shift"] for i in info])
    return RR.check_bounds(tag, xy, np.concatenate([r[:, :2] for r in ref]), got["f32"], got.get("fx"), coord=xy, T=float(shift.max()) if shift.size else 0.0)


# ---------------------------------------------------------------------------------------------------------------
# 1. logits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 2049])
def test_logits_against_float64_on_both_chains(sd, models, n):
    """xfh_fine_matcher at the 64-row wave tiles and 256-row blocks of both linear kernels, inputs of three magnitudes (hidden activations stay far below 65504)."""
    _assert_chains(models)
    rng = np.random.default_rng(100 + n)
    for scale in (1.0, 1e-3, 300.0):
        v = (rng.standard_normal((n, 128)) * scale).astype(np.float32)
        truth = RR.fine_matcher(sd, v)
        RR.check_bounds(f"logits n={n} scale={scale}", truth, O.fine_matcher(sd, torch.from_numpy(v)).numpy(), _logits(models["f32"], v), _logits(models["fx"], v))
    assert models["fx"].net.take_status() == 0 and models["f32"].net.take_status() == 0


# ---------------------------------------------------------------------------------------------------------------
# 2. one pair, full count, permuted lists, fine_conf inside the widest gap
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1023, 1024, 1025, 2500])
def test_one_pair_against_float64(sd, models, N):
    """The 256-row blocks of the chain and the 1024-thread rounds of refine_compact_kernel with mixed keep flags; idx0 and idx1 are permutations, so a kernel that took row
    r for idx[r] reads another key-point, scale and descriptor."""
    _assert_chains(models)
    s = RS.scene(200 + N, 1, N)
    assert N == 1 or (not np.array_equal(s["idx0"][0], np.arange(N)) and not np.array_equal(s["idx1"][0], np.arange(N)))
    fine_conf = _gap_conf(sd, s, [N])
    _check_rows(f"one pair N={N}", sd, models, s, [N], fine_conf)
    assert models["fx"].net.take_status() == 0 and models["f32"].net.take_status() == 0


def test_offsets_alone_against_float64(sd, models):
    """Key-points of the first image at the origin: columns 0-1 ARE offset times scale, so the bounds weigh the soft-argmax itself (behind a coordinate near 1600 half an
    ulp of the sum, 6e-5 px, hides it)."""
    _assert_chains(models)
    N = 1025
    s = RS.scene(250, 1, N)
    s["kp0"][:] = 0
    fine_conf = _gap_conf(sd, s, [N])
    _check_rows("offsets alone", sd, models, s, [N], fine_conf)


# ---------------------------------------------------------------------------------------------------------------
# 3. the default fine_conf
# ---------------------------------------------------------------------------------------------------------------
def test_default_fine_conf_counts_and_sets_are_exact(sd, models):
    _assert_chains(models)
    N = 4096
    for draw in range(20):
        s = RS.scene(300 + 1000 * draw, 1, N)
        margin = RR.confidence_margin(sd, s["desc0"], s["desc1"], s["idx0"], s["idx1"], [N], 0.25)
        if margin > 1e-5:
            break
    print("draw", draw, "margin", margin)
    assert margin > 1e-5
    _check_rows("fine_conf 0.25", sd, models, s, [N], 0.25)


# ---------------------------------------------------------------------------------------------------------------
# 4. ragged batch
# ---------------------------------------------------------------------------------------------------------------
def test_ragged_batch_with_padding_clamped_counts_and_repeats(sd, models):
    """P = 6 pairs of capacity 600 with counts [0, 600, 1, 257, 900, -3] (900 -> 600, -3 -> 0): the packed row list differs from p N + r, the second set has 520 rows
    (zero padded by _refine_device, its index lists repeat), pair 3 draws its idx0 with repeats.  Two calls: equal bytes."""
    _assert_chains(models)
    P, N, N1 = 6, 600, 520
    counts = [0, 600, 1, 257, 900, -3]
    s = RS.scene(400, P, N, N1=N1)
    s["idx0"][3] = RS.repeated_index_lists(np.random.default_rng(401), 1, N)[0]
    assert len(np.unique(s["idx0"][3, :257])) < 257 and s["idx1"].max() < N1 and s["desc1"].shape[1] == N1
    fine_conf = _gap_conf(sd, s, counts)
    results = {}
    for c in CHAINS:
        a, b = _refine(models[c], s, counts, fine_conf), _refine(models[c], s, counts, fine_conf)
        assert a[1].tobytes() == b[1].tobytes(), c
        for p in range(P):
            assert a[0][p, :a[1][p]].tobytes() == b[0][p, :b[1][p]].tobytes(), (c, p)
        results[c] = a
    assert results["f32"][1][0] == 0 and results["f32"][1][5] == 0 and 0 < results["f32"][1][4] < N
    _check_rows("ragged", sd, models, s, counts, fine_conf, results=results)


# ---------------------------------------------------------------------------------------------------------------
# 5. many pairs: the second round of the offsets scan; no live row at all
# ---------------------------------------------------------------------------------------------------------------
def test_many_pairs_and_no_live_rows(sd, models):
    _assert_chains(models)
    P, N = 1025, 8
    counts = [p % 9 for p in range(P)]
    s = RS.scene(500, P, N)
    fine_conf = _gap_conf(sd, s, counts)
    _check_rows("many pairs", sd, models, s, counts, fine_conf)
    s = RS.scene(501, 1, N)
    for c in CHAINS:
        out, n_out = _refine(models[c], s, [0], 0.25)
        assert n_out.tolist() == [0], c


# ---------------------------------------------------------------------------------------------------------------
# 6. the chain's range guard
# ---------------------------------------------------------------------------------------------------------------
OVERFLOW_GAIN = 2.0e4
OVERFLOW_NORM = 5.0


def _overflow_scene(sd, seed, N):
    """Descriptors of norm 5 (times OVERFLOW_GAIN at the call): in float64 the hidden activations then pass 1.1 x 65504.  (Unit-norm descriptors times 2e4 stay below 1.8e4
    with these weights: no overflow to report.)  -> (scene, the 128-wide rows the chain sees, the float64 maxima behind the four ReLUs)."""
    s = RS.scene(seed, 1, N, norm=OVERFLOW_NORM)
    v = np.concatenate([s["desc0"][0][s["idx0"][0]], s["desc1"][0][s["idx1"][0]]], -1) * np.float32(OVERFLOW_GAIN)
    hidden = []
    RR.fine_matcher(sd, v, hidden_max=hidden)
    print("float64 hidden maxima", hidden)
    assert max(hidden) > 1.1 * 65504
    return s, v, hidden


def test_chain_reports_its_range_and_the_f32_chain_carries_it(sd, models):
    """Descriptors times 2e4 that drive the hidden activations past 65504: the fp16-pair chain sets bit 0 of the status word (its output is unspecified), the f32 chain
    computes the same call with status 0, finite rows and logits inside the usual bound."""
    _assert_chains(models)
    N = 300
    s, v, _ = _overflow_scene(sd, 600, N)
    for m in models.values():
        m.net.take_status()
    _refine(models["fx"], s, [N], 0.25, gain=OVERFLOW_GAIN)
    assert models["fx"].net.take_status() & 1                     # ... so this model ran the fp16-pair kernels
    assert models["fx"].net.take_status() == 0
    out, n_out = _refine(models["f32"], s, [N], 0.25, gain=OVERFLOW_GAIN)
    assert models["f32"].net.take_status() == 0                   # ... and this one did not
    assert 0 <= n_out[0] <= N and np.isfinite(out[0, :n_out[0]]).all()
    RR.check_bounds("overflow logits, f32 chain", RR.fine_matcher(sd, v), O.fine_matcher(sd, torch.from_numpy(v)).numpy(), _logits(models["f32"], v))
    assert models["f32"].net.take_status() == 0


# ---------------------------------------------------------------------------------------------------------------
# 7. a fine layer without an fp16-pair image
# ---------------------------------------------------------------------------------------------------------------
def test_fine_layer_beyond_the_pair_range_runs_the_f32_chain(sd):
    """One folded weight of fine_matcher.3 is 40 (>= 31: xfh_create leaves the layer's fragments out).  A model with DEFAULT options must take the f32 kernels by itself:
    logits and rows equal the restatement on that state dict, status 0 -- also on the overflowing input of case 6, which the fp16-pair chain would flag."""
    from accelerated_features_amd import XFeat
    from accelerated_features_amd.spec import BN_EPS
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["fine_matcher.3.weight"][7, 11] = 40.0 * float(torch.sqrt(sd2["fine_matcher.4.running_var"][7].double() + BN_EPS))
    m = XFeat(weights=sd2, top_k=512)
    models = {"f32": m}
    v = np.random.default_rng(700).standard_normal((300, 128)).astype(np.float32)
    RR.check_bounds("weight 40: logits", RR.fine_matcher(sd2, v), O.fine_matcher(sd2, torch.from_numpy(v)).numpy(), _logits(m, v))
    N = 700
    s = RS.scene(701, 1, N)
    fine_conf = _gap_conf(sd2, s, [N])
    _check_rows("weight 40: rows", sd2, models, s, [N], fine_conf, chains=("f32",))
    assert m.net.take_status() == 0
    s, _, _ = _overflow_scene(sd2, 702, 300)
    out, n_out = _refine(m, s, [300], 0.25, gain=OVERFLOW_GAIN)
    assert m.net.take_status() == 0 and np.isfinite(out[0, :n_out[0]]).all()


# ---------------------------------------------------------------------------------------------------------------
# 8. match_xfeat_star repeats its call on the f32 kernels
# ---------------------------------------------------------------------------------------------------------------
def test_match_xfeat_star_repeats_on_the_f32_kernels(sd):
    from accelerated_features_amd import XFeat
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["skip1.1.bias"] = sd2["skip1.1.bias"] + 2.0e5
    a, b = XFeat(weights=sd2, top_k=512), XFeat(weights=sd2, top_k=512)
    b.set_option("fx", 0); b.set_option("block1", 5)
    ia, ib = fixtures.star_pair(2, 96, 128)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ra = a.match_xfeat_star(ia.cuda(), ib.cuda(), top_k=512)
    named = [x for x in w if "fp16-pair" in str(x.message)]
    assert len(named) == 1, [str(x.message) for x in w]
    assert a.net._options["fx"] == 0 and a.net._effective_option("block1") == 5
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rb = b.match_xfeat_star(ia.cuda(), ib.cuda(), top_k=512)
    assert not [x for x in w if "fp16-pair" in str(x.message)]
    assert isinstance(ra, list) and len(ra) == len(rb) == 2
    print("rows", [tuple(r.shape) for r in ra])
    for u, v in zip(ra, rb):
        assert u.shape == v.shape and u.shape[1] == 4 and len(u) > 0 and torch.equal(u, v)
