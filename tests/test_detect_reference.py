"""tests/detect_reference.py against torch in float64, and the promises of the planted scenes (tests/detect_support.py) that tests/test_gpu_detect.py relies on.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detect_reference as DR
import detect_support as DS
from oracle import xfeat_oracle as O

H, W = DS.SPARSE_H, DS.SPARSE_W


@pytest.mark.parametrize("ks", [1, 3, 5, 7])
def test_nms_is_the_max_pool_formula(ks):
    """oracle/xfeat_oracle.py: (heat == max_pool2d(heat, ks, 1, ks // 2)) & (heat > thr), row-major"""
    n = 0
    for cls, thrs in DS.NMS_CLASSES.items():
        for Hm, Wm in ((1, 1), (2, 3), (17, 65), (35, 130)):
            maps = DS.nms_maps(cls, 3, Hm, Wm)
            for thr in thrs:
                want = O.nms(torch.from_numpy(maps).double()[:, None], thr, ks)
                for b in range(3):
                    got = DR.nms(maps[b], thr, ks)
                    assert got.dtype == np.int64 and np.array_equal(got, want[b].numpy()), (cls, Hm, Wm, thr, b)
                    n += len(got)
    assert n > 0


def _grid(ux, uy, Hm, Wm):
    """the float64 grid that puts grid_sample (align_corners=False) at the pixel coordinates (ux, uy)"""
    g = np.stack([(2.0 * ux.astype(np.float64) + 1.0) / Wm - 1.0, (2.0 * uy.astype(np.float64) + 1.0) / Hm - 1.0], -1)
    return torch.from_numpy(g)[None, None]


def _points(rng, n):
    ys = np.concatenate([[0, 0, H - 1, H - 1, 0, H // 2], rng.integers(0, H, n)])
    xs = np.concatenate([[0, W - 1, 0, W - 1, W // 2, 0], rng.integers(0, W, n)])
    return ys, xs


def test_sample_coord_is_the_oracles():
    rng = np.random.default_rng(1)
    ys, xs = _points(rng, 500)
    for Hm, Wm in ((H, W), (H // 8, W // 8)):
        ux, uy = O.sample_coords(torch.from_numpy(np.stack([xs, ys], -1)), H, W, Hm, Wm)
        assert np.array_equal(DR.sample_coord(xs, W, Wm), ux.numpy()) and np.array_equal(DR.sample_coord(ys, H, Hm), uy.numpy())
    assert DR.sample_coord(5, W, W).dtype == np.float32 and DR.sample_coord(np.array([5]), W, W).shape == (1,)


def test_scores_against_grid_sample():
    """nearest (round half to even, zeros outside) times bilinear (zeros outside) in float64 at the restatement's own fp32 coordinates; (0, 0) -> -1"""
    rng = np.random.default_rng(2)
    heat = rng.random((H, W)).astype(np.float32)
    rel = rng.random((H // 8, W // 8)).astype(np.float32)
    ys, xs = _points(rng, 3000)
    got = DR.scores(heat, rel, ys, xs)
    sn = F.grid_sample(torch.from_numpy(heat).double()[None, None], _grid(DR.sample_coord(xs, W, W), DR.sample_coord(ys, H, H), H, W), mode="nearest", align_corners=False)[0, 0, 0]
    sb = F.grid_sample(torch.from_numpy(rel).double()[None, None], _grid(DR.sample_coord(xs, W, W // 8), DR.sample_coord(ys, H, H // 8), H // 8, W // 8), mode="bilinear",
                       align_corners=False)[0, 0, 0]
    want = (sn * sb).numpy()
    origin = (xs == 0) & (ys == 0)
    assert origin.any() and (got[origin] == -1.0).all()
    assert np.abs(got - want)[~origin].max() <= 1e-14
    assert (got[(xs == W - 1) | (ys == H - 1)] == 0).all()          # nearest lands outside on the last row and column of this size


def test_descriptors_against_grid_sample():
    rng = np.random.default_rng(3)
    s = DS.planted_scene(7, H, W, 100, (0, 0), "random")
    s["feats"][14:18, 14:18] = 0.0
    ys, xs = _points(rng, 2000)
    ys, xs = np.concatenate([ys, [124, 127, 130]]), np.concatenate([xs, [124, 127, 130]])      # all sixteen taps inside the block of zero cells
    got = DR.descriptors(s["feats"], ys, xs, H, W)
    fn = F.normalize(torch.from_numpy(s["feats"]).double().permute(2, 0, 1)[None], dim=1)
    smp = F.grid_sample(fn, _grid(DR.sample_coord(xs, W, W // 8), DR.sample_coord(ys, H, H // 8), H // 8, W // 8), mode="bicubic", align_corners=False)[0, :, 0].T
    want = F.normalize(smp, dim=1).numpy()
    assert np.abs(got - want).max() <= 1e-12
    assert not got[-3:].any() and np.isfinite(got).all()
    inv = (1.0 / np.maximum(np.sqrt((s["feats"].astype(np.float64) ** 2).sum(-1)), 1e-12))
    assert np.array_equal(DR.descriptors(s["feats"], ys, xs, H, W, inv=inv), got)


def test_topk_order_is_a_stable_descending_sort():
    for cls in DS.DENSE_CLASSES:
        for n in (1, 2, 257, 4097):
            v = DS.dense_values(cls, n, 2)
            for b in range(2):
                want = torch.sort(torch.from_numpy(v[b]).double(), descending=True, stable=True).indices.numpy()
                for k in DS.dense_ks(n):
                    assert np.array_equal(DR.topk_order(v[b], k), want[:k])
                keys = DS.dense_keys(v[b])
                assert np.array_equal(np.argsort(keys, kind="stable"), want) and len(np.unique(keys)) == n


def test_dense_case_lists():
    assert DS.dense_shapes(257) == [(1, 257)] and DS.dense_shapes(4096) == [(1, 4096), (64, 64)] and DS.dense_shapes(20481) == [(1, 20481), (3, 6827)]
    assert DS.dense_ks(1) == [1] and DS.dense_ks(257) == [1, 2, 255, 256, 257] and DS.dense_ks(4097) == [1, 2, 255, 256, 257, 2048, 2049, 4096, 4097]
    for cls in DS.DENSE_CLASSES:
        v = DS.dense_values(cls, 300, 3)
        assert np.isfinite(v).all() and not np.signbit(v[v == 0]).any() and not np.array_equal(v[0], v[1])


@pytest.mark.parametrize("case", DS.sparse_scene_cases(), ids=lambda c: f"{c[1]}-{c[2][0]}{c[2][1]}-{c[3]}")
def test_planted_scene_promises(case):
    """exactly n candidates; at most 1 % of the neighbours in the restatement's sorted scores are closer than 2e-6 relative without being exact ties (the share whose order
    the GPU test leaves free)"""
    seed, n, origin, rel_kind = case
    s = DS.planted_scene(seed, H, W, n, origin, rel_kind)
    sites = s["sites"]
    got = DR.nms(s["heat"], DS.SPARSE_THR, 5)
    assert len(got) == n and np.array_equal(got, sites[:, ::-1])
    assert n == 0 or (s["heat"][sites[:, 0], sites[:, 1]] >= np.float32(0.06)).all()
    if origin == (0, 0) and n >= 3:
        assert (sites == 0).all(-1).any() and (sites[:, 1] == W - 1).any()
    if origin == (1, 0) and n >= 3:
        assert (sites[:, 0] == H - 1).any()
    assert (~s["feats"].any(-1)).sum() == DS.ZERO_CELLS
    norm = DR.bicubic_norm(s["feats"], sites[:, 0], sites[:, 1], H, W)
    assert ((norm >= DS.MIN_BICUBIC_NORM) | (norm == 0)).all()
    sc = np.sort(DR.scores(s["heat"], s["rel"], sites[:, 0], sites[:, 1]))[::-1]
    if n >= 2:
        gap = np.abs(np.diff(sc))
        near = (gap <= 2e-6 * np.maximum(np.abs(sc[:-1]), np.abs(sc[1:]))) & (gap != 0)
        share = near.sum() / (n - 1)
        print(f"n {n} {origin} {rel_kind}: unpinned share {share:.4%}, exact ties {(gap == 0).sum()}")
        assert share <= 0.01
    if rel_kind == "ones_zero_block" and n >= 2049:
        assert (sc == 0).sum() >= 100


def test_every_count_sees_both_origins_and_rel_kinds():
    cases = DS.sparse_scene_cases()
    assert {c[1] for c in cases} == set(DS.SPARSE_N)
    assert {(c[2], c[3]) for c in cases} == {(o, r) for o in DS.ORIGINS for r in DS.REL_KINDS}
    for n in DS.SPARSE_N:
        mine = [c for c in cases if c[1] == n]
        assert {c[2] for c in mine} == set(DS.ORIGINS) and {c[3] for c in mine} == set(DS.REL_KINDS)
