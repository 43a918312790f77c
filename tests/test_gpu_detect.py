"""The detection stage alone on the GPU (csrc/k_detect.hip), fed planted maps whose answer is known exactly; the restatement is tests/detect_reference.py, the inputs and call
helpers tests/detect_support.py.

  NMS      XFeat.NMS / xfh_nms against detect_reference.nms, exact: the zero-padding DPP kernel (threshold >= 0), the -inf-padding kernel (negative threshold), the generic
           window kernel (sizes 1, 3, 7) and the capacity clipping of the compaction, at the widths around one and two 64-lane words and the heights around one and two
           16-row strips, on maps full of plateaus, of negative values, of signed values and of isolated peaks.
  top-k    xfh_extract_dense: values in, permutation out -- cell_index is detect_reference.topk_order (value descending, index ascending) at every count around the sort's
           256-key wave blocks, the 2048-key runs, the four LDS runs and the five striding workgroups; the gathered rows and the key-points are exact.
           (tests/test_topk_emulated.py runs the same cases through the host emulation: this test adds that the hardware's lane exchanges are what the emulation assumes.)
  sparse   xfh_detect_sparse on planted scenes: counts, sites, key-points, order and padding exact; scores within 1e-6 relative and descriptors within 1.5e-6 of float64.

Where the bars come from ("Detection against planted maps"): a score is at most eight fp32 roundings from the restatement, which shares its fp32 coordinates
(8 * 2^-24 = 4.8e-7; the bar is twice that); the order is pinned wherever the restatement's scores differ by more than 2e-6 relative, twice the score bar; 1.5e-6 is what
tests/test_descriptor_emulated.py holds for descriptor_kernel against the same restatement (on maps without zero cells: detect_support.MIN_BICUBIC_NORM says what the planted
zero cells may do to a row's conditioning).  Nothing measured on a GPU enters them.

Measured on an MI355X: worst score error 1.97e-7 relative, worst descriptor error 8.2e-7; every test under half a second."""
import numpy as np
import pytest
import torch

import detect_reference as DR
import detect_support as DS
import fixtures

pytestmark = pytest.mark.gpu
H, W = DS.SPARSE_H, DS.SPARSE_W


@pytest.fixture(scope="module")
def xf():
    from accelerated_features_amd import XFeat
    m = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=4096, detection_threshold=0.05)
    assert m.dev.type == "cuda"
    return m


# ---------------------------------------------------------------------------------------------------------------
# 1. NMS
# ---------------------------------------------------------------------------------------------------------------
def _padded(lists):
    n = max(len(l) for l in lists)
    out = np.zeros((len(lists), n, 2), np.int64)
    for b, l in enumerate(lists):
        out[b, :len(l)] = l
    return out


def _check_nms(xf, cls, B, Hm, Wm, ks):
    maps = DS.nms_maps(cls, B, Hm, Wm)
    total = 0
    for thr in DS.NMS_CLASSES[cls]:
        want = _padded([DR.nms(maps[b], thr, ks) for b in range(B)])
        got = DS.call_nms(xf, maps, thr, ks)
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (cls, B, Hm, Wm, ks, thr, got.shape, want.shape)
        if cls == "negative":
            assert want.shape[1] == 0 if thr >= 0 else want.shape[1] > 0
        total += want.shape[1]
    return total


@pytest.mark.parametrize("Hm", DS.NMS_H)
def test_nms_5x5_both_paddings_are_exact(xf, Hm):
    """B = 3 different maps per shape; every class at a threshold >= 0 (nms_flags_zp_kernel) and at a negative one (nms_flags_kernel)"""
    total = 0
    for Wm in DS.NMS_W:
        for cls in DS.NMS_CLASSES:
            total += _check_nms(xf, cls, 3, Hm, Wm, 5)
    assert total > 0


@pytest.mark.parametrize("B", [8, 9])
def test_nms_5x5_both_workgroup_mappings(xf, B):
    for cls in DS.NMS_CLASSES:
        assert _check_nms(xf, cls, B, 35, 130, 5) > 0


@pytest.mark.parametrize("ks", [1, 3, 7])
def test_nms_generic_window_is_exact(xf, ks):
    for Hm, Wm in ((17, 65), (35, 130)):
        for cls in DS.NMS_CLASSES:
            assert _check_nms(xf, cls, 3, Hm, Wm, ks) > 0


@pytest.mark.parametrize("Hm,Wm,ks", [(1, 1, 5), (3, 200, 5), (16, 64, 5), (17, 65, 5), (35, 130, 5), (17, 65, 3), (35, 130, 7)])
def test_nms_capacity_clips_in_row_major_order(xf, Hm, Wm, ks):
    """capacity = max(1, n // 2): n_candidates stays the uncapped count, xy is the first `capacity` candidates in row-major order, the rows behind are zero"""
    clipped = 0
    for cls, thr in (("levels", 0.1), ("levels", -1.0), ("sparse", 0.5), ("negative", -10.0)):
        maps = DS.nms_maps(cls, 3, Hm, Wm, seed=1)
        want = [DR.nms(maps[b], thr, ks) for b in range(3)]
        counts = [len(w) for w in want]
        for sel in ([0], [1], [0, 1, 2]):                       # one image, another image, the batch (capacity from its largest count: some images fit, some do not)
            cap = max(1, max(counts[b] for b in sel) // 2)
            xy, nc = DS.call_nms_capacity(xf, maps[sel], thr, ks, cap)
            assert nc.tolist() == [counts[b] for b in sel], (cls, thr, sel)
            for i, b in enumerate(sel):
                m = min(counts[b], cap)
                assert np.array_equal(xy[i, :m], want[b][:m]) and not xy[i, m:].any(), (cls, thr, sel, b)
                clipped += counts[b] > cap
    assert clipped > 0 or Hm * Wm == 1


# ---------------------------------------------------------------------------------------------------------------
# 2. the top-k machinery through xfh_extract_dense
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DS.DENSE_N)
def test_dense_topk_is_the_exact_permutation(xf, n):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    calls = 0
    for B in DS.DENSE_B:
        feats = torch.randn((B, n, 64), generator=gen, device="cuda")
        rows = torch.arange(B, device="cuda")[:, None]
        for cls in DS.DENSE_CLASSES:
            vals = DS.dense_values(cls, n, B)
            order = np.stack([DR.topk_order(vals[b], n) for b in range(B)])
            if cls == "constant":
                assert np.array_equal(order, np.tile(np.arange(n), (B, 1)))
            vals_d, order_d = torch.from_numpy(vals).cuda(), torch.from_numpy(order.astype(np.int32)).cuda()
            rows_ref = feats[rows, order_d.long()].view(torch.int32)
            for hc, wc in DS.dense_shapes(n):
                for sd in DS.SCALE_DIVS:
                    kref = DS.dense_kpts(order, wc, sd)
                    kref_d = torch.from_numpy(kref).cuda()
                    ulp_d = torch.from_numpy(np.spacing(np.abs(kref))).cuda()
                    for k in DS.dense_ks(n):
                        kpts, desc, cell = DS.call_dense(xf, vals_d, feats, hc, wc, k, sd)
                        ok_cell = (cell == order_d[:, :k]).all()
                        ok_desc = (desc.view(torch.int32) == rows_ref[:, :k]).all()             # bit for bit feats[cell]
                        if sd in (1.0, 2.0):
                            ok_kp = (kpts.view(torch.int32) == kref_d[:, :k].view(torch.int32)).all()
                        else:                                                                    # a division that need not be exact: one ulp
                            ok_kp = ((kpts - kref_d[:, :k]).abs() <= ulp_d[:, :k]).all()
                        if not bool(ok_cell & ok_desc & ok_kp):
                            c = cell.cpu().numpy()
                            bad = np.argwhere(c != order[:, :k])
                            raise AssertionError((cls, B, (hc, wc), k, sd, bool(ok_cell), bool(ok_desc), bool(ok_kp), bad[:5].tolist(),
                                                  [(int(c[b, j]), int(order[b, j])) for b, j in bad[:5]]))
                        calls += 1
    print(f"n {n}: {calls} calls")


# ---------------------------------------------------------------------------------------------------------------
# 3. the sparse path on planted scenes
# ---------------------------------------------------------------------------------------------------------------
_SCENES = {}


def _scene(case):
    """the planted scene of a case of DS.sparse_scene_cases() with its restatement: scores and descriptors of every site (computed once, never changed)"""
    if case not in _SCENES:
        seed, n, origin, rel_kind = case
        s = DS.planted_scene(seed, H, W, n, origin, rel_kind)
        ys, xs = s["sites"][:, 0], s["sites"][:, 1]
        s["ref_scores"] = DR.scores(s["heat"], s["rel"], ys, xs)
        s["ref_desc"] = DR.descriptors(s["feats"], ys, xs, H, W)
        kx, ky = xs.astype(np.float32) * DS.RW, ys.astype(np.float32) * DS.RH
        s["kp_key"] = (kx.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ky.view(np.uint32).astype(np.uint64)      # the exact key-point (x rw, y rh) of each site
        assert len(np.unique(s["kp_key"])) == n
        s["kp_sort"] = np.argsort(s["kp_key"])
        for v in s.values():
            v.setflags(write=False)
        _SCENES[case] = s
    return _SCENES[case]


def _cases_of(n):
    return [c for c in DS.sparse_scene_cases() if c[1] == n]


WORST = {"score": 0.0, "desc": 0.0}


def _check_image(s, o, b, top_k, cap, tag):
    """every assertion of one image of one call; o: DS.call_sparse's dict"""
    sites, n = s["sites"], len(s["sites"])
    m = min(n, cap)                                       # the selection is over the first `cap` candidates in row-major order
    L = min(top_k, m)
    assert o["n_candidates"][b] == n, (tag, int(o["n_candidates"][b]), n)
    kp, sc, de, d16 = o["kpts"][b], o["scores"][b], o["desc"][b], o["desc_f16"][b]
    for name, a in (("kpts", kp), ("scores", sc), ("desc", de), ("desc_f16", d16)):
        assert not a[L:].view(np.uint16 if a.dtype == np.float16 else np.uint32).any(), (tag, name, "rows behind the list are not zero bits")
    nv = int(o["n_valid"][b])
    assert nv == int((sc[:L] > 0).sum()) and (sc[:nv] > 0).all(), (tag, "n_valid", nv)
    if L == 0:
        return
    # every returned key-point is a planted site among the first m, none twice, its coordinates exactly (x rw, y rh)
    key = (kp[:L, 0].view(np.uint32).astype(np.uint64) << np.uint64(32)) | kp[:L, 1].view(np.uint32).astype(np.uint64)
    pos = np.searchsorted(s["kp_key"][s["kp_sort"]], key)
    idx = s["kp_sort"][np.minimum(pos, n - 1)]
    assert np.array_equal(s["kp_key"][idx], key) and (idx < m).all() and len(np.unique(idx)) == L, (tag, "key-points")
    ys, xs = sites[idx, 0], sites[idx, 1]
    # scores
    ref = s["ref_scores"][idx]
    err = np.abs(sc[:L].astype(np.float64) - ref)
    rel_err = float((err / np.maximum(np.abs(ref), 1e-300))[ref != 0].max()) if (ref != 0).any() else 0.0
    WORST["score"] = max(WORST["score"], rel_err)
    assert (err <= 1e-6 * np.abs(ref)).all(), (tag, "scores", rel_err)
    origin_px = (xs == 0) & (ys == 0)
    assert (sc[:L][origin_px] == -1.0).all()
    border = ((xs == W - 1) | (ys == H - 1)) & ~origin_px
    zero = (ref == 0)
    assert zero[border].all() and not (sc[:L][zero].view(np.uint32)).any(), (tag, "exact +0 scores")
    assert (np.diff(sc[:L]) <= 0).all(), (tag, "not sorted")
    # order: wherever the restatement's neighbours differ by more than 2e-6 relative, position j holds a candidate of the restatement's group at position j
    r = s["ref_scores"][:m]
    order = np.lexsort((np.arange(m), -r))
    rs = r[order]
    pinned = np.abs(np.diff(rs)) > 2e-6 * np.maximum(np.abs(rs[:-1]), np.abs(rs[1:]))
    gid = np.concatenate([[0], np.cumsum(pinned)])
    gid_of = np.empty(m, np.int64)
    gid_of[order] = gid
    assert np.array_equal(gid_of[idx], gid[:L]), (tag, "order or cut", int(np.flatnonzero(gid_of[idx] != gid[:L])[0]))
    # bit-equal neighbours: candidate (row-major) order
    eq = sc[:L - 1].view(np.uint32) == sc[1:L].view(np.uint32)
    assert (idx[:-1][eq] < idx[1:][eq]).all(), (tag, "ties out of candidate order")
    # descriptors
    assert np.isfinite(de[:L]).all()
    rd = s["ref_desc"][idx]
    derr = float(np.abs(de[:L] - rd).max())
    WORST["desc"] = max(WORST["desc"], derr)
    assert derr <= 1.5e-6, (tag, "desc", derr)
    dead = ~rd.any(-1)
    assert not de[:L][dead].view(np.uint32).any(), (tag, "all-zero neighbourhoods")
    assert np.array_equal(d16[:L].view(np.uint16), (de[:L] * np.float32(256.0)).astype(np.float16).view(np.uint16)), (tag, "desc_f16")
    return int(eq.sum()), int(dead.sum())


def _caps(n):
    return sorted({c for c in (H * W, 6000, 2048, n - 1) if 1 <= c <= H * W}, reverse=True)


@pytest.mark.parametrize("n", DS.SPARSE_N)
def test_sparse_planted_scenes(xf, n):
    ties = dead = 0
    for case in _cases_of(n):
        s = _scene(case)
        for cap in _caps(n):
            for top_k in DS.SPARSE_TOP_K + ((n,) if n > max(DS.SPARSE_TOP_K) else ()):       # (top_k = n: the whole sorted list, the zero-score tie group included)
                o = DS.call_sparse(xf, [s], top_k, cap)
                r = _check_image(s, o, 0, top_k, cap, (case, top_k, cap))
                if r:
                    ties += r[0]; dead += r[1]
    print(f"n {n}: bit-equal neighbours {ties}, all-zero neighbourhoods {dead}, worst score error {WORST['score']:.3g} (relative), worst descriptor error {WORST['desc']:.3g}")
    if n >= 2049:
        assert ties >= 100          # the zero block (576 lattice sites at full density) and the last row and column: equal keys across run boundaries


def test_sparse_ragged_batch(xf):
    """B = 3 with n = [0, 257, 2049]: the lists fill top_k differently"""
    scenes = [_scene(_cases_of(n)[0]) for n in (0, 257, 2049)]
    for top_k in (300, 2048, 4096):
        for cap in (H * W, 2048):
            o = DS.call_sparse(xf, scenes, top_k, cap)
            for b, s in enumerate(scenes):
                _check_image(s, o, b, top_k, cap, ("ragged", b, top_k, cap))


def test_sparse_all_zero_features_give_zero_rows(xf):
    """every neighbourhood all-zero: F.normalize divides 0 by 1e-12 -- zero rows, never NaN (_check_image: rows whose restatement is zero are zero bits)"""
    s = dict(_scene(_cases_of(2049)[0]))
    s["feats"] = np.zeros_like(s["feats"])
    s["ref_desc"] = DR.descriptors(s["feats"], s["sites"][:, 0], s["sites"][:, 1], H, W)
    assert not s["ref_desc"].any()
    o = DS.call_sparse(xf, [s], 4096, H * W)
    assert _check_image(s, o, 0, 4096, H * W, "zero feats")[1] == 2049


@pytest.mark.parametrize("B", [8, 9])
def test_sparse_batches_of_repeats_equal_single_images(xf, B):
    """both workgroup mappings: every image of the batch is bit-identical to its B = 1 run"""
    base = [_scene(_cases_of(n)[0]) for n in (2049, 0, 10241, 257)]
    top_k, cap = 4096, 6000
    single = [DS.call_sparse(xf, [s], top_k, cap) for s in base]
    for i, s in enumerate(base):
        _check_image(s, single[i], 0, top_k, cap, ("single", i))
    o = DS.call_sparse(xf, [base[b % 4] for b in range(B)], top_k, cap)
    for b in range(B):
        for name, a in o.items():
            assert a[b].tobytes() == single[b % 4][name][0].tobytes(), (B, b, name)
