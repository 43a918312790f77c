"""xfh_match_mnn_guided (csrc/k_match_guided.hip) and accelerated_features_amd.guided on the MI355X against the float64 checker of
tests/guided_reference.py: tile and chunk boundaries, ragged batches, the XCD mapping, the strided counts, the exactly representable
boundary fixtures, the wide gate against the exact plain matcher, empty rows / columns, invalid models, and the callers
(rematch_fundamental, ReferenceTracker(guided=True), match_guided)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fixtures
import guided_reference as GR
import twoview_support as TS

pytestmark = pytest.mark.gpu


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def _run(s, thr, model=None, min_cossim=-1.0, kind=None):
    """One scene as a batch of one through match_guided_device: (idx0, idx1) numpy."""
    from accelerated_features_amd.guided import match_guided_device
    model = s['model'] if model is None else model
    n1 = torch.tensor([len(s['d1'])], dtype=torch.int32).cuda()
    n2 = torch.tensor([len(s['d2'])], dtype=torch.int32).cuda()
    i0, i1, n = match_guided_device(_t(s['d1'])[None], _t(s['k1'])[None], n1, _t(s['d2'])[None], _t(s['k2'])[None], n2,
                                    _t(np.asarray(model, np.float64).reshape(1, 3, 3)), kind or s['kind'], thr, min_cossim)
    k = int(n.item())
    return i0[0, :k].cpu().numpy(), i1[0, :k].cpu().numpy()


@pytest.mark.parametrize("kind", GR.KINDS)
@pytest.mark.parametrize("n1,n2,thr", [(1, 1, 3.0), (31, 33, 3.0), (257, 129, 1.0), (300, 1025, 3.0), (1300, 1100, 2.0)])
def test_guided_matches_against_float64(kind, n1, n2, thr):
    """(1300, 1100) crosses a 256-row block, a 128-column fill and the finalize's 1024-row chunk."""
    s = GR.scene(kind, n1, n2, 100 + n1)
    i0, i1 = _run(s, thr)
    must, und = GR.check_guided_mnn_fp64(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, thr, i0, i1)
    print(f"{kind} {n1} x {n2}: {len(i0)} matches, {must} strict, {und} undecided, true {GR.true_matches(s, i0, i1)} of {len(s['truth'])}")
    assert must >= min(1, len(s['truth'])) and len(i0) >= must


@pytest.mark.parametrize("kind", GR.KINDS)
@pytest.mark.parametrize("P", [3, 16])
def test_ragged_batches(kind, P):
    """P = 3: plain order of the workgroups; P = 16: xcd_group_map swizzles (a multiple of 8).  Every pair its own scene, counts and model; one pair
    empty, one with an all-zero model."""
    from accelerated_features_amd.guided import match_guided_device
    N1, N2 = 300, 280
    rng = np.random.default_rng(P)
    sc = [GR.scene(kind, N1, N2, 1000 + 10 * P + p) for p in range(P)]
    c1 = rng.integers(1, N1 + 1, P)
    c2 = rng.integers(1, N2 + 1, P)
    c1[0], c2[0] = N1, N2
    c1[1] = 0
    models = np.stack([s['model'] for s in sc])
    models[2] = 0
    a = [_t(np.stack([s[k] for s in sc])) for k in ('d1', 'k1', 'd2', 'k2')]
    i0, i1, n = match_guided_device(a[0], a[1], _t(c1, torch.int32), a[2], a[3], _t(c2, torch.int32), _t(models), kind, 3.0, 0.3)
    n = n.cpu().numpy()
    assert n[1] == 0 and n[2] == 0
    tot = 0
    for p in range(P):
        if p in (1, 2):
            continue
        s = sc[p]
        must, _ = GR.check_guided_mnn_fp64(s['d1'][:c1[p]], s['d2'][:c2[p]], s['k1'][:c1[p]], s['k2'][:c2[p]], s['model'], kind, 3.0,
                                           i0[p, :n[p]].cpu().numpy(), i1[p, :n[p]].cpu().numpy(), 0.3)
        tot += must
    assert tot > 10 * (P - 2)


def test_strided_counts_through_the_c_entry():
    """n_stride = 2, n_offset2 = 1: the n_valid array of one detection batch addresses consecutive frame pairs, as for xfh_match_mnn; descriptors and
    key-points of pair p are frames 2p and 2p + 1 of one buffer (pair strides of two frames)."""
    from accelerated_features_amd import _lib
    lib = _lib.load()
    K, P = 200, 2
    sc = [GR.scene('fundamental', K, K, 60 + p) for p in range(P)]
    desc = _t(np.stack([v for s in sc for v in (s['d1'], s['d2'])]))          # (2P, K, 64)
    kpts = _t(np.stack([v for s in sc for v in (s['k1'], s['k2'])]))
    nv = _t(np.array([150, 200, 200, 90], np.int32))
    models = _t(np.stack([s['model'] for s in sc]))
    i0 = torch.empty((P, K), dtype=torch.int64).cuda()
    i1 = torch.empty_like(i0)
    n = torch.empty((P,), dtype=torch.int32).cuda()
    nb = lib.xfh_match_guided_workspace_bytes(P, K, K)
    ws = torch.empty(nb + 256, dtype=torch.uint8).cuda()
    off = (-ws.data_ptr()) % 256
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.xfh_match_mnn_guided(p(desc), 2 * K * 64, p(desc[1]), 2 * K * 64, p(kpts), 2 * K * 2, p(kpts[1]), 2 * K * 2, p(nv), p(nv), 2, 1, P, K, K,
                                        p(models), 0, 3.0, -1.0, p(i0), p(i1), p(n), C.c_void_p(ws.data_ptr() + off), nb,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "xfh_match_mnn_guided")
    nm = n.cpu().numpy()
    for q, (a, b) in enumerate(((150, 200), (200, 90))):
        s = sc[q]
        must, _ = GR.check_guided_mnn_fp64(s['d1'][:a], s['d2'][:b], s['k1'][:a], s['k2'][:b], s['model'], 'fundamental', 3.0, i0[q, :nm[q]].cpu().numpy(),
                                           i1[q, :nm[q]].cpu().numpy())
        assert must > 20
    # argument errors: no launch, an error code and a message
    bad = lambda kind, thr: lib.xfh_match_mnn_guided(p(desc), 2 * K * 64, p(desc[1]), 2 * K * 64, p(kpts), 2 * K * 2, p(kpts[1]), 2 * K * 2, p(nv), p(nv), 2, 1, P, K, K,
                                                     p(models), kind, thr, -1.0, p(i0), p(i1), p(n), C.c_void_p(ws.data_ptr() + off), nb, None)
    for kind, thr in ((0, 0.0), (1, -1.0), (0, float('nan')), (1, float('inf')), (2, 3.0)):
        assert bad(kind, thr) != 0
    assert b"xfh_match_mnn_guided" in lib.xfh_last_error()


def test_exact_fixtures_equal_the_restatement():
    for s, thr_of in ((GR.horizontal_fixture(), GR.sampson_threshold_at), (GR.translation_fixture(), float)):
        for k in range(4):
            thr = thr_of(float(s['dys'][k]))
            i0, i1 = _run(s, thr)
            w0, w1 = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], s['kind'], thr)
            assert i0.tolist() == w0.tolist() and i1.tolist() == w1.tolist() == [4 * i + k for i in range(6)]


@pytest.fixture(scope="module")
def xf():
    from accelerated_features_amd import XFeat
    return XFeat(weights=fixtures.synthetic_state_dict(0), top_k=1024, detection_threshold=0.05)


def test_wide_gate_equals_the_exact_plain_matcher(xf):
    """H = identity at max_error 1e6: everything passes, and the result is xfh_match_mnn's with match_exact = 1 pair for pair."""
    from accelerated_features_amd.guided import match_guided_device
    P, K = 3, 700
    sc = [GR.scene('homography', K, K, 300 + p) for p in range(P)]
    d1, k1, d2, k2 = (_t(np.stack([s[k] for s in sc])) for k in ('d1', 'k1', 'd2', 'k2'))
    na, nb = _t(np.array([700, 1, 333], np.int32)), _t(np.array([650, 700, 257], np.int32))
    eye = torch.eye(3, dtype=torch.float64).cuda().expand(P, 3, 3).contiguous()
    for mc in (-1.0, 0.8):
        g0, g1, gn = match_guided_device(d1, k1, na, d2, k2, nb, eye, 'homography', 1e6, mc)
        xf.set_option("match_exact", 1)
        try:
            e0, e1, en = xf.match_sets_device(d1, na, d2, nb, mc)
        finally:
            xf.set_option("match_exact", 0)
        assert torch.equal(gn, en) and int(gn.sum()) > 100
        for p in range(P):
            k = int(gn[p])
            assert torch.equal(g0[p, :k], e0[p, :k]) and torch.equal(g1[p, :k], e1[p, :k])


@pytest.mark.parametrize("kind", GR.KINDS)
def test_edge_cases(kind):
    from accelerated_features_amd import _lib
    from accelerated_features_amd.guided import match_guided_device
    # an empty row 0 together with an empty column 0, their descriptors each other's best, the similarity cut disabled
    s = GR.scene(kind, 31, 33, 131)
    s['k1'][0] = (-5.0e4, 7.0e4)
    s['k2'][0] = (9.0e4, -6.0e4)
    s['d2'][0] = s['d1'][0]
    passes, _ = GR.gate(s['k1'], s['k2'], s['model'], kind, 3.0)
    assert not passes[0].any() and not passes[:, 0].any()
    i0, i1 = _run(s, 3.0)
    assert 0 not in i0.tolist() and 0 not in i1.tolist() and len(i0) > 5
    GR.check_guided_mnn_fp64(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, 3.0, i0, i1)
    # invalid models
    s = GR.scene(kind, 31, 33, 131)
    assert len(_run(s, 3.0)[0]) > 5
    assert len(_run(s, 3.0, model=np.zeros((3, 3)))[0]) == 0
    for v in (np.nan, np.inf):
        bad = np.array(s['model'], np.float64)
        bad[1, 1] = v
        assert len(_run(s, 3.0, model=bad)[0]) == 0
    # duplicates inside the gate: the lowest index wins, in both directions
    s = GR.scene(kind, 70, 45, 99)
    r = int(np.argmin(s['truth'][:20]))
    a = int(s['truth'][r])
    b = 44 if a != 44 else 43
    s['d2'][b], s['k2'][b] = s['d2'][a], s['k2'][a]
    s['d1'][69], s['k1'][69] = s['d1'][r], s['k1'][r]
    i0, i1 = _run(s, 3.0)
    got = dict(zip(i0.tolist(), i1.tolist()))
    assert got.get(r) == a and 69 not in got and b not in i1.tolist()
    # the padding lanes: rows 30 and 31 of the tile are copies of row 29, whose descriptor is column j's best but whose place fails j's gate; behind the count
    # sits row 0's place, which passes it.  A copy that took its constants from there would take column j from row 0.
    s = GR.scene(kind, 40, 40, 5)
    j = int(s['truth'][0])
    s['d1'][29] = s['d2'][j]
    s['d1'][30:] = s['d1'][29]
    s['k1'][30:] = s['k1'][0]
    assert not GR.gate(s['k1'][:30], s['k2'], s['model'], kind, 3.0)[0][29, j]
    n1 = torch.tensor([30], dtype=torch.int32).cuda()
    n2 = torch.tensor([40], dtype=torch.int32).cuda()
    i0, i1, n = match_guided_device(_t(s['d1'])[None], _t(s['k1'])[None], n1, _t(s['d2'])[None], _t(s['k2'])[None], n2, _t(np.asarray(s['model'], np.float64)[None]),
                                    kind, 3.0, -1.0)
    k = int(n.item())
    i0, i1 = i0[0, :k].cpu().numpy(), i1[0, :k].cpu().numpy()
    GR.check_guided_mnn_fp64(s['d1'][:30], s['d2'], s['k1'][:30], s['k2'], s['model'], kind, 3.0, i0, i1)
    assert int(i0.max()) < 30 and dict(zip(i0.tolist(), i1.tolist())).get(0) == j
    with pytest.raises(_lib.XFeatHipError):
        _run(s, 0.0)
    with pytest.raises(_lib.XFeatHipError):
        _run(s, float('nan'))


def _rematch(s):
    from accelerated_features_amd.guided import rematch_fundamental
    K = max(len(s['d1']), len(s['d2']))
    pad = lambda v: np.r_[v, np.zeros((K - len(v),) + v.shape[1:], v.dtype)]
    r = rematch_fundamental(_t(pad(s['k1']))[None], _t(pad(s['d1']))[None], _t(np.array([len(s['d1'])], np.int32)), _t(pad(s['k2']))[None], _t(pad(s['d2']))[None],
                            _t(np.array([len(s['d2'])], np.int32)), ransac_thr=2.0, seed=1)
    out = {}
    for st, i0, i1, n in (('first', 'idx0_first', 'idx1_first', 'n_first'), ('second', 'idx0', 'idx1', 'n_matches')):
        k = int(r[n][0])
        out[st] = dict(inl=int(r[st]['info'][0, 3]), found=int(r[st]['info'][0, 0]), dist=TS.f_distance(r[st]['F'][0].cpu().numpy(), s['model']) if int(r[st]['info'][0, 0]) else 2.0,
                       true=GR.true_matches(s, r[i0][0, :k].cpu().numpy(), r[i1][0, :k].cpu().numpy()), n=k)
    return out


def test_rematch_fundamental_on_the_distractor_fixture():
    """Plain matcher -> F -> guided matcher -> F on the fixture whose every image-0 descriptor has an exact copy at a random place in image 1: the second
    stage has at least the first stage's inliers and its F is no farther from the true one (f_distance; 2.0 = nothing found)."""
    o = _rematch(GR.distractor_scene())
    print(f"distractor fixture: {o}")
    assert o['second']['inl'] >= o['first']['inl']
    assert o['second']['dist'] <= o['first']['dist']


def test_rematch_fundamental_recovers_the_matches_behind_partial_distractors():
    """Half of the image-0 descriptors have a copy elsewhere: the first stage estimates F from the other half, the guided stage gets the rest back."""
    s = GR.distractor_scene()
    keep = len(s['d2']) - len(s['truth']) // 2
    s['d2'], s['k2'] = s['d2'][:keep], s['k2'][:keep]
    o = _rematch(s)
    print(f"partial distractors: {o}")
    n = len(s['truth'])
    assert o['first']['found'] and o['second']['found']
    assert o['first']['true'] < 0.6 * n and o['second']['true'] >= 0.95 * n
    assert o['second']['inl'] >= o['first']['inl'] and o['second']['dist'] <= max(o['first']['dist'], 1e-3)


class _Stream:
    """What ReferenceTracker asks of an XFeat, fed with prepared detections: frame f is the key of a dict of (kpts, desc, n_valid)."""

    def __init__(self, xf, frames):
        self.xf, self.frames, self.net = xf, frames, xf.net

    def parse_input(self, f):
        return f

    def _detect_device(self, f, top_k):
        kp, de, nv = self.frames[f]
        return kp, None, de, nv, nv, top_k, None

    def match_sets_device(self, *a):
        return self.xf.match_sets_device(*a)


def _tracker_frames(B, K, n, distract):
    """B streams: a reference of n points, two frames under each stream's homography (the second moved on by (1.5, -1) px), the first n / 2 reference
    descriptors copied to random places in both frames when `distract`."""
    ref, f1, f2 = [], [], []
    for b in range(B):
        rng = np.random.default_rng(40 + b)
        p0, p1, H, _ = TS.homography_pair(n, 0.0, 0.3, 70 + b)
        d0 = GR.unit_rows(rng, n)
        for dst, shift in ((f1, (0.0, 0.0)), (f2, (1.5, -1.0))):
            t = d0.astype(np.float64) + 0.03 * rng.normal(size=d0.shape)
            d = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
            k = (p1 + np.float32(shift)).astype(np.float32)
            if distract:
                k = np.r_[k, np.c_[rng.uniform(0, 640, n // 2), rng.uniform(0, 480, n // 2)].astype(np.float32)]
                d = np.r_[d, d0[:n // 2]]
            perm = rng.permutation(len(k))
            dst.append((k[perm], d[perm]))
        ref.append((p0, d0))

    def pack(lst):
        kp, de = np.zeros((B, K, 2), np.float32), np.zeros((B, K, 64), np.float32)
        for b, (k, d) in enumerate(lst):
            kp[b, :len(k)], de[b, :len(k)] = k, d
        return _t(kp), _t(de), _t(np.array([len(k) for k, _ in lst], np.int32))
    return {'ref': pack(ref), 1: pack(f1), 2: pack(f2)}


def test_reference_tracker_guided(xf):
    from accelerated_features_amd.homography import ReferenceTracker, find_homography_matches
    B, K, n = 2, 1024, 400
    # guided=False is today's path, bit for bit: match_sets_device -> find_homography_matches
    fr = _tracker_frames(B, K, n, False)
    tr = ReferenceTracker(_Stream(xf, fr), top_k=K, min_cossim=0.5, min_inliers=50, seed=3)
    tr.set_reference('ref')
    r = tr.track(1)
    i0, i1, nm = xf.match_sets_device(fr['ref'][1], fr['ref'][2], fr[1][1], fr[1][2], 0.5)
    w = find_homography_matches(fr['ref'][0], fr[1][0], i0, i1, nm, 4.0, 700, 0.995, 3)
    assert torch.equal(r['n_matches'], nm) and all(torch.equal(r[k], w[k]) for k in ('H', 'inliers', 'info')) and 'guided' not in r
    assert r['valid'].cpu().tolist() == [True] * B
    # with distractors: the guided tracker has at least the plain tracker's inliers on the second frame (the first has no H to guide with)
    fr = _tracker_frames(B, K, n, True)
    res = {}
    for g in (False, True):
        tr = ReferenceTracker(_Stream(xf, fr), top_k=K, min_cossim=0.5, min_inliers=50, seed=3, guided=g, guide_thr=8.0)
        tr.set_reference('ref')
        first = tr.track(1)
        res[g] = tr.track(2)
        if g:
            assert first['guided'].cpu().tolist() == [False] * B and torch.equal(first['H'], plain_first['H'])
        plain_first = first
    a, b = res[False]['info'][:, 3].cpu().numpy(), res[True]['info'][:, 3].cpu().numpy()
    print(f"tracker inliers on frame 2: plain {a.tolist()}, guided {b.tolist()}, guided flags {res[True]['guided'].cpu().tolist()}")
    assert (b >= a).all() and res[True]['valid'].cpu().tolist() == [True] * B
    assert res[True]['guided'].cpu().tolist() == [True] * B and (b >= 0.9 * n).all()


def test_match_guided_equals_match_guided_device():
    from accelerated_features_amd.guided import fundamental_from_pose, match_guided
    for kind in GR.KINDS:
        s = GR.scene(kind, 300, 280, 8)
        i0, i1 = _run(s, 3.0)
        j0, j1 = match_guided({'keypoints': _t(s['k1']), 'descriptors': _t(s['d1'])}, {'keypoints': _t(s['k2']), 'descriptors': _t(s['d2'])}, s['model'], kind, 3.0)
        assert j0.cpu().numpy().tolist() == i0.tolist() and j1.cpu().numpy().tolist() == i1.tolist() and len(i0) > 100
    f = TS.fixture()
    T = f["T_0to1"][7]
    F = fundamental_from_pose(torch.from_numpy(T[:3, :3].copy()), torch.from_numpy(T[:3, 3].copy()), torch.from_numpy(f["K0"][7]), torch.from_numpy(f["K1"][7]))
    assert TS.f_distance(F.numpy(), TS.true_F(f["K0"][7], f["K1"][7], T)) < 1e-12
