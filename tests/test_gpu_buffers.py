"""Every entry of the C ABI that writes device memory, held to the buffer contract of include/xfeat_hip.h (Conventions) by tests/guarded.py:

  - a workspace of EXACTLY xfh_*_workspace_bytes() bytes, between guard bands, and every output between guard bands: no stray write;
  - three starting states of the workspace and the outputs -- zeros, the leftovers of a call on other inputs of the same shape, the leftovers
    of a call on a smaller shape -- give the same bytes in every output, and the guarded call returns what the plain wrapper call returns;
  - the inputs are not written, the return code is XFH_OK, and a workspace one byte short is refused with XFH_ERR_WORKSPACE before anything
    is written.

A case is make(seed, small) -> Case(inputs, call): seed 0 at the full shape is the call under test, seed 1 its stale-same predecessor,
small=True the stale-other predecessor (every dimension reduced to a smaller non-multiple of the tiles).  The shapes are the smallest ragged
ones of each entry's own GPU test: no dimension a multiple of 64 lanes, 256-thread blocks, the matcher's 32-wide blocks or the 64 x 16
resize tile where the entry allows it; counts ragged with 0 and the full capacity among them.

OUTPUT REGIONS THE HEADER LEAVES UNSPECIFIED are listed in SPECIFIED below, each with the header's words; everything else is compared whole.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import guarded

pytestmark = pytest.mark.gpu

CASES = {}           # case id -> (entry, make)


class Case:
    def __init__(self, inputs, call):
        self.inputs, self.call = [t for t in inputs if t is not None], call


def case(entry, tag=None):
    def register(make):
        CASES[entry + (f"[{tag}]" if tag else "")] = (entry, make)
        return make
    return register


def T(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def P_(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from accelerated_features_amd import _lib
    return _lib.load()               # (the Proxy while a case is driven)


def ok(rc, what):
    from accelerated_features_amd import _lib
    _lib.check(rc, what)


_models = {}


def xfeat():
    if "xf" not in _models:
        import fixtures
        from accelerated_features_amd import XFeat
        _models["xf"] = XFeat(weights=fixtures.synthetic_state_dict(0), top_k=256, detection_threshold=0.05)
    return _models["xf"]


def lighterglue():
    if "lg" not in _models:
        import fixtures
        from accelerated_features_amd.lighterglue import LighterGlue
        _models["lg"] = LighterGlue(weights=fixtures.lighterglue_state_dict(0))
    return _models["lg"]


class option:
    """A kernel switch of the model's handle for the duration of a call."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        xfeat().net.set_option(self.key, self.value)

    def __exit__(self, *exc):
        xfeat().net.set_option(self.key, None)
        return False


# ---------------------------------------------------------------------------------------------------------------------------------------
# network and detection
# ---------------------------------------------------------------------------------------------------------------------------------------
def _images(seed, small, channels=3):
    import fixtures
    B, H, W = (1, 64, 96) if small else (2, 96, 160)          # (H, W multiples of 32: the entry's own condition)
    return fixtures.texture_images(B, H, W, seed=11 + seed, channels=channels)


@case("xfh_backbone")
def _(seed, small):
    x = _images(seed, small).cuda()
    return Case([x], lambda: xfeat().net.backbone(x, want_logits=True, want_heat=True, want_invnorm=True))


@case("xfh_backbone_u8", "nchw")
def _(seed, small):
    x = (_images(seed, small) * 255).to(torch.uint8).cuda()
    return Case([x], lambda: xfeat().net.backbone(x, want_logits=True, want_heat=True, want_invnorm=True))


@case("xfh_backbone_u8", "nhwc")
def _(seed, small):
    from accelerated_features_amd.xfeat import _U8Image
    x = (_images(seed, small) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    return Case([x], lambda: xfeat().net.backbone(_U8Image(x, 255.0), want_logits=True, want_heat=True, want_invnorm=True))


def _resized(resize2):
    def make(seed, small):
        from accelerated_features_amd.xfeat import _LazyResize
        import fixtures
        B, H, W = (1, 90, 132) if small else (2, 110, 164)      # Win % 4 == 0: the staged form of resize2 = 1 applies
        x = fixtures.texture_images(B, H, W, seed=21 + seed).cuda()
        s = np.float32(1.0 / 0.6)
        Hm, Wm = int(H * 0.6), int(W * 0.6)
        Ho, Wo = Hm // 32 * 32, Wm // 32 * 32
        lazy = _LazyResize(x, Hm, Wm, s, s, Ho, Wo, np.float32(Hm) / np.float32(Ho), np.float32(Wm) / np.float32(Wo))

        def call():
            with option("resize2", resize2):
                return xfeat().net.backbone(lazy, want_logits=True, want_heat=True, want_invnorm=True)
        return Case([x], call)
    return make


case("xfh_backbone_resized", "resize2=1")(_resized(1))
case("xfh_backbone_resized", "resize2=0")(_resized(0))


def _conv(name):
    def make(seed, small):
        from accelerated_features_amd.spec import CONVS, CONV_INDEX
        c = next(c for c in CONVS if c.name == name)
        B, H, W = (1, 39, 41) if small else (2, 41, 43)
        g = torch.Generator().manual_seed(31 + seed)
        x = torch.randn(B, c.cin, H, W, generator=g).cuda()
        pad = c.k // 2 if hasattr(c, "k") else 1
        k = getattr(c, "k", 3)
        Ho, Wo = (H + 2 * pad - k) // c.stride + 1, (W + 2 * pad - k) // c.stride + 1

        def call():
            out = torch.empty((B, c.cout, Ho, Wo), dtype=torch.float32, device=x.device)
            ok(lib().xfh_conv_layer(xfeat().net.handle(), CONV_INDEX[name], P_(x), B, H, W, P_(out), 0, stream()), "xfh_conv_layer")
            return out
        return Case([x], call)
    return make


for _name in ("block2.0", "block3.1", "block4.0"):
    case("xfh_conv_layer", _name)(_conv(_name))


@case("xfh_resize_bilinear")
def _(seed, small):
    g = torch.Generator().manual_seed(41 + seed)
    B, H, W, Ho, Wo = (1, 43, 67, 35, 99) if small else (2, 45, 70, 37, 101)          # no multiple of the 64 x 16 tile
    x = torch.rand(B, 3, H, W, generator=g).cuda()
    return Case([x], lambda: xfeat()._resize(x, Ho, Wo, np.float32(H) / np.float32(Ho), np.float32(W) / np.float32(Wo)))


@case("xfh_kpts_heatmap")
def _(seed, small):
    g = torch.Generator().manual_seed(51 + seed)
    B, h, w = (1, 5, 7) if small else (2, 7, 9)
    x = torch.randn(B, 65, h, w, generator=g).cuda()
    return Case([x], lambda: xfeat().get_kpts_heatmap(x))


@case("xfh_nms")
def _(seed, small):
    import detect_support as DS
    B, H, W = (1, 18, 129) if small else (2, 35, 130)
    x = T(DS.nms_maps("sparse", B, H, W, seed=seed))[:, None].contiguous()
    return Case([x], lambda: xfeat().NMS(x, threshold=0.5, kernel_size=5))


@case("xfh_nms", "capacity reached")
def _(seed, small):
    import detect_support as DS
    B, H, W, cap = (1, 18, 129, 9) if small else (2, 35, 130, 11)
    x = T(DS.nms_maps("levels", B, H, W, seed=seed))

    def call():
        xy = torch.empty((B, cap, 2), dtype=torch.int64, device=x.device)
        nc = torch.empty((B,), dtype=torch.int32, device=x.device)
        ws, n = xfeat().net.workspace("detect", lib().xfh_detect_workspace_bytes(B, H, W, 1, cap))
        ok(lib().xfh_nms(xfeat().net.handle(), P_(x), B, H, W, 0.1, 3, cap, P_(xy), P_(nc), P_(ws), n, stream()), "xfh_nms")
        return xy, nc
    return Case([x], call)


def _sample(mode):
    def make(seed, small):
        from accelerated_features_amd.interpolator import InterpolateSparse2d
        g = torch.Generator().manual_seed(61 + seed)
        B, Cc, Hm, Wm, N = (1, 3, 11, 19, 75) if small else (2, 5, 12, 20, 77)
        x = torch.randn(B, Cc, Hm, Wm, generator=g).cuda()
        pos = (torch.rand(B, N, 2, generator=g) * torch.tensor([8.0 * Wm + 4, 8.0 * Hm + 4]) - 2).cuda()      # a few sites outside the frame
        return Case([x, pos], lambda: InterpolateSparse2d(mode)(x, pos, 8 * Hm, 8 * Wm))
    return make


for _mode in ("nearest", "bilinear", "bicubic"):
    case("xfh_sample_sparse", _mode)(_sample(_mode))


def _detect(with_options):
    def make(seed, small):
        import detect_support as DS
        H, W, top_k, cap, ns = (64, 96, 75, 290, (60, 0)) if small else (96, 160, 77, 300, (0, 50, 300))      # 300 candidates: the capacity exactly
        sc = [DS.planted_scene(1000 * seed + 10 * i + H, H, W, n, (0, 0), "random") for i, n in enumerate(ns)]
        heat, rel, feats = (T(np.stack([s[k] for s in sc])) for k in ("heat", "rel", "feats"))
        inv = (1.0 / feats.norm(dim=-1).clamp_min(1e-12)).contiguous() if with_options else None
        B = len(ns)
        return Case([heat, rel, feats, inv], lambda: xfeat()._detect_call(feats, heat, rel, B, H, W, DS.SPARSE_THR, top_k, cap, DS.RW, DS.RH, inv=inv,
                                                                         want_f16=with_options))
    return make


case("xfh_detect_sparse", "plain")(_detect(False))
case("xfh_detect_sparse", "invnorm and desc_f16")(_detect(True))


@case("xfh_extract_dense")
def _(seed, small):
    g = torch.Generator().manual_seed(71 + seed)
    B, hc, wc, k = (1, 7, 9, 61) if small else (2, 9, 11, 99)                  # k = hc * wc at the full shape
    rel = torch.rand(B, hc, wc, generator=g).cuda()
    feats = torch.randn(B, hc, wc, 64, generator=g).cuda()

    def call():
        kpts = torch.empty((B, k, 2), dtype=torch.float32, device=rel.device)
        desc = torch.empty((B, k, 64), dtype=torch.float32, device=rel.device)
        cell = torch.empty((B, k), dtype=torch.int32, device=rel.device)
        ws, n = xfeat().net.workspace("dense", lib().xfh_dense_workspace_bytes(B, hc, wc, k))
        ok(lib().xfh_extract_dense(xfeat().net.handle(), P_(rel), P_(feats), B, hc, wc, k, 1.25, 0.75, 1.3, P_(kpts), P_(desc), P_(cell), P_(ws), n,
                                   stream()), "xfh_extract_dense")
        return kpts, desc, cell
    return Case([rel, feats], call)


@case("xfh_fine_matcher")
def _(seed, small):
    g = torch.Generator().manual_seed(81 + seed)
    x = torch.randn(75 if small else 77, 128, generator=g).cuda()
    return Case([x], lambda: xfeat().net._fine_matcher(x))


# ---------------------------------------------------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------------------------------------------------
def _descriptor_sets(seed, small):
    """P pairs of unit rows (tests/adversarial.py: every component next to an fp16 rounding midpoint) and device-side counts with a 0 and a 1
    among them, the first pair full."""
    import adversarial
    P, N1, N2 = (2, 290, 331) if small else (3, 300, 333)
    d = [adversarial._aligned_unit(N1, N2, 100 * seed + p + 7) for p in range(P)]
    d1, d2 = T(np.stack([a for a, _ in d])), T(np.stack([b for _, b in d]))
    counts = [N1, 0, 1][:P] + [N2, 5, 1][:P]
    return P, N1, N2, d1, d2, torch.tensor(counts, dtype=torch.int32).cuda()


def _mnn(options=(), f16=False, counts=True):
    def make(seed, small):
        P, N1, N2, d1, d2, nv = _descriptor_sets(seed, small)
        h1 = (256.0 * d1).to(torch.float16).contiguous() if f16 else None
        h2 = (256.0 * d2).to(torch.float16).contiguous() if f16 else None
        if not counts:
            nv = None

        def call():
            idx0 = torch.empty((P, N1), dtype=torch.int64, device=d1.device)
            idx1 = torch.empty((P, N1), dtype=torch.int64, device=d1.device)
            n = torch.empty((P,), dtype=torch.int32, device=d1.device)
            net = xfeat().net
            ws, nb = net.workspace("match", lib().xfh_match_workspace_bytes(P, N1, N2))
            for key, value in options:
                net.set_option(key, value)
            try:
                ok(lib().xfh_match_mnn(net.handle(), P_(d1), N1 * 64, P_(d2), N2 * 64, P_(h1), P_(h2), P_(nv), P_(nv), 1, P, P, N1, N2, 0.3,
                                       P_(idx0), P_(idx1), P_(n), P_(ws), nb, stream()), "xfh_match_mnn")
            finally:
                for key, _v in options:
                    net.set_option(key, None)
            return idx0, idx1, n
        return Case([d1, d2, h1, h2, nv], call)
    return make


case("xfh_match_mnn", "default")(_mnn())
case("xfh_match_mnn", "all rows")(_mnn(counts=False))
case("xfh_match_mnn", "match_exact")(_mnn((("match_exact", 1),)))
case("xfh_match_mnn", "match_sweep=1")(_mnn((("match_sweep", 1),)))
case("xfh_match_mnn", "match_sweep=2")(_mnn((("match_sweep", 2),)))
case("xfh_match_mnn", "fp16 copies")(_mnn(f16=True))


def _guided(kind):
    def make(seed, small):
        import guided_reference as GR
        from accelerated_features_amd.guided import match_guided_device
        P, N1, N2 = (2, 290, 275) if small else (3, 300, 280)
        sc = [GR.scene(kind, N1, N2, 500 + 50 * seed + p) for p in range(P)]
        a = [T(np.stack([s[k] for s in sc])) for k in ("d1", "k1", "d2", "k2")]
        models = np.stack([np.asarray(s["model"], np.float64).reshape(3, 3) for s in sc])
        models[P - 1] = 0                                          # "an all-zero model ... gives no matches for its pair"
        models = T(models)
        c1 = torch.tensor([N1, 0, 1][:P], dtype=torch.int32).cuda()
        c2 = torch.tensor([N2, 7, 1][:P], dtype=torch.int32).cuda()
        return Case(a + [models, c1, c2], lambda: match_guided_device(a[0], a[1], c1, a[2], a[3], c2, models, kind, 3.0, 0.3))
    return make


case("xfh_match_mnn_guided", "fundamental")(_guided("fundamental"))
case("xfh_match_mnn_guided", "homography")(_guided("homography"))


def _refine(fx):
    def make(seed, small):
        import refine_support as RS
        P, N = (2, 75) if small else (3, 77)
        s = RS.scene(900 + seed, P, N)
        d0 = {"descriptors": T(s["desc0"]), "keypoints": T(s["kp0"]), "scales": T(s["scale0"])}
        d1 = {"descriptors": T(s["desc1"]), "keypoints": T(s["kp1"])}
        idx0, idx1 = T(s["idx0"]), T(s["idx1"])
        nm = torch.tensor([N, 0, 41][:P], dtype=torch.int32).cuda()

        def call():
            with option("fx", fx):
                return xfeat()._refine_device(d0, d1, idx0, idx1, nm, 0.25)
        return Case(list(d0.values()) + list(d1.values()) + [idx0, idx1, nm], call)
    return make


case("xfh_refine_matches", "fp16-pair kernels")(_refine(None))
case("xfh_refine_matches", "f32 kernels")(_refine(1 | 2 | 8))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the RANSAC estimators: list and _matches forms
# ---------------------------------------------------------------------------------------------------------------------------------------
ITERS = 200


def _ragged(small):
    """P, cap and the counts: an empty pair, a full one, one between."""
    return (2, 75, [75, 0]) if small else (3, 77, [0, 77, 41])


def _as_matches(pts0, pts1, counts, seed):
    """The point lists as key-point tables of cap + 5 rows in another order plus index lists (the matcher's output)."""
    P, cap = pts0.shape[:2]
    K = cap + 5
    rng = np.random.default_rng(seed)
    k0, k1 = np.zeros((P, K, pts0.shape[2]), np.float32), np.zeros((P, K, pts1.shape[2]), np.float32)
    i0, i1 = np.zeros((P, cap), np.int64), np.zeros((P, cap), np.int64)
    for p in range(P):
        i0[p], i1[p] = rng.permutation(K)[:cap], rng.permutation(K)[:cap]
        k0[p, i0[p]], k1[p, i1[p]] = pts0[p], pts1[p]
    return T(k0), T(k1), T(i0), T(i1), torch.tensor(counts, dtype=torch.int32).cuda()


def _twoview_points(seed, small, homography=False):
    import twoview_support as TS
    P, cap, counts = _ragged(small)
    p0, p1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    K0, K1 = np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
    for p, n in enumerate(counts):
        if homography:
            a, b = TS.homography_pair(max(n, 1), 0.3, 0.5, seed=300 + 10 * seed + p)[:2]
        else:
            a, b, _, K0[p], K1[p], _ = TS.scene(p, max(n, 1), 0.5, 0.3, 300 + 10 * seed + p)
        p0[p, :n], p1[p, :n] = a[:n], b[:n]
    return P, cap, counts, p0, p1, K0, K1


def _estimator(fn_name, module, matches, points, kwargs):
    def make(seed, small):
        import importlib
        fn = getattr(importlib.import_module("accelerated_features_amd." + module), fn_name)
        P, cap, counts, a, b, extra = points(seed, small)
        if matches:
            k0, k1, i0, i1, nm = _as_matches(a, b, counts, seed)
            args = [k0, k1, i0, i1, nm] + extra
        else:
            args = [T(a), T(b), torch.tensor(counts, dtype=torch.int32).cuda()] + extra
        return Case([t for t in args if torch.is_tensor(t)], lambda: fn(*args, **kwargs))
    return make


def _h_points(seed, small):
    P, cap, counts, p0, p1, _, _ = _twoview_points(seed, small, homography=True)
    return P, cap, counts, p0, p1, []


def _e_points(seed, small):
    P, cap, counts, p0, p1, K0, K1 = _twoview_points(seed, small)
    return P, cap, counts, p0, p1, [T(K0), T(K1)]


def _f_points(seed, small):
    return _e_points(seed, small)[:5] + ([],)


def _abs_points(seed, small):
    import abspose_support as AS
    P, cap, counts = _ragged(small)
    p2, p3, K = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 3), np.float32), np.zeros((P, 3, 3))
    for p, n in enumerate(counts):
        X, px, _, K[p], _ = AS.scene3d(p, max(n, 1), 0.5, 0.3, 400 + 10 * seed + p)
        p2[p, :n], p3[p, :n] = px[:n], X[:n]
    return P, cap, counts, p2, p3, [T(K)]


def _align_points(seed, small):
    import alignment_support as AL
    P, cap, counts = _ragged(small)
    A, B = np.zeros((P, cap, 3), np.float32), np.zeros((P, cap, 3), np.float32)
    thr = 0.0
    for p, n in enumerate(counts):
        sc = AL.scene(max(n, 1), 0.01, 0.3, 0.1, 500 + 10 * seed + p, scale=2.5)
        A[p, :n], B[p, :n], thr = sc["A"][:n], sc["B"][:n], sc["thr"]
    return P, cap, counts, A, B, [thr]


_H = dict(ransac_thr=4.0, max_iters=ITERS, confidence=0.995, seed=9)
_F = dict(ransac_thr=3.0, max_iters=ITERS, confidence=0.99, seed=9)
_E = dict(max_epipolar_error=1.0, max_iterations=ITERS, seed=9)
_S = dict(thresholds=[0.5, 2.5, 1.0], max_iterations=ITERS, seed=9)
_A = dict(max_reproj_error=12.0, max_iterations=ITERS, seed=9)
_L = dict(max_iterations=ITERS, seed=9)
case("xfh_find_homography")(_estimator("find_homography_batch", "homography", False, _h_points, _H))
case("xfh_find_homography_matches")(_estimator("find_homography_matches", "homography", True, _h_points, _H))
case("xfh_find_fundamental")(_estimator("find_fundamental_batch", "fundamental", False, _f_points, _F))
case("xfh_find_fundamental_matches")(_estimator("find_fundamental_matches", "fundamental", True, _f_points, _F))
case("xfh_estimate_relpose")(_estimator("estimate_relative_pose_batch", "pose", False, _e_points, _E))
case("xfh_estimate_relpose_matches")(_estimator("estimate_relative_pose_matches", "pose", True, _e_points, _E))
case("xfh_estimate_relpose_sweep")(_estimator("estimate_relative_pose_sweep_batch", "pose", False, _e_points, _S))
case("xfh_estimate_relpose_sweep_matches")(_estimator("estimate_relative_pose_sweep_matches", "pose", True, _e_points, _S))
case("xfh_estimate_abspose")(_estimator("estimate_absolute_pose_batch", "absolute_pose", False, _abs_points, _A))
case("xfh_estimate_abspose_matches")(_estimator("estimate_absolute_pose_matches", "absolute_pose", True, _abs_points, _A))
case("xfh_estimate_alignment")(_estimator("estimate_alignment_batch", "alignment", False, _align_points, _L))
case("xfh_estimate_alignment_matches")(_estimator("estimate_alignment_matches", "alignment", True, _align_points, _L))


@case("xfh_homography_tables")
def _(seed, small):
    def call():
        st = torch.empty(4096, dtype=torch.int32, device="cuda")
        wt = torch.empty(4096, dtype=torch.float64, device="cuda")
        ok(lib().xfh_homography_tables(4.0, P_(st), P_(wt), stream()), "xfh_homography_tables")
        return st, wt
    return Case([], call)


# ---------------------------------------------------------------------------------------------------------------------------------------
# retrieval
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tables(seed, small):
    import retrieval_support as RS
    G, K, Cb = (2, 290, 32) if small else (3, 300, 32)
    desc, counts, book = RS.tables(np.random.default_rng(600 + seed), G, K, Cb)
    return T(desc), T(counts), T(book)


@case("xfh_vlad")
def _(seed, small):
    from accelerated_features_amd.retrieval import global_descriptors_batch
    desc, counts, book = _tables(seed, small)
    return Case([desc, counts, book], lambda: global_descriptors_batch(desc, counts, book))


@case("xfh_kmeans_step")
def _(seed, small):
    from accelerated_features_amd.retrieval import kmeans_step
    desc, counts, book = _tables(seed, small)
    return Case([desc, counts, book], lambda: kmeans_step(desc, counts, book))


@case("xfh_retrieve_topk")
def _(seed, small):
    import retrieval_support as RS
    from accelerated_features_amd.retrieval import retrieve_topk
    G, Q, N, D, k = (2, 35, 67, 64, 9) if small else (3, 37, 70, 128, 11)
    q, db = RS.global_vectors(np.random.default_rng(700 + seed), G, Q, N, D)
    q, db, n_db = T(q), T(db), torch.tensor([N, 0, 5][:G], dtype=torch.int32).cuda()      # 5 rows: fewer than k found
    return Case([q, db, n_db], lambda: retrieve_topk(q, db, k, n_db))


@case("xfh_pairs_from_shortlists")
def _(seed, small):
    import retrieval_support as RS
    from accelerated_features_amd.retrieval import pairs_from_shortlists
    S, V, k = (2, 5, 2) if small else (3, 5, 3)
    idx, n_views = RS.shortlists(np.random.default_rng(800 + seed), S, V, k)
    idx, n_views = T(idx), T(n_views)
    return Case([idx, n_views], lambda: pairs_from_shortlists(idx, n_views))


# ---------------------------------------------------------------------------------------------------------------------------------------
# LighterGlue (the weights of tests/test_gpu_lighterglue.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
@case("xfh_lg_match")
def _(seed, small):
    import fixtures
    n0, n1 = (75, 61) if small else (77, 67)
    k0, d0, s0, k1, d1, s1 = (t.cuda() for t in fixtures.lighterglue_inputs(n0, n1, seed=2 + seed))
    return Case([k0, d0, k1, d1], lambda: lighterglue().match_device(k0, d0, s0.tolist(), k1, d1, s1.tolist(), 0.01, -1))


@case("xfh_lg_match_pairs")
def _(seed, small):
    import fixtures
    P, cap = (1, 75) if small else (2, 77)
    sets = [fixtures.lighterglue_inputs(cap, cap, seed=20 + 10 * seed + p) for p in range(P)]
    kpts = torch.stack([t for s in sets for t in (s[0], s[3])]).cuda()
    desc = torch.stack([t for s in sets for t in (s[1], s[4])]).cuda()
    counts = torch.tensor([cap, 41, 0, cap][:2 * P], dtype=torch.int32).cuda()
    return Case([kpts, desc, counts], lambda: lighterglue().match_pairs_device(kpts, desc, counts, (640, 480), 0.01, -1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# two-view structure
# ---------------------------------------------------------------------------------------------------------------------------------------
def _structure_inputs(seed, small):
    """Per pair a group of tests/structure_support.py: noise-free, tight gates with a mask, far / behind / not finite."""
    import structure_support as SS
    import twoview_support as TS
    P, cap, counts = _ragged(small)
    rng = np.random.default_rng(1100 + seed)
    p0, p1 = np.zeros((P, cap, 2), np.float32), np.zeros((P, cap, 2), np.float32)
    R, t, E, mask = np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros((P, 3, 3)), np.ones((P, cap), np.uint8)
    for p, n in enumerate(counts):
        g = SS.mixed_group(rng, (0, 5, 3)[p % 3], max(n, 8))
        p0[p, :n], p1[p, :n], R[p], t[p] = g["p0"][:n], g["p1"][:n], g["R"], g["t"]
        E[p] = TS.essential_from_pose(g["R"], g["t"])
        if g["mask"] is not None:
            mask[p, :n] = g["mask"][:n]
    return P, cap, counts, p0, p1, R, t, E, T(mask), SS.K


def _structure(fn_name, matches, recover):
    def make(seed, small):
        from accelerated_features_amd import structure
        fn = getattr(structure, fn_name)
        P, cap, counts, p0, p1, R, t, E, mask, K = _structure_inputs(seed, small)
        if matches:
            lists = list(_as_matches(p0, p1, counts, seed))
        else:
            lists = [T(p0), T(p1), torch.tensor(counts, dtype=torch.int32).cuda()]
        if recover:
            return Case(lists + [mask], lambda: fn(E, *lists, K, K, 50.0, mask=mask))
        return Case(lists + [mask], lambda: fn(*lists, K, K, R, t, max_reproj_error=4.0, min_parallax_deg=1.0, mask=mask))
    return make


case("xfh_triangulate")(_structure("triangulate_batch", False, False))
case("xfh_triangulate_matches")(_structure("triangulate_matches", True, False))
case("xfh_recover_pose")(_structure("recover_pose_batch", False, True))
case("xfh_recover_pose_matches")(_structure("recover_pose_matches", True, True))


# ---------------------------------------------------------------------------------------------------------------------------------------
# tracks, multi-view triangulation, bundle adjustment
# ---------------------------------------------------------------------------------------------------------------------------------------
def _svk(small):
    """Scenes, views, key-point rows."""
    return (2, 4, 75) if small else (3, 5, 77)


def _stack(scenes, *keys):
    return [np.stack([sc[k] for sc in scenes]) for k in keys]


@case("xfh_build_tracks")
def _(seed, small):
    import multiview_support as MS
    from accelerated_features_amd import multiview as mv
    S, V, K = _svk(small)
    rng = np.random.default_rng(1200 + seed)
    lists = [MS.match_lists(rng, MS.arc_scene(rng, V, K)["tracks"], dup=3) for _ in range(S)]
    a, b, n = (T(np.stack([l[i] for l in lists])) for i in range(3))
    return Case([a, b, n], lambda: mv.build_tracks(a, b, n, K))


@case("xfh_triangulate_views")
def _(seed, small):
    import multiview_support as MS
    from accelerated_features_amd import multiview as mv
    S, V, K = _svk(small)
    rng = np.random.default_rng(1300 + seed)
    scenes = [MS.arc_scene(rng, V, K, noise=0.5) for _ in range(S)]
    for sc in scenes:
        MS.plant_outliers(rng, sc)
    kp, tr, Ks, Rs, ts = _stack(scenes, "kpts", "tracks", "Ks", "Rs", "ts")
    kp, tr, nv = T(kp), T(tr), T(np.array([V, V - 1, V][:S], np.int32))
    return Case([kp, tr, nv], lambda: mv.triangulate_views_batch(kp, tr, nv, Ks, Rs, ts))


def _chain_scenes(seed, small):
    import tracks_support as TKS
    S, V, K = _svk(small)
    scenes = [TKS.chain_scene(1400 + 10 * seed + s, K=K, V=V) for s in range(S)]
    lists = [T(np.stack([sc["lists"][i] for sc in scenes])) for i in range(4)]
    kp, Ks, Rs, ts = _stack(scenes, "kpts", "Ks", "Rs", "ts")
    return T(kp), lists, Ks, Rs, ts


@case("xfh_triangulate_tracks")
def _(seed, small):
    from accelerated_features_amd import multiview as mv
    kp, lists, Ks, Rs, ts = _chain_scenes(seed, small)
    return Case([kp] + lists, lambda: mv.triangulate_graph_matches(kp, *lists, None, Ks, Rs, ts))


@case("xfh_build_tracks_graph")
def _(seed, small):
    import tracks_support as TKS
    from accelerated_features_amd import multiview as mv
    S, V, K = _svk(small)
    rng = np.random.default_rng(1500 + seed)
    per = [TKS.noisy_lists(rng, V, K, TKS.all_pairs(V)) for _ in range(S)]
    lists = [T(np.stack([l[i] for l in per])) for i in range(4)]
    return Case(lists, lambda: mv.build_tracks_graph(*lists, V, K, max_tracks=K + 7))


@case("xfh_bundle_adjust")
def _(seed, small):
    import bundle_support as BS
    from accelerated_features_amd import multiview as mv
    S, V, K = (1, 4, 75) if small else (2, 5, 77)
    scenes = [BS.scene(1600 + 10 * seed + s, V, K, holes=0.1) for s in range(S)]
    kp, tr, inl, X, Ks, Rs, ts = _stack(scenes, "kpts", "tracks", "inlier_views", "points3d", "Ks", "Rs0", "ts0")
    kp, tr, inl, X = T(kp), T(tr), T(inl), T(X)
    return Case([kp, tr, inl, X], lambda: mv.bundle_adjust_batch(kp, tr, inl, X, None, Ks, Rs, ts, fixed_views=3, max_iterations=5))


# ---------------------------------------------------------------------------------------------------------------------------------------
# pose graph and baseline ratios
# ---------------------------------------------------------------------------------------------------------------------------------------
@case("xfh_average_poses")
def _(seed, small):
    import posegraph_support as PS
    from accelerated_features_amd import multiview as mv
    Vs = (4, 3) if small else (5, 4, 5)                     # the smaller scenes are padded with edges of weight 0
    scenes = [PS.scene(1700 + 10 * seed + i, V, PS.all_pairs(V), sigma_deg=0.5, outliers=0.2) for i, V in enumerate(Vs)]
    pairs, Rrel, trel, weight, nv, V = PS.batch(scenes)
    a = [T(pairs), T(Rrel), T(trel), T(weight), T(nv)]
    return Case(a, lambda: mv.average_poses_batch(*a, V=V, iterations=10, redescend=3))


def _ratio_scenes(seed, small):
    import posescale_support as QS
    import tracks_support as TKS
    from test_gpu_posescale import _pad
    S, V, K = (1, 4, 75) if small else (2, 5, 77)
    scenes = [QS.scene(1800 + 10 * seed + s, V, K, TKS.chain_pairs(V)) for s in range(S)]
    b, V = _pad(scenes)
    return scenes, b, V


@case("xfh_baseline_ratios")
def _(seed, small):
    from accelerated_features_amd import multiview as mv
    _scenes, b, V = _ratio_scenes(seed, small)
    a = [T(b[k]) for k in ("kpts", "tracks", "track_of", "pairs", "Rrel", "trel", "weight", "Ks", "nv")]
    return Case(a, lambda: mv.baseline_ratios_batch(*a, min_common=4))


@case("xfh_average_poses_ratios")
def _(seed, small):
    import posescale_support as QS
    from accelerated_features_amd import multiview as mv
    scenes, b, V = _ratio_scenes(seed, small)
    r = [QS.ratios(sc, min_common=4) for sc in scenes]     # the ratios of the restatement: inputs like any other
    ratio, count = T(np.stack([x["ratio"] for x in r]).astype(np.float64)), T(np.stack([x["count"] for x in r]).astype(np.int32))
    a = [T(b[k]) for k in ("pairs", "Rrel", "trel", "weight", "nv")]
    return Case(a + [ratio, count], lambda: mv.average_poses_batch(*a, V=V, iterations=10, redescend=3, ratio=ratio, ratio_count=count))


# ---------------------------------------------------------------------------------------------------------------------------------------
# map and verification
# ---------------------------------------------------------------------------------------------------------------------------------------
@case("xfh_build_map")
def _(seed, small):
    import localization_support as LS
    from accelerated_features_amd import localization as loc
    S, V, Tn, kcap = (2, 4, 75, 31) if small else (3, 5, 77, 33)
    rng = np.random.default_rng(1900 + seed)
    per = [LS.map_inputs(rng, V, Tn, kcap) for _ in range(S)]
    a = [T(np.stack([x[i] for x in per])) for i in range(5)]
    return Case(a, lambda: loc.build_map_batch(*a, max_points=Tn // 3))      # fewer rows than selected tracks: the capacity is reached


@case("xfh_map_project")
def _(seed, small):
    import localization_support as LS
    from accelerated_features_amd import localization as loc
    Q, M = (2, 75) if small else (3, 77)
    pts, n, R, t, K = LS.project_case(np.random.default_rng(2000 + seed), Q, M)
    pts, n = T(pts), T(n)
    return Case([pts, n], lambda: loc.project_map(pts, n, R, t, K, (640, 480), 4.0))


@case("xfh_filter_matches")
def _(seed, small):
    import verification_support as VS
    from accelerated_features_amd import verification as ver
    L, cap = (4, 75) if small else (5, 77)
    rng = np.random.default_rng(2100 + seed)
    ia, ib, n, mask = VS.filter_case(rng, L, cap)
    keep = (rng.random(L) > 0.2).astype(np.uint8)
    a = [T(ia), T(ib), T(n), T(mask), T(keep)]
    return Case(a, lambda: ver.filter_matches_batch(*a, 2))


@case("xfh_verify_matches")
def _(seed, small):
    import tracks_support as TKS
    import verification_support as VS
    from accelerated_features_amd import verification as ver
    V, K = (4, 75) if small else (5, 77)
    b = VS.verify_batch(2200 + seed, V, K, TKS.chain_pairs(V))
    a = [T(b[k][:3]) for k in ("kpts", "view_pairs", "idx_a", "idx_b", "n_matches", "n_views", "Ks", "Rs", "ts")]      # three of its four scenes
    return Case(a, lambda: ver.verify_matches_graph(*a, 1.0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Output regions the header leaves unspecified: (entry, output argument) -> a function of the recorded call and the number of bytes that
# returns the bool mask of the SPECIFIED bytes, with the header's words.
# ---------------------------------------------------------------------------------------------------------------------------------------
SPECIFIED = {}


def specified(entry, arg, call, nbytes):
    f = SPECIFIED.get((entry, arg))
    return None if f is None else f(call, nbytes)


def test_every_output_entry_is_driven():
    """(Runs with the GPU suite; the same census without a GPU is in tests/test_guarded_harness.py.)"""
    assert {e for e, _ in CASES.values()} == set(guarded.TABLE)


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_holds_the_buffer_contract(name):
    from accelerated_features_amd import _lib
    entry, make = CASES[name]
    t0 = time.perf_counter()
    problems, _ = guarded.hold(make, _lib, guarded.TABLE, "cuda", entry, specified=specified, error=_lib.XFeatHipError)
    print(f"{name}: {time.perf_counter() - t0:.2f} s")
    assert not problems, "\n".join(problems)
