"""Planted inputs of the detection tests and the helpers that call the three entries (xfh_nms, xfh_extract_dense, xfh_detect_sparse) on them.  Every generator consumes its
numpy Generator in a fixed order, so a seed names one input on every machine.  Nothing here imports torch or the package before a caller asks for a GPU call, so the CPU
tests (tests/test_detect_reference.py, tests/test_topk_emulated.py) share the case lists with tests/test_gpu_detect.py."""
import ctypes as C
import zlib

import numpy as np

import detect_reference as DR

# ---------------------------------------------------------------------------------------------------------------
# planted scenes of the sparse path
# ---------------------------------------------------------------------------------------------------------------
SPARSE_H, SPARSE_W = 320, 352          # 107 x 118 = 12626 lattice sites from either origin
SPARSE_THR = 0.05
SPARSE_N = (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 8192, 8193, 10240, 10241, 12626)
SPARSE_TOP_K = (1, 300, 2048, 4096, 5000)
ORIGINS = ((0, 0), (1, 0))
REL_KINDS = ("ones_zero_block", "random")
RW, RH = np.float32(1.25), np.float32(0.75)
ZERO_CELLS = 6
# The descriptor bar (1.5e-6 absolute) is the figure tests/test_descriptor_emulated.py holds on feature maps without zero cells, where the bicubic sum of unit vectors has a norm of
# about 0.35 or more before the final normalisation (0.33-0.46 over these scenes' sites away from zero cells).  The cubic weights carry an ABSOLUTE fp32 error (in the reference's
# own arithmetic too), which that normalisation divides by the norm: a site in the middle of an all-zero cell keeps only weights of a few hundredths and loses two digits, whatever
# the kernel does.  The planted zero cells may lower the norm to 0.22, not further (tests/test_detect_reference.py asserts it for every scene).
MIN_BICUBIC_NORM = 0.22


def lattice(H, W, origin):
    """the sites (y, x) of spacing 3 from `origin`, row-major"""
    ys, xs = np.arange(origin[0], H, 3), np.arange(origin[1], W, 3)
    return np.stack(np.meshgrid(ys, xs, indexing="ij"), -1).reshape(-1, 2)


def planted_scene(seed, H, W, n, origin, rel_kind):
    """One image whose answer is known: n peaks on the lattice of spacing 3 from `origin` (neighbours lie outside each other's 5 x 5 window: exactly n candidates above any
    threshold in [0, 0.06)), background 0, heights 0.06 + 0.9 (perm(i) + 1) / n.  The first site (pixel (0, 0) for origin (0, 0)), one site of the last column and one of
    the last row, where the lattice has them, are planted first, the others drawn without replacement.  -> dict heat (H, W), rel (H/8, W/8), feats (H/8, W/8, 64) float32,
    sites (n, 2) int64 (y, x) in row-major order."""
    rng = np.random.default_rng(seed)
    lat = lattice(H, W, origin)
    assert 0 <= n <= len(lat)
    last_col, last_row = np.flatnonzero(lat[:, 1] == W - 1), np.flatnonzero(lat[:, 0] == H - 1)
    forced = [0] + [int(v[len(v) // 2]) for v in (last_col, last_row) if len(v)]
    forced = list(dict.fromkeys(forced))
    forced = forced[:n]
    rest = np.setdiff1d(np.arange(len(lat)), forced)
    pick = np.sort(np.concatenate([np.asarray(forced, np.int64), rng.choice(rest, n - len(forced), replace=False)])) if n else np.zeros(0, np.int64)
    sites = lat[pick]
    heat = np.zeros((H, W), np.float32)
    if n:
        heat[sites[:, 0], sites[:, 1]] = (0.06 + 0.9 * (rng.permutation(n) + 1) / n).astype(np.float32)
    hc, wc = H // 8, W // 8
    if rel_kind == "ones_zero_block":
        rel = np.ones((hc, wc), np.float32)
        rel[10:20, 10:20] = 0.0
    elif rel_kind == "random":
        rel = rng.uniform(0.25, 1.0, (hc, wc)).astype(np.float32)
    else:
        raise ValueError(rel_kind)
    feats = (rng.standard_normal((hc, wc, 64)) * rng.uniform(0.2, 3.0, (hc, wc, 1))).astype(np.float32)
    # a handful of all-zero cells.  A cell is taken only if it leaves every site's bicubic sum at a norm of MIN_BICUBIC_NORM or more (or at exactly zero): see there
    zeroed = 0
    for _ in range(200):
        cy, cx = int(rng.integers(0, hc)), int(rng.integers(0, wc))
        keep = feats[cy, cx].copy()
        if not keep.any():
            continue
        feats[cy, cx] = 0.0
        near = (np.abs(sites[:, 0] / 8.0 - 0.5 - cy) < 3) & (np.abs(sites[:, 1] / 8.0 - 0.5 - cx) < 3) if n else np.zeros(0, bool)
        norm = DR.bicubic_norm(feats, sites[near, 0], sites[near, 1], H, W)
        if ((norm >= MIN_BICUBIC_NORM) | (norm == 0)).all():
            zeroed += 1
            if zeroed == ZERO_CELLS:
                break
        else:
            feats[cy, cx] = keep
    assert zeroed == ZERO_CELLS
    return {"heat": heat, "rel": rel, "feats": feats, "sites": sites.astype(np.int64)}


def sparse_scene_cases():
    """(seed, n, origin, rel_kind) of every scene tests/test_gpu_detect.py runs: each n with both rel kinds and both origins (the pairing alternates with n, the largest
    counts get all four)."""
    out = []
    for i, n in enumerate(SPARSE_N):
        combos = [(o, r) for o in ORIGINS for r in REL_KINDS]                     # [(00, zero block), (00, random), (10, zero block), (10, random)]
        use = combos if n >= 10241 else [combos[i % 2], combos[3 - i % 2]]
        for o, r in use:
            out.append((scene_seed(n, o, r), n, o, r))
    return out


# scenes whose first draw left more than 1 % of the neighbouring scores closer than 2e-6 relative (tests/test_detect_reference.py holds every scene to that cap): drawn again
RESEEDED = {(10240, (1, 0), "random"): 1, (12626, (0, 0), "random"): 1}      # 1.02 % -> 0.85 %, 1.11 % -> 0.93 %


def scene_seed(n, origin, rel_kind):
    return zlib.crc32(f"{n}/{origin}/{rel_kind}".encode()) % 100000 + 100000 * RESEEDED.get((n, origin, rel_kind), 0)


# ---------------------------------------------------------------------------------------------------------------
# the dense top-k cases (values in, permutation out)
# ---------------------------------------------------------------------------------------------------------------
DENSE_N = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193, 10240, 10241, 12289, 20481)
DENSE_K = (1, 2, 255, 256, 257, 2048, 2049)
DENSE_B = (1, 3, 8, 9)
DENSE_CLASSES = ("levels7", "constant", "distinct", "signed")
SCALE_DIVS = (1.0, 2.0, 1.3)


def dense_ks(n):
    return sorted({k for k in DENSE_K + (n - 1, n) if 1 <= k <= n})


def dense_shapes(n):
    """(1, n) and, where n factors, the two-dimensional (hc, wc) with hc the largest divisor up to sqrt(n)"""
    d = max([h for h in range(2, int(n ** 0.5) + 1) if n % h == 0], default=None)
    return [(1, n)] + ([(d, n // d)] if d else [])


def dense_values(cls, n, B):
    """(B, n) float32, another draw per image.  No NaN and no -0.0."""
    rng = np.random.default_rng(zlib.crc32(f"{cls}/{n}/{B}".encode()))
    if cls == "levels7":          # seven dyadic levels: tie groups of about n / 7
        v = (rng.integers(1, 8, (B, n)) / 8.0)
    elif cls == "constant":       # the answer is 0 .. k - 1
        v = np.repeat(0.25 + 0.125 * np.arange(B)[:, None], n, 1)
    elif cls == "distinct":
        v = np.stack([(rng.permutation(n) + 1) / n for _ in range(B)])
    elif cls == "signed":
        v = np.asarray([-1.0, -0.5, 0.5, 1.0])[rng.integers(0, 4, (B, n))]
    else:
        raise ValueError(cls)
    return v.astype(np.float32)


def float_ord(v):
    """common.hpp's monotone map float32 -> uint32"""
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dense_keys(vals):
    """the 64-bit keys of topk_sort_runs_kernel<1>: (~ord(value) << 32) | index; ascending key == (value descending, index ascending)"""
    v = np.asarray(vals, np.float32).ravel()
    return ((~float_ord(v)).astype(np.uint64) << np.uint64(32)) | np.arange(len(v), dtype=np.uint64)


def dense_kpts(cells, wc, scale_div):
    """float32 restatement of dense_gather_kernel: ((8 cj) rw) / scale_div, ((8 ci) rh) / scale_div"""
    ci, cj = cells // wc, cells % wc
    sd = np.float32(scale_div)
    return np.stack([((cj * 8).astype(np.float32) * RW) / sd, ((ci * 8).astype(np.float32) * RH) / sd], -1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# NMS maps
# ---------------------------------------------------------------------------------------------------------------
NMS_W = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 200)
NMS_H = (1, 2, 3, 15, 16, 17, 18, 35)
NMS_CLASSES = {"levels": (0.1, -1.0), "negative": (-10.0, 0.0), "signed": (0.0, -0.25), "sparse": (0.5, -1.0)}      # class -> its thresholds


def nms_maps(cls, B, H, W, seed=0):
    """(B, H, W) float32, another draw per image"""
    rng = np.random.default_rng(zlib.crc32(f"{cls}/{B}/{H}/{W}/{seed}".encode()))
    levels = rng.integers(0, 4, (B, H, W)) / 4.0
    if cls == "levels":           # plateaus everywhere
        v = levels
    elif cls == "negative":       # every value below 0: zero padding would beat every border maximum
        v = -1.0 - levels
    elif cls == "signed":
        v = rng.integers(-1, 2, (B, H, W)) / 2.0
    elif cls == "sparse":         # isolated peaks and pairs at every distance
        v = np.where(rng.random((B, H, W)) < 0.03, rng.integers(1, 3, (B, H, W)), 0).astype(np.float64)
    else:
        raise ValueError(cls)
    return v.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# calls (GPU)
# ---------------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def call_nms(xf, maps, thr, ks=5):
    """XFeat.NMS on (B, H, W) maps -> (B, Nmax, 2) int64 numpy, zero padded"""
    import torch
    return xf.NMS(torch.from_numpy(np.ascontiguousarray(maps))[:, None].cuda(), threshold=thr, kernel_size=ks).cpu().numpy()


def call_nms_capacity(xf, maps, thr, ks, cap):
    """lib.xfh_nms with a caller's capacity -> (xy (B, cap, 2) int64, n_candidates (B,) int32); the outputs start as -1 patterns"""
    import torch
    from accelerated_features_amd import _lib
    lib = _lib.load()
    x = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    B, H, W = x.shape
    xy = torch.full((B, cap, 2), -1, dtype=torch.int64, device=x.device)
    nc = torch.full((B,), -1, dtype=torch.int32, device=x.device)
    ws, n = xf.net.workspace("detect", lib.xfh_detect_workspace_bytes(B, H, W, 1, cap))
    rc = lib.xfh_nms(xf.net.handle(), _p(x), B, H, W, float(thr), int(ks), int(cap), _p(xy), _p(nc), _p(ws), n, None)
    assert rc == 0, lib.xfh_last_error()
    torch.cuda.synchronize()
    return xy.cpu().numpy(), nc.cpu().numpy()


def call_dense(xf, vals, feats, hc, wc, k, scale_div):
    """lib.xfh_extract_dense on DEVICE tensors vals (B, hc * wc), feats (B, hc * wc, 64) -> device (kpts (B, k, 2), desc (B, k, 64), cell_index (B, k) int32); the outputs
    start as NaN / -1 patterns"""
    import torch
    from accelerated_features_amd import _lib
    lib = _lib.load()
    B = vals.shape[0]
    assert vals.shape == (B, hc * wc) and feats.shape == (B, hc * wc, 64) and vals.is_contiguous() and feats.is_contiguous()
    kpts = torch.full((B, k, 2), float("nan"), dtype=torch.float32, device=vals.device)
    desc = torch.full((B, k, 64), float("nan"), dtype=torch.float32, device=vals.device)
    cell = torch.full((B, k), -1, dtype=torch.int32, device=vals.device)
    ws, n = xf.net.workspace("dense", lib.xfh_dense_workspace_bytes(B, hc, wc, k))
    rc = lib.xfh_extract_dense(xf.net.handle(), _p(vals), _p(feats), B, hc, wc, k, float(RW), float(RH), float(scale_div), _p(kpts), _p(desc), _p(cell), _p(ws), n, None)
    assert rc == 0, lib.xfh_last_error()
    return kpts, desc, cell


def call_sparse(xf, scenes, top_k, cap, thr=SPARSE_THR):
    """XFeat._detect_call on a batch of planted scenes -> dict of numpy arrays: kpts (B, top_k, 2), scores (B, top_k), desc (B, top_k, 64), desc_f16 (B, top_k, 64),
    n_valid (B,), n_candidates (B,)"""
    import torch
    heat = torch.from_numpy(np.stack([s["heat"] for s in scenes])).cuda()
    rel = torch.from_numpy(np.stack([s["rel"] for s in scenes])).cuda()
    feats = torch.from_numpy(np.stack([s["feats"] for s in scenes])).cuda()
    B, H, W = heat.shape
    kpts, scores, desc, n_valid, n_cand, d16 = xf._detect_call(feats, heat, rel, B, H, W, thr, top_k, cap, RW, RH, inv=None, want_f16=True)
    torch.cuda.synchronize()
    return {"kpts": kpts.cpu().numpy(), "scores": scores.cpu().numpy(), "desc": desc.cpu().numpy(), "desc_f16": d16.cpu().numpy(), "n_valid": n_valid.cpu().numpy(),
            "n_candidates": n_cand.cpu().numpy()}
