"""The detection stage (csrc/k_detect.hip; modules/xfeat.py:70-103, 249-263, 362-375) restated in numpy: what is a key-point, what is its score and descriptor, and in which
order the top-k come out.  Comparisons are exact; arithmetic is float64, except the sampling COORDINATES, which follow the reference's fp32 operation order (sample_coord):
they decide which pixel or cell is read, and a float64 coordinate would put a different fraction into the interpolation than the reference itself does (3e-6 in a score).

Shapes: one image at a time -- heat (H, W), rel (H/8, W/8), feats (H/8, W/8, 64) or (H/8 * W/8, 64), ys / xs integer arrays of pixel coordinates."""
import numpy as np


def sample_coord(p, S, Sm):      # the kernel's (= the reference's) fp32 operation order; the last step is one fused multiply-add
    q = np.asarray(p, np.float32) / np.float32(S - 1)
    g1 = ((np.float32(2.0) * q).astype(np.float32) - np.float32(1.0)).astype(np.float32) + np.float32(1.0)
    return (g1.astype(np.float64) * np.float64(np.float32(Sm) * np.float32(0.5)) - 0.5).astype(np.float32)


def nms(heat, thr, ks=5):
    """-> (N, 2) int64 (x, y) in row-major order: pixels with v > thr and v == max over the ks x ks window clipped to the image (= -inf padding).  Plateaus keep every equal
    pixel.  Pure comparisons on the values as given."""
    heat = np.asarray(heat)
    assert heat.ndim == 2 and ks >= 1 and ks % 2 == 1
    H, W = heat.shape
    r = ks // 2
    pad = np.full((H + 2 * r, W + 2 * r), -np.inf, heat.dtype)
    pad[r:r + H, r:r + W] = heat
    m = np.full((H, W), -np.inf, heat.dtype)
    for dy in range(ks):
        for dx in range(ks):
            m = np.maximum(m, pad[dy:dy + H, dx:dx + W])
    ys, xs = np.nonzero((heat > thr) & (heat == m))      # (np.nonzero walks row-major)
    return np.stack([xs, ys], -1).astype(np.int64)


def _fetch0(m, y, x):
    """m[y, x] as float64, 0 outside the map"""
    Hm, Wm = m.shape
    inside = (y >= 0) & (y < Hm) & (x >= 0) & (x < Wm)
    return np.where(inside, m[np.clip(y, 0, Hm - 1), np.clip(x, 0, Wm - 1)].astype(np.float64), 0.0)


def scores(heat, rel, ys, xs):
    """nearest(heat) * bilinear(rel) at the pixels (ys, xs) (xfeat.py:77-80) -> float64; the pixel (0, 0) gives -1.  Nearest rounds half to even; both samplers read zeros
    outside their map."""
    heat, rel = np.asarray(heat), np.asarray(rel)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    H, W = heat.shape
    hc, wc = rel.shape
    ix = np.rint(sample_coord(xs, W, W)).astype(np.int64)
    iy = np.rint(sample_coord(ys, H, H)).astype(np.int64)
    sn = _fetch0(heat, iy, ix)
    ux, uy = sample_coord(xs, W, wc), sample_coord(ys, H, hc)
    fx, fy = np.floor(ux), np.floor(uy)
    tx, ty = (ux - fx).astype(np.float64), (uy - fy).astype(np.float64)      # fp32 fractions: inputs of the interpolation
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    sb = (_fetch0(rel, y0, x0) * ((1.0 - tx) * (1.0 - ty)) + _fetch0(rel, y0, x0 + 1) * (tx * (1.0 - ty))
          + _fetch0(rel, y0 + 1, x0) * ((1.0 - tx) * ty) + _fetch0(rel, y0 + 1, x0 + 1) * (tx * ty))
    s = sn * sb
    return np.where((xs == 0) & (ys == 0), -1.0, s)


def _cubic(t):
    A = -0.75
    def near(x): return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    def far(x): return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return [far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)]


def _bicubic(feats, ys, xs, H, W, inv=None):
    """bicubic(normalize(feats)) at the pixels (ys, xs), before the second normalisation -> (N, C) float64"""
    hc, wc = H // 8, W // 8
    f = np.asarray(feats, np.float64).reshape(hc * wc, -1)
    if inv is None:
        inv = 1.0 / np.maximum(np.sqrt((f * f).sum(-1)), 1e-12)
    fn = f * np.asarray(inv, np.float64).reshape(hc * wc, 1)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    ux, uy = sample_coord(xs, W, wc), sample_coord(ys, H, hc)
    fx, fy = np.floor(ux), np.floor(uy)
    wx, wy = _cubic((ux - fx).astype(np.float64)), _cubic((uy - fy).astype(np.float64))
    x0, y0 = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
    acc = np.zeros((len(ys), f.shape[1]))
    for r in range(4):
        for i in range(4):
            yy, xx = y0 + r, x0 + i
            inside = (yy >= 0) & (yy < hc) & (xx >= 0) & (xx < wc)
            w = np.where(inside, wy[r] * wx[i], 0.0)
            acc += w[:, None] * fn[np.clip(yy, 0, hc - 1) * wc + np.clip(xx, 0, wc - 1)]
    return acc


def bicubic_norm(feats, ys, xs, H, W):
    """|bicubic(normalize(feats))| at the pixels: what the second normalisation divides by.  The cubic weights are evaluated in fp32 by the kernel as by the reference, with
    an ABSOLUTE error, so a descriptor's error grows like 1 / this norm: about 0.35-0.45 among ordinary cells, a few hundredths where the dominant cells are all-zero."""
    acc = _bicubic(feats, ys, xs, H, W)
    return np.sqrt((acc * acc).sum(-1))


def descriptors(feats, ys, xs, H, W, inv=None):
    """normalize(bicubic(normalize(feats))) at the pixels (ys, xs) of an H x W image (xfeat.py:70, 90-93) -> (N, 64) float64.  Keys' cubic convolution with A = -0.75, zeros
    outside the map; a norm below 1e-12 divides by 1e-12 (F.normalize), so an all-zero neighbourhood gives a zero row.  inv: 1 / max(|feats|, 1e-12) per cell where the
    caller has it as an INPUT of the code under test (descriptor_kernel takes it from the backbone in fp32); None: float64 here."""
    acc = _bicubic(feats, ys, xs, H, W, inv)
    return acc / np.maximum(np.sqrt((acc * acc).sum(-1, keepdims=True)), 1e-12)


def topk_order(values, k):
    """indices of the k largest values, by (value descending, index ascending): the tie rule of k_detect.hip's keys.  Exact (no NaN, no -0.0: the keys order -0.0 below
    +0.0, which nothing promises)."""
    v = np.asarray(values).ravel()
    return np.lexsort((np.arange(len(v)), -v.astype(np.float64)))[:k]
