"""Float64 restatement of the match refinement (XFeat.refine_matches, modules/xfeat.py:306-325; fine_matcher, modules/model.py:97-111) and the error bounds its tests share.

The specification, not the kernels: no folded weights, no packed row list, no compaction rounds.

  fine_matcher(v)     four times Linear(+bias) -> eval BatchNorm1d without affine ((y - mean) / sqrt(var + BN_EPS)) -> ReLU, then one Linear: (n, 128) -> (n, 64).
  confidence(o)       max of softmax(3 o) over the 64 logits.
  offsets(o)          expectation of (x - 4, y - 4) under softmax(3 o), flat index 8 y + x.
  refine(...)         for pair p of a (P, N) batch: n = clamp(n_matches[p], 0, N); for r < n, i0 = idx0[p, r], i1 = idx1[p, r], o = fine_matcher(cat(desc0[p, i0], desc1[p, i1]));
                      the row (kp0[p, i0] + offsets(o) scale0[p, i0], kp1[p, i1]) is kept iff confidence(o) > fine_conf; kept rows stay in match order.

The bounds (the pair test_fp16_pair_conv_is_fp32_accurate applies to the same two kernel kinds), with e = max |value - float64 value| over one case and T = max |float64 value|:

  e_f32 <= max(4 e_ref, 5e-6 T)         the f32-MFMA chain against the fp32 torch oracle (e_ref);
  e_fx  <= max(2 e_f32, 1e-6 T)         the fp16-pair chain against the f32-MFMA chain.

For the refined coordinates T is the largest |offset scale| of the case (the quantity the kernels compute; the key-point itself is data), and every element gets two fp32 ulps of
its own coordinate on top of the floor: kp0 + offset scale is rounded once more, and a coordinate near 1600 has an ulp of 1.2e-4 px."""
import numpy as np

from accelerated_features_amd.spec import BN_EPS, FINE

TEMP = 3.0


def _f64(t):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, np.float64)


def fine_matcher(sd, v, hidden_max=None):
    """hidden_max: a list that receives the largest activation behind each of the four ReLUs."""
    v = _f64(v)
    for li, fin, fout, bi in FINE:
        v = v @ _f64(sd[f"fine_matcher.{li}.weight"]).T + _f64(sd[f"fine_matcher.{li}.bias"])
        if bi is not None:
            v = (v - _f64(sd[f"fine_matcher.{bi}.running_mean"])) / np.sqrt(_f64(sd[f"fine_matcher.{bi}.running_var"]) + BN_EPS)
            v = np.maximum(v, 0.0)
            if hidden_max is not None:
                hidden_max.append(float(v.max()) if v.size else 0.0)
    return v


def softmax3(o):
    z = TEMP * _f64(o)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def confidence(o):
    return softmax3(o).max(-1)


def offsets(o):
    p = softmax3(o)
    k = np.arange(64)
    return np.stack([(p * (k % 8 - 4)).sum(-1), (p * (k // 8 - 4)).sum(-1)], -1)


def _live(desc0, desc1, idx0, idx1, n_matches):
    """(p, r, i0, i1) of every live row in packed order, and the clamped counts."""
    idx0, idx1 = np.asarray(idx0, np.int64), np.asarray(idx1, np.int64)
    P, N = idx0.shape
    assert idx1.shape == (P, N) and N == max(desc0.shape[1], desc1.shape[1])
    n = np.clip(np.asarray(n_matches, np.int64).reshape(P), 0, N)
    p = np.repeat(np.arange(P), n)
    r = np.concatenate([np.arange(k) for k in n]) if n.sum() else np.zeros(0, np.int64)
    return p, r, idx0[p, r], idx1[p, r], n


def live_logits(sd, desc0, desc1, idx0, idx1, n_matches):
    """Float64 logits of every live row in packed order (pair after pair, match order inside a pair): (total, 64)."""
    p, r, i0, i1, _ = _live(desc0, desc1, idx0, idx1, n_matches)
    return fine_matcher(sd, np.concatenate([_f64(desc0)[p, i0], _f64(desc1)[p, i1]], -1))


def refine(sd, desc0, desc1, kp0, kp1, scale0, idx0, idx1, n_matches, fine_conf):
    """-> (rows, n_out, info): rows[p] the (n_out[p], 4) float64 rows of pair p; info[p] = dict(kept: the match numbers r of the kept rows, conf: the confidences of the
    live rows, shift: |offset scale| of the kept rows (n_out[p], 2))."""
    p, r, i0, i1, n = _live(desc0, desc1, idx0, idx1, n_matches)
    o = fine_matcher(sd, np.concatenate([_f64(desc0)[p, i0], _f64(desc1)[p, i1]], -1))
    conf = confidence(o)
    shift = offsets(o) * _f64(scale0)[p, i0][:, None]
    full = np.concatenate([_f64(kp0)[p, i0] + shift, _f64(kp1)[p, i1]], -1)
    keep = conf > float(fine_conf)
    rows, info = [], []
    for q in range(len(n)):
        m = p == q
        k = keep[m]
        rows.append(full[m][k])
        info.append({"kept": r[m][k], "conf": conf[m], "shift": np.abs(shift[m][k])})
    return rows, np.array([len(x) for x in rows], np.int64), info


def confidence_margin(sd, desc0, desc1, idx0, idx1, n_matches, fine_conf):
    """The smallest |conf - fine_conf| over the live rows (inf without any)."""
    c = confidence(live_logits(sd, desc0, desc1, idx0, idx1, n_matches))
    return float(np.abs(c - float(fine_conf)).min()) if len(c) else float("inf")


# ---------------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def max_err(got, truth):
    got, truth = _f64(got), _f64(truth)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    if not got.size:
        return 0.0
    d = np.abs(got - truth)
    return float(np.where(np.isfinite(d), d, np.inf).max())


def check_bounds(tag, truth, ref, f32, fx=None, coord=None, T=None):
    """Print the three errors of one case and assert the two bounds.  coord: the float64 coordinates whose two ulps join the floors (None for logits); T: the magnitude the
    floors scale with (max |truth| when None).  -> (e_ref, e_f32, e_fx, ratio_f32, ratio_fx): the ratios are error / bound, at most 1 when the case passes."""
    truth = _f64(truth)
    if T is None:
        T = float(np.abs(truth).max()) if truth.size else 0.0
    extra = 2.0 * ulp32(coord) if coord is not None else np.zeros(truth.shape)
    e_ref, e_f32 = max_err(ref, truth), max_err(f32, truth)

    def ratio(got, rel, floor):
        if not truth.size:
            return 0.0
        d = np.abs(_f64(got) - truth)
        d = np.where(np.isfinite(d), d, np.inf)
        return float((d / np.maximum(rel, floor * T + extra)).max())
    r_f32 = ratio(f32, 4.0 * e_ref, 5e-6)
    e_fx = r_fx = None
    if fx is not None:
        e_fx, r_fx = max_err(fx, truth), ratio(fx, 2.0 * e_f32, 1e-6)
    print(f"{tag}: T {T:.4g} e_ref {e_ref:.3e} e_f32 {e_f32:.3e} e_fx {'-' if e_fx is None else format(e_fx, '.3e')} "
          f"f32/bound {r_f32:.3f} fx/bound {'-' if r_fx is None else format(r_fx, '.3f')}")
    assert r_f32 <= 1.0, (tag, "f32 chain", e_ref, e_f32, T)
    if fx is not None:
        assert r_fx <= 1.0, (tag, "fp16-pair chain", e_f32, e_fx, T)
    return e_ref, e_f32, e_fx, r_f32, r_fx
