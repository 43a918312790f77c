"""Guided matching on MI355X: the matcher's arg-max taken again under a known two-view geometry.

``XFeat.match`` and ``xfh_match_mnn`` are unconstrained mutual nearest neighbours: on repeated structure (facades, tiles, a planar
target seen twice) the globally most similar descriptor is often the wrong instance, and the estimators can only verify what survived.
Once a model is known -- F from ``find_fundamental_matches``, E from ``estimate_relative_pose_matches`` brought to pixels by
``fundamental_from_pose``, last frame's H in ``ReferenceTracker`` -- ``match_guided_device`` repeats the mutual arg-max among only those
candidates whose key-points agree with it: Sampson error (``kind='fundamental'``, the quantity ``find_fundamental_*`` thresholds, so
``max_error`` means what ``ransac_thr`` means there) or forward transfer error (``kind='homography'``, as ``find_homography_*``) at most
``max_error`` pixels.  The kernel behind ``xfh_match_mnn_guided`` (include/xfeat_hip.h, csrc/k_match_guided.hip) is the exact f32
matrix-core sweep of the matcher with that test in its epilogue; descriptors, key-points and models stay in HBM and nothing is read back.
There is no CPU path: without the HIP library and a gfx950 device these functions raise.
"""
import ctypes as C

import torch

from . import _lib, _twoview
from ._twoview import ptr as _ptr

KINDS = {'fundamental': _lib.GUIDE_FUNDAMENTAL, 'homography': _lib.GUIDE_HOMOGRAPHY}


def _workspace(nbytes, dev):
    ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    ws.record_stream(torch.cuda.current_stream(dev))
    return C.c_void_p(ws.data_ptr() + off), ws.numel() - off, ws


def _check_sets(who, desc_a, n_a, desc_b, n_b):
    if not desc_a.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident descriptors")
    if desc_a.dim() != 3 or desc_b.dim() != 3 or desc_a.shape[2] != 64 or desc_b.shape[2] != 64 or desc_a.shape[0] != desc_b.shape[0]:
        raise RuntimeError('descriptors must be (P,N1,64) and (P,N2,64)')
    P = desc_a.shape[0]
    for t in (desc_a, desc_b):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != desc_a.device:
            raise RuntimeError(f'{who}: contiguous float32 descriptors on one device expected')
    # one count array so that a single (stride, offset) addresses both sides
    nv = torch.cat([n_a.to(desc_a.device).to(torch.int32).reshape(-1), n_b.to(desc_a.device).to(torch.int32).reshape(-1)]).contiguous()
    if nv.shape != (2 * P,):
        raise RuntimeError('n_a and n_b must have one entry per pair')
    return P, nv


def _outputs(P, N1, dev):
    return (torch.empty((P, N1), dtype=torch.int64, device=dev), torch.empty((P, N1), dtype=torch.int64, device=dev),
            torch.empty((P,), dtype=torch.int32, device=dev))


def _plain_mnn(desc_a, n_a, desc_b, n_b, min_cossim):
    """The shipped matcher (xfh_match_mnn, no handle: default options) on two descriptor sets with a workspace of its own."""
    P, nv = _check_sets("rematch_fundamental", desc_a, n_a, desc_b, n_b)
    N1, N2, dev = desc_a.shape[1], desc_b.shape[1], desc_a.device
    idx0, idx1, n = _outputs(P, N1, dev)
    if P == 0 or N1 == 0 or N2 == 0:
        n.zero_()
        return idx0, idx1, n
    lib = _lib.load()
    ws, nb, _keep = _workspace(lib.xfh_match_workspace_bytes(P, N1, N2), dev)
    _lib.check(lib.xfh_match_mnn(None, _ptr(desc_a), N1 * 64, _ptr(desc_b), N2 * 64, None, None, _ptr(nv), _ptr(nv), 1, P, P, N1, N2, float(min_cossim),
                                 _ptr(idx0), _ptr(idx1), _ptr(n), ws, nb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "xfh_match_mnn")
    return idx0, idx1, n


def match_guided_device(desc_a, kpts_a, n_a, desc_b, kpts_b, n_b, models, kind='fundamental', max_error=3.0, min_cossim=-1):
    """Mutual nearest neighbours of pair p = (desc_a[p], desc_b[p]) among the candidates (i, j) whose key-points kpts_a[p, i], kpts_b[p, j]
    agree with models[p] within ``max_error`` pixels.

    desc_a (P,N1,64), desc_b (P,N2,64) float32; kpts_a (P,N1,2), kpts_b (P,N2,2) float32 pixel coordinates; n_a, n_b (P,) valid rows
    models : (P,3,3) float64 -- kind 'fundamental': x_b' F x_a = 0 (the F of ``find_fundamental_*``; for a pose see
             ``fundamental_from_pose``), Sampson error; kind 'homography': x_b ~ H x_a (the H of ``find_homography_*``), forward transfer error
    A pair whose model is all zero (what the estimators write where they found nothing) or holds a non-finite entry gets no matches.
    Returns idx0, idx1 (P,N1) int64 (idx0 ascending, ties to the lowest index) and n_matches (P,) int32 on the device, no read-back: the
    shape of ``XFeat.match_sets_device``, so the outputs feed ``find_*_matches`` / ``estimate_*_matches`` directly.  Asynchronous."""
    if kind not in KINDS:
        raise _lib.XFeatHipError(f"match_guided_device: kind {kind!r} is not implemented ('fundamental' and 'homography' are)")
    if not (float(max_error) > 0.0 and float(max_error) < float('inf')):
        raise _lib.XFeatHipError(f"match_guided_device: max_error {max_error} must be positive and finite")
    P, nv = _check_sets("match_guided_device", desc_a, n_a, desc_b, n_b)
    N1, N2, dev = desc_a.shape[1], desc_b.shape[1], desc_a.device
    for k, N in ((kpts_a, N1), (kpts_b, N2)):
        if k.shape != (P, N, 2) or k.dtype != torch.float32 or not k.is_contiguous() or k.device != dev:
            raise RuntimeError('match_guided_device: contiguous float32 key-points (P,N,2) beside their descriptors expected')
    models = torch.as_tensor(models).to(dev).to(torch.float64).contiguous()
    if models.shape != (P, 3, 3):
        raise RuntimeError('models must be (P,3,3)')
    idx0, idx1, n = _outputs(P, N1, dev)
    if P == 0 or N1 == 0 or N2 == 0:
        n.zero_()
        return idx0, idx1, n
    lib = _lib.load()
    ws, nb, _keep = _workspace(lib.xfh_match_guided_workspace_bytes(P, N1, N2), dev)
    _lib.check(lib.xfh_match_mnn_guided(_ptr(desc_a), N1 * 64, _ptr(desc_b), N2 * 64, _ptr(kpts_a), N1 * 2, _ptr(kpts_b), N2 * 2, _ptr(nv), _ptr(nv), 1, P,
                                        P, N1, N2, _ptr(models), KINDS[kind], float(max_error), float(min_cossim), _ptr(idx0), _ptr(idx1), _ptr(n), ws, nb,
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "xfh_match_mnn_guided")
    return idx0, idx1, n


def match_guided(feats1, feats2, model, kind='fundamental', max_error=3.0, min_cossim=-1):
    """One pair, on the dicts ``XFeat.detectAndCompute`` returns ('keypoints' (N,2), 'descriptors' (N,64)); model (3,3).  Returns
    (idx0, idx1) like ``XFeat.match``: rows of feats1 / feats2 of the guided mutual matches (one read-back: the count)."""
    dev = _twoview.device("match_guided")
    k1, d1 = feats1['keypoints'].to(dev).float().contiguous(), feats1['descriptors'].to(dev).float().contiguous()
    k2, d2 = feats2['keypoints'].to(dev).float().contiguous(), feats2['descriptors'].to(dev).float().contiguous()
    if len(d1) == 0 or len(d2) == 0:
        e = torch.empty((0,), dtype=torch.int64, device=dev)
        return e, e.clone()
    n1 = torch.tensor([len(d1)], dtype=torch.int32, device=dev)
    n2 = torch.tensor([len(d2)], dtype=torch.int32, device=dev)
    idx0, idx1, n = match_guided_device(d1[None], k1[None], n1, d2[None], k2[None], n2, torch.as_tensor(model).reshape(1, 3, 3), kind, max_error, min_cossim)
    k = int(n.item())
    return idx0[0, :k], idx1[0, :k]


def fundamental_from_pose(R, t, K0, K1):
    """F = K1^-T [t]x R K0^-1 of X1 = R X0 + t, batched float64 torch ((...,3,3), (...,3), (...,3,3), (...,3,3)): the result of
    ``estimate_relative_pose_*`` (its 'R', 't' and the intrinsics it was given) as a model for ``match_guided_device``.  A zero t
    (nothing found) gives a zero F, which guides nothing."""
    R, t, K0, K1 = (torch.as_tensor(v).to(torch.float64) for v in (R, t, K0, K1))
    tx = torch.zeros(t.shape[:-1] + (3, 3), dtype=torch.float64, device=t.device)
    tx[..., 0, 1], tx[..., 0, 2], tx[..., 1, 2] = -t[..., 2], t[..., 1], -t[..., 0]
    tx[..., 1, 0], tx[..., 2, 0], tx[..., 2, 1] = t[..., 2], -t[..., 1], t[..., 0]
    return torch.linalg.inv(K1).transpose(-1, -2) @ tx @ R @ torch.linalg.inv(K0)


def rematch_fundamental(kpts_a, desc_a, n_a, kpts_b, desc_b, n_b, ransac_thr=3.0, max_error=None, min_cossim=-1, max_iters=1000, confidence=0.99,
                        seed=0, min_inlier_ratio=0.1):
    """Plain mutual nearest neighbours -> ``find_fundamental_matches`` -> guided mutual nearest neighbours under that F ->
    ``find_fundamental_matches`` again, all on the device (no read-back).  max_error: the gate in pixels (None = ransac_thr).
    Pairs whose first stage found nothing keep their plain matches in the second, and so do pairs whose first F is supported by fewer than
    ``min_inlier_ratio`` of their plain matches: a sample of seven points always fits its own F, so a handful of inliers says nothing about
    the scene, and a gate around such an F would only select matches that agree with it.  Returns a dict: 'first' / 'second' (the two result
    dicts of find_fundamental_matches), 'idx0_first', 'idx1_first', 'n_first', 'idx0', 'idx1', 'n_matches' (the second stage's lists)."""
    from .fundamental import find_fundamental_matches
    max_error = ransac_thr if max_error is None else max_error
    i0, i1, n = _plain_mnn(desc_a, n_a, desc_b, n_b, min_cossim)
    first = find_fundamental_matches(kpts_a, kpts_b, i0, i1, n, ransac_thr, max_iters, confidence, seed)
    g0, g1, gn = match_guided_device(desc_a, kpts_a, n_a, desc_b, kpts_b, n_b, first['F'], 'fundamental', max_error, min_cossim)
    found = (first['info'][:, 0] > 0) & (first['info'][:, 3].to(torch.float64) >= float(min_inlier_ratio) * n.to(torch.float64))
    j0, j1, jn = torch.where(found[:, None], g0, i0), torch.where(found[:, None], g1, i1), torch.where(found, gn, n)
    second = find_fundamental_matches(kpts_a, kpts_b, j0, j1, jn, ransac_thr, max_iters, confidence, seed)
    return {'first': first, 'second': second, 'idx0_first': i0, 'idx1_first': i1, 'n_first': n, 'idx0': j0, 'idx1': j1, 'n_matches': jn}
