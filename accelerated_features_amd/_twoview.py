"""What the RANSAC estimators over pairs (homography.py, pose.py, fundamental.py, absolute_pose.py, alignment.py) share on the Python side:
the device and argument checks of their two kinds of entry point (point tensors; tables + the matcher's index lists), the intrinsics
argument, the seed of a chunk of pairs and the loop that runs a batch in chunks of pairs under the workspace limit.  structure.py and the
scene-batched stages (_scenes.py) use the device, the pointers and that loop.  Private: the public names live in those modules."""
import ctypes as C

import numpy as np
import torch

from . import _lib

WORKSPACE_LIMIT = 512 << 20                  # bytes of workspace per library call: larger batches are split into chunks of pairs or scenes


def device(what):
    if not torch.cuda.is_available():
        raise _lib.XFeatHipError(f"{what} needs an AMD MI355X (gfx950) GPU; no CPU fallback exists")
    return torch.device('cuda', torch.cuda.current_device())


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def tensors(who, *ts):
    for t in ts:
        if not torch.is_tensor(t):
            raise RuntimeError(f'{who}: tensors expected')


def intrinsics(K, P, dev):
    K = torch.as_tensor(K, dtype=torch.float64)
    if K.shape == (3, 3):
        K = K.expand(P, 3, 3)
    if K.shape != (P, 3, 3):
        raise RuntimeError('intrinsics must be (3,3) or (P,3,3)')
    return K.to(dev).contiguous()


def as_points(x):
    """(N, 2) tensor from an (N,2) / (N,1,2) array or tensor."""
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).reshape(-1, 2)


def chunk_seed(seed, first_pair):
    """The draws of pair p take (seed, p): a chunk that starts at pair `first_pair` sees its pairs as 0, 1, ..., so its seed is advanced by
    the counter stride of `first_pair` pairs (golden * 2^24 per pair, mod 2^64) and the draws stay those of the whole batch."""
    return (int(seed) + first_pair * 0x9e3779b97f4a7c15 * (1 << 24)) & ((1 << 64) - 1)


def check_points(what, pts0, pts1, counts):
    """Two (P, cap, 2) point lists (anything torch.as_tensor takes) and their counts or None -> float32 / int32 tensors on the device."""
    dev = pts0.device if torch.is_tensor(pts0) and pts0.is_cuda else device(what)
    pts0 = torch.as_tensor(pts0).to(dev).float().contiguous()
    pts1 = torch.as_tensor(pts1).to(dev).float().contiguous()
    if pts0.dim() != 3 or pts0.shape[2] != 2 or pts1.shape != pts0.shape:
        raise RuntimeError('expected two (P, cap, 2) point tensors of the same shape')
    if counts is not None:
        counts = torch.as_tensor(counts).to(dev).to(torch.int32).contiguous()
        if counts.shape != (pts0.shape[0],):
            raise RuntimeError('counts must have one entry per pair')
    return pts0, pts1, counts, dev


def check_matches(who, kpts0, kpts1, idx0, idx1, n_matches):
    """The matcher's device-resident output: kpts (P,K,2) float32, idx (P,cap) int64, n_matches (P,) int32.  Returns (device, P, cap)."""
    if not kpts0.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    P, cap = idx0.shape
    if kpts0.shape != kpts1.shape or kpts0.shape[0] != P or kpts0.shape[2] != 2 or idx1.shape != idx0.shape or n_matches.shape != (P,):
        raise RuntimeError('expected kpts (P,K,2), idx (P,cap), n_matches (P,)')
    for t, dt in ((kpts0, torch.float32), (kpts1, torch.float32), (idx0, torch.int64), (idx1, torch.int64), (n_matches, torch.int32)):
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f'{who}: contiguous float32 key-points, int64 indices, int32 counts expected')
    return kpts0.device, P, cap


def list_args(pts0, pts1, index, counts, n_const, a, b, cap):
    """The leading arguments of xfh_<estimator> (index None) or xfh_<estimator>_matches (index = (idx0, idx1, kcap)) for pairs [a, b)."""
    if index is None:
        return (ptr(pts0[a:b]), ptr(pts1[a:b]), ptr(counts[a:b]) if counts is not None else None, n_const, b - a, cap)
    idx0, idx1, kcap = index
    return (ptr(pts0[a:b]), ptr(pts1[a:b]), kcap, ptr(idx0[a:b]), ptr(idx1[a:b]), ptr(counts[a:b]), b - a, cap)


def run_chunked(who, P, limit, workspace_bytes, dev, call):
    """One library call per chunk of pairs whose workspace (workspace_bytes(pairs)) stays under `limit` bytes: call(a, b, workspace
    pointer, workspace size, stream pointer) runs pairs [a, b) and returns the library's status.  A chunk's seed is chunk_seed(seed, a)."""
    stream = torch.cuda.current_stream(dev)
    step = max(1, min(P, limit // max(workspace_bytes(1), 1)))
    for a in range(0, P, step):
        b = min(P, a + step)
        ws = torch.empty(workspace_bytes(b - a) + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        ws.record_stream(stream)
        _lib.check(call(a, b, C.c_void_p(ws.data_ptr() + off), ws.numel() - off, C.c_void_p(stream.cuda_stream)), who)


def check_points_2d3d(what, pts2d, pts3d, counts):
    """A (P, cap, 2) and a (P, cap, 3) point list (anything torch.as_tensor takes) and their counts or None -> float32 / int32 tensors on
    the device."""
    dev = pts2d.device if torch.is_tensor(pts2d) and pts2d.is_cuda else device(what)
    pts2d = torch.as_tensor(pts2d).to(dev).float().contiguous()
    pts3d = torch.as_tensor(pts3d).to(dev).float().contiguous()
    if pts2d.dim() != 3 or pts2d.shape[2] != 2 or pts3d.dim() != 3 or pts3d.shape[2] != 3 or pts3d.shape[:2] != pts2d.shape[:2]:
        raise RuntimeError('expected a (P, cap, 2) and a (P, cap, 3) point tensor of the same P and cap')
    if counts is not None:
        counts = torch.as_tensor(counts).to(dev).to(torch.int32).contiguous()
        if counts.shape != (pts2d.shape[0],):
            raise RuntimeError('counts must have one entry per pair')
    return pts2d, pts3d, counts, dev


def check_matches_2d3d(who, kpts2d, points3d, idx2d, idx3d, n_matches):
    """Key-points (P,K2,2) float32, 3D points (P,K3,3) float32 (K2 and K3 independent), idx (P,cap) int64, n_matches (P,) int32, all
    device-resident.  Returns (device, P, cap)."""
    if not kpts2d.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    P, cap = idx2d.shape
    if (kpts2d.dim() != 3 or points3d.dim() != 3 or kpts2d.shape[0] != P or points3d.shape[0] != P or kpts2d.shape[2] != 2
            or points3d.shape[2] != 3 or idx3d.shape != idx2d.shape or n_matches.shape != (P,)):
        raise RuntimeError('expected kpts (P,K2,2), points3d (P,K3,3), idx (P,cap), n_matches (P,)')
    for t, dt in ((kpts2d, torch.float32), (points3d, torch.float32), (idx2d, torch.int64), (idx3d, torch.int64), (n_matches, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != kpts2d.device:
            raise RuntimeError(f'{who}: contiguous float32 points, int64 indices, int32 counts on one device expected')
    return kpts2d.device, P, cap


def check_points_3d3d(what, pts_a, pts_b, counts):
    """Two (P, cap, 3) point lists (anything torch.as_tensor takes) and their counts or None -> float32 / int32 tensors on the device.
    The shapes are checked before the device is asked for."""
    pts_a, pts_b = torch.as_tensor(pts_a), torch.as_tensor(pts_b)
    if pts_a.dim() != 3 or pts_a.shape[2] != 3 or pts_b.shape != pts_a.shape:
        raise RuntimeError('expected two (P, cap, 3) point tensors of the same shape')
    if counts is not None:
        counts = torch.as_tensor(counts)
        if counts.shape != (pts_a.shape[0],):
            raise RuntimeError('counts must have one entry per pair')
    dev = pts_a.device if pts_a.is_cuda else device(what)
    pts_a, pts_b = pts_a.to(dev).float().contiguous(), pts_b.to(dev).float().contiguous()
    if counts is not None:
        counts = counts.to(dev).to(torch.int32).contiguous()
    return pts_a, pts_b, counts, dev


def check_matches_3d3d(who, points_a, points_b, idx_a, idx_b, n_matches):
    """Two point tables (P,Ka,3), (P,Kb,3) float32 (Ka and Kb independent), idx (P,cap) int64, n_matches (P,) int32, all device-resident.
    Returns (device, P, cap)."""
    tensors(who, points_a, points_b, idx_a, idx_b, n_matches)
    if idx_a.dim() != 2:
        raise RuntimeError('expected idx (P,cap)')
    P, cap = idx_a.shape
    if (points_a.dim() != 3 or points_b.dim() != 3 or points_a.shape[0] != P or points_b.shape[0] != P or points_a.shape[2] != 3
            or points_b.shape[2] != 3 or idx_b.shape != idx_a.shape or n_matches.shape != (P,)):
        raise RuntimeError('expected points_a (P,Ka,3), points_b (P,Kb,3), idx (P,cap), n_matches (P,)')
    for t, dt in ((points_a, torch.float32), (points_b, torch.float32), (idx_a, torch.int64), (idx_b, torch.int64), (n_matches, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != points_a.device:
            raise RuntimeError(f'{who}: contiguous float32 points, int64 indices, int32 counts on one device expected')
    if not points_a.is_cuda:
        raise _lib.XFeatHipError(f"{who} works on device-resident match lists")
    return points_a.device, P, cap
