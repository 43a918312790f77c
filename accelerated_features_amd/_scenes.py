"""What the scene-batched stages (multiview.py, verification.py, localization.py) share on the Python side: the limits of one library call,
the argument checks that several of them word alike and the loop that runs a batch in chunks of scenes.  Each function raises what the
stages raised in its place, text and type; a check that only looks like one of these stays in its stage.  Private: the public names live in
the three modules."""
import torch

from . import _lib, _twoview
from ._twoview import WORKSPACE_LIMIT, tensors      # noqa: F401 (the stages take both from here)

MAX_VIEWS = 32
MAX_SCENES = 65535                           # of one library call; larger batches are split into chunks of scenes


def chunks(S):
    return [(a, min(S, a + MAX_SCENES)) for a in range(0, S, MAX_SCENES)]


def run_scenes(name, S, workspace_bytes, dev, call):
    """One library call per chunk of at most MAX_SCENES scenes whose workspace (workspace_bytes(scenes)) stays under WORKSPACE_LIMIT:
    call(a, b, workspace pointer, workspace size, stream pointer) runs scenes [a, b) and returns the library's status."""
    for a, b in chunks(S):
        _twoview.run_chunked(name, b - a, WORKSPACE_LIMIT, workspace_bytes, dev, lambda c, d, ws, nb, st, a=a: call(a + c, a + d, ws, nb, st))


def views(who, V):
    if not 2 <= V <= MAX_VIEWS:
        raise _lib.XFeatHipError(f"{who}: V {V} outside [2, {MAX_VIEWS}]")


def f64(x, shape, dev, name):
    x = torch.as_tensor(x, dtype=torch.float64)
    if x.shape != shape:
        raise RuntimeError(f'{name} must be {tuple(shape)}')
    return x.to(dev).contiguous()


def n_views_arg(n_views, S, dev):
    """n_views (S,) or None -> int32 on the device, or None (every scene uses all its views)."""
    if n_views is None:
        return None
    n_views = torch.as_tensor(n_views)
    if n_views.shape != (S,):
        raise RuntimeError('n_views must have one entry per scene')
    return n_views.to(dev).to(torch.int32).contiguous()


def kpts_tracks(kpts, tracks):
    """The shapes of kpts (S,V,Kcap,2) and tracks (S,K,V) -> S, V, Kcap, K."""
    if kpts.dim() != 4 or kpts.shape[3] != 2 or tracks.dim() != 3 or tracks.shape[0] != kpts.shape[0] or tracks.shape[2] != kpts.shape[1]:
        raise RuntimeError('expected kpts (S,V,Kcap,2) and tracks (S,K,V)')
    return tuple(kpts.shape[:3]) + (tracks.shape[1],)


def check_view_pairs(view_pairs, S, P):
    if view_pairs.shape not in ((S, P, 2), (P, 2)):
        raise RuntimeError('expected view_pairs (S,P,2) or (P,2)')


def view_pairs_arg(view_pairs, S, P, dev):
    """view_pairs (S,P,2), or (P,2) for every scene -> (S,P,2) int32 on the device."""
    if view_pairs.dim() == 2:
        view_pairs = view_pairs.expand(S, P, 2)
    return view_pairs.to(dev).to(torch.int32).contiguous()


def check_edges(view_pairs, t_rel, weight, S, P):
    """The edges of a pose graph behind R_rel (S,P,3,3), which the stage checks itself: t_rel (S,P,3), weight (S,P), then the pairs."""
    if t_rel.shape != (S, P, 3) or weight.shape != (S, P):
        raise RuntimeError('expected t_rel (S,P,3) and weight (S,P)')
    check_view_pairs(view_pairs, S, P)


def edges_arg(view_pairs, R_rel, t_rel, weight, S, P, dev):
    """-> the pairs as int32 (S,P,2) and R_rel, t_rel, weight as float64, contiguous on the device."""
    return (view_pairs_arg(view_pairs, S, P, dev),) + tuple(x.to(dev).to(torch.float64).contiguous() for x in (R_rel, t_rel, weight))
