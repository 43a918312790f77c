"""Image retrieval on MI355X: which images to match, and which map to query.

``relative_poses_graph_matches`` / ``reconstruct_graph_matches`` take ``view_pairs`` and ``localize_map_batch`` takes ``scene_of``; the functions
here produce both from the local descriptors the detector already computes, without a trained network.  ``train_codebook`` learns a small
codebook by spherical k-means from the descriptors, ``global_descriptors_batch`` turns the descriptors of an image into one VLAD vector over
that codebook, ``retrieve_topk`` reads a shortlist off the inner products of the global vectors and ``select_pairs`` turns the shortlists of
the views of a scene into its pair list.  The kernels behind ``xfh_kmeans_step`` / ``xfh_vlad`` / ``xfh_retrieve_topk`` /
``xfh_pairs_from_shortlists`` (include/xfeat_hip.h, csrc/k_retrieval.hip) are specified in DESIGN.md 3.23: fp32 in fixed orders of summation,
two calls give the same bytes.  There is no CPU path: without the HIP library and a gfx950 device the functions raise.
"""
import ctypes as C

import torch

from . import _lib, _scenes, _twoview
from ._scenes import MAX_SCENES, MAX_VIEWS, WORKSPACE_LIMIT      # noqa: F401 (public here)
from ._twoview import ptr as _ptr

CODEBOOK_SIZES = (32, 64, 128, 256)
MAX_SHORTLIST = 128
MAX_DIM = 16384
MAX_VLAD_ROWS = 1 << 24                      # descriptor rows of one xfh_vlad call
MAX_KMEANS_ROWS = 1 << 22                    # descriptor rows of a training set
VLAD_INFO_FIELDS = ("valid", "invalid", "blocks", "empty")
KMEANS_INFO_FIELDS = ("valid", "invalid", "kept", "spare")
_WHAT = "image retrieval"


def _tables(who, desc, counts):
    """desc (G,K,64) (or (K,64): one group) and counts (G,) or None -> the tensors as given, G, K."""
    desc = torch.as_tensor(desc)
    if desc.dim() == 2:
        desc = desc.unsqueeze(0)
    if desc.dim() != 3 or desc.shape[2] != 64:
        raise RuntimeError('expected desc (G,K,64)')
    G, K = desc.shape[:2]
    if counts is not None:
        counts = torch.as_tensor(counts)
        if counts.shape != (G,):
            raise RuntimeError('counts must have one entry per group')
    return desc, counts, G, K


def _codebook_size(who, n):
    if isinstance(n, bool) or int(n) not in CODEBOOK_SIZES:
        raise _lib.XFeatHipError(f"{who}: {n} centroids; the codebook sizes are {CODEBOOK_SIZES}")
    return int(n)


def _shortlist(who, k):
    if isinstance(k, bool) or not 1 <= int(k) <= MAX_SHORTLIST:
        raise _lib.XFeatHipError(f"{who}: k {k} outside [1, {MAX_SHORTLIST}]")
    return int(k)


def _workspace(nbytes, dev):
    ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    ws.record_stream(torch.cuda.current_stream(dev))
    return C.c_void_p(ws.data_ptr() + off), ws.numel() - off, ws


def initial_codebook(desc, counts, n_centroids):
    """The start of ``train_codebook`` with init=None.  The rows that are below their group's count and finite are numbered 0 .. R - 1 in
    (group, row) order; centroid c starts as row number floor(c R / n_centroids).  Fewer such rows than centroids repeat rows (the repeated
    centroids attract nothing and stay); R = 0 gives the last row of the table.  Index arithmetic only, on the descriptors' device."""
    G, K = desc.shape[:2]
    flat = desc.reshape(G * K, 64)
    ok = torch.isfinite(flat).all(dim=1)
    if counts is not None:
        ok &= (torch.arange(K, device=desc.device)[None, :] < counts.to(desc.device)[:, None]).reshape(G * K)
    order = torch.cumsum(ok.to(torch.int64), 0)
    want = (torch.arange(n_centroids, device=desc.device, dtype=torch.int64) * order[-1]) // n_centroids
    at = torch.searchsorted(order, want + 1).clamp(max=G * K - 1)
    return flat[at].contiguous()


def train_codebook(desc, counts=None, n_centroids=64, iterations=10, init=None):
    """A codebook for ``global_descriptors_batch``: `iterations` steps of spherical k-means (``xfh_kmeans_step``) over all rows as one set.

    desc        : (G,K,64) float32 unit descriptors (or (K,64)), G K <= 2^22;  counts (G,) valid rows per group, None = K
    n_centroids : 32, 64, 128 or 256;  init: (n_centroids,64) float32 start, None = ``initial_codebook`` (rows at a fixed stride)
    A step assigns every valid row to the centroid of its largest inner product (the lowest index among equals), sums the rows of a cluster in
    ascending row order and scales the sum to unit length; a cluster that is empty or whose sum has no direction keeps its centroid.
    Returns a dict of CUDA tensors: 'codebook' (C,64) float32, 'objective' (iterations,) float64 (the sum of the winning scores of each step,
    under the codebook the step started from), 'info' (iterations,4) int32 (KMEANS_INFO_FIELDS).  A fixed number of steps, nothing
    synchronises with the host; two calls give the same bytes."""
    who = "train_codebook"
    desc, counts, G, K = _tables(who, desc, counts)
    n_centroids = _codebook_size(who, n_centroids)
    if isinstance(iterations, bool) or not 1 <= int(iterations) <= 1000:
        raise _lib.XFeatHipError(f"{who}: iterations {iterations} outside [1, 1000]")
    iterations = int(iterations)
    if init is not None:
        init = torch.as_tensor(init)
        if init.shape != (n_centroids, 64):
            raise RuntimeError('init must be (n_centroids,64)')
    if G * K < 1:
        raise _lib.XFeatHipError(f"{who}: no descriptor rows")
    if G > MAX_SCENES or G * K > MAX_KMEANS_ROWS:
        raise _lib.XFeatHipError(f"{who}: {G} x {K} rows; a training set holds at most {MAX_SCENES} groups and {MAX_KMEANS_ROWS} rows")
    dev = desc.device if desc.is_cuda else _twoview.device(_WHAT)
    desc = desc.to(dev).float().contiguous()
    counts = counts.to(dev).to(torch.int32).contiguous() if counts is not None else None
    book = [initial_codebook(desc, counts, n_centroids) if init is None else init.to(dev).float().contiguous().clone(),
            torch.empty((n_centroids, 64), dtype=torch.float32, device=dev)]
    objective = torch.empty((iterations,), dtype=torch.float64, device=dev)
    info = torch.empty((iterations, 4), dtype=torch.int32, device=dev)
    assign = torch.empty((G, K), dtype=torch.int32, device=dev)
    n_assigned = torch.empty((n_centroids,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws, nb, _keep = _workspace(lib.xfh_kmeans_workspace_bytes(G, K, n_centroids), dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for it in range(iterations):
        _lib.check(lib.xfh_kmeans_step(_ptr(desc), _ptr(counts), G, K, _ptr(book[it & 1]), n_centroids, _ptr(book[1 - (it & 1)]), _ptr(assign),
                                       _ptr(n_assigned), _ptr(objective[it:]), _ptr(info[it:]), ws, nb, stream), "xfh_kmeans_step")
    return {'codebook': book[iterations & 1], 'objective': objective, 'info': info}


def kmeans_step(desc, counts, codebook):
    """One ``xfh_kmeans_step``: -> 'codebook' (C,64), 'assign' (G,K) int32, 'n_assigned' (C,) int32, 'objective' () float64, 'info' (4,) int32."""
    who = "kmeans_step"
    desc, counts, G, K = _tables(who, desc, counts)
    codebook = torch.as_tensor(codebook)
    if codebook.dim() != 2 or codebook.shape[1] != 64:
        raise RuntimeError('expected codebook (C,64)')
    n = _codebook_size(who, codebook.shape[0])
    if G * K < 1 or G > MAX_SCENES or G * K > MAX_KMEANS_ROWS:
        raise _lib.XFeatHipError(f"{who}: {G} x {K} rows outside what a training set holds")
    dev = desc.device if desc.is_cuda else _twoview.device(_WHAT)
    desc, codebook = desc.to(dev).float().contiguous(), codebook.to(dev).float().contiguous()
    counts = counts.to(dev).to(torch.int32).contiguous() if counts is not None else None
    out = {'codebook': torch.empty_like(codebook), 'assign': torch.empty((G, K), dtype=torch.int32, device=dev),
           'n_assigned': torch.empty((n,), dtype=torch.int32, device=dev), 'objective': torch.empty((), dtype=torch.float64, device=dev),
           'info': torch.empty((4,), dtype=torch.int32, device=dev)}
    lib = _lib.load()
    ws, nb, _keep = _workspace(lib.xfh_kmeans_workspace_bytes(G, K, n), dev)
    _lib.check(lib.xfh_kmeans_step(_ptr(desc), _ptr(counts), G, K, _ptr(codebook), n, _ptr(out['codebook']), _ptr(out['assign']), _ptr(out['n_assigned']),
                                   _ptr(out['objective']), _ptr(out['info']), ws, nb, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "xfh_kmeans_step")
    return out


def global_descriptors_batch(desc, counts, codebook):
    """One VLAD vector per image (``xfh_vlad``).

    desc (G,K,64) float32 unit descriptors, counts (G,) valid rows or None = K (``XFeat._detect_device`` per image); codebook (C,64) float32
    of ``train_codebook``.  A row is valid when it is below its count and finite; it goes to the centroid of its largest inner product.  Per
    centroid the residuals row - centroid are summed in ascending row order, the 64-block is scaled to unit length (zero when it has no
    direction) and the vector is divided by the square root of the number of non-zero blocks: a unit vector, or zero.
    Returns a dict of CUDA tensors: 'vlad' (G, C*64) float32, 'assign' (G,K) int32 (-1: not valid), 'n_assigned' (G,C) int32, 'info' (G,4)
    int32 (VLAD_INFO_FIELDS).  Asynchronous; two calls give the same bytes."""
    who = "global_descriptors_batch"
    desc, counts, G, K = _tables(who, desc, counts)
    codebook = torch.as_tensor(codebook)
    if codebook.dim() != 2 or codebook.shape[1] != 64:
        raise RuntimeError('expected codebook (C,64)')
    n = _codebook_size(who, codebook.shape[0])
    if K > MAX_VLAD_ROWS:
        raise _lib.XFeatHipError(f"{who}: K {K} above {MAX_VLAD_ROWS}")
    empty = G == 0 or K == 0
    dev = desc.device if desc.is_cuda or empty else _twoview.device(_WHAT)
    desc, codebook = desc.to(dev).float().contiguous(), codebook.to(dev).float().contiguous()
    counts = counts.to(dev).to(torch.int32).contiguous() if counts is not None else None
    out = {'vlad': torch.empty((G, n * 64), dtype=torch.float32, device=dev), 'assign': torch.empty((G, K), dtype=torch.int32, device=dev),
           'n_assigned': torch.empty((G, n), dtype=torch.int32, device=dev), 'info': torch.empty((G, 4), dtype=torch.int32, device=dev)}
    if empty:                                 # no row: written like the kernels write it
        out['vlad'].zero_(); out['n_assigned'].zero_(); out['info'].zero_()
        out['info'][:, 3] = 1
        return out
    lib = _lib.load()

    def call(a, b, ws, nb, stream):
        return lib.xfh_vlad(_ptr(desc[a:b]), _ptr(counts[a:b]) if counts is not None else None, b - a, K, _ptr(codebook), n, _ptr(out['vlad'][a:b]),
                            _ptr(out['assign'][a:b]), _ptr(out['n_assigned'][a:b]), _ptr(out['info'][a:b]), ws, nb, stream)
    per_group = max(lib.xfh_vlad_workspace_bytes(1, K, n), 1)
    limit = min(WORKSPACE_LIMIT, per_group * max(1, MAX_VLAD_ROWS // K))      # (a call also holds at most MAX_VLAD_ROWS rows)
    for a, b in _scenes.chunks(G):
        _twoview.run_chunked("xfh_vlad", b - a, limit, lambda g: lib.xfh_vlad_workspace_bytes(g, K, n), dev,
                             lambda c, d, ws, nb, st, a=a: call(a + c, a + d, ws, nb, st))
    return out


def retrieve_topk(query, database, k, n_database=None, exclude_self=False):
    """The k database vectors of the largest inner product for every query (``xfh_retrieve_topk``).

    query (G,Q,D), database (G,N,D) float32 -- or (Q,D), (N,D): one group, the global case -- with D a multiple of 64 up to 16384;
    n_database (G,) (a scalar tensor or int for one group) valid database rows, None = N;  1 <= k <= 128;
    exclude_self: query j never returns database row j (the database is the query set).
    Returns a dict of CUDA tensors: 'idx' (G,Q,k) int32 and 'score' (G,Q,k) float32 (without G for 2-D inputs): the rows with a finite score,
    by score descending and then index ascending; -1 and NaN past the number found.  Asynchronous; two calls give the same bytes."""
    who = "retrieve_topk"
    query, database = torch.as_tensor(query), torch.as_tensor(database)
    flat = query.dim() == 2
    if flat:
        query = query.unsqueeze(0)
        if database.dim() == 2:
            database = database.unsqueeze(0)
    if query.dim() != 3 or database.dim() != 3 or query.shape[0] != database.shape[0] or query.shape[2] != database.shape[2]:
        raise RuntimeError('expected query (G,Q,D) and database (G,N,D), or (Q,D) and (N,D)')
    G, Q, D = query.shape
    N = database.shape[1]
    if n_database is not None:
        n_database = torch.as_tensor(n_database).reshape(-1) if flat else torch.as_tensor(n_database)
        if n_database.shape != (G,):
            raise RuntimeError('n_database must have one entry per group')
    k = _shortlist(who, k)
    if D < 64 or D % 64 != 0 or D > MAX_DIM:
        raise _lib.XFeatHipError(f"{who}: D {D} is not a multiple of 64 in [64, {MAX_DIM}]")
    empty = G == 0 or Q == 0 or N == 0
    dev = query.device if query.is_cuda or empty else _twoview.device(_WHAT)
    query, database = query.to(dev).float().contiguous(), database.to(dev).float().contiguous()
    n_database = n_database.to(dev).to(torch.int32).contiguous() if n_database is not None else None
    idx = torch.empty((G, Q, k), dtype=torch.int32, device=dev)
    score = torch.empty((G, Q, k), dtype=torch.float32, device=dev)
    if empty:
        idx.fill_(-1); score.fill_(float('nan'))
    else:
        lib = _lib.load()
        if lib.xfh_retrieve_workspace_bytes(1, Q, N) == 0:
            raise _lib.XFeatHipError(f"{who}: {Q} x {N} scores are more than one call holds")

        def call(a, b, ws, nb, stream):
            return lib.xfh_retrieve_topk(_ptr(query[a:b]), _ptr(database[a:b]), _ptr(n_database[a:b]) if n_database is not None else None, b - a, Q, N, D,
                                         k, int(bool(exclude_self)), _ptr(idx[a:b]), _ptr(score[a:b]), ws, nb, stream)
        _scenes.run_scenes("xfh_retrieve_topk", G, lambda g: lib.xfh_retrieve_workspace_bytes(g, Q, N), dev, call)
    return {'idx': idx[0] if flat else idx, 'score': score[0] if flat else score}


def pairs_from_shortlists(idx, n_views=None):
    """``xfh_pairs_from_shortlists``: idx (S,V,k) int32 shortlists of the V <= 32 views -> 'view_pairs' (S,Pcap,2) int32 with a < b in ascending
    order, padded with (-1,-1), Pcap = min(V k, V (V - 1) / 2), and 'n_pairs' (S,) int32."""
    who = "pairs_from_shortlists"
    idx = torch.as_tensor(idx)
    if idx.dim() != 3:
        raise RuntimeError('expected idx (S,V,k)')
    S, V, k = idx.shape
    _scenes.views(who, V)
    k = _shortlist(who, k)
    if n_views is not None and torch.as_tensor(n_views).shape != (S,):
        raise RuntimeError('n_views must have one entry per scene')
    pcap = min(V * k, V * (V - 1) // 2)
    dev = idx.device if idx.is_cuda or S == 0 else _twoview.device(_WHAT)
    idx = idx.to(dev).to(torch.int32).contiguous()
    n_views = _scenes.n_views_arg(n_views, S, dev)
    out = {'view_pairs': torch.empty((S, pcap, 2), dtype=torch.int32, device=dev), 'n_pairs': torch.empty((S,), dtype=torch.int32, device=dev)}
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if S else None
    for a, b in _scenes.chunks(S):
        _lib.check(_lib.load().xfh_pairs_from_shortlists(_ptr(idx[a:b]), _ptr(n_views[a:b]) if n_views is not None else None, b - a, V, k,
                                                         _ptr(out['view_pairs'][a:b]), _ptr(out['n_pairs'][a:b]), stream), "xfh_pairs_from_shortlists")
    return out


def select_pairs(vlad, n_views=None, k=4):
    """The pairs of views worth matching, per scene: every view with the k views of the most similar global descriptor.

    vlad (S,V,D) float32 global descriptors of the V <= 32 views (``global_descriptors_batch`` reshaped), n_views (S,) or None = V.
    Returns a dict of CUDA tensors: 'view_pairs' (S,Pcap,2) int32 and 'n_pairs' (S,) int32 -- the undirected union of the shortlists as pairs
    a < b in ascending order, padded with (-1,-1), which ``relative_poses_graph_matches`` / ``reconstruct_graph_matches`` give weight 0 --
    and the shortlists themselves: 'neighbours' (S,V,k) int32, 'score' (S,V,k) float32 (``retrieve_topk`` with exclude_self).  Asynchronous."""
    who = "select_pairs"
    vlad = torch.as_tensor(vlad)
    if vlad.dim() != 3:
        raise RuntimeError('expected vlad (S,V,D)')
    S, V = vlad.shape[:2]
    _scenes.views(who, V)
    k = _shortlist(who, k)
    if n_views is not None and torch.as_tensor(n_views).shape != (S,):
        raise RuntimeError('n_views must have one entry per scene')
    top = retrieve_topk(vlad, vlad, k, n_views, exclude_self=True)
    out = pairs_from_shortlists(top['idx'], n_views)
    out.update(neighbours=top['idx'], score=top['score'])
    return out
