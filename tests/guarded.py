"""Guard bands, stale prefills and an exact-size workspace for every entry of the C ABI.

The library promises (include/xfeat_hip.h, Conventions) that it needs `xfh_*_workspace_bytes()` bytes and nothing more, that workspace and
outputs need no initialisation, and that it writes nothing outside them.  This module is the harness that holds an entry to that:

  Guarded   one uint8 block: [guard band | payload, 256-byte aligned | guard band], the bands filled with a position-dependent pattern.
  Session   a context manager.  Inside the `with` block the device allocations the Python wrappers make (torch.empty / zeros / full /
            empty_like) come from Guarded blocks, `empty` payloads prefilled with zeros or with what an earlier Session left in the same
            allocation; nothing is patched outside the block.
  Proxy     stands in for the object `_lib.load()` returns.  An entry with the (void* workspace, size_t bytes) pair gets a Guarded workspace
            of exactly the size the header names for it (TABLE: entry -> size function and its arguments), passed without slack; every
            output pointer of a driven entry must lie in a Guarded payload; every call is recorded.
  drive     one wrapper call under Session + Proxy -> a Result (return codes, the bytes of every output block, the wrapper's return values).
  hold      the whole contract for one case: three modes, the plain call, the inputs, the short workspace.

Device-agnostic: tests/test_guarded_harness.py runs it on CPU tensors against a fake entry written in Python.
"""
import ctypes as C

import torch

XFH_OK = 0
XFH_ERR_WORKSPACE = -3
MODES = ("zero", "stale-same", "stale-other")

_real = {name: getattr(torch, name) for name in ("empty", "zeros", "full", "empty_like")}
_patterns = {}


class GuardError(AssertionError):
    pass


def band_bytes(payload_bytes):
    return max(4096, min(int(payload_bytes), 1 << 20))


def _pattern(n, device):
    """The first n bytes of (131 i + 7) & 255 on `device`."""
    have = _patterns.get(device)
    if have is None or have.numel() < n:
        i = torch.arange(max(n, 1 << 16), dtype=torch.int64, device=device)
        have = ((131 * i + 7) & 255).to(torch.uint8)
        _patterns[device] = have
    return have[:n]


class Guarded:
    """`nbytes` of payload between two guard bands."""

    def __init__(self, nbytes, device, what=""):
        self.nbytes, self.what = int(nbytes), what
        self.device = torch.device(device)
        band = band_bytes(self.nbytes)
        self.block = _real["empty"](band + 256 + self.nbytes + band, dtype=torch.uint8, device=self.device)
        self.lo = band + (-(self.block.data_ptr() + band)) % 256          # payload offset: 256-byte aligned
        self.hi = self.lo + self.nbytes
        self.block[:self.lo] = _pattern(self.lo, self.device)
        self.block[self.hi:] = _pattern(self.block.numel() - self.hi, self.device)
        self.payload = self.block[self.lo:self.hi]
        self.payload.zero_()
        self.ptr = self.block.data_ptr() + self.lo

    def prefill(self, leftover, ones=False):
        if self.nbytes:
            self.payload.copy_(expected_prefill(self.nbytes, leftover, ones))

    def view(self, dtype, shape):
        return self.payload.view(dtype).view(shape)

    def contains(self, ptr):
        return self.nbytes > 0 and self.ptr <= ptr < self.ptr + self.nbytes

    def bytes(self):
        return self.payload.detach().cpu().clone()

    def check(self):
        """Raises GuardError naming the first differing offset relative to the payload (negative: before it)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        lo, hi = self.block[:self.lo], self.block[self.hi:]
        bad = (lo != _pattern(self.lo, self.device)).nonzero()
        if bad.numel():
            raise GuardError(f"stray write before {self.what}: first at payload offset {int(bad[0]) - self.lo} (payload {self.nbytes} bytes)")
        bad = (hi != _pattern(hi.numel(), self.device)).nonzero()
        if bad.numel():
            raise GuardError(f"stray write behind {self.what}: first at payload offset {self.nbytes + int(bad[0])} (payload {self.nbytes} bytes)")


def expected_prefill(nbytes, leftover=None, ones=False):
    """What a payload holds before the call (a CPU uint8 tensor): zeros -- or, with `ones`, the bytes 01 00 00 00 repeating, so that every
    32-bit word reads as 1 and every byte as 0 or 1: small defined values that are in range wherever a word could be taken for a count --
    with `leftover` (what an earlier call left in the same buffer; None: nothing) over the front part."""
    want = _real["zeros"](nbytes, dtype=torch.uint8)
    if ones:
        want[0::4] = 1
    if leftover is not None and leftover.numel() and nbytes:
        n = min(leftover.numel(), nbytes)
        want[:n] = leftover[:n].cpu()
    return want


def leftover_of(prior, k, meta):
    """What the k-th `empty` allocation of the earlier Session `prior` held at its end -- if that was a tensor of the same type and rank
    (the same buffer of the same wrapper); None otherwise."""
    if prior is None or k >= len(prior.empties) or prior.empties[k][0] != meta:
        return None
    return prior.empties[k][1]


def _nbytes(shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return n * _real["empty"]((), dtype=dtype).element_size()


def _shape(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = size[0]
    return tuple(int(s) for s in size)


class Session:
    """Guarded allocations on `device` while the `with` block runs.  `prior`: the Result of an earlier Session whose leftovers prefill the
    n-th `empty` allocation (front part) -- behind it, and everywhere without a prior, zeros or (ones=True) expected_prefill's small words."""

    def __init__(self, device, prior=None, ones=False):
        self.device = torch.device(device)
        self.prior, self.ones = prior, ones
        self.allocs = []                       # every Guarded handed out, in order
        self.empties = []                      # those that came from empty / empty_like, in order

    def _mine(self, device):
        if device is None:
            return self.device.type == "cpu"   # torch's default device
        d = torch.device(device)
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    def _new(self, shape, dtype, kind):
        dtype = dtype or torch.get_default_dtype()
        g = Guarded(_nbytes(shape, dtype), self.device, f"{kind}{list(shape)} (allocation {len(self.allocs)})")
        self.allocs.append(g)
        if kind == "empty":
            g.meta = (dtype, len(shape))
            g.prefill(leftover_of(self.prior, len(self.empties), g.meta), self.ones)
            self.empties.append(g)
        return g, g.view(dtype, shape)

    def _empty(self, *size, dtype=None, device=None, **kw):
        if kw or not self._mine(device):
            return _real["empty"](*size, dtype=dtype, device=device, **kw)
        return self._new(_shape(size), dtype, "empty")[1]

    def _zeros(self, *size, dtype=None, device=None, **kw):
        if kw or not self._mine(device):
            return _real["zeros"](*size, dtype=dtype, device=device, **kw)
        return self._new(_shape(size), dtype, "zeros")[1]

    def _full(self, size, fill_value, dtype=None, device=None, **kw):
        if kw or not self._mine(device):
            return _real["full"](size, fill_value, dtype=dtype, device=device, **kw)
        if dtype is None:
            dtype = _real["full"]((), fill_value).dtype
        t = self._new(_shape((size,)), dtype, "full")[1]
        t.fill_(fill_value)
        return t

    def _empty_like(self, x, dtype=None, device=None, **kw):
        if kw or not self._mine(device if device is not None else x.device) or not x.is_contiguous():
            return _real["empty_like"](x, dtype=dtype, device=device, **kw)
        return self._new(tuple(x.shape), dtype or x.dtype, "empty")[1]

    def __enter__(self):
        torch.empty, torch.zeros, torch.full, torch.empty_like = self._empty, self._zeros, self._full, self._empty_like
        return self

    def __exit__(self, *exc):
        for name, fn in _real.items():
            setattr(torch, name, fn)
        return False

    def find(self, ptr):
        for g in self.allocs:
            if g.contains(ptr):
                return g
        return None


class Entry:
    """outputs: positions of the pointer arguments the entry writes through.  size_fn / size_args: the header's size function for the
    entry's workspace and the positions of the call's own arguments it takes (an int stands for args[i], a tuple ('const', v) for v)."""

    def __init__(self, outputs, size_fn=None, size_args=()):
        self.outputs, self.size_fn, self.size_args = tuple(outputs), size_fn, tuple(size_args)


def _val(a):
    return a.value if isinstance(a, C.c_void_p) else a


class Call:
    def __init__(self, name, args):
        self.name, self.args, self.rc, self.workspace, self.need, self.outputs = name, args, None, None, None, {}


class Proxy:
    """What `_lib.load()` returns while a case is driven."""

    def __init__(self, real, table, signatures, session, prior=None, short_entry=None):
        self._real, self._table, self._signatures, self._session = real, table, signatures, session
        self._prior, self._short_entry = prior, short_entry
        self.calls = []
        self.problems = []

    @staticmethod
    def has_workspace(argtypes):
        return len(argtypes) >= 3 and argtypes[-3] is C.c_void_p and argtypes[-2] is C.c_size_t

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        entry = self._table.get(name)
        if entry is None:
            return fn

        def call(*args):
            args = list(args)
            rec = Call(name, args)
            nth = sum(1 for c in self.calls if c.name == name)
            if entry.size_fn is not None:
                assert self.has_workspace(self._signatures[name][1]), f"{name}: no workspace pair in its signature"
                sz = [a[1] if isinstance(a, tuple) else _val(args[a]) for a in entry.size_args]
                rec.need = int(getattr(self._real, entry.size_fn)(*sz))
                rec.workspace = Guarded(rec.need, self._session.device, f"the workspace of {name} ({rec.need} bytes)")
                rec.workspace.prefill(self._prior.workspaces.get((name, nth)) if self._prior is not None else None)
                short = self._short_entry == name and rec.need > 0
                args[-3] = C.c_void_p(rec.workspace.ptr)
                args[-2] = rec.need - 1 if short else rec.need
            for i in entry.outputs:
                p = _val(args[i])
                if p:
                    g = self._session.find(p)
                    if g is None:
                        self.problems.append(f"{name}: output argument {i} is not in a guarded allocation")
                    rec.outputs[i] = g
            self.calls.append(rec)
            rec.rc = fn(*args)
            return rec.rc
        return call


class Result:
    pass


def flatten(x, out=None):
    """The tensors (and plain values) of a wrapper's return value, in a fixed order."""
    out = [] if out is None else out
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            flatten(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            flatten(v, out)
    elif torch.is_tensor(x):
        out.append(x.detach().cpu().contiguous().clone())
    elif type(x).__module__ == "numpy" and hasattr(x, "tobytes"):
        out.append((str(getattr(x, "dtype", "")), getattr(x, "shape", ()), x.tobytes()))
    else:
        out.append(x)
    return out


def raw(t):
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1).to(torch.uint8)


def same_bytes(a, b):
    if torch.is_tensor(a) and torch.is_tensor(b):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))
    if torch.is_tensor(a) or torch.is_tensor(b):
        return False
    return a == b or (a != a and b != b)


def drive(case, lib_module, table, device, prior=None, short_entry=None, error=Exception, ones=False):
    """One call of case.call() under a Session and a Proxy (lib_module.load is replaced for the duration and put back).  -> Result."""
    session = Session(device, prior, ones)
    real_load = lib_module.load
    proxy = Proxy(real_load(), table, lib_module.SIGNATURES, session, prior, short_entry)
    inputs = list(case.inputs)
    before = [t.detach().clone() for t in inputs]
    res = Result()
    res.raised = None
    lib_module.load = lambda: proxy
    try:
        with session:
            try:
                res.returns = flatten(case.call())
            except error as e:                 # the wrapper's own error for a return code: expected with a short workspace only
                res.raised, res.returns = e, []
    finally:
        lib_module.load = real_load
    if device is not None and torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    res.calls = proxy.calls
    res.problems = list(proxy.problems)
    for g in session.allocs:
        try:
            g.check()
        except GuardError as e:
            res.problems.append(str(e))
    for c in proxy.calls:
        if c.workspace is not None:
            try:
                c.workspace.check()
            except GuardError as e:
                res.problems.append(str(e))
    for i, (t, b) in enumerate(zip(inputs, before)):
        if not same_bytes(t.detach().cpu(), b.cpu()):
            res.problems.append(f"input {i} was written")
    res.empties = [(g.meta, g.bytes()) for g in session.empties]
    res.workspaces, res.outputs, seen = {}, {}, {}
    for c in proxy.calls:
        nth = seen.get(c.name, 0)
        seen[c.name] = nth + 1
        if c.workspace is not None:
            res.workspaces[(c.name, nth)] = c.workspace.bytes()
        for i, g in c.outputs.items():
            if g is not None:
                res.outputs[(c.name, nth, i)] = g.bytes()
    res.session = session
    return res


def first_difference(a, b):
    if a.numel() != b.numel():
        return f"sizes {a.numel()} and {b.numel()}"
    d = (a != b).nonzero()
    return None if not d.numel() else f"{d.numel()} of {a.numel()} bytes, first at byte {int(d[0])}"


def compare_outputs(a, b, what, specified=None):
    """The output blocks of two Results, byte for byte.  specified(name, arg, call, nbytes) -> a bool byte mask (or None: everything) of the part
    of that output the header specifies."""
    problems = []
    if sorted(a.outputs) != sorted(b.outputs):
        return [f"{what}: the calls differ: {sorted(a.outputs)} / {sorted(b.outputs)}"]
    calls = {}
    seen = {}
    for c in a.calls:
        calls[(c.name, seen.get(c.name, 0))] = c
        seen[c.name] = seen.get(c.name, 0) + 1
    for key in sorted(a.outputs):
        x, y = a.outputs[key], b.outputs[key]
        if x.numel() == y.numel() and specified is not None:
            m = specified(key[0], key[2], calls[key[:2]], x.numel())
            if m is not None:
                x, y = x[m], y[m]
        d = first_difference(x, y)
        if d:
            problems.append(f"{what}: output argument {key[2]} of {key[0]} (call {key[1]}) differs: {d}")
    return problems


def hold(make, lib_module, table, device, entry, specified=None, error=Exception, plain=True):
    """The contract of section 2 for one case.  make(seed, small) -> a case (inputs, call()); seed 0 at the full shape is the case under test,
    seed 1 its stale-same predecessor, small=True its stale-other predecessor (every dimension smaller or equal).  Returns the list of
    problems (empty: the entry holds) and the Results by mode."""
    problems, results = [], {}
    want = flatten(make(0, False).call()) if plain else None       # first: whatever the wrappers cache (handles, workspaces) exists before a Session
    for mode in MODES:
        prior = None
        if mode != "zero":
            prior = drive(make(1, mode == "stale-other"), lib_module, table, device, ones=True)
            problems += [f"predecessor of {mode}: {p}" for p in prior.problems]
        r = drive(make(0, False), lib_module, table, device, prior, ones=mode != "zero")
        results[mode] = r
        problems += [f"{mode}: {p}" for p in r.problems]
        if r.raised is not None:
            problems.append(f"{mode}: the call raised {r.raised!r}")
        problems += [f"{mode}: {c.name} returned {c.rc}" for c in r.calls if c.rc != XFH_OK]
        if not any(c.name == entry for c in r.calls):
            problems.append(f"{mode}: {entry} was not called")
    zero = results["zero"]
    for mode in MODES[1:]:
        problems += compare_outputs(zero, results[mode], f"{mode} against zero", specified)
        if len(zero.returns) != len(results[mode].returns) or not all(same_bytes(a, b) for a, b in zip(zero.returns, results[mode].returns)):
            problems.append(f"{mode} against zero: the wrapper's return values differ")
    if plain:
        if len(want) != len(zero.returns) or not all(same_bytes(a, b) for a, b in zip(want, zero.returns)):
            bad = [i for i, (a, b) in enumerate(zip(want, zero.returns)) if not same_bytes(a, b)]
            problems.append(f"the guarded call and the plain call return different values (items {bad} of {len(want)})")
    if table[entry].size_fn is not None:
        problems += hold_short(make, lib_module, table, device, entry, error)
    return problems, results


def hold_short(make, lib_module, table, device, entry, error=Exception):
    """The same call with a workspace one byte short: XFH_ERR_WORKSPACE, and every payload keeps its prefill."""
    problems = []
    prior = drive(make(1, False), lib_module, table, device, ones=True)
    r = drive(make(0, False), lib_module, table, device, prior, short_entry=entry, error=error, ones=True)
    problems += [f"short workspace: {p}" for p in r.problems]
    mine = [c for c in r.calls if c.name == entry]
    if not mine:
        return problems + [f"short workspace: {entry} was not called"]
    c = mine[0]
    if c.need == 0:
        return problems                        # nothing to be short of
    if c.rc != XFH_ERR_WORKSPACE:
        problems.append(f"short workspace: {entry} returned {c.rc}, not XFH_ERR_WORKSPACE")
    if not torch.equal(c.workspace.bytes(), expected_prefill(c.need, prior.workspaces.get((entry, 0)))):
        problems.append(f"short workspace: {entry} wrote its workspace before refusing")
    for i, g in c.outputs.items():
        if g is None:
            continue
        k = r.session.empties.index(g) if g in r.session.empties else None
        if k is None:
            continue                           # zeros / full: wrapper-defined values, compared below through the guards only
        if not torch.equal(g.bytes(), expected_prefill(g.nbytes, leftover_of(prior, k, g.meta), True)):
            problems.append(f"short workspace: {entry} wrote output argument {i} before refusing")
    return problems


# ---------------------------------------------------------------------------------------------------------------------------------------
# The C ABI (include/xfeat_hip.h): for every entry that writes device memory, the positions of its output pointers and the size function
# the header names for its workspace with the positions of the call's own arguments that function takes.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _one(v=1):
    return ("const", v)


def _ransac(outputs, size_fn, P, iters):
    return Entry(outputs, size_fn, (P, iters))


TABLE = {
    "xfh_resize_bilinear": Entry((4,)),
    "xfh_backbone": Entry(range(6, 11), "xfh_backbone_workspace_bytes", (2, 3, 4, 5)),
    "xfh_backbone_u8": Entry(range(8, 13), "xfh_backbone_workspace_bytes", (4, 5, 6, 7)),
    "xfh_backbone_resized": Entry(range(14, 19), "xfh_backbone_workspace_bytes", (2, 3, 10, 11)),
    "xfh_conv_layer": Entry((6,)),
    "xfh_detect_sparse": Entry(range(13, 19), "xfh_detect_workspace_bytes", (5, 6, 7, 9, 10)),
    "xfh_extract_dense": Entry(range(10, 13), "xfh_dense_workspace_bytes", (3, 4, 5, 6)),
    "xfh_match_mnn": Entry((15, 16, 17), "xfh_match_workspace_bytes", (11, 12, 13)),
    "xfh_match_mnn_guided": Entry((19, 20, 21), "xfh_match_guided_workspace_bytes", (12, 13, 14)),
    "xfh_refine_matches": Entry((12, 13), "xfh_refine_workspace_bytes", (9, 10)),
    "xfh_kpts_heatmap": Entry((4,)),
    "xfh_nms": Entry((8, 9), "xfh_detect_workspace_bytes", (2, 3, 4, _one(), 7)),           # header: xfh_detect_workspace_bytes(B,H,W,1,capacity)
    "xfh_sample_sparse": Entry((10,)),
    "xfh_fine_matcher": Entry((3,), "xfh_refine_workspace_bytes", (_one(), 2)),             # header: xfh_refine_workspace_bytes(1, n)
    "xfh_find_homography": _ransac((10, 11, 12), "xfh_homography_workspace_bytes", 4, 7),
    "xfh_find_homography_matches": _ransac((12, 13, 14), "xfh_homography_workspace_bytes", 6, 9),
    "xfh_homography_tables": Entry((1, 2)),
    "xfh_estimate_relpose": _ransac(range(13, 18), "xfh_relpose_workspace_bytes", 4, 10),
    "xfh_estimate_relpose_matches": _ransac(range(15, 20), "xfh_relpose_workspace_bytes", 6, 12),
    "xfh_estimate_relpose_sweep": Entry(range(14, 19), "xfh_relpose_sweep_workspace_bytes", (4, 11, 9)),
    "xfh_estimate_relpose_sweep_matches": Entry(range(16, 21), "xfh_relpose_sweep_workspace_bytes", (6, 13, 11)),
    "xfh_estimate_abspose": _ransac(range(12, 16), "xfh_abspose_workspace_bytes", 4, 9),
    "xfh_estimate_abspose_matches": _ransac(range(15, 19), "xfh_abspose_workspace_bytes", 7, 12),
    "xfh_estimate_alignment": _ransac(range(12, 17), "xfh_align_workspace_bytes", 4, 9),
    "xfh_estimate_alignment_matches": _ransac(range(15, 20), "xfh_align_workspace_bytes", 7, 12),
    "xfh_find_fundamental": _ransac((11, 12, 13), "xfh_fundamental_workspace_bytes", 4, 8),
    "xfh_find_fundamental_matches": _ransac((13, 14, 15), "xfh_fundamental_workspace_bytes", 6, 10),
    "xfh_triangulate": Entry(range(14, 18)),
    "xfh_triangulate_matches": Entry(range(16, 21)),
    "xfh_recover_pose": Entry(range(11, 17)),
    "xfh_recover_pose_matches": Entry(range(13, 19)),
    "xfh_build_tracks": Entry((8,)),
    "xfh_triangulate_views": Entry(range(14, 20)),
    "xfh_triangulate_tracks": Entry(range(14, 20)),
    "xfh_build_tracks_graph": Entry(range(11, 15), "xfh_track_graph_workspace_bytes", (4, 7, 8)),
    "xfh_bundle_adjust": Entry(range(15, 22), "xfh_bundle_workspace_bytes", (6, 7, 8)),
    "xfh_average_poses": Entry(range(13, 18), "xfh_pose_graph_workspace_bytes", (5, 6, 7)),
    "xfh_baseline_ratios": Entry(range(18, 22), "xfh_baseline_ratios_workspace_bytes", (9, 10, 11, 12)),
    "xfh_average_poses_ratios": Entry(range(17, 23), "xfh_pose_graph_ratios_workspace_bytes", (7, 8, 9)),
    "xfh_build_map": Entry(range(11, 19), "xfh_map_workspace_bytes", (6, 7, 8)),
    "xfh_map_project": Entry((10,)),
    "xfh_filter_matches": Entry(range(8, 13)),
    "xfh_verify_matches": Entry((15, 16, 17)),
    "xfh_vlad": Entry(range(6, 10), "xfh_vlad_workspace_bytes", (2, 3, 5)),
    "xfh_kmeans_step": Entry(range(6, 11), "xfh_kmeans_workspace_bytes", (2, 3, 5)),
    "xfh_retrieve_topk": Entry((9, 10), "xfh_retrieve_workspace_bytes", (3, 4, 5)),
    "xfh_pairs_from_shortlists": Entry((5, 6)),
    "xfh_lg_match": Entry((13, 14, 15), "xfh_lg_workspace_bytes", (3, 8)),
    "xfh_lg_match_pairs": Entry((10, 11, 12), "xfh_lg_workspace_bytes", (5, 5)),
}

# Entries the harness does not drive, each with its reason.
EXEMPT = {
    "xfh_version": "writes no device memory",
    "xfh_last_error": "the calling thread's error string: host memory",
    "xfh_num_weight_arrays": "a constant", "xfh_weight_array_floats": "a constant",
    "xfh_lg_num_weight_arrays": "a constant", "xfh_lg_weight_array_floats": "a constant",
    "xfh_create": "create: allocates its own device memory (the one place the header allows it)",
    "xfh_destroy": "destroy",
    "xfh_lg_create": "create: allocates its own device memory",
    "xfh_lg_destroy": "destroy",
    "xfh_set_option": "options: host state of the handle", "xfh_get_option": "options: writes a host int",
    "xfh_set_status_buffer": "status buffer: stores a pointer; the word is OR-ed into, never initialised, by contract the caller's to zero",
    "xfh_profile_select": "profile hook", "xfh_profile_read": "profile hook: host outputs", "xfh_profile_read_spans": "profile hook: host outputs",
    "xfh_lg_profile": "profile hook", "xfh_lg_profile_read": "profile hook: host outputs",
    "xfh_debug_trace": "debug hook", "xfh_debug_match_occupancy": "debug hook", "xfh_debug_cold_start": "debug hook",
    "xfh_debug_block1": "debug hook (a thin launcher of the kernel xfh_backbone runs, which is driven)",
}


def census(signatures):
    """(entries neither driven nor exempt nor size functions, names in the tables that the signature table does not have)."""
    sizes = {n for n in signatures if n.endswith("_workspace_bytes")}
    known = set(TABLE) | set(EXEMPT) | sizes
    return sorted(set(signatures) - known), sorted(known - set(signatures))
