"""The buffer harness (tests/guarded.py) has teeth: on CPU tensors, against a fake entry written in Python, it fails for every kind of
fault it exists to find and passes for a correct entry.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded


class FakeError(RuntimeError):
    pass


def _floats(ptr, n, first=0):
    return np.ctypeslib.as_array((C.c_float * n).from_address(ptr + 4 * first))


def _bytes(ptr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr))


class FakeLib:
    """dst[i] = 2 src[i] through a scratch row in the workspace, count[0] = the rows written, counted in a workspace word.
    `bug` names the one thing it gets wrong."""

    def __init__(self, bug=None):
        self.bug = bug

    @staticmethod
    def xfh_fake_workspace_bytes(n):
        return 4 * n + 4

    def xfh_fake(self, src, n, dst, count, workspace, nbytes, stream):
        src, dst, count, workspace = (guarded._val(p) for p in (src, dst, count, workspace))
        need = self.xfh_fake_workspace_bytes(n)
        if nbytes < need:
            return guarded.XFH_ERR_WORKSPACE
        s, d, scratch = _floats(src, n), _floats(dst, n), _floats(workspace, n)
        counter = np.ctypeslib.as_array((C.c_int32 * 1).from_address(workspace + 4 * n))
        if self.bug != "no_reset":
            counter[0] = 0
        scratch[:] = 2 * s
        rows = n - 1 if self.bug == "unwritten" else n
        d[:rows] = scratch[:rows]
        counter[0] += n
        np.ctypeslib.as_array((C.c_int32 * 1).from_address(count))[0] = counter[0]
        if self.bug == "past":
            _floats(dst, 1, first=n)[0] = 1.0
        if self.bug == "before":
            _floats(dst, 1, first=-1)[0] = 1.0
        if self.bug == "ws_overrun":
            _bytes(workspace + need, 1)[0] = 0         # a constant that a constant guard fill could have hidden
        if self.bug == "input":
            s[0] = 0.0
        return guarded.XFH_OK


class FakeModule:
    """What the wrappers see as `_lib`: SIGNATURES and load()."""
    _p, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
    SIGNATURES = {"xfh_fake_workspace_bytes": (_sz, [_i]), "xfh_fake": (_i, [_p, _i, _p, _p, _p, _sz, _p])}

    def __init__(self, bug=None):
        self.lib = FakeLib(bug)

    def load(self):
        return self.lib


TABLE = {"xfh_fake": guarded.Entry(outputs=(2, 3), size_fn="xfh_fake_workspace_bytes", size_args=(1,))}


def wrapper(module, src):
    """The idiom of the package's wrappers: empty outputs, a workspace of the named size + 256."""
    lib = module.load()
    n = src.numel()
    dst = torch.empty((n,), dtype=torch.float32, device=src.device)
    count = torch.empty((1,), dtype=torch.int32, device=src.device)
    ws = torch.empty(lib.xfh_fake_workspace_bytes(n) + 256, dtype=torch.uint8, device=src.device)
    off = (-ws.data_ptr()) % 256
    rc = lib.xfh_fake(C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()), C.c_void_p(count.data_ptr()),
                      C.c_void_p(ws.data_ptr() + off), ws.numel() - off, None)
    if rc != guarded.XFH_OK:
        raise FakeError(rc)
    return dst, count


class Case:
    def __init__(self, module, seed, small):
        g = torch.Generator().manual_seed(seed)
        self.src = torch.rand(37 if small else 77, generator=g) + 1.0
        self.inputs = [self.src]
        self.module = module

    def call(self):
        return wrapper(self.module, self.src)


def problems_of(bug):
    module = FakeModule(bug)
    plain = bug not in ("past", "before")      # (without the guard bands those two would write into the host allocator's own words)
    return guarded.hold(lambda seed, small: Case(module, seed, small), module, TABLE, "cpu", "xfh_fake", error=FakeError, plain=plain)[0]


def test_a_correct_entry_passes():
    assert problems_of(None) == []


@pytest.mark.parametrize("bug,needle", [
    ("past", "stray write behind empty[77]"),
    ("before", "stray write before empty[77]"),
    ("ws_overrun", "stray write behind the workspace of xfh_fake"),
    ("unwritten", "stale-same against zero: output argument 2"),
    ("no_reset", "stale-same against zero: output argument 3"),
    ("input", "input 0 was written"),
])
def test_each_fault_is_found(bug, needle):
    found = problems_of(bug)
    assert any(needle in p for p in found), found


def test_offsets_are_relative_to_the_payload():
    found = problems_of("past")
    assert any("first at payload offset 308 (payload 308 bytes)" in p for p in found), found
    found = problems_of("before")
    assert any("first at payload offset -4 " in p for p in found), found
    found = problems_of("ws_overrun")
    assert any("first at payload offset 312 (payload 312 bytes)" in p for p in found), found


def test_the_slack_idiom_hides_the_overrun_the_harness_finds():
    module = FakeModule("ws_overrun")
    case = Case(module, 0, False)
    dst, count = case.call()                   # plain call: the byte lands in the wrapper's 256 spare bytes, nothing notices
    assert torch.equal(dst, 2 * case.src) and int(count) == 77


def test_the_short_workspace_is_refused_and_checked():
    module = FakeModule(None)
    assert guarded.hold_short(lambda seed, small: Case(module, seed, small), module, TABLE, "cpu", "xfh_fake", error=FakeError) == []

    class Lenient(FakeLib):                    # takes the short workspace: the harness has to say so
        def xfh_fake(self, src, n, dst, count, workspace, nbytes, stream):
            return FakeLib.xfh_fake(self, src, n, dst, count, workspace, nbytes + 1, stream)
    module.lib = Lenient()
    found = guarded.hold_short(lambda seed, small: Case(module, seed, small), module, TABLE, "cpu", "xfh_fake", error=FakeError)
    assert any("not XFH_ERR_WORKSPACE" in p for p in found) and any("wrote output argument 2 before refusing" in p for p in found), found


def test_guarded_layout():
    for n in (0, 1, 255, 4097, (1 << 20) + 3):
        g = guarded.Guarded(n, "cpu")
        band = max(4096, min(n, 1 << 20))
        assert g.ptr % 256 == 0 and g.lo >= band and g.block.numel() - g.hi >= band and g.payload.numel() == n
        i = torch.arange(g.lo)
        assert torch.equal(g.block[:g.lo], ((131 * i + 7) & 255).to(torch.uint8))
        g.check()
        g.payload.fill_(255)
        g.check()
        g.block[g.hi] = g.block[g.hi] ^ 1
        with pytest.raises(guarded.GuardError, match=f"payload offset {n} "):
            g.check()


def test_nothing_stays_patched():
    before = (torch.empty, torch.zeros, torch.full, torch.empty_like)
    with guarded.Session("cpu") as s:
        a = torch.empty(3, 5)
        b = torch.zeros((2, 2), dtype=torch.int32)
        c = torch.full((4,), 7.0)
        d = torch.empty_like(b)
        assert torch.empty is not before[0]
    assert (torch.empty, torch.zeros, torch.full, torch.empty_like) == before
    assert len(s.allocs) == 4 and a.shape == (3, 5) and not b.any() and bool((c == 7).all()) and d.dtype == torch.int32
    assert all(s.find(t.data_ptr()) is not None for t in (a, b, c, d))
    with pytest.raises(ZeroDivisionError):
        with guarded.Session("cpu"):
            1 / 0
    assert (torch.empty, torch.zeros, torch.full, torch.empty_like) == before


def test_every_entry_is_driven_or_exempt():
    """driven + exempt + the size functions = the signature table: a new entry cannot skip the harness silently."""
    import test_gpu_buffers
    from accelerated_features_amd import _lib
    assert guarded.census(_lib.SIGNATURES) == ([], [])
    assert not set(guarded.TABLE) & set(guarded.EXEMPT)
    assert {entry for entry, _ in test_gpu_buffers.CASES.values()} == set(guarded.TABLE)
    for name, e in guarded.TABLE.items():
        argtypes = _lib.SIGNATURES[name][1]
        assert all(argtypes[i] is C.c_void_p for i in e.outputs), name
        assert (e.size_fn is not None) == guarded.Proxy.has_workspace(argtypes), name      # every (void* workspace, size_t bytes) pair has its size function
        if e.size_fn is not None:
            assert len(_lib.SIGNATURES[e.size_fn][1]) == len(e.size_args) and max(e.outputs) < len(argtypes) - 3, name
    for name in guarded.EXEMPT:
        assert guarded.EXEMPT[name]
