"""The top-k machinery of csrc/k_detect.hip compiled for the HOST (tests/emu/topk_emu.cpp) on the exact cases of the dense GPU test (tests/test_gpu_detect.py): cswap ..
bitonic_sort_lds, topk_sort_runs_kernel<1>, run_lower_bound and topk_rank_merge_kernel, sliced out of the product source.  Values in, permutation out: every run must be the
sorted keys of its 2048 candidates, and the key list of every k must be detect_reference.topk_order -- (value descending, index ascending) -- bit for bit.

The lane exchanges of the sort (DPP quad permutes, row_shl / row_shr:4, row_ror:8, the permlane16 / permlane32 swaps) are emu.hpp's restatements of the instructions; that
the hardware does what they assume is what the GPU test adds.  The merge logic -- ranks over LDS and global runs, five striding workgroups, both workgroup mappings --
is the product's own text."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import detect_reference as DR
import detect_support as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated_features_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LDS = "emu::wg->lds_base()"


def _must_sub(s, old, new):
    assert s.count(old) == 1, old
    return s.replace(old, new)


def _function(t, head):
    a = t.index(head)
    return t[a:t.index("\n}\n", a) + 3]


def slice_source(edit=None):
    """common.hpp's float_ord and xhalf_u32 + k_detect.hip from cswap to the end of topk_rank_merge_kernel; `edit` (text -> text) is applied to the k_detect.hip part first"""
    c = open(os.path.join(CSRC, "common.hpp")).read()
    t = open(os.path.join(CSRC, "k_detect.hip")).read()
    k = t[t.index("__device__ inline void cswap("):t.index("// keys/runs: (B, n_cap) u64 scratch.")]
    if edit:
        k = edit(k)
    k = _must_sub(k, "__shared__ __attribute__((aligned(16))) unsigned long long lk[TK_CH];", f"unsigned long long* lk = reinterpret_cast<unsigned long long*>({LDS});")
    k = _must_sub(k, "extern __shared__ __attribute__((aligned(16))) unsigned long long lr[];", f"unsigned long long* lr = reinterpret_cast<unsigned long long*>({LDS});")
    s = _function(c, "__device__ inline unsigned xhalf_u32(unsigned v) {") + _function(c, "__device__ inline unsigned float_ord(float f) {") + k
    s = s.replace("__global__ ", "inline ").replace("__device__ ", "")
    for name in ("bitonic_sort_lds", "topk_sort_runs_kernel", "run_lower_bound", "topk_rank_merge_kernel", "permlane16_swap", "permlane32_swap", "0x104", "0x114", "0x128"):
        assert name in s, name
    assert "asm" not in s and "__shared__" not in s and "<<<" not in s
    return s


def build_emu(edit=None):
    td = tempfile.mkdtemp()
    open(os.path.join(td, "topk_slice.hpp"), "w").write(slice_source(edit))
    out = os.path.join(td, "topk_emu")
    subprocess.run([CLANG, "-O1", "-w", "-std=c++20", "-pthread", "-I", td, "-I", EMU, os.path.join(EMU, "topk_emu.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu_bin():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    return build_emu()


def run_emu(emu_bin, vals, ks):
    """-> nsel (B,), runs (B, n) u64, {k: skeys (B, k) u64}"""
    B, n = vals.shape
    blob = np.array([B, n, len(ks)], np.int32).tobytes() + np.array(ks, np.int32).tobytes() + np.ascontiguousarray(vals, np.float32).tobytes()
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=900).stdout
    nsel = np.frombuffer(out[:4 * B], np.int32)
    o = 4 * B
    runs = np.frombuffer(out[o:o + 8 * B * n], np.uint64).reshape(B, n); o += 8 * B * n
    skeys = {}
    for k in ks:
        skeys[k] = np.frombuffer(out[o:o + 8 * B * k], np.uint64).reshape(B, k); o += 8 * B * k
    assert o == len(out)
    return nsel, runs, skeys


def check_case(emu_bin, cls, n, B):
    vals, ks = DS.dense_values(cls, n, B), DS.dense_ks(n)
    nsel, runs, skeys = run_emu(emu_bin, vals, ks)
    assert nsel.tolist() == [min(ks[0], n)] * B
    for b in range(B):
        keys = DS.dense_keys(vals[b])
        for q in range(0, n, 2048):
            assert np.array_equal(runs[b, q:q + 2048], np.sort(keys[q:q + 2048])), (cls, n, B, b, "run", q // 2048)
        order = DR.topk_order(vals[b], n)
        assert np.array_equal(keys[order], np.sort(keys))              # the keys restate the tie rule
        for k in ks:
            assert np.array_equal(skeys[k][b], keys[order[:k]]), (cls, n, B, b, k)


@pytest.mark.parametrize("n", DS.DENSE_N)
def test_topk_kernels_on_the_host(emu_bin, n):
    for B in (1, 9):
        for cls in DS.DENSE_CLASSES:
            check_case(emu_bin, cls, n, B)
