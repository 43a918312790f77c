"""xfh_match_mnn_guided on the HOST: guided_prep_kernel, mnn_guided_kernel<KIND> (csrc/k_match_guided.hip) and the shared finalize
(csrc/k_match.hip), sliced out of the product sources and run through tests/emu/emu.hpp (tests/emu/guided_match_emu.cpp), against the
float64 checker of tests/guided_reference.py: tile layouts, the clamped padding lanes, the key layout, empty rows and columns, invalid
models."""
import os
import re
import subprocess

import numpy as np
import pytest

import guided_reference as GR
import twoview_support as TS

KIND_ID = {'fundamental': 0, 'homography': 1}


def _sub(s, old, new):
    assert s.count(old) == 1, old
    return s.replace(old, new)


def _slices():
    t = open(os.path.join(TS.CSRC, "k_match_guided.hip")).read()
    a = t.index("// ---- guided kernels begin")
    g = t[a:t.index("// ---- guided kernels end", a)]
    lds = "emu::wg->lds_base()"
    g = _sub(g, "__shared__ __attribute__((aligned(16))) float Dl[GM_COLS * GM_DS];", f"float* Dl = reinterpret_cast<float*>({lds});")
    g = _sub(g, "__shared__ unsigned long long colbest[8][GM_COLS];",
             f"unsigned long long (*colbest)[GM_COLS] = reinterpret_cast<unsigned long long (*)[GM_COLS]>({lds} + 4 * GM_COLS * GM_DS);")
    g = _sub(g, "__shared__ __attribute__((aligned(16))) float4 Rl[GM_ROWS];", f"float4* Rl = reinterpret_cast<float4*>({lds} + 4 * GM_COLS * GM_DS + 64 * GM_COLS);")
    g = _sub(g, "__shared__ __attribute__((aligned(16))) float4 Cl[GM_COLS];",
             f"float4* Cl = reinterpret_cast<float4*>({lds} + 4 * GM_COLS * GM_DS + 64 * GM_COLS + 16 * GM_ROWS);")
    m = open(os.path.join(TS.CSRC, "k_match.hip")).read()
    a = m.index("__device__ inline int pair_count(")
    f = m[a:m.index("// 512 threads = 8 waves", a)]
    a = m.index("__device__ inline bool mutual_keep(")
    f += m[a:m.index("int match_debug_occupancy()", a)]
    f = _sub(f, "__shared__ int wsum[16];", f"int* wsum = reinterpret_cast<int*>({lds});")
    f = _sub(f, "__shared__ int s_before;", f"int& s_before = *reinterpret_cast<int*>({lds} + 64);")
    f = re.sub(r"__global__ __launch_bounds__\(1024\) void mnn_finalize_kernel\(", "inline void mnn_finalize_kernel(", f)
    for s in (g, f):
        assert "__shared__" not in s and "<<<" not in s and "asm" not in s
    assert "mnn_finalize_kernel" in f and "0x007fffffu" in f and "mnn_guided_kernel" in g and "guided_prep_kernel" in g
    return g, f


@pytest.fixture(scope="module")
def emu_bin():
    import tempfile
    if not os.path.exists(TS.CLANG):
        pytest.skip("no host clang")
    g, f = _slices()
    td = tempfile.mkdtemp()
    open(os.path.join(td, "guided_slice.hpp"), "w").write(g)
    open(os.path.join(td, "finalize_slice.hpp"), "w").write(f)
    out = os.path.join(td, "guided_match_emu")
    subprocess.run([TS.CLANG, "-O2", "-w", "-std=c++20", "-pthread", "-ffp-contract=off", "-I", td, "-I", TS.EMU, os.path.join(TS.EMU, "guided_match_emu.cpp"), "-o", out],
                   check=True)
    return out


def run_emu(emu_bin, kind, d1, d2, k1, k2, models, thr, min_cossim=-1.0, counts=None, n_stride=1, n_off2=0):
    """d1 (P,N1,64), d2 (P,N2,64), k1 (P,N1,2), k2 (P,N2,2), models (P,3,3): list of (idx0, idx1) per pair."""
    P, N1, N2 = d1.shape[0], d1.shape[1], d2.shape[1]
    counts = np.zeros(0, np.int32) if counts is None else np.asarray(counts, np.int32)
    blob = (np.array([KIND_ID[kind], P, N1, N2, n_stride, n_off2], np.int32).tobytes() + np.array([thr, min_cossim], np.float64).tobytes()
            + np.int32(len(counts)).tobytes() + counts.tobytes()
            + b"".join(np.ascontiguousarray(v, np.float32).tobytes() for v in (d1, d2, k1, k2)) + np.ascontiguousarray(models, np.float64).tobytes())
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=900).stdout
    nm = np.frombuffer(out[:4 * P], np.int32)
    i0 = np.frombuffer(out[4 * P:4 * P + 8 * P * N1], np.int64).reshape(P, N1)
    i1 = np.frombuffer(out[4 * P + 8 * P * N1:], np.int64).reshape(P, N1)
    return [(i0[p, :nm[p]], i1[p, :nm[p]]) for p in range(P)]


def _one(emu_bin, s, thr, model=None, min_cossim=-1.0):
    model = s['model'] if model is None else model
    return run_emu(emu_bin, s['kind'], s['d1'][None], s['d2'][None], s['k1'][None], s['k2'][None], np.asarray(model, np.float64).reshape(1, 3, 3), thr, min_cossim)[0]


@pytest.mark.parametrize("kind", GR.KINDS)
@pytest.mark.parametrize("n1,n2,thr", [(1, 1, 3.0), (31, 33, 3.0), (257, 129, 1.0), (300, 1025, 3.0)])
def test_guided_kernels_on_the_host(emu_bin, kind, n1, n2, thr):
    s = GR.scene(kind, n1, n2, 100 + n1)
    i0, i1 = _one(emu_bin, s, thr)
    must, und = GR.check_guided_mnn_fp64(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, thr, i0, i1)
    print(f"{kind} {n1} x {n2}: {len(i0)} matches, {must} strict, {und} undecided elements, true {GR.true_matches(s, i0, i1)} of {len(s['truth'])}")
    assert must >= min(1, len(s['truth'])) and len(i0) >= must
    if und == 0:
        w0, w1 = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, thr)
        assert len(i0) >= 0.98 * len(w0)


@pytest.mark.parametrize("kind", GR.KINDS)
def test_ragged_counts_and_min_cossim_on_the_host(emu_bin, kind):
    """P = 2 in one buffer with counts through n_stride 2 / n_offset2 1: pair 0 uses (40, 70) of (96, 80), pair 1 is empty on one side; rows and columns past the
    counts hold descriptors that would win and key-points that pass."""
    N1, N2 = 96, 80
    s = GR.scene(kind, N1, N2, 77)
    d1, d2, k1, k2 = (np.stack([s[k], s[k]]) for k in ('d1', 'd2', 'k1', 'k2'))
    counts = [40, 70, 0, 50]
    got = run_emu(emu_bin, kind, d1, d2, k1, k2, np.stack([s['model']] * 2), 3.0, 0.5, counts, 2, 1)
    assert len(got[1][0]) == 0
    i0, i1 = got[0]
    must, _ = GR.check_guided_mnn_fp64(s['d1'][:40], s['d2'][:70], s['k1'][:40], s['k2'][:70], s['model'], kind, 3.0, i0, i1, 0.5)
    assert must > 5


@pytest.mark.parametrize("kind", GR.KINDS)
def test_empty_row_0_and_empty_column_0_are_no_match(emu_bin, kind):
    """Row 0 and column 0 moved far off every gate: both keep -inf keys whose arg-max is index 0, which must not come out as the match (0, 0) with the
    similarity cut disabled -- although their descriptors are each other's best."""
    s = GR.scene(kind, 31, 33, 131)
    s['k1'][0] = (-5.0e4, 7.0e4)
    s['k2'][0] = (9.0e4, -6.0e4)
    s['d2'][0] = s['d1'][0]
    passes, _ = GR.gate(s['k1'], s['k2'], s['model'], kind, 3.0)
    assert not passes[0].any() and not passes[:, 0].any()
    i0, i1 = _one(emu_bin, s, 3.0, min_cossim=-1.0)
    assert 0 not in i0.tolist() and 0 not in i1.tolist() and len(i0) > 5
    GR.check_guided_mnn_fp64(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, 3.0, i0, i1)


@pytest.mark.parametrize("kind", GR.KINDS)
def test_duplicates_inside_the_gate_go_to_the_lowest_index(emu_bin, kind):
    """Columns a < b with one descriptor at one place (both inside row r's gate): row r takes a.  Rows r < r2 with one descriptor at one place: column a takes r."""
    s = GR.scene(kind, 70, 45, 99)
    r = int(np.argmin(s['truth'][:20]))
    a = int(s['truth'][r])
    b = 44 if a != 44 else 43
    assert a < b
    s['d2'][b], s['k2'][b] = s['d2'][a], s['k2'][a]
    r2 = 69
    s['d1'][r2], s['k1'][r2] = s['d1'][r], s['k1'][r]
    i0, i1 = _one(emu_bin, s, 3.0)
    got = dict(zip(i0.tolist(), i1.tolist()))
    assert got.get(r) == a and r2 not in got and b not in i1.tolist()


@pytest.mark.parametrize("kind", GR.KINDS)
def test_padding_lanes_take_the_constants_of_the_last_valid_row(emu_bin, kind):
    """Rows 30 and 31 of the tile are copies of row 29, whose descriptor is column j's best but whose place fails j's gate; behind the count sits row 0's place,
    which passes it.  A copy that took its constants from there would take column j from row 0."""
    s = GR.scene(kind, 40, 40, 5)
    j = int(s['truth'][0])
    s['d1'][29] = s['d2'][j]
    s['d1'][30:] = s['d1'][29]
    s['k1'][30:] = s['k1'][0]
    assert not GR.gate(s['k1'][:30], s['k2'], s['model'], kind, 3.0)[0][29, j]
    i0, i1 = run_emu(emu_bin, kind, s['d1'][None], s['d2'][None], s['k1'][None], s['k2'][None], np.asarray(s['model'], np.float64).reshape(1, 3, 3), 3.0, -1.0, [30, 40], 1, 1)[0]
    GR.check_guided_mnn_fp64(s['d1'][:30], s['d2'], s['k1'][:30], s['k2'], s['model'], kind, 3.0, i0, i1)
    assert int(i0.max()) < 30 and dict(zip(i0.tolist(), i1.tolist())).get(0) == j


def test_wide_gate_is_the_plain_mutual_nearest_neighbour(emu_bin):
    """H = identity at 1e6 px: everything passes; the result is the float64 plain matcher's."""
    import adversarial
    s = GR.scene('homography', 150, 140, 3)
    i0, i1 = _one(emu_bin, s, 1e6, model=np.eye(3))
    assert adversarial.check_mnn_fp64(s['d1'], s['d2'], i0, i1) > 50


@pytest.mark.parametrize("kind", GR.KINDS)
def test_invalid_models_give_no_matches(emu_bin, kind):
    s = GR.scene(kind, 31, 33, 131)
    assert len(_one(emu_bin, s, 3.0)[0]) > 5
    assert len(_one(emu_bin, s, 3.0, model=np.zeros((3, 3)))[0]) == 0
    bad = np.array(s['model'], np.float64)
    bad[1, 1] = np.nan
    assert len(_one(emu_bin, s, 3.0, model=bad)[0]) == 0
    bad[1, 1] = np.inf
    assert len(_one(emu_bin, s, 3.0, model=bad)[0]) == 0


def test_exact_fixtures_equal_the_restatement(emu_bin):
    for s, thr_of in ((GR.horizontal_fixture(), GR.sampson_threshold_at), (GR.translation_fixture(), float)):
        for k in range(4):
            thr = thr_of(float(s['dys'][k]))
            i0, i1 = _one(emu_bin, s, thr)
            w0, w1 = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], s['kind'], thr)
            assert i0.tolist() == w0.tolist() and i1.tolist() == w1.tolist() == [4 * i + k for i in range(6)]
