"""The solver slice of csrc/k_align.hip (al_solve, al_fit from its centred sums, the residual and its cost, on the shared geometry of
csrc/twoview_math.hpp) compiled for the HOST (tests/emu/alignment_emu.cpp, fp contraction off) against the numpy restatement
tests/alignment_reference.py: on noise-free, noisy, near-collinear, planar and far-from-origin inputs the models must be equal bit for
bit."""
import subprocess

import numpy as np
import pytest

import alignment_reference as AL
import alignment_support as AS
import twoview_support as TS

THR2 = 0.25


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("alignment_slice.hpp", "alignment_emu", TS.slice_solver("k_align.hip", "// ---- solver begin", "// ---- solver end"))


def _run(emu_bin, A, B, S, ca, cb, with_scale):
    H = A.shape[0]
    blob = np.array([H, int(with_scale)], np.int32).tobytes() + np.float64(THR2).tobytes() + b"".join(
        np.ascontiguousarray(v, np.float64).tobytes() for v in (A, B, S, ca, cb))
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    ints = np.frombuffer(out[:12 * H], np.int32).reshape(3, H)
    dbl = np.frombuffer(out[12 * H:], np.float64)
    return ints[0], ints[1], ints[2], dbl[:13 * H].reshape(H, 13), dbl[13 * H:26 * H].reshape(H, 13), dbl[26 * H:]


def _want(A, B, S, ca, cb, with_scale):
    ms, oks = AL.solve(A, B, with_scale)
    mf, okf = AL.fit(S, ca, cb, with_scale)
    with np.errstate(all="ignore"):
        r2 = AL.residual2(AL.scaled_rotation(mf), [mf[:, 9 + k] for k in range(3)], *(A[:, 2, k] for k in range(3)), *(B[:, 2, k] for k in range(3)))
        r2 = np.where(okf, r2, 0.0)
        cost = np.where(okf, AL.cost(r2, THR2), 0)
    return oks, okf, cost, ms, mf, r2


def _equal_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("with_scale", [True, False])
def test_host_solver_slice_equals_the_restatement_bit_for_bit(emu_bin, with_scale):
    rng = np.random.default_rng(2026)
    H = 12000
    inputs = AS.mixed_inputs(rng, H)
    oks, okf, cost, ms, mf, r2 = _run(emu_bin, *inputs, with_scale)
    w_oks, w_okf, w_cost, w_ms, w_mf, w_r2 = _want(*inputs, with_scale)
    assert np.array_equal(oks, w_oks.astype(np.int32)), np.nonzero(oks != w_oks)[0][:10]
    assert np.array_equal(okf, w_okf.astype(np.int32)), np.nonzero(okf != w_okf)[0][:10]
    kind = np.arange(H) % len(AS.KINDS)
    assert oks[kind == 0].all() and oks[kind == 4].all() and 0.02 < (oks[kind == 2] == 0).mean() < 0.98      # the threshold is crossed both ways
    assert okf[kind != 2].all()
    for h in np.nonzero(~(ms == w_ms).all(axis=1) | ~(mf == w_mf).all(axis=1))[0][:5]:
        assert False, (h, ms[h], w_ms[h], mf[h], w_mf[h])
    assert _equal_bits(ms, w_ms) and _equal_bits(mf, w_mf) and _equal_bits(r2, w_r2)
    assert np.array_equal(cost, w_cost)
    assert 0 < (cost < 1048576).sum() and (cost == 1048576).sum() > 0


def test_host_solver_on_degenerate_and_non_finite_inputs(emu_bin):
    rng = np.random.default_rng(0)
    H = 8
    A, B, _ = AS.true_samples(rng, H)
    S, ca, cb = np.zeros((H, 10)), np.zeros((H, 3)), np.zeros((H, 3))
    for h in range(H):
        S[h], ca[h], cb[h] = AS.centred_sums(*AS.shaped_cloud(rng, 20, 0))
    A[0] = A[0, :1]                                    # three coincident points: va = 0
    B[1] = B[1, :1]                                    # vb = 0
    A[2, 1, 2] = np.nan
    B[3, 0, 0] = np.inf
    A[4, 2] = A[4, 0] + 2.0 * (A[4, 1] - A[4, 0])      # collinear in A
    B[5, 2] = B[5, 0] - 0.5 * (B[5, 1] - B[5, 0])      # collinear in B
    A[6, 1] = A[6, 0]                                  # a zero first side
    S[0] = 0.0                                         # a cloud of coincident points: sum |x|^2 = 0
    S[1] = -S[1]                                       # every sum negated, sum |x|^2 too: the scale comes out negative
    S[2, 4] = np.nan
    got = _run(emu_bin, A, B, S, ca, cb, True)
    want = _want(A, B, S, ca, cb, True)
    assert list(got[0]) == [0, 0, 0, 0, 0, 0, 0, 1] == [int(v) for v in want[0]]
    assert list(got[1]) == [0, 0, 0, 1, 1, 1, 1, 1] == [int(v) for v in want[1]]
    assert np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    rigid = _run(emu_bin, A, B, S, ca, cb, False)
    assert list(rigid[0]) == [0, 0, 0, 0, 0, 0, 0, 1] and list(rigid[1]) == [1, 1, 0, 1, 1, 1, 1, 1]      # s = 1 needs no sum |x|^2
    assert (rigid[3][7, 12], rigid[4][0, 12]) == (1.0, 1.0)
