"""ap_solve (csrc/k_abspose.hip, on the shared geometry of csrc/twoview_math.hpp) compiled for the HOST (tests/emu/abspose_emu.cpp, fp
contraction off) against the numpy restatement tests/abspose_reference.py: on random, noise-free, noisy and near-degenerate samples the
candidate poses must be equal bit for bit."""
import subprocess

import numpy as np
import pytest

import abspose_reference as AR
import abspose_support as AS
import twoview_support as TS


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("abspose_slice.hpp", "abspose_emu", TS.slice_solver("k_abspose.hip", "// ---- solver begin", "// ---- solver end"))


def _run(emu_bin, x, y, X):
    H = x.shape[0]
    blob = np.int32(H).tobytes() + b"".join(np.ascontiguousarray(v, np.float64).tobytes() for v in (x, y, X))
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    nc = np.frombuffer(out[:4 * H], np.int32)
    cand = np.frombuffer(out[4 * H:], np.float64).reshape(H, 4, 12)
    return cand, nc


def test_host_solver_equals_the_restatement_bit_for_bit(emu_bin):
    rng = np.random.default_rng(2025)
    H = 12000
    x, y, X = AS.mixed_samples(rng, H)
    cand, nc = _run(emu_bin, x, y, X)
    want, wnc = AR.solve(x, y, X)
    assert np.array_equal(nc, wnc), np.nonzero(nc != wnc)[0][:10]
    assert (nc > 0).mean() > 0.5
    kind = np.arange(H) % 4
    assert (nc[kind == 1] > 0).mean() > 0.95 and (nc[kind == 3] == 0).mean() > 0.3      # scenes leave candidates, degenerate ones are seen
    for h in range(H):
        assert np.array_equal(cand[h, :nc[h]].view(np.uint64), want[h, :nc[h]].view(np.uint64)), h


def test_host_solver_on_degenerate_and_non_finite_samples(emu_bin):
    rng = np.random.default_rng(0)
    H = 6
    x, y, X, _ = AS.true_samples(rng, H)
    X[0] = X[0, :1]                                    # all three points identical
    x[1, 2] = np.nan                                    # a NaN image coordinate
    X[2, 1, 0] = np.inf                                 # an infinite 3D coordinate
    X[3, 2] = X[3, 0] + 2.0 * (X[3, 1] - X[3, 0])      # collinear
    x[4], y[4] = x[4, 0], y[4, 0]                      # one pixel for three different points
    cand, nc = _run(emu_bin, x, y, X)
    want, wnc = AR.solve(x, y, X)
    assert list(nc) == list(wnc)
    assert list(nc[:5]) == [0, 0, 0, 0, 0] and nc[5] > 0
    assert np.isfinite(cand).all()
