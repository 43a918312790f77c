"""relpose_solve (csrc/k_relpose.hip, on the shared geometry of csrc/twoview_math.hpp) compiled for the HOST (tests/emu/relpose_emu.cpp,
fp contraction off) against the numpy restatement tests/pose_reference.py: on random, noise-free, noisy and near-degenerate samples the
candidate poses must be equal bit for bit."""
import subprocess

import numpy as np
import pytest

import pose_reference as PR
import twoview_support as TS


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("relpose_slice.hpp", "relpose_emu", TS.slice_solver("k_relpose.hip", "// ---- solver begin", "// ---- solver end"))


def _run(emu_bin, x1, y1, x2, y2):
    H = x1.shape[0]
    blob = np.int32(H).tobytes() + b"".join(np.ascontiguousarray(v, np.float64).tobytes() for v in (x1, y1, x2, y2))
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    nc = np.frombuffer(out[:4 * H], np.int32)
    cand = np.frombuffer(out[4 * H:], np.float64).reshape(H, 10, 12)
    return cand, nc


def _degenerate(X, sub):
    if sub == 0:
        X[:, 2] = 4.0 + 0.0 * X[:, 0]          # coplanar (fronto-parallel plane)
    elif sub == 1:
        X[:, 1] = X[:, 0] * 0.5                 # points on a plane through the centre
    else:
        X[4] = X[3] * (1 + 1e-9)                # a repeated point


def _samples(rng, H):
    """Random samples of four kinds: uniform noise, noise-free scenes, noisy scenes, near-degenerate (coplanar / collinear / repeated)."""
    return TS.mixed_samples(rng, H, 5, 0.8, _degenerate)


def test_host_solver_equals_the_restatement_bit_for_bit(emu_bin):
    rng = np.random.default_rng(2024)
    H = 12000
    x = _samples(rng, H)
    cand, nc = _run(emu_bin, *x)
    want, wnc = PR.solve(*x)
    assert np.array_equal(nc, wnc), np.nonzero(nc != wnc)[0][:10]
    assert (nc > 0).mean() > 0.5
    for h in range(H):
        assert np.array_equal(cand[h, :nc[h]].view(np.uint64), want[h, :nc[h]].view(np.uint64)), h


def test_host_solver_on_degenerate_and_non_finite_samples(emu_bin):
    H = 4
    x = np.zeros((4, H, 5))
    x[:, 1] = 0.3                                      # all five points identical
    x[:, 2] = np.random.default_rng(0).uniform(-1, 1, (4, 5))
    x[0, 2, 3] = np.nan                                 # a NaN coordinate
    x[:, 3] = np.random.default_rng(1).uniform(-1, 1, (4, 5))
    x[2, 3], x[3, 3] = x[0, 3], x[1, 3]                # identity motion: x2 = x1
    cand, nc = _run(emu_bin, *x)
    want, wnc = PR.solve(*x)
    assert list(nc) == list(wnc)
    assert nc[0] == 0 and nc[1] == 0 and nc[2] == 0
    assert np.isfinite(cand).all()
