"""fm_solve and fm_fit8 (csrc/k_fundamental.hip, on the shared geometry of csrc/twoview_math.hpp) compiled for the HOST
(tests/emu/fundamental_emu.cpp, fp contraction off) against the numpy restatement tests/fundamental_reference.py: on random, noise-free,
noisy and near-degenerate samples the candidates must be equal bit for bit, and so must the 8-point fit; two negative controls edit the
slice (the solver's part, the shared header's part) and show that the comparison notices."""
import subprocess

import numpy as np
import pytest

import fundamental_reference as FR
import twoview_support as TS


def _slice():
    return TS.slice_solver("k_fundamental.hip", "// ---- fm solver begin", "// ---- fm solver end")


def _build(src):
    return TS.build_emu("fundamental_slice.hpp", "fundamental_emu", src)


@pytest.fixture(scope="module")
def emu_bin():
    return _build(_slice())


def _run_solve(emu_bin, X, nt, oriented=True):
    H = X[0].shape[0]
    blob = np.int32(0).tobytes() + np.int32(H).tobytes() + np.int32(int(oriented)).tobytes()
    blob += b"".join(np.ascontiguousarray(v, np.float64).tobytes() for v in X) + np.ascontiguousarray(nt, np.float64).tobytes()
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    return np.frombuffer(out[4 * H:], np.float64).reshape(H, 3, 9), np.frombuffer(out[:4 * H], np.int32)


def _run_fit(emu_bin, sums, nt):
    H = sums.shape[0]
    blob = np.int32(1).tobytes() + np.int32(H).tobytes() + np.ascontiguousarray(sums, np.float64).tobytes()
    blob += np.ascontiguousarray(nt, np.float64).tobytes()
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    return np.frombuffer(out[:4 * H], np.int32), np.frombuffer(out[4 * H:], np.float64).reshape(H, 9)


def _degenerate(X, sub):
    if sub == 0:
        X[:, 2] = 4.0 + 0.1 * X[:, 0]                   # coplanar
    elif sub == 1:
        X[:, 1] = 0.3 * X[:, 2]                         # all on one plane through the first centre: collinear in image 0
    else:
        X[6] = X[5] * (1 + 1e-9)                         # a repeated point


def _samples(rng, H):
    """7-point samples in normalised coordinates, four kinds: uniform noise, noise-free scenes, noisy scenes, near-degenerate (coplanar,
    collinear in one image, a repeated point); and a random conditioning per sample."""
    x = TS.mixed_samples(rng, H, 7, 1.5, _degenerate)
    nt = np.c_[rng.uniform(100, 900, (H, 2)), rng.uniform(1e-3, 1e-2, H), rng.uniform(100, 900, (H, 2)), rng.uniform(1e-3, 1e-2, H)]
    return x, nt


def _compare(cand, nc, want, wnc):
    assert np.array_equal(nc, wnc), np.nonzero(nc != wnc)[0][:10]
    for h in range(len(nc)):
        if not np.array_equal(cand[h, :nc[h]].view(np.uint64), want[h, :nc[h]].view(np.uint64)):
            return h
    return None


@pytest.mark.parametrize("oriented", [True, False])
def test_host_solver_equals_the_restatement_bit_for_bit(emu_bin, oriented):
    rng = np.random.default_rng(2025 + oriented)
    H = 12000
    x, nt = _samples(rng, H)
    cand, nc = _run_solve(emu_bin, x, nt, oriented)
    want, wnc = FR.solve(*x, nt.T, oriented=oriented)
    assert _compare(cand, nc, want, wnc) is None
    assert (nc > 0).mean() > 0.5
    assert np.isfinite(cand).all()


def test_host_solver_on_degenerate_and_non_finite_samples(emu_bin):
    H = 4
    x = np.zeros((4, H, 7))
    x[:, 1] = 0.3                                      # all seven points identical
    x[:, 2] = np.random.default_rng(0).uniform(-1, 1, (4, 7))
    x[0, 2, 3] = np.nan                                 # a NaN coordinate
    x[:, 3] = np.random.default_rng(1).uniform(-1, 1, (4, 7))
    x[2, 3], x[3, 3] = x[0, 3], x[1, 3]                # identity motion: x1 = x0
    nt = np.tile([0.0, 0.0, 1.0, 0.0, 0.0, 1.0], (H, 1))
    cand, nc = _run_solve(emu_bin, x, nt)
    want, wnc = FR.solve(*x, nt.T)
    assert list(nc) == list(wnc)
    assert nc[0] == 0 and nc[1] == 0 and nc[2] == 0
    assert np.isfinite(cand).all()


def test_host_fit8_equals_the_restatement_bit_for_bit(emu_bin):
    rng = np.random.default_rng(7)
    H = 300
    sums, nts = np.zeros((H, 45)), np.zeros((H, 6))
    for h in range(H):
        R, t = TS.rotation(rng.normal(size=3) * 0.4), rng.normal(size=3)
        n = int(rng.integers(8, 200))
        X = np.c_[rng.uniform(-1, 1, (n, 2)), rng.uniform(2, 6, n)]
        X2 = X @ R.T + t
        x0, y0 = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
        x1, y1 = X2[:, 0] / X2[:, 2] + rng.normal(size=n) * 1e-3 * (h % 2), X2[:, 1] / X2[:, 2]
        w = rng.uniform(0, 1, n) if h % 3 else np.ones(n)
        r = [x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, np.ones(n)]
        T = np.stack([(w * r[i]) * r[j] for i in range(9) for j in range(i, 9)], axis=1)
        sums[h] = FR.block_sums(T)
        nts[h] = [rng.uniform(0, 900), rng.uniform(0, 900), rng.uniform(1e-3, 1e-2), rng.uniform(0, 900), rng.uniform(0, 900), rng.uniform(1e-3, 1e-2)]
    ok, F = _run_fit(emu_bin, sums, nts)
    for h in range(H):
        want = FR.fit8(sums[h], nts[h])
        assert ok[h] == (want is not None)
        if want is not None:
            assert np.array_equal(F[h].view(np.uint64), np.array(want).view(np.uint64)), h


def test_negative_control_an_edited_solver_is_caught():
    """One re-associated sum in the slice (the denormalisation's translation column) must break the bit-for-bit comparison."""
    src = _slice()
    edited = src.replace("Fn[3 * i + 2] - (Fn[3 * i] * tx0 + Fn[3 * i + 1] * ty0)", "(Fn[3 * i + 2] - Fn[3 * i] * tx0) - Fn[3 * i + 1] * ty0")
    assert edited != src
    emu = _build(edited)
    rng = np.random.default_rng(11)
    x, nt = _samples(rng, 400)
    cand, nc = _run_solve(emu, x, nt)
    want, wnc = FR.solve(*x, nt.T)
    assert not np.array_equal(nc, wnc) or _compare(cand, nc, want, wnc) is not None


def test_negative_control_an_edited_shared_header_is_caught():
    """The same for the shared geometry: one differently rounded operation in twoview_math.hpp's Gauss-Jordan (the pivot row divided by
    the pivot instead of multiplied by its reciprocal) must break the bit-for-bit comparison."""
    src = _slice()
    edited = src.replace("s[base + c * cols + j] = s[base + c * cols + j] * inv;", "s[base + c * cols + j] = s[base + c * cols + j] / (1.0 / inv);")
    assert edited != src
    emu = _build(edited)
    rng = np.random.default_rng(12)
    x, nt = _samples(rng, 400)
    cand, nc = _run_solve(emu, x, nt)
    want, wnc = FR.solve(*x, nt.T)
    assert not np.array_equal(nc, wnc) or _compare(cand, nc, want, wnc) is not None
