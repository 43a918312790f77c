"""relpose_solve (csrc/k_relpose.hip, on the shared geometry of csrc/twoview_math.hpp) compiled for the HOST (tests/emu/relpose_emu.cpp,
fp contraction off) against the numpy restatement tests/pose_reference.py: on random, noise-free, noisy and near-degenerate samples the
candidate poses must be equal bit for bit."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pose_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated_features_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _between(name, begin, end):
    """(whole text, text between the two markers) of a product source file."""
    t = open(os.path.join(CSRC, name)).read()
    a = t.index(begin)
    return t, t[a:t.index(end, a)]


def _slice():
    """The shared geometry (twoview_math.hpp, which must be host-compilable as a whole file) in front of the solver's own slice."""
    header, shared = _between("twoview_math.hpp", "// ---- twoview math begin", "// ---- twoview math end")
    _, solver = _between("k_relpose.hip", "// ---- solver begin", "// ---- solver end")
    for s in (header, solver):
        assert "__shared__" not in s and "asm" not in s and "__builtin_amdgcn" not in s
    assert "gauss_jordan" in shared and "gauss_jordan(S s" not in solver
    return (shared + solver).replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    td = tempfile.mkdtemp()
    open(os.path.join(td, "relpose_slice.hpp"), "w").write(_slice())
    out = os.path.join(td, "relpose_emu")
    subprocess.run([CLANG, "-O2", "-w", "-std=c++20", "-ffp-contract=off", "-I", td, "-I", EMU, os.path.join(EMU, "relpose_emu.cpp"), "-o", out],
                   check=True)
    return out


def _run(emu_bin, x1, y1, x2, y2):
    H = x1.shape[0]
    blob = np.int32(H).tobytes() + b"".join(np.ascontiguousarray(v, np.float64).tobytes() for v in (x1, y1, x2, y2))
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    nc = np.frombuffer(out[:4 * H], np.int32)
    cand = np.frombuffer(out[4 * H:], np.float64).reshape(H, 10, 12)
    return cand, nc


def _samples(rng, H):
    """Random samples of four kinds: uniform noise, noise-free scenes, noisy scenes, near-degenerate (coplanar / collinear / repeated)."""
    x = rng.uniform(-0.8, 0.8, (4, H, 5))
    kind = np.arange(H) % 4
    for h in np.nonzero(kind > 0)[0]:
        w = rng.normal(size=3) * 0.3
        th = np.linalg.norm(w)
        k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        t = rng.normal(size=3)
        X = np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(2, 6, 5)]
        if kind[h] == 3:
            sub = h % 3
            if sub == 0:
                X[:, 2] = 4.0 + 0.0 * X[:, 0]          # coplanar (fronto-parallel plane)
            elif sub == 1:
                X[:, 1] = X[:, 0] * 0.5                 # points on a plane through the centre
            else:
                X[4] = X[3] * (1 + 1e-9)                # a repeated point
        X2 = X @ R.T + t
        x[0, h], x[1, h] = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
        x[2, h], x[3, h] = X2[:, 0] / X2[:, 2], X2[:, 1] / X2[:, 2]
        if kind[h] == 2:
            x[:, h] += rng.normal(size=(4, 5)) * 1e-3
    return x


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
