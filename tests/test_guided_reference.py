"""The float64 restatement of guided matching (tests/guided_reference.py) on the CPU: against a literal triple loop, the fp32 evaluation of
both gates against the error window, the distractor fixture, the exactly representable boundary fixtures."""
import math

import numpy as np
import pytest

import guided_reference as GR

# the scenes of the emulated and the GPU tests: (kind, n1, n2, seed, threshold)
SCENES = [(k, n1, n2, 100 + n1, thr) for k in GR.KINDS for (n1, n2), thr in (((1, 1), 3.0), ((31, 33), 3.0), ((257, 129), 1.0), ((300, 1025), 3.0), ((1300, 1100), 2.0))]


def _literal(d1, d2, k1, k2, M, kind, thr, min_cossim):
    """The definition, element by element, nothing vectorised."""
    n1, n2 = len(d1), len(d2)
    M = np.asarray(M, np.float64)
    valid = all(math.isfinite(v) for v in M.reshape(-1)) and any(v != 0 for v in M.reshape(-1))
    S = [[-math.inf] * n2 for _ in range(n1)]
    for i in range(n1):
        x0, y0 = float(k1[i][0]), float(k1[i][1])
        for j in range(n2):
            x1, y1 = float(k2[j][0]), float(k2[j][1])
            if not valid:
                continue
            if kind == 'fundamental':
                l = [M[r][0] * x0 + M[r][1] * y0 + M[r][2] for r in range(3)]
                m = [M[0][c] * x1 + M[1][c] * y1 + M[2][c] for c in range(2)]
                e = (l[0] * x1 + l[1] * y1) + l[2]
                ok = e * e <= thr * thr * (l[0] ** 2 + l[1] ** 2 + m[0] ** 2 + m[1] ** 2)
            else:
                w = M[2][0] * x0 + M[2][1] * y0 + M[2][2]
                if not math.isfinite(w) or abs(w) <= np.finfo(np.float64).eps * math.sqrt(sum(v * v for v in M[2])):
                    continue
                U, V = (M[0][0] * x0 + M[0][1] * y0 + M[0][2]) / w, (M[1][0] * x0 + M[1][1] * y0 + M[1][2]) / w
                ok = (U - x1) ** 2 + (V - y1) ** 2 <= thr * thr
            if ok:
                S[i][j] = sum(float(a) * float(b) for a, b in zip(d1[i], d2[j]))
    out = []
    for i in range(n1):
        j = max(range(n2), key=lambda c: (S[i][c], -c))
        if S[i][j] == -math.inf or (min_cossim > 0 and not S[i][j] > min_cossim):
            continue
        if max(range(n1), key=lambda r: (S[r][j], -r)) == i:
            out.append((i, j))
    return out


@pytest.mark.parametrize("kind", GR.KINDS)
@pytest.mark.parametrize("n1,n2,min_cossim", [(1, 1, -1.0), (5, 9, -1.0), (12, 7, 0.5), (20, 20, -1.0)])
def test_restatement_equals_the_literal_loop(kind, n1, n2, min_cossim):
    s = GR.scene(kind, n1, n2, 5 * n1 + n2)
    for thr in (0.5, 3.0, 50.0):
        i0, i1 = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, thr, min_cossim)
        want = _literal(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], kind, thr, min_cossim)
        # (the literal loop sums 64 products in another order than the matrix product: scenes without near-ties, so the order is immaterial)
        assert list(zip(i0.tolist(), i1.tolist())) == want
    for bad in (np.zeros((3, 3)), np.where(np.eye(3) > 0, np.nan, s['model'])):
        assert _literal(s['d1'], s['d2'], s['k1'], s['k2'], bad, kind, 3.0, -1.0) == []
        assert len(GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], bad, kind, 3.0)[0]) == 0


@pytest.mark.parametrize("kind,n1,n2,seed,thr", SCENES)
def test_fp32_gate_never_flips_a_decided_element(kind, n1, n2, seed, thr):
    """On the scenes of the kernel tests: the kernel's arithmetic (numpy fp32) agrees with float64 wherever the window calls the element
    decided, and the scenes stay under the cap on undecided elements."""
    s = GR.scene(kind, n1, n2, seed)
    passes, decided = GR.gate(s['k1'], s['k2'], s['model'], kind, thr)
    p32 = GR.gate_fp32(s['k1'], s['k2'], s['model'], kind, thr)
    flips = (p32 != passes) & decided
    und = int((~decided).sum())
    print(f"{kind} {n1} x {n2} thr {thr}: pass {passes.mean():.4f}, undecided {und} of {decided.size}, fp32 != fp64 on {int((p32 != passes).sum())}")
    assert not flips.any()
    assert und <= GR.MAX_UNDECIDED * decided.size
    assert passes.any()


def test_the_window_is_not_vacuous():
    """fp32 and float64 do disagree somewhere (inside the window) once there are enough elements near the threshold: points ON the
    transferred position at a distance of exactly thr in float64 terms."""
    rng = np.random.default_rng(3)
    n = 4000
    H = np.array([[1.01, 0.02, 3.3], [-0.015, 0.99, -2.7], [1e-5, -2e-5, 1.0]])
    k1 = np.c_[rng.uniform(0, 640, n), rng.uniform(0, 480, n)].astype(np.float32)
    q = np.c_[k1.astype(np.float64), np.ones(n)] @ H.T
    a = rng.uniform(0, 2 * np.pi, n)
    k2 = (q[:, :2] / q[:, 2:] + 3.0 * np.c_[np.cos(a), np.sin(a)]).astype(np.float32)
    passes, decided = GR.gate(k1, k2, H, 'homography', 3.0)
    p32 = GR.gate_fp32(k1, k2, H, 'homography', 3.0)
    d = np.arange(n)
    assert (p32 != passes)[d, d].any() or (~decided)[d, d].sum() > 0
    assert not ((p32 != passes) & decided).any()


def test_distractors_defeat_the_plain_matcher_and_not_the_guided_one():
    """pair 7, 512 true correspondences at 0.5 px, an exact descriptor copy of every image-0 point somewhere in image 1: the plain mutual
    nearest neighbours take the copies, the gate at 2 px Sampson under the true F removes them (prototype: 0 and 510 of 512)."""
    s = GR.distractor_scene()
    n = len(s['truth'])
    wide = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], np.eye(3), 'homography', 1e6)      # everything passes: plain mutual nearest neighbours
    assert len(wide[0]) == n
    plain = GR.true_matches(s, *wide)
    guided = GR.true_matches(s, *GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], 'fundamental', 2.0))
    print(f"true matches of {n}: plain {plain}, guided {guided}")
    assert plain < 0.05 * n and guided >= 0.95 * n


@pytest.mark.parametrize("k", range(4))
def test_horizontal_epipolar_fixture_pins_the_inclusive_compare(k):
    """Sampson error |y1 - y0| / sqrt(2) exactly: at the threshold that equals copy k's error the copy passes (<=), the next one does not."""
    s = GR.horizontal_fixture()
    thr = GR.sampson_threshold_at(float(s['dys'][k]))
    assert thr * thr * 2.0 >= s['dys'][k] ** 2 and np.nextafter(thr, 0) ** 2 * 2.0 < s['dys'][k] ** 2
    i0, i1 = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], 'fundamental', thr)
    assert i0.tolist() == list(range(6)) and i1.tolist() == [4 * i + k for i in range(6)]
    assert np.array_equal(GR.gate_fp32(s['k1'], s['k2'], s['model'], 'fundamental', thr), GR.gate(s['k1'], s['k2'], s['model'], 'fundamental', thr)[0])
    below = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], 'fundamental', 0.99 * thr)[1]
    assert below.tolist() == ([4 * i + k - 1 for i in range(6)] if k else [])


@pytest.mark.parametrize("k", range(4))
def test_dyadic_translation_fixture_pins_the_inclusive_compare(k):
    s = GR.translation_fixture()
    thr = float(s['dys'][k])
    i0, i1 = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], 'homography', thr)
    assert i0.tolist() == list(range(6)) and i1.tolist() == [4 * i + k for i in range(6)]
    assert np.array_equal(GR.gate_fp32(s['k1'], s['k2'], s['model'], 'homography', thr), GR.gate(s['k1'], s['k2'], s['model'], 'homography', thr)[0])
    below = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], s['model'], 'homography', np.nextafter(thr, 0))[1]
    assert below.tolist() == ([4 * i + k - 1 for i in range(6)] if k else [])


def test_checker_rejects_wrong_lists():
    s = GR.scene('fundamental', 31, 33, 131)
    a = (s['d1'], s['d2'], s['k1'], s['k2'], s['model'], 'fundamental', 3.0)
    i0, i1 = GR.guided_mnn(*a)
    must, _ = GR.check_guided_mnn_fp64(*a, i0, i1)
    assert must > 10
    with pytest.raises(AssertionError):
        GR.check_guided_mnn_fp64(*a, i0[1:], i1[1:])                       # a strict winner missing
    with pytest.raises(AssertionError):
        GR.check_guided_mnn_fp64(*a, i0[::-1], i1[::-1])                   # not ascending
    plain = GR.guided_mnn(s['d1'], s['d2'], s['k1'], s['k2'], np.eye(3), 'homography', 1e6)
    extra = [(i, j) for i, j in zip(*plain) if not GR.gate(s['k1'], s['k2'], s['model'], 'fundamental', 3.0)[0][i, j]]
    if extra:
        i, j = extra[0]
        keep = i0 != i
        w0, w1 = np.r_[i0[keep], i], np.r_[i1[keep], j]
        o = np.argsort(w0)
        with pytest.raises(AssertionError):
            GR.check_guided_mnn_fp64(*a, w0[o], w1[o])                     # a pair that fails the gate
