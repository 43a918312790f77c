"""The LighterGlue kernels (csrc/k_lighterglue.hip, and linear_mfma_kernel of csrc/k_linear_mfma.hip for the similarity matrix) compiled for the HOST (tests/emu/) and run
against float64 restatements of the operations they implement: the key-point encoding, the linear layers with their four epilogues, softmax attention, matchability and width
pruning, the similarity matrix, the double log-softmax assignment and the mutual filter.  The kernels are sliced out of the product sources at test time (nothing is copied);
tests/emu/lighterglue_emu.cpp repeats the launchers' grid arithmetic and allocates every buffer at exactly its capacity, filled with NaN past the live counts.

Bars are fp32 error bounds, u = 2^-24 (unit roundoff):
  * a dot product of K terms plus a bias, accumulated in fp32 in any order: |err| <= (K + 2) u (|b| + sum |x_k w_k|);
  * a softmax whose base-2 logits each carry |err| <= E (the logit's dot product bound above, scaled by scale*log2(e), plus one rounding of q * scale*log2(e)): the weights move
    by at most 4 ln2 E in L1, so an output column moves by at most 4 ln2 E max|V|; the exponentials, the running sums and the per-tile / per-split rescales add
    (2 nk + 3 ntiles + 32) u max|V|; values that v_exp_f32 flushes (below 2^-126 of the maximum) add nk 2^-126 max|V|;
  * a log-sum-exp over n terms: (n + 4) u + u |lse|; a score sim - rlse + sim - clse + ls0 + ls1: the sum of its parts' bounds plus 4 u times the sum of their magnitudes.
Integer outputs (maps, counts, arg-max indices, match lists) must match exactly wherever the float64 margin exceeds the bound; the cases are built so that it does everywhere,
except on EXACT ties (duplicated rows / columns: bit-identical fp32 scores), where the kernels' rule is "first index".
The negative controls edit the sliced text and show that the same comparison then fails."""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated_features_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
U = 2.0 ** -24
LOG2E = 1.4426950408889634
D = 96
STORE, RESIDUAL, ROTARY, LNGELU = 0, 1, 2, 3


def _between(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


def _must_sub(text, old, new):
    assert text.count(old) == 1, f"marker not found once in the kernel source: {old[:70]!r}"
    return text.replace(old, new)


def _lds(seg):
    """__shared__ declarations of one kernel -> references into emu.hpp's LDS buffer (NaN patterns at the start), consecutive 16-byte aligned offsets"""
    off, out, pos = "0", [], 0
    for m in re.finditer(r"__shared__\s+(?:__attribute__\(\(aligned\(16\)\)\)\s+)?([A-Za-z_][\w ]*?)\s+(\w+)((?:\[[^\]]+\])*);", seg):
        ty, name, dims = m.group(1), m.group(2), m.group(3)
        base = f"(emu::wg->lds_base() + {off})"
        out.append(seg[pos:m.start()] + (f"auto& {name} = *reinterpret_cast<{ty} (*){dims}>{base};" if dims else f"{ty}& {name} = *reinterpret_cast<{ty}*>{base};"))
        pos = m.end()
        off = f"{off} + (sizeof({ty}{dims}) + 15) / 16 * 16"
    return "".join(out) + seg[pos:]


def _slice(mutate=None):
    """common.hpp's helpers, the structs of kernels.hpp, linear_mfma_kernel and every kernel and host helper of k_lighterglue.hip but the launchers (which use <<< >>>)."""
    com = open(os.path.join(CSRC, "common.hpp")).read()
    s = _between(com, "__host__ __device__ inline int ceil_div(", "__host__ __device__ inline size_t align_up(")
    s += _between(com, "__device__ inline float wave_sum(float v) {", "__device__ inline double wave_sum(double v) {")
    s += _between(com, "__device__ inline float wave_max(float v) {", "__device__ inline int wave_sum_i(int v) {")
    s += _between(com, "__device__ inline unsigned long long shfl_xor_u64(", "// Value held by the lane 32 positions away")
    s += _between(com, "__device__ inline unsigned long long u64_max(", "// Barrier that covers global->LDS DMA")
    kh = open(os.path.join(CSRC, "kernels.hpp")).read()
    s += _between(kh, "enum LinLoader {", "// y (M,n) row-major with leading dimension ldy.")
    s += _between(kh, "enum { LG_EPI_STORE = 0,", "void launch_lg_encode(")
    s += _between(open(os.path.join(CSRC, "k_linear_mfma.hip")).read(), "typedef float f32x16", "int launch_linear_mfma(")
    k = _between(open(os.path.join(CSRC, "k_lighterglue.hip")).read(), "typedef float f32x16", "}  // namespace xfh")
    k, n = re.subn(r"^(?:void|int) launch_lg_\w+\([^{]*\{.*?^\}\n", "", k, flags=re.S | re.M)
    assert n == 7, n
    k = _must_sub(k, "__shared__ float sm[4][64], ss[4][64];", "__shared__ float sm[4][64];\n    __shared__ float ss[4][64];")
    if mutate:
        k = mutate(k)
    s += k
    s = "".join(_lds(p) for p in re.split(r"(?=(?:template <[^>]*>\n)?__global__ )", s))
    s, n = re.subn(r"__global__ __launch_bounds__\([^)]*\) void", "inline void", s)
    assert n == 17, n
    s = s.replace("__device__ ", "").replace("__host__ ", "")
    assert "<<<" not in s and "__shared__" not in s and "asm" not in s and "__global__" not in s
    return s


def _build(mutate=None, flags=()):
    td = tempfile.mkdtemp()
    open(os.path.join(td, "lighterglue_slice.hpp"), "w").write(_slice(mutate))
    out = os.path.join(td, "lighterglue_emu")
    subprocess.run([CLANG, "-O1", "-w", "-std=c++20", "-pthread", *flags, "-I", td, "-I", EMU, os.path.join(EMU, "lighterglue_emu.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def emu_bin():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    return _build()


def _i(*v):
    return np.array(v, np.int32).tobytes()


def _f(*v):
    return np.array(v, np.float32).tobytes()


def _a(x, dt=np.float32):
    return np.ascontiguousarray(x, dt).tobytes()


class _Out:
    def __init__(self, b):
        self.b, self.o = b, 0

    def take(self, n, dt=np.float32):
        a = np.frombuffer(self.b[self.o:self.o + n * np.dtype(dt).itemsize], dt)
        assert a.size == n, "short output"
        self.o += a.nbytes
        return a.copy()

    def done(self):
        assert self.o == len(self.b), (self.o, len(self.b))


def _exe(binary, blob, env=None):
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    return _Out(r.stdout)


def _is_nan(a):
    return np.isnan(a).all()


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# lg_encode_kernel
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _encode(binary, kp, W, H, wr):
    N = len(kp)
    o = _exe(binary, _i(0, N) + _f(W, H) + _a(kp) + _a(wr))
    cs, sn = o.take(N * D).reshape(N, D), o.take(N * D).reshape(N, D)
    o.done()
    return cs, sn


@pytest.mark.parametrize("N,W,H", [(1, 640, 480), (7, 480, 640), (300, 1000, 300)])
def test_encode_kernel(emu_bin, N, W, H):
    """kn = (kp - size/2) / (max(W,H)/2), proj = Wr kn, (cos, sin) with every frequency repeated twice.  Bar: kn carries 4 u |kn|, proj 8 u sum |Wr kn|, cos / sin one more
    rounding each (the host's libm: within an ulp)."""
    rng = np.random.default_rng(N)
    kp = np.stack([rng.uniform(0, W - 1, N), rng.uniform(0, H - 1, N)], -1).astype(np.float32)
    extreme = [(0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0), (-50, H + 100), (3 * W, -2 * H), (W / 2, H / 2)]      # corners, outside the image, the centre
    for i, p in enumerate(extreme[:N]):
        kp[i] = p
    wr = (2.0 * rng.standard_normal((48, 2))).astype(np.float32)
    cs, sn = _encode(emu_bin, kp, np.float32(W), np.float32(H), wr)
    sc = max(W, H) / 2.0
    kn = (kp.astype(np.float64) - np.array([W / 2.0, H / 2.0])) / sc
    proj = kn @ wr.astype(np.float64).T
    mag = np.abs(kn) @ np.abs(wr.astype(np.float64)).T
    bar = 12 * U * (mag + 1.0)
    for got, ref in ((cs, np.cos(proj)), (sn, np.sin(proj))):
        assert np.array_equal(got[:, 0::2], got[:, 1::2])
        assert (np.abs(got[:, 0::2] - ref) <= bar).all(), float((np.abs(got[:, 0::2] - ref) / bar).max())


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# lg_linear_kernel: STORE (K 64 / 96), ROTARY, RESIDUAL, LNGELU
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _pack(W):
    """api_lg.hip's operand order: float4 index ((cb*2 + half)*(K/8) + j)*32 + lane = W[cb*32 + lane][half*K/2 + 4j .. +3]"""
    N, K = W.shape
    return np.ascontiguousarray(W.reshape(N // 32, 32, 2, K // 8, 4).transpose(0, 2, 3, 1, 4)).reshape(-1)


def _linear(binary, K, N, epi, W, b, sides, gamma=None, beta=None, env=None):
    """sides: dicts with cap, live, x (cap, ldx), y (cap, ldy) initial contents, cs / sn (cap, 96) or None"""
    gamma = np.ones(192, np.float32) if gamma is None else gamma
    beta = np.zeros(192, np.float32) if beta is None else beta
    blob = _i(1, K, N, epi, len(sides)) + _a(_pack(W)) + _a(b) + _a(gamma) + _a(beta)
    for s in sides:
        cap = s["cap"]
        cs = s.get("cs"); sn = s.get("sn")
        cs = np.full((cap, D), np.nan, np.float32) if cs is None else cs
        sn = np.full((cap, D), np.nan, np.float32) if sn is None else sn
        blob += _i(cap, s["live"], s["x"].shape[1], s["y"].shape[1]) + _a(s["x"]) + _a(s["y"]) + _a(cs) + _a(sn)
    o = _exe(binary, blob, env)
    ys = [o.take(s["y"].size).reshape(s["y"].shape) for s in sides]
    o.done()
    return ys


def _ln_gelu_ref(h, gamma, beta, dh, dmu):
    """float64 LayerNorm(192) + exact GELU of h, and the bound of an fp32 two-pass evaluation whose h carries dh (per row) and whose mean carries dmu (per row)"""
    mu = h.mean(1, keepdims=True)
    var = ((h - mu) ** 2).mean(1, keepdims=True)
    sig = np.sqrt(var + 1e-5)
    yh = (h - mu) / sig
    y = yh * gamma + beta
    out = 0.5 * y * (1.0 + torch.special.erf(torch.from_numpy(y / math.sqrt(2.0))).numpy())
    e_yh = 2.0 * ((dh + dmu)[:, None] / sig * (1.0 + np.abs(yh)) + 200 * U * np.abs(yh) + 4 * U)
    e_y = np.abs(gamma) * e_yh + 4 * U * (np.abs(yh * gamma) + np.abs(beta))
    return out, 1.13 * e_y + 8 * U * (np.abs(out) + np.abs(y))


def _rand_side(rng, cap, live, ldx, ldy, K, N, epi):
    x = np.full((cap, ldx), np.nan, np.float32)
    x[:live, :] = rng.standard_normal((live, ldx)).astype(np.float32)
    y = np.full((cap, ldy), np.nan, np.float32)
    side = dict(cap=cap, live=live, x=x, y=y)
    if epi == RESIDUAL:
        y[:live, :N] = rng.standard_normal((live, N)).astype(np.float32)
    if epi == ROTARY:
        ang = rng.uniform(-4, 4, (cap, D // 2))
        side["cs"] = np.repeat(np.cos(ang), 2, 1).astype(np.float32)
        side["sn"] = np.repeat(np.sin(ang), 2, 1).astype(np.float32)
        side["cs"][live:] = np.nan; side["sn"][live:] = np.nan
    return side


def _check_linear(K, N, epi, W, b, sides, ys, gamma=None, beta=None, exact_pre=False):
    worst = 0.0
    for s, y in zip(sides, ys):
        live, x = s["live"], s["x"][:s["live"], :K].astype(np.float64)
        h = x @ W.astype(np.float64).T + b.astype(np.float64)
        dh = (K + 2) * U * (np.abs(b.astype(np.float64)) + np.abs(x) @ np.abs(W.astype(np.float64)).T)
        if epi == STORE:
            ref, bar = h, dh
        elif epi == RESIDUAL:
            old = s["y"][:live, :N].astype(np.float64)
            ref, bar = h + old, dh + U * np.abs(h + old)
        elif epi == ROTARY:
            ref, bar = h.copy(), dh.copy()
            c = np.tile(s["cs"][:live].astype(np.float64), (1, 2)); sn = np.tile(s["sn"][:live].astype(np.float64), (1, 2))
            q = h[:, :192]
            rh = np.empty_like(q); rh[:, 0::2] = -q[:, 1::2]; rh[:, 1::2] = q[:, 0::2]      # the oracle's rotate_half
            dq = dh[:, :192]
            drh = np.empty_like(q); drh[:, 0::2] = dq[:, 1::2]; drh[:, 1::2] = dq[:, 0::2]
            ref[:, :192] = q * c + rh * sn
            bar[:, :192] = dh[:, :192] * np.abs(c) + drh * np.abs(sn) + 3 * U * (np.abs(q * c) + np.abs(rh * sn))
        else:
            g = np.ones(192) if gamma is None else gamma.astype(np.float64)
            be = np.zeros(192) if beta is None else beta.astype(np.float64)
            dmax = np.zeros(live) if exact_pre else dh.max(1)
            dmu = np.zeros(live) if exact_pre else dh.mean(1) + 194 * U * np.abs(h).mean(1)
            ref, bar = _ln_gelu_ref(h, g, be, dmax, dmu)
        got = y[:live, :N].astype(np.float64)
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got - ref) / bar).max()))
        assert np.array_equal(y[:live, N:].view(np.uint32), s["y"][:live, N:].view(np.uint32)), "columns past N written"
        assert np.array_equal(y[live:].view(np.uint32), s["y"][live:].view(np.uint32)), "rows past the live count written"
    return worst


@pytest.mark.parametrize("K,N,epi,shapes", [
    (64, 96, STORE, [(1, 1), (33, 40)]),
    (96, 96, STORE, [(31, 64), (300, 300)]),
    (96, 288, ROTARY, [(32, 33), (97, 128)]),
    (192, 96, RESIDUAL, [(33, 33), (1, 7)]),
    (192, 192, LNGELU, [(300, 320), (31, 31)]),
])
def test_linear_kernel_epilogues(emu_bin, K, N, epi, shapes):
    """y = x W^T + b on v_mfma_f32_32x32x2_f32 with its fused epilogues; two sides of different live counts and capacities in one launch; rows past the live count
    (NaN in x) never read into a live row and never written.  Bar: (K + 2) u (|b| + sum |x w|) for the product, then the epilogue's own roundings (module docstring);
    LNGELU: the two-pass LayerNorm bound of _ln_gelu_ref."""
    rng = np.random.default_rng(K * 1000 + N + epi)
    W = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(192)).astype(np.float32) if epi == LNGELU else None
    beta = (0.1 * rng.standard_normal(192)).astype(np.float32) if epi == LNGELU else None
    ldx, ldy = {64: 64, 96: 192, 192: 192}[K], {96: 192, 288: 288, 192: 192}[N]
    sides = [_rand_side(rng, cap, live, ldx, ldy, K, N, epi) for live, cap in shapes]
    ys = _linear(emu_bin, K, N, epi, W, b, sides, gamma, beta)
    worst = _check_linear(K, N, epi, W, b, sides, ys, gamma, beta)
    print(f"K {K} N {N} epi {epi}: max |err| / bar {worst:.3g}")
    assert worst <= 1.0


def _ln_large_mean_case(rng):
    """Rows whose pre-LN values are 1024 + k/64 (k in {-2..2}, sum k = 0): mean 1024, spread ~1e-2.  Every product, partial sum and the mean (196608 * fl(1/192) rounds to
    1024) are exact in fp32, so the two-pass LayerNorm owes only its own roundings -- a one-pass variance (E[h^2] - mean^2, terms ~1e6 with ulp 0.06) cannot pass."""
    K, N, live, cap = 192, 192, 5, 8
    k = np.tile(np.array([-1, 1, 0, 2, -2, 0]), 32)[:N].astype(np.float64)
    rng.shuffle(k)
    W = np.zeros((N, K), np.float32)
    W[:, 0] = k / 64
    W[:, 1] = np.roll(k, 7) / 64
    b = np.full(N, 1024.0, np.float32)
    x = np.full((cap, K), np.nan, np.float32)
    x[:live] = 0.0
    x[:live, 0] = [1, -1, 0.5, 0, 1]
    x[:live, 1] = [0, 1, 0.5, 1, -1]
    y = np.full((cap, N), np.nan, np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(192)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(192)).astype(np.float32)
    return K, N, W, b, [dict(cap=cap, live=live, x=x, y=y)], gamma, beta


def test_linear_lngelu_large_mean_small_spread(emu_bin):
    K, N, W, b, sides, gamma, beta = _ln_large_mean_case(np.random.default_rng(5))
    ys = _linear(emu_bin, K, N, LNGELU, W, b, sides, gamma, beta)
    worst = _check_linear(K, N, LNGELU, W, b, sides, ys, gamma, beta, exact_pre=True)
    print(f"LN mean 1024 spread 1e-2: max |err| / bar {worst:.3g}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# lg_attention_kernel + lg_attention_combine_kernel
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _lg_attention_splits(qcap, kcap):      # only to choose cases; the driver uses the sliced host function itself
    nqb = -(-max(qcap, 1) // 128)
    return max(min(-(-256 // nqb), 16, max(kcap, 1) // 64), 1)


def _attention(binary, sides, scale, ld=D, env=None):
    blob = _i(2, len(sides), ld) + _f(scale)
    for s in sides:
        blob += _i(s["qcap"], s["kcap"], s["nq"], s["nk"]) + _a(s["Q"]) + _a(s["K"]) + _a(s["V"])
    o = _exe(binary, blob, env)
    res = []
    for s in sides:
        ns = int(o.take(1, np.int32)[0])
        res.append((ns, o.take(s["qcap"] * D).reshape(s["qcap"], D)))
    o.done()
    return res


def _att_side(rng, qcap, kcap, nq, nk, peaked=None, spike_split=None):
    """Q, K, V of one side (NaN past the live counts).  peaked = a: feature 0 carries the logits' structure -- Q0 cycles through (+a, -a, 0, +a/3) so that lanes of one
    wave disagree about where their maximum is, K0 ramps from -1 to 1 so that the maximum of the +a queries first appears in the LAST tile (a new maximum in every tile),
    the -a queries peak in the first tile; spike_split = s: one key of split s gets K0 = 3 (the maximum of the +a queries lives in that split only, every other
    split's keys underflow relative to it)."""
    Q = np.full((qcap, D), np.nan, np.float32); K = np.full((kcap, D), np.nan, np.float32); V = np.full((kcap, D), np.nan, np.float32)
    Q[:nq] = rng.standard_normal((nq, D)); K[:nk] = rng.standard_normal((nk, D)); V[:nk] = rng.standard_normal((nk, D))
    if peaked:
        Q[:nq] *= 0.3; K[:nk] *= 0.3
        Q[:nq, 0] = np.array([peaked, -peaked, 0.0, peaked / 3])[np.arange(nq) % 4]
        K[:nk, 0] = np.linspace(-1.0, 1.0, nk) if nk > 1 else 1.0
        if spike_split is not None:
            ns = _lg_attention_splits(qcap, kcap)
            ntile = -(-nk // 32)
            t0 = ntile * spike_split // ns
            K[min(32 * t0 + 5, nk - 1), 0] = 3.0
    return dict(qcap=qcap, kcap=kcap, nq=nq, nk=nk, Q=Q, K=K, V=V)


def _check_attention(sides, res, scale, min_spread=None):
    worst, spread = 0.0, np.inf
    sc = float(np.float32(scale)) * LOG2E
    for s, (ns, O) in zip(sides, res):
        assert ns == _lg_attention_splits(s["qcap"], s["kcap"])
        nq, nk = s["nq"], s["nk"]
        assert _is_nan(O[nq:]), "rows past the live query count written"
        if nq == 0:
            continue
        if nk == 0:
            assert (O[:nq] == 0).all()
            continue
        Q, K, V = s["Q"][:nq].astype(np.float64), s["K"][:nk].astype(np.float64), s["V"][:nk].astype(np.float64)
        S2 = (Q @ K.T) * sc                                     # base-2 logits
        P = np.exp2(S2 - S2.max(1, keepdims=True))
        ref = (P / P.sum(1, keepdims=True)) @ V
        spread = min(spread, float((S2.max(1) - S2.min(1)).max()))
        E = (D + 4) * U * sc * (np.abs(Q) @ np.abs(K).T).max(1) + 2 * U * np.abs(S2).max(1)
        vmax = np.abs(V).max()
        ntile = -(-nk // 32)
        bar = 4 * math.log(2) * E * vmax + ((2 * nk + 3 * ntile + 32) * U + nk * 2.0 ** -126) * vmax
        err = np.abs(O[:nq].astype(np.float64) - ref).max(1)
        assert np.isfinite(O[:nq]).all()
        worst = max(worst, float((err / bar).max()))
    if min_spread is not None:
        assert spread >= min_spread, f"the case is not peaked enough: base-2 spread {spread:.1f}"
    return worst


# (nq, nk) of side 0 and side 1 (a cross-attention pair: side 1 attends from the other set), capacities, peaked
ATT_CASES = [
    ((1, 1), (1, 1), None),
    ((31, 33), (31, 33), None),
    ((32, 32), (64, 64), None),
    ((33, 64), (33, 64), 260.0),
    ((127, 128), (127, 128), None),
    ((129, 129), (129, 129), 260.0),
    ((257, 513), (257, 513), 260.0),
    ((513, 257), (513, 257), None),
]


@pytest.mark.parametrize("live,caps,peaked", ATT_CASES)
def test_attention_kernel(emu_bin, live, caps, peaked):
    """Flash attention with key splits (split count from the capacities, partials folded by the combine kernel) against a float64 softmax.  Bar: module docstring."""
    a, b = live
    ca, cb = caps
    rng = np.random.default_rng(a * 7 + b)
    scale = 1.0 / math.sqrt(D)
    sides = [_att_side(rng, ca, cb, a, b, peaked), _att_side(rng, cb, ca, b, a, peaked)]
    res = _attention(emu_bin, sides, scale)
    worst = _check_attention(sides, res, scale, 60.0 if peaked else None)
    print(f"{live} caps {caps} splits {[r[0] for r in res]}: max |err| / bar {worst:.3g}")
    assert worst <= 1.0


def _sparse_sides(rng):
    """live key counts far below the capacity: kcap 1024 -> 16 splits of which nk = 40 fills two tiles (14 empty splits), nk = 1 one (15 empty), nk = 0 all; the second
    pair of sides has different capacities (qcap 300 / kcap 100: one split, beside qcap 100 / kcap 600: nine, so smax > that side's nsplit)"""
    return [
        [_att_side(rng, 64, 1024, 50, 40, 260.0, spike_split=1), _att_side(rng, 100, 1024, 33, 1)],
        [_att_side(rng, 300, 100, 300, 70, 260.0), _att_side(rng, 100, 600, 97, 577, 260.0, spike_split=5)],
        [_att_side(rng, 64, 1024, 31, 0), _att_side(rng, 128, 1024, 128, 129)],
    ]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_attention_empty_splits_and_mixed_caps(emu_bin, which):
    rng = np.random.default_rng(11 + which)
    sides = _sparse_sides(rng)[which]
    scale = 1.0 / math.sqrt(D)
    res = _attention(emu_bin, sides, scale)
    ns = [r[0] for r in res]
    if which == 0:
        assert ns == [16, 16] and sides[0]["nk"] < 32 * 16
    if which == 1:
        assert ns[0] == 1 and ns[1] > 1
    worst = _check_attention(sides, res, scale)
    print(f"case {which} splits {ns}: max |err| / bar {worst:.3g}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# lg_dot_kernel, lg_prune_map_kernel, lg_gather_rows_kernel
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _prune(binary, sides, w, b, thr, min_kpts):
    blob = _i(3, len(sides)) + _f(thr) + _i(min_kpts) + _a(w) + _a([b])
    for s in sides:
        blob += _i(s["cap"], s["n"]) + _a(s["x"]) + _a(s["cs"]) + _a(s["sn"]) + _a(s["ind"], np.int32)
    o = _exe(binary, blob)
    res = []
    for s in sides:
        cap = s["cap"]
        r = dict(z=o.take(cap), map=o.take(cap, np.int32), n_out=int(o.take(1, np.int32)[0]), xo=o.take(cap * 192).reshape(cap, 192),
                 cso=o.take(cap * D).reshape(cap, D), sno=o.take(cap * D).reshape(cap, D), indo=o.take(cap, np.int32))
        res.append(r)
    o.done()
    return res


def _prune_side(rng, cap, n, bias_shift=0.0):
    x = np.full((cap, 192), np.nan, np.float32); x[:n] = rng.standard_normal((n, 192))
    cs = np.full((cap, D), np.nan, np.float32); cs[:n] = rng.standard_normal((n, D))
    sn = np.full((cap, D), np.nan, np.float32); sn[:n] = rng.standard_normal((n, D))
    ind = np.full(cap, -5, np.int32); ind[:n] = rng.permutation(10 * cap)[:n]
    return dict(cap=cap, n=n, x=x, cs=cs, sn=sn, ind=ind)


@pytest.mark.parametrize("shapes,bias,min_kpts", [
    ([(40, 33), (40, 40)], -2.5, 100),          # n <= min_kpts: nothing pruned
    ([(50, 47), (9, 1)], -40.0, -1),            # every row pruned: n_out = 0
    ([(2600, 2500), (1100, 1030)], -2.5, 64),   # n > 1024: rows removed on both sides of every 1024-row block boundary
    ([(3, 3), (64, 0)], -2.5, -1),
])
def test_dot_prune_gather(emu_bin, shapes, bias, min_kpts):
    """z = x[:, :96] . w + b (bar (96 + 2) u (|b| + sum |x w|)); rows with sigmoid(z) > 0.05 kept in order while the set holds more than min_kpts; the descriptor
    (x[:, :96]), cos and sin rows and the index list gathered.  The keep decision is exact wherever |z - logit(0.05)| exceeds the bound plus the fp32 sigmoid's (asserted to hold for every row)."""
    rng = np.random.default_rng(len(shapes) + shapes[0][0])
    w = (rng.standard_normal(96) / 4).astype(np.float32)
    sides = [_prune_side(rng, cap, n) for cap, n in shapes]
    thr = 0.05
    res = _prune(emu_bin, sides, w, np.float32(bias), thr, min_kpts)
    zthr = math.log(thr / (1 - thr))
    for s, r in zip(sides, res):
        n, cap = s["n"], s["cap"]
        x = s["x"][:n, :96].astype(np.float64)
        z = x @ w.astype(np.float64) + bias
        bar = 98 * U * (abs(bias) + np.abs(x) @ np.abs(w.astype(np.float64)))
        assert (np.abs(r["z"][:n] - z) <= bar).all() and _is_nan(r["z"][n:])
        assert (np.abs(z - zthr) > bar + 1e-5).all(), "a row sits on the threshold: change the seed"
        keep = np.arange(n) if n <= min_kpts else np.nonzero(z > zthr)[0]
        k = len(keep)
        assert r["n_out"] == k
        assert np.array_equal(r["map"][:k], keep) and (r["map"][k:] == -7).all()
        assert np.array_equal(r["xo"][:k, :96], s["x"][keep, :96]) and _is_nan(r["xo"][k:]) and _is_nan(r["xo"][:, 96:])      # (columns 96.. hold the message: scratch)
        assert np.array_equal(r["cso"][:k], s["cs"][keep]) and _is_nan(r["cso"][k:])
        assert np.array_equal(r["sno"][:k], s["sn"][keep]) and _is_nan(r["sno"][k:])
        assert np.array_equal(r["indo"][:k], s["ind"][keep]) and (r["indo"][k:] == -7).all()
        if n > 1024 and min_kpts < n:
            assert 0 < k < n and (keep // 1024 != np.arange(k) // 1024).any(), "no row moved across a block boundary"
        print(f"cap {cap} n {n}: kept {k}")


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# lg_transpose_kernel + linear_mfma_kernel: the similarity matrix
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap0,n0,cap1,n1", [(1, 1, 31, 31), (300, 257, 33, 32), (64, 63, 64, 33), (40, 40, 100, 65), (260, 259, 130, 129), (5, 5, 70, 64)])
def test_transpose_and_similarity(emu_bin, cap0, n0, cap1, n1):
    """md1^T with zeros past the live count up to n1pad; sim = md0 md1^T (bar (96 + 2) u sum |a b|), zeros in the padding columns, rows past n0 untouched."""
    rng = np.random.default_rng(cap0 + n1)
    md0 = np.full((cap0, D), np.nan, np.float32); md0[:n0] = rng.standard_normal((n0, D))
    md1 = np.full((cap1, D), np.nan, np.float32); md1[:n1] = rng.standard_normal((n1, D))
    o = _exe(emu_bin, _i(4, cap0, n0, cap1, n1) + _a(md0) + _a(md1))
    npad = (cap1 + 63) // 64 * 64
    t, sim = o.take(D * npad).reshape(D, npad), o.take(cap0 * npad).reshape(cap0, npad)
    o.done()
    assert np.array_equal(t[:, :n1], md1[:n1].T) and (t[:, n1:] == 0).all()
    a, b = md0[:n0].astype(np.float64), md1[:n1].astype(np.float64)
    ref, bar = a @ b.T, 98 * U * (np.abs(a) @ np.abs(b).T)
    assert (np.abs(sim[:n0, :n1] - ref) <= bar).all()
    assert (sim[:n0, n1:] == 0).all() and _is_nan(sim[n0:])


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# the assignment: logsigmoid, row / column LSE, row / column best, mutual filter
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _assign(binary, sim, z0, z1, cap0, n0, cap1, n1, thr, ind0, ind1):
    npad = (cap1 + 63) // 64 * 64
    S = np.full((cap0, npad), np.nan, np.float32); S[:n0, :n1] = sim
    Z0 = np.full(cap0, np.nan, np.float32); Z0[:n0] = z0
    Z1 = np.full(npad, np.nan, np.float32); Z1[:n1] = z1
    o = _exe(binary, _i(5, cap0, n0, cap1, n1) + _f(thr) + _a(S) + _a(Z0) + _a(Z1) + _a(ind0, np.int32) + _a(ind1, np.int32))
    r = dict(z0=o.take(cap0), z1=o.take(npad), rlse=o.take(cap0), clse=o.take(npad), m0=o.take(cap0, np.int32), m1=o.take(npad, np.int32), best0=o.take(cap0),
             matches=o.take(2 * cap0, np.int64).reshape(cap0, 2), scores=o.take(cap0), n_out=int(o.take(1, np.int32)[0]))
    o.done()
    return r


def _logsigmoid(z):
    return np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z)))


def _lse(a, axis):
    m = a.max(axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis, keepdims=True))).squeeze(axis)


def _first_best(S, E, axis):
    """first index of the maximum along `axis` where it is decided: the best value beats every value not EXACTLY equal to it by more than 2 E; -2 where undecided"""
    Sm = np.moveaxis(S, axis, -1)
    out = np.full(Sm.shape[0], -2)
    for i in range(Sm.shape[0]):
        row = Sm[i]
        best = row.max()
        tied = np.nonzero(row == best)[0]
        rest = row[row != best]
        if rest.size == 0 or best - rest.max() > 2 * E:
            out[i] = tied[0]
    return out


def _assign_case(rng, n0, n1, dup=True):
    sim = (3.0 * rng.standard_normal((n0, n1))).astype(np.float32)
    z0 = rng.standard_normal(n0).astype(np.float32) + 1.0
    z1 = rng.standard_normal(n1).astype(np.float32) + 1.0
    if dup and n1 >= 3:        # exact duplicates: columns 1 == 2 (one lane's float4) == n1 - 1 (another lane's, when n1 > 4), with their z; rows 0 == n0 - 1
        if n0:
            sim[0, 1] = sim.max() + 5.0                  # row 0 (duplicated too) and the duplicated columns are each other's best
        sim[:, 2] = sim[:, 1]; z1[2] = z1[1]
        sim[:, n1 - 1] = sim[:, 1]; z1[n1 - 1] = z1[1]
    if dup and n0 >= 3:
        sim[n0 - 1] = sim[0]; z0[n0 - 1] = z0[0]
    return sim, z0, z1


def _check_assign(sim, z0, z1, n0, n1, cap0, cap1, thr, ind0, ind1, r):
    npad = (cap1 + 63) // 64 * 64
    assert r["n_out"] >= 0
    assert _is_nan(r["z0"][n0:]) and _is_nan(r["z1"][n1:]) and _is_nan(r["rlse"][n0:]) and _is_nan(r["clse"][n1:]) and _is_nan(r["best0"][n0:])
    assert (r["m0"][n0:] == -7).all() and (r["m1"][n1:] == -7).all()
    n = r["n_out"]
    assert (r["matches"][n:] == -7).all() and _is_nan(r["scores"][n:])
    ls0, ls1 = _logsigmoid(z0.astype(np.float64)), _logsigmoid(z1.astype(np.float64))
    els0, els1 = 8 * U * (1 + np.abs(ls0)), 8 * U * (1 + np.abs(ls1))
    assert (np.abs(r["z0"][:n0] - ls0) <= els0).all() and (np.abs(r["z1"][:n1] - ls1) <= els1).all()
    if n1 == 0:
        assert (r["m0"][:n0] == -1).all() and n == 0
        return 0
    if n0 == 0:
        assert (r["m1"][:n1] == -1).all() and n == 0
        return 0
    s = sim.astype(np.float64)
    rl, cl = _lse(s, 1), _lse(s, 0)
    erl, ecl = (n1 + 4) * U + 2 * U * np.abs(rl), (n0 + 4) * U + 2 * U * np.abs(cl)
    assert (np.abs(r["rlse"][:n0] - rl) <= erl).all() and (np.abs(r["clse"][:n1] - cl) <= ecl).all()
    score = (s - rl[:, None]) + (s - cl[None, :]) + (ls0[:, None] + ls1[None, :])
    E = float(erl.max() + ecl.max() + els0.max() + els1.max() + 4 * U * (2 * np.abs(s).max() + np.abs(rl).max() + np.abs(cl).max() + np.abs(ls0).max() + np.abs(ls1).max()))
    m0, m1 = _first_best(score, E, 1), _first_best(score, E, 0)
    assert (m0 >= 0).all() and (m1 >= 0).all(), "undecided arg-max: change the seed"
    assert np.array_equal(r["m0"][:n0], m0) and np.array_equal(r["m1"][:n1], m1)
    best = score[np.arange(n0), m0]
    assert (np.abs(r["best0"][:n0] - best) <= E).all()
    mutual = m1[m0] == np.arange(n0)
    sc = np.exp(best)
    assert (np.abs(sc - thr) > 2 * E * sc + 1e-6).all(), "a score sits on the threshold: change the seed"
    keep = np.nonzero(mutual & (sc > thr))[0]
    assert n == len(keep)
    assert np.array_equal(r["matches"][:n, 0], ind0[keep]) and np.array_equal(r["matches"][:n, 1], ind1[m0[keep]])
    assert (np.abs(r["scores"][:n] - sc[keep]) <= 2 * E * sc[keep] + 2 * U).all()
    return n


ASSIGN_CASES = [(5, 5, 1, 1), (7, 9, 2, 2), (13, 20, 3, 70), (15, 15, 4, 4), (3, 3, 5, 5), (20, 20, 63, 63), (9, 16, 64, 64), (40, 40, 65, 65), (10, 10, 0, 4), (0, 4, 6, 6), (1100, 1100, 5, 9)]


@pytest.mark.parametrize("n0,cap0,n1,cap1", ASSIGN_CASES)
def test_assignment_kernels(emu_bin, n0, cap0, n1, cap1):
    """logsigmoid, row / column LSE (16 row slices: n0 < 16 leaves slices empty), row / column best with the first-index tie rule on exactly duplicated rows and columns, the
    mutual filter and its ordered compaction.  Bars: module docstring."""
    rng = np.random.default_rng(n0 * 100 + n1)
    sim, z0, z1 = _assign_case(rng, n0, n1)
    ind0 = np.full(cap0, -3, np.int32); ind0[:n0] = rng.permutation(5 * cap0 + 5)[:n0]
    ind1 = np.full(cap1, -3, np.int32); ind1[:n1] = rng.permutation(5 * cap1 + 5)[:n1]
    thr = 0.02
    r = _assign(emu_bin, sim, z0, z1, cap0, n0, cap1, n1, thr, ind0, ind1)
    n = _check_assign(sim, z0, z1, n0, n1, cap0, cap1, thr, ind0, ind1, r)
    if n1 >= 3 and n0 >= 1:
        assert r["m0"][0] == 1 and not np.isin(r["m0"][:n0], [2, n1 - 1]).any()      # the first of identical columns, never a later one
    if n0 >= 3 and n1 >= 1:
        assert (n1 < 3 or r["m1"][1] == 0) and (r["m1"][:n1] != n0 - 1).all()
    print(f"n0 {n0}/{cap0} n1 {n1}/{cap1}: {n} matches")


def _mutual(binary, m0, m1, best0, ind0, ind1, n0, thr):
    cap0, npad = len(m0), len(m1)
    o = _exe(binary, _i(6, cap0, n0, npad) + _f(thr) + _a(m0, np.int32) + _a(m1, np.int32) + _a(best0) + _a(ind0, np.int32) + _a(ind1, np.int32))
    r = o.take(2 * cap0, np.int64).reshape(cap0, 2), o.take(cap0), int(o.take(1, np.int32)[0])
    o.done()
    return r


def test_mutual_ordered_compaction_and_strict_threshold(emu_bin):
    """n0 = 2100 (three 1024-row blocks): the match list stays in ascending row order; a match whose exp(score) equals the threshold EXACTLY is dropped (strict >)."""
    rng = np.random.default_rng(3)
    n0, cap0, n1, npad = 2100, 2110, 1500, 1536
    m0 = np.full(cap0, -9, np.int32); m0[:n0] = rng.integers(-1, n1, n0)
    m1 = np.full(npad, -9, np.int32); m1[:n1] = rng.integers(-1, n0, n1)
    for i in rng.choice(n0, 900, replace=False):         # make many pairs mutual
        if m0[i] >= 0:
            m1[m0[i]] = i
    best0 = np.full(cap0, np.nan, np.float32); best0[:n0] = rng.uniform(-6, 0, n0)
    ind0 = np.full(cap0, -9, np.int32); ind0[:n0] = rng.permutation(10 ** 6)[:n0]
    ind1 = np.full(npad, -9, np.int32); ind1[:n1] = rng.permutation(10 ** 6)[:n1]
    mutual = np.array([m0[i] >= 0 and m1[m0[i]] == i for i in range(n0)])
    mt, sc, n = _mutual(emu_bin, m0, m1, best0, ind0, ind1, n0, 0.0)
    keep = np.nonzero(mutual)[0]
    assert n == len(keep) and keep.max() > 2048
    assert np.array_equal(mt[:n, 0], ind0[keep]) and np.array_equal(mt[:n, 1], ind1[m0[keep]]) and (mt[n:] == -7).all() and _is_nan(sc[n:])
    assert np.allclose(sc[:n], np.exp(best0[keep].astype(np.float64)), rtol=4 * U, atol=0)
    thr = sc[n // 2]            # the kernel's own fp32 exp of one match's score
    mt2, sc2, n2 = _mutual(emu_bin, m0, m1, best0, ind0, ind1, n0, float(thr))
    want = sc[:n] > thr
    assert n2 == int(want.sum()) and np.array_equal(mt2[:n2], mt[:n][want]) and np.array_equal(sc2[:n2], sc[:n][want])
    assert not (sc2[:n2] == thr).any()


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# negative controls: the same comparisons fail on subtly wrong kernels
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _mutant(old, new):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    return _build(lambda k: _must_sub(k, old, new))


def test_control_rescale_skipped_after_the_first_tile():
    """A stale running maximum is harmless in exact arithmetic (numerator and denominator share the scale); it shows once the maximum grows by more than 128 (base 2)
    after the first tile: the un-rescaled exponentials overflow."""
    b = _mutant("if (__any(mnew != mrun)) {", "if (t == t_begin && __any(mnew != mrun)) {")
    rng = np.random.default_rng(1)
    scale = 1.0 / math.sqrt(D)
    sides = [_att_side(rng, 33, 64, 33, 64, 1000.0), _att_side(rng, 64, 1024, 64, 600, 1000.0, spike_split=3)]
    res = _attention(b, sides, scale)
    with pytest.raises(AssertionError):
        assert _check_attention(sides, res, scale) <= 1.0


def test_control_ragged_tile_mask_removed():
    b = _mutant("s[r] = -INFINITY;", "s[r] = s[r];")
    rng = np.random.default_rng(2)
    scale = 1.0 / math.sqrt(D)
    sides = [_att_side(rng, 31, 33, 31, 33), _att_side(rng, 33, 31, 33, 31)]
    res = _attention(b, sides, scale)
    with pytest.raises(AssertionError):
        assert _check_attention(sides, res, scale) <= 1.0


def test_control_combine_without_the_empty_slice_skip():
    b = _mutant("if (ms == -INFINITY) continue;", "")
    rng = np.random.default_rng(13)
    scale = 1.0 / math.sqrt(D)
    sides = _sparse_sides(rng)[2]                      # a side with nk = 0 over 16 splits
    with pytest.raises(AssertionError):
        _check_attention(sides, _attention(b, sides, scale), scale)


def test_control_row_best_ties_to_the_last_index():
    b = _mutant("if (j + e < n1 && v > bv)", "if (j + e < n1 && v >= bv)")
    rng = np.random.default_rng(40 * 100 + 65)
    n0, cap0, n1, cap1 = 40, 40, 65, 65
    sim, z0, z1 = _assign_case(rng, n0, n1)
    ind0 = np.arange(cap0, dtype=np.int32); ind1 = np.arange(cap1, dtype=np.int32)
    r = _assign(b, sim, z0, z1, cap0, n0, cap1, n1, 0.02, ind0, ind1)
    with pytest.raises(AssertionError):
        _check_assign(sim, z0, z1, n0, n1, cap0, cap1, 0.02, ind0, ind1, r)


def test_control_one_pass_variance():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    K, N, W, bias, sides, gamma, beta = _ln_large_mean_case(np.random.default_rng(5))
    src = _slice()
    assert "var * (1.f / 192.f) + 1e-5f" in src
    b2 = _build(lambda k: _must_sub(_must_sub(k, "const float d = acc[r] - mean; q += d * d;", "q += acc[r] * acc[r];"),
                                    "var * (1.f / 192.f) + 1e-5f", "fmaxf(var * (1.f / 192.f) - mean * mean, 0.f) + 1e-5f"))
    ys = _linear(b2, K, N, LNGELU, W, bias, sides, gamma, beta)
    with pytest.raises(AssertionError):
        assert _check_linear(K, N, LNGELU, W, bias, sides, ys, gamma, beta, exact_pre=True) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
# the same driver under AddressSanitizer (host code only): the capacity edges, where the min(row, n - 1) clamps and the n1pad-sized arrays keep every read in bounds
# ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_edges_under_address_sanitizer():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang")
    try:
        b = _build(flags=("-fsanitize=address", "-fno-omit-frame-pointer", "-g"))
    except subprocess.CalledProcessError as e:
        pytest.skip(f"no AddressSanitizer build here: {e}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    probe = subprocess.run([b], input=_i(0, 1) + _f(64, 48) + _a(np.zeros(2)) + _a(np.zeros(96)), capture_output=True, timeout=120, env=env)
    if probe.returncode != 0 and b"AddressSanitizer" in probe.stderr and b"ERROR" not in probe.stderr:
        pytest.skip("the AddressSanitizer runtime did not start: " + probe.stderr.decode(errors="replace")[-500:])
    assert probe.returncode == 0, probe.stderr.decode(errors="replace")[-3000:]
    rng = np.random.default_rng(77)
    # lg_linear: cap % 32 != 0, one-row sets
    for K, N, epi, shapes in ((96, 288, ROTARY, [(1, 1), (33, 33)]), (192, 192, LNGELU, [(31, 31), (1, 1)]), (192, 96, RESIDUAL, [(65, 65), (2, 3)])):
        W = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32); bb = (0.1 * rng.standard_normal(N)).astype(np.float32)
        sides = [_rand_side(rng, cap, live, K, N, K, N, epi) for live, cap in shapes]
        ys = _linear(b, K, N, epi, W, bb, sides, env=env)
        assert _check_linear(K, N, epi, W, bb, sides, ys) <= 1.0
    # attention: one-row sets, cap % 32 != 0, split edges
    scale = 1.0 / math.sqrt(D)
    for sides in ([_att_side(rng, 1, 1, 1, 1), _att_side(rng, 1, 1, 1, 1)], [_att_side(rng, 33, 129, 33, 129), _att_side(rng, 129, 33, 129, 33)]):
        assert _check_attention(sides, _attention(b, sides, scale, env=env), scale) <= 1.0
    # similarity matrix and assignment at n1pad edges
    for cap0, n0, cap1, n1 in ((1, 1, 1, 1), (33, 33, 64, 64), (2, 2, 65, 65)):
        md0 = rng.standard_normal((cap0, D)).astype(np.float32); md1 = rng.standard_normal((cap1, D)).astype(np.float32)
        _exe(b, _i(4, cap0, n0, cap1, n1) + _a(md0) + _a(md1), env)
    for n0, cap0, n1, cap1 in ((1, 1, 1, 1), (17, 17, 64, 64), (3, 3, 65, 65), (1, 1, 63, 63)):
        sim, z0, z1 = _assign_case(rng, n0, n1)
        ind0 = np.arange(cap0, dtype=np.int32); ind1 = np.arange(cap1, dtype=np.int32)
        npad = (cap1 + 63) // 64 * 64
        S = np.zeros((cap0, npad), np.float32); S[:n0, :n1] = sim
        Z1 = np.zeros(npad, np.float32); Z1[:n1] = z1
        _exe(b, _i(5, cap0, n0, cap1, n1) + _f(0.02) + _a(S) + _a(z0) + _a(Z1) + _a(ind0, np.int32) + _a(ind1, np.int32), env)
    # pruning: one-row sets, cap % 32 != 0
    sides = [_prune_side(rng, 1, 1), _prune_side(rng, 33, 33)]
    blob = _i(3, 2) + _f(0.05) + _i(-1) + _a(rng.standard_normal(96)) + _a([0.0])
    for s in sides:
        blob += _i(s["cap"], s["n"]) + _a(s["x"]) + _a(s["cs"]) + _a(s["sn"]) + _a(s["ind"], np.int32)
    _exe(b, blob, env)

