"""The views-solver slice of csrc/k_triangulate.hip (behind the two-view solver slice of the same file and the shared geometry of
csrc/twoview_math.hpp) compiled for the HOST (tests/emu/multiview_emu.cpp, fp contraction off) against the numpy restatement
tests/multiview_reference.py: on several thousand tracks of mixed kinds (tests/multiview_support.mixed_scene: holes in the table, NaN pixels,
a view with a pose that is not finite, a zero-baseline view, views behind the point, far points, outliers; V in {2, 3, 8, 32}) the points and
errors (as float32 bits), the status, the inlier mask and count, the winner, the score and the refit's costs must be equal bit for bit."""
import math
import subprocess

import numpy as np
import pytest

import multiview_reference as MR
import multiview_support as MS
import twoview_support as TS

BEGIN, END = "// ---- views solver begin", "// ---- views solver end"


def _slice():
    two = TS.slice_solver("k_triangulate.hip", "// ---- solver begin", "// ---- solver end")
    _, views = TS._between("k_triangulate.hip", BEGIN, END)
    assert "__shared__" not in views and "asm" not in views and "__builtin_amdgcn" not in views
    return two + views.replace("__device__ ", "")


@pytest.fixture(scope="module")
def emu_bin():
    return TS.build_emu("multiview_slice.hpp", "multiview_emu", _slice())


def test_the_slice_is_what_the_issue_asks_of_the_device_code():
    text = open(TS.CSRC + "/k_triangulate.hip").read()
    _, views = TS._between("k_triangulate.hip", BEGIN, END)
    assert "#pragma clang fp contract(off)" in text and text.index("#pragma clang fp contract(off)") < text.index(BEGIN)
    for word in ("sin(", "cos(", "acos(", "atan", "pow(", "exp(", "log("):
        assert word not in views, word
    # the two-view functions are called, not duplicated
    for name in ("tg_correct(", "tg_depths(", "tg_depth_status(", "tg_pose_E("):
        assert name in views and ("inline TgRays " + name not in views) and ("void " + name not in views) and ("int " + name not in views), name
    assert text.index("// ---- solver end") < text.index(BEGIN) < text.index(END)


def _record(sc, V, m):
    cam = np.concatenate([np.concatenate([sc["Rs"][v].reshape(9), sc["ts"][v], sc["Ks"][v].reshape(9)]) for v in range(V)])
    t = sc["tracks"]
    kcap = sc["kpts"].shape[1]
    inr = (t >= 0) & (t < kcap)
    px = sc["kpts"].astype(np.float64)[np.arange(V)[None, :], np.where(inr, t, 0)]         # (m, V, 2)
    obs = np.concatenate([np.where(inr[..., None], px, 0.0), inr[..., None].astype(np.float64)], axis=2)
    thr2, cos_min = sc["thr"] * sc["thr"], math.cos(math.radians(sc["deg"]))
    return np.concatenate([[V, sc["n_views"], m, sc["min_views"], thr2, cos_min, sc["max_depth"]], cam, obs.reshape(-1)])


def test_tracks_equal_the_restatement_bit_for_bit(emu_bin):
    rng = np.random.default_rng(2026)
    G = 96                                                 # 8 kinds x 4 view counts x 3 rounds
    scenes = []
    for g in range(G):
        V = MS.MIXED_V[g % 4]
        sc = MS.mixed_scene(rng, g, 40 if V == 32 else 100)
        if g % 7 == 3 and V > 2:
            sc["n_views"] = V - 1                          # a scene that uses fewer views than the call holds
        scenes.append(sc)
    blob = np.array([G], np.int32).tobytes() + b"".join(_record(sc, sc["Rs"].shape[0], sc["tracks"].shape[0]).astype(np.float64).tobytes() for sc in scenes)
    out = subprocess.run([emu_bin], input=blob, capture_output=True, check=True, timeout=600).stdout
    H = sum(sc["tracks"].shape[0] for sc in scenes)
    assert H == 8160 and len(out) == H * (16 + 16 + 24)
    iv = np.frombuffer(out[:16 * H], np.int32).reshape(H, 4)
    fv = np.frombuffer(out[16 * H:32 * H], np.uint32).reshape(H, 4)
    dv = np.frombuffer(out[32 * H:], np.uint64).reshape(H, 3)
    seen, moved, a = np.zeros(7, int), 0, 0
    for g, sc in enumerate(scenes):
        m = sc["tracks"].shape[0]
        w = MR.triangulate_views(sc["kpts"], sc["tracks"], sc["n_views"], sc["Ks"], sc["Rs"], sc["ts"], sc["thr"], sc["deg"], sc["max_depth"], sc["min_views"])
        s = slice(a, a + m)
        a += m
        assert np.array_equal(iv[s, 0], w["status"]), (g, np.nonzero(iv[s, 0] != w["status"])[0][:5])
        assert np.array_equal(iv[s, 1], w["n_inliers"]) and np.array_equal(iv[s, 2], w["inlier_views"]), g
        assert np.array_equal(iv[s, 3], w["winner"]), g
        for got, want in ((fv[s, :3], w["points3d"]), (fv[s, 3], w["reproj_error"])):
            nan = np.isnan(got.view(np.float32)) & np.isnan(want)
            assert np.array_equal(got[~nan], want.view(np.uint32)[~nan]), g
        want = np.stack([w["score"], w["cost0"], w["cost1"]], axis=1)
        assert np.array_equal(dv[s], want.view(np.uint64)), (g, np.nonzero(dv[s] != want.view(np.uint64))[0][:5])
        assert (np.isnan(w["points3d"]).all(axis=1) == (w["status"] != 0)).all() and np.isfinite(w["points3d"][w["status"] == 0]).all()
        assert (np.isnan(w["reproj_error"]) == ((w["status"] == 1) | (w["status"] == 2))).all()
        seen += np.bincount(w["status"], minlength=7)
        moved += int((w["cost1"] < w["cost0"]).sum())
    assert (seen > 100).all(), seen                        # every status is exercised
    assert seen[0] > 3000 and moved > 3000
