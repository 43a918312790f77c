"""What the camera tests share that is not specification (that is tests/cameras_reference.py): the cameras, the point and image cases, the
emulation's driver, the comparison rules.

The rules: pinhole and Brown outputs equal the restatement bit for bit (only + - * / sqrt floor, correctly rounded everywhere).  The fisheye
branch calls atan and tan, which differ between numpy, the host's libm and the device's by a few fp64 ulp: about 1e-10 px at f <= 4000, which
can only move the final rounding to fp32, so a fisheye coordinate is within ONE fp32 spacing of the expected one, with equal status (the
test points stay away from the theta = 1.5 threshold)."""
import subprocess

import numpy as np

import cameras_reference as CR

# (k1, k2, p1, p2): the sets whose Newton inverse was checked on a 640 x 480 grid at f = 500, and one fisheye (k1..k4)
BROWN_SETS = ((-0.12, 0.0, 0.0, 0.0), (0.08, 0.0, 0.0, 0.0), (-0.28, 0.07, 0.0, 0.0), (-0.25, 0.08, 1e-3, -5e-4), (-0.35, 0.12, 0.0, 0.0))
FISHEYE_SET = (-0.03, 0.006, -0.002, 0.0003)
# (kind, d0..d3, r_d): models far from any lens on which Newton wanders for 32 iterations -- status NOT_CONVERGED.  (The iterations use only
# + - * /, so the wandering is the same on every machine.)
NOT_CONVERGING = ((1, (-38.0, -73.0, 0.0, 0.0), 0.64), (2, (-0.25, 11.75, -20.36, 0.0), 0.646))
WIDTH, HEIGHT = 640, 480
KS = (1, 63, 64, 65, 257)                     # rows of a point table: below, at and above a wave, more than one workgroup


def brown_camera(i, f=500.0, w=WIDTH, h=HEIGHT):
    return {"model": "OPENCV", "width": w, "height": h, "params": [f, f * 1.01, w / 2 + 3.0, h / 2 - 2.0, *BROWN_SETS[i]]}


def fisheye_camera(f=320.0, w=WIDTH, h=HEIGHT):
    return {"model": "OPENCV_FISHEYE", "width": w, "height": h, "params": [f, f * 0.99, w / 2 - 1.5, h / 2 + 2.5, *FISHEYE_SET]}


def pinhole_camera(f=480.0, w=WIDTH, h=HEIGHT):
    return {"model": "PINHOLE", "width": w, "height": h, "params": [f, f + 7.0, w / 2 + 0.5, h / 2 - 0.25]}


def packed(cams):
    """kind (C,) int32, params (C,12) float64 of a list of camera dicts."""
    ks, ps = zip(*(CR.pack(c) for c in cams))
    return np.array(ks, np.int32), np.stack(ps)


def cameras_for(family, n):
    """n cameras of a family: 'brown' cycles through BROWN_SETS, 'pinhole' and 'fisheye' vary the focal length."""
    if family == "brown":
        return [brown_camera(i % len(BROWN_SETS), 500.0 + 20.0 * i) for i in range(n)]
    if family == "fisheye":
        return [fisheye_camera(320.0 + 15.0 * i) for i in range(n)]
    return [pinhole_camera(480.0 + 30.0 * i) for i in range(n)]


def points_case(seed, P, K, family, shared, ragged=True, bad_rows=True, bad_camera=False, other=False):
    """A batch for xfh_camera_points: pts (P,K,2) float32 inside the image, counts (ragged, the first image 0 when P > 1, the last K), NaN and
    Inf rows, optionally an unusable camera (the last) and a K_other."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, WIDTH, (P, K)), rng.uniform(0, HEIGHT, (P, K))], axis=2).astype(np.float32)
    counts = None
    if ragged:
        counts = rng.integers(0, K + 1, P).astype(np.int32)
        counts[-1] = K
        if P > 1:
            counts[0] = 0
        if P > 2:
            counts[1] = K + 5                                  # read clamped
    if bad_rows and K >= 4:
        pts[-1, 1, 0], pts[-1, 2, 1], pts[-1, 3, 0] = np.nan, np.inf, -np.inf
    kind, params = packed(cameras_for(family, 1 if shared else P))
    if bad_camera:
        params[-1, rng.integers(0, 12)] = np.nan
    k_other = None
    if other:
        k_other = np.stack([np.array([430.0 + 10 * c, 445.0, 300.0 + c, 250.0]) for c in range(len(kind))])
    return dict(pts=pts, counts=counts, kind=kind, params=params, k_other=k_other)


def image_case(seed, B, C, H, W, dtype, family, shared=False):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (B, C, H, W)).astype(np.uint8) if dtype == np.uint8 else rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32)
    if dtype != np.uint8:
        src.flat[0], src.flat[-1] = -1.0, 1.0                  # the range is [-1, 1] at every shape
    cams = []
    for c in range(1 if shared else B):                        # cameras of the image's own size: the principal point near its centre
        cam = cameras_for(family, c + 1)[c]
        cam = dict(cam, width=W, height=H, params=[max(W, H) * 0.8, max(W, H) * 0.8 + 0.5, W / 2 + 0.25, H / 2 - 0.25, *cam["params"][4:]])
        cams.append(cam)
    kind, params = packed(cams)
    return dict(src=src, kind=kind, params=params)


def not_converging_case():
    """Two images, one per model of NOT_CONVERGING: the row that does not converge and the principal point."""
    kind = np.array([k for k, _, _ in NOT_CONVERGING], np.int32)
    params = np.zeros((2, 12))
    params[:, :4] = [400.0, 400.0, 320.0, 240.0]
    pts = np.zeros((2, 2, 2), np.float32)
    for i, (_, d, rd) in enumerate(NOT_CONVERGING):
        params[i, 4:8] = d
        pts[i] = [[320.0 + 400.0 * rd, 240.0], [320.0, 240.0]]
    return dict(pts=pts, counts=None, kind=kind, params=params, k_other=None)


def run_points(binary, c, direction):
    P, K = c["pts"].shape[:2]
    nc = len(c["kind"])
    blob = np.array([0, P, K, nc, int(c["counts"] is not None), int(c["k_other"] is not None), direction], np.int32).tobytes()
    blob += c["pts"].astype(np.float32).tobytes() + (c["counts"].astype(np.int32).tobytes() if c["counts"] is not None else b"")
    blob += c["kind"].astype(np.int32).tobytes() + c["params"].astype(np.float64).tobytes()
    blob += c["k_other"].astype(np.float64).tobytes() if c["k_other"] is not None else b""
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-2000:])
    n = P * K
    assert len(r.stdout) == n * 9
    return np.frombuffer(r.stdout[:n * 8], np.float32).reshape(P, K, 2), np.frombuffer(r.stdout[n * 8:], np.uint8).reshape(P, K)


def run_images(binary, c, k_new, Ho, Wo, fill, with_valid):
    src = c["src"]
    B, C, H, W = src.shape
    nc = len(c["kind"])
    blob = np.array([1, int(src.dtype == np.float32), B, C, H, W, nc, int(k_new is not None), Ho, Wo, int(with_valid)], np.int32).tobytes()
    blob += np.array([fill], np.float64).tobytes() + src.tobytes() + c["kind"].astype(np.int32).tobytes() + c["params"].astype(np.float64).tobytes()
    blob += np.asarray(k_new, np.float64).tobytes() if k_new is not None else b""
    r = subprocess.run([binary], input=blob, capture_output=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode()[-2000:])
    nd = B * C * Ho * Wo * src.dtype.itemsize
    assert len(r.stdout) == nd + (B * Ho * Wo if with_valid else 0)
    dst = np.frombuffer(r.stdout[:nd], src.dtype).reshape(B, C, Ho, Wo)
    return dst, (np.frombuffer(r.stdout[nd:], np.uint8).reshape(B, Ho, Wo) if with_valid else None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_points(got, want, fisheye):
    """(out, status) of a kernel against camera_points' (out, status, exact) by the rules above."""
    out, status = got
    w_out, w_status = want[0], want[1]
    assert status.dtype == np.uint8 and np.array_equal(status, w_status), (status[status != w_status][:8], w_status[status != w_status][:8])
    if not fisheye:
        assert same_bits(out, w_out)
        return
    nan = np.isnan(w_out)
    assert np.array_equal(np.isnan(out), nan) and np.array_equal(nan[..., 0], w_status != 0)
    assert same_bits(out[nan], w_out[nan])                     # one NaN pattern
    assert (np.abs(out[~nan].astype(np.float64) - w_out[~nan].astype(np.float64)) <= np.spacing(np.abs(w_out[~nan])).astype(np.float64)).all()


def check_fisheye_f32(dst, exact, src, fill):
    """A rectified fp32 fisheye image against the unrounded restatement: 2^-22 (max - min of src) -- half an fp32 ulp of rounding at values
    within the source's range (`fill` must lie in it), plus a coordinate term nine orders smaller, times four."""
    lo, hi = float(src.min()), float(src.max())
    assert lo <= fill <= hi
    assert np.abs(dst.astype(np.float64) - exact).max() <= 2.0 ** -22 * (hi - lo)


def check_fisheye_u8(dst, want, exact):
    """A rectified uint8 fisheye image: equal to the restatement except where the unrounded value is within 1e-6 of a rounding boundary
    (n + 0.5), where the ~1e-10 px of the coordinates may round it either way."""
    differ = dst != want
    assert (np.abs(dst.astype(np.int32) - want.astype(np.int32))[differ] <= 1).all()
    assert (np.abs(exact[differ] + 0.5 - np.round(exact[differ] + 0.5)) < 1e-6).all()


def new_k(c, scale=0.9):
    """A K_new per camera: a slightly shorter focal length and a shifted centre."""
    p = c["params"]
    return np.stack([p[:, 0] * scale, p[:, 1] * scale, p[:, 2] + 0.5, p[:, 3] - 0.75], axis=1)


# ---- the end-to-end scene: a synthetic two-view scene of twoview_support seen through distorting cameras --------------------------------------
E2E = dict(pair=3, n=400, noise=0.5, outliers=0.2, seed=24, max_iterations=1000, pose_seed=3)
E2E_MODELS = {"brown": ("OPENCV", (-0.28, 0.07, 0.0, 0.0)), "fisheye": ("OPENCV_FISHEYE", FISHEYE_SET)}


def distorted_scene(which):
    """The correspondences of twoview_support.scene(E2E) as the raw pixels of two cameras with the scene's fx, fy, cx, cy and the distortion
    `which` of E2E_MODELS (the float64 forward model of the restatement, rounded to fp32 like a detector's output).
    -> raw0, raw1 (n, 2) float32, the two camera dicts, K0, K1, T_0to1, and the undistorted observations."""
    import twoview_support as TS
    p0, p1, _, K0, K1, T = TS.scene(E2E["pair"], E2E["n"], E2E["noise"], E2E["outliers"], E2E["seed"])
    model, d = E2E_MODELS[which]
    cams, raws = [], []
    for p, K in ((p0, K0), (p1, K1)):
        cam = {"model": model, "width": 0, "height": 0, "params": [K[0, 0], K[1, 1], K[0, 2], K[1, 2], *d]}
        kind, params = packed([cam])
        raws.append(CR.camera_points(p[None], None, kind, params, None, 1)[2][0].astype(np.float32))
        cams.append(cam)
    return raws[0], raws[1], cams[0], cams[1], K0, K1, T, (p0, p1)


def restatement_chain(raw0, raw1, cam0, cam1, K0, K1):
    """cameras_reference undistortion, the rows whose status is not 0 dropped, then pose_reference.estimate with E2E's seed."""
    import pose_reference as PR
    und = []
    for raw, cam in ((raw0, cam0), (raw1, cam1)):
        kind, params = packed([cam])
        out, st, _ = CR.camera_points(raw[None], None, kind, params, None, 0)
        und.append((out[0], st[0]))
    keep = (und[0][1] == 0) & (und[1][1] == 0)
    return PR.estimate(und[0][0][keep], und[1][0][keep], K0, K1, 1.0, max_iterations=E2E["max_iterations"], seed=E2E["pose_seed"]), keep
