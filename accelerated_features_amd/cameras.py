"""Camera models on MI355X: the front end that lets images with lens distortion into the geometry of this package.

Every geometric entry here takes PINHOLE intrinsics.  ``undistort_keypoints`` turns the raw pixels of a COLMAP / poselib camera
(SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE) into pixels of an ideal pinhole camera -- by default the one with the
camera's own fx, fy, cx, cy, so that pixel thresholds still mean pixels -- which the estimators, the triangulation, the pose graph, the bundle
adjustment and the localisation consume unchanged; ``distort_keypoints`` is the way back (a projection into the raw image).
``undistort_images`` is ``cv2.undistort`` for a batch: strongly distorted frames are rectified before detection, since XFeat was trained on
perspective images.  ``estimate_relative_pose`` / ``estimate_absolute_pose`` have poselib's call shape for any of the models: both sides are
undistorted, the rows without a pinhole image are dropped and the PINHOLE wrappers of ``pose`` / ``absolute_pose`` do the rest.
The kernels behind ``xfh_camera_points`` / ``xfh_undistort_images`` (include/xfeat_hip_cameras.h, csrc/k_cameras.hip) are specified in
DESIGN.md 3.24.  There is no CPU path: without the HIP library and a gfx950 device everything that would launch raises.

The two entries are declared in a header of their own; this module carries their prototypes (``SIGNATURES``) and ``load()``, which attaches
them to the library that ``_lib.load()`` returns.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, _twoview
from ._twoview import ptr as _ptr

PINHOLE, BROWN, FISHEYE = 0, 1, 2                          # the kind of a camera (XFH_CAMERA_*)
N_PARAMS = 12                                              # fx, fy, cx, cy, d0..d7
UNDISTORT, DISTORT = 0, 1
STATUS = ("ok", "beyond_count", "not_finite", "fold", "not_converged", "outside_field_of_view", "camera_not_usable")
IMAGE_U8, IMAGE_F32 = 0, 1
MAX_CHANNELS = 4
MAX_IMAGES = 65535                                         # of one xfh_undistort_images call; larger batches are split
MAX_POINT_BLOCKS = (1 << 31) - 1                           # workgroups of 256 points of one xfh_camera_points call
# model -> (kind, number of parameters, where each of them goes among the 12 doubles); names and orders are COLMAP's and poselib's
MODELS = {
    "SIMPLE_PINHOLE": (PINHOLE, (0, 2, 3)),                # f, cx, cy (f goes to fx and fy)
    "PINHOLE": (PINHOLE, (0, 1, 2, 3)),                    # fx, fy, cx, cy
    "SIMPLE_RADIAL": (BROWN, (0, 2, 3, 4)),                # f, cx, cy, k
    "RADIAL": (BROWN, (0, 2, 3, 4, 5)),                    # f, cx, cy, k1, k2
    "OPENCV": (BROWN, (0, 1, 2, 3, 4, 5, 6, 7)),           # fx, fy, cx, cy, k1, k2, p1, p2
    "OPENCV_FISHEYE": (FISHEYE, (0, 1, 2, 3, 4, 5, 6, 7)),  # fx, fy, cx, cy, k1, k2, k3, k4
}

_p, _i = C.c_void_p, C.c_int
# name -> (restype, argtypes); mirrors include/xfeat_hip_cameras.h one to one
SIGNATURES = {
    "xfh_camera_points": (_i, [_p, _p, C.c_longlong, _i, _p, _p, _i, _p, _i, _p, _p, _p]),
    "xfh_undistort_images": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _i, _i, C.c_double, _p, _p, _p]),
}


def load():
    """The library of ``_lib.load()`` with the prototypes of this module's two entries attached."""
    lib = _lib.load()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


def pack_cameras(cameras):
    """Camera dicts {"model", "width", "height", "params"} (one, or a list) -> kind (C,) int32, params (C, 12) float64 numpy arrays: what the
    library takes.  An unknown model or a wrong number of parameters raises XFeatHipError naming the model."""
    if isinstance(cameras, dict):
        cameras = [cameras]
    kind = np.zeros(len(cameras), np.int32)
    params = np.zeros((len(cameras), N_PARAMS), np.float64)
    for c, cam in enumerate(cameras):
        if not isinstance(cam, dict) or "model" not in cam or "params" not in cam:
            raise _lib.XFeatHipError(f"camera {c}: a dict with 'model' and 'params' expected, got {cam!r}")
        model = cam["model"]
        if model not in MODELS:
            raise _lib.XFeatHipError(f"camera {c}: model {model!r} is not supported (supported: {', '.join(MODELS)})")
        k, slots = MODELS[model]
        values = [float(v) for v in cam["params"]]
        if len(values) != len(slots):
            raise _lib.XFeatHipError(f"camera {c}: model {model} takes {len(slots)} parameters, got {len(values)}")
        kind[c] = k
        for s, v in zip(slots, values):
            params[c, s] = v
        if slots[1] != 1:                                  # one focal length
            params[c, 1] = params[c, 0]
    return kind, params


def _packed(who, cameras):
    """cameras (dicts, or the (kind, params) pair of pack_cameras as arrays or tensors) -> kind (C,) int32, params (C,12) float64 tensors."""
    if isinstance(cameras, tuple) and len(cameras) == 2 and not isinstance(cameras[0], dict):
        kind, params = (torch.as_tensor(v) for v in cameras)
    else:
        kind, params = (torch.from_numpy(v) for v in pack_cameras(cameras))
    if kind.dim() != 1 or params.shape != (kind.shape[0], N_PARAMS) or kind.shape[0] < 1:
        raise RuntimeError(f'{who}: cameras must pack to kind (C,) and params (C,{N_PARAMS}) with C >= 1')
    return kind.to(torch.int32).contiguous(), params.to(torch.float64).contiguous()


def _matrix(k4):
    z, o = torch.zeros_like(k4[:, 0]), torch.ones_like(k4[:, 0])
    return torch.stack([k4[:, 0], z, k4[:, 2], z, k4[:, 1], k4[:, 3], z, z, o], dim=1).view(-1, 3, 3)


def camera_matrix(cameras):
    """(C, 3, 3) float64 tensor [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] of the cameras: the PINHOLE intrinsics that the undistorted key-points
    of ``undistort_keypoints(kpts, cameras)`` belong to."""
    return _matrix(_packed("camera_matrix", cameras)[1][:, :4])


def _pinhole_side(who, K, n_cameras, dev):
    """K_new / K_src: (3,3) or (C,3,3) intrinsics (fx, fy, cx, cy are read) -> (C,4) float64 on dev; None stays None."""
    if K is None:
        return None
    K = torch.as_tensor(K, dtype=torch.float64)
    if K.shape == (3, 3):
        K = K.expand(n_cameras, 3, 3)
    if K.shape != (n_cameras, 3, 3):
        raise RuntimeError(f'{who}: intrinsics must be (3,3) or one (3,3) per camera')
    return torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], dim=1).to(dev).contiguous()


def _points(who, kpts, cameras, counts, K_other, direction):
    kpts = torch.as_tensor(np.asarray(kpts) if not torch.is_tensor(kpts) else kpts)
    single = kpts.dim() == 2
    if kpts.dim() not in (2, 3) or kpts.shape[-1] != 2:
        raise RuntimeError(f'{who}: expected kpts (K,2) or (P,K,2)')
    pts = kpts[None] if single else kpts
    P, K = pts.shape[:2]
    kind, params = _packed(who, cameras)
    n_cam = kind.shape[0]
    if n_cam not in (1, P) and P > 0:
        raise _lib.XFeatHipError(f"{who}: {n_cam} cameras for {P} images (one for all, or one each)")
    if counts is not None:
        counts = torch.as_tensor(counts)
        if counts.shape != (P,):
            raise RuntimeError(f'{who}: counts must have one entry per image')
    empty = P == 0 or K == 0
    dev = pts.device if pts.is_cuda or empty else _twoview.device(who)
    pts = pts.to(dev).float().contiguous()
    kind, params = kind.to(dev), params.to(dev)
    k4 = _pinhole_side(who, K_other, n_cam, dev)
    out = torch.empty((P, K, 2), dtype=torch.float32, device=dev)
    status = torch.empty((P, K), dtype=torch.uint8, device=dev)
    res = {'kpts': out[0] if single else out, 'status': status[0] if single else status, 'K': _matrix(k4 if k4 is not None else params[:, :4])}
    if empty:                                 # no point: nothing is read, nothing is mapped
        return res
    if counts is not None:
        counts = counts.to(dev).to(torch.int32).contiguous()
    lib = load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    step = max(1, (MAX_POINT_BLOCKS * 256) // K)          # images of one call
    for a in range(0, P, step):
        b = min(P, a + step)
        one = n_cam == 1
        _lib.check(lib.xfh_camera_points(_ptr(pts[a:b]), _ptr(counts[a:b]) if counts is not None else None, b - a, K, _ptr(kind if one else kind[a:b]),
                                         _ptr(params if one else params[a:b]), 1 if one else b - a,
                                         (_ptr(k4 if one else k4[a:b])) if k4 is not None else None, direction, _ptr(out[a:b]), _ptr(status[a:b]), stream),
                   "xfh_camera_points")
    return res


def undistort_keypoints(kpts, cameras, counts=None, K_new=None):
    """Raw pixels -> pixels of an ideal pinhole camera.

    kpts    : (K, 2) or (P, K, 2) pixels (x, y) of P images; a CUDA tensor stays where it is
    cameras : a camera dict or a list of them (one for all images, or one per image), or the (kind, params) pair of ``pack_cameras``
    counts  : (P,) int32 or None: rows at or beyond counts[p] are not read
    K_new   : (3,3) or (C,3,3) PINHOLE intrinsics of the result; None = the camera's own fx, fy, cx, cy
    Returns {'kpts': (.., K, 2) float32, 'status': (.., K) uint8 (STATUS), 'K': (C, 3, 3) float64 = the intrinsics the result belongs to};
    a row whose status is not 0 (beyond the count, not finite, beyond the fold radius of a barrel model, outside a fisheye's useful field of
    view, a camera that is not usable) is NaN, NaN.  Two calls give the same bytes.  Asynchronous: nothing synchronises with the host."""
    return _points("undistort_keypoints", kpts, cameras, counts, K_new, UNDISTORT)


def distort_keypoints(kpts, cameras, counts=None, K_src=None):
    """Pixels of an ideal pinhole camera (K_src; None = the camera's own fx, fy, cx, cy) -> raw pixels of the cameras: the projection of
    ``undistort_keypoints`` backwards, with the same arguments and the same result dict ('K' = the intrinsics the input belongs to)."""
    return _points("distort_keypoints", kpts, cameras, counts, K_src, DISTORT)


def undistort_images(images, cameras, K_new=None, out_size=None, fill=0.0, return_valid=False):
    """``cv2.undistort`` for a batch: images of the ideal pinhole camera K_new (None = the camera's own fx, fy, cx, cy) from raw images.

    images (B, C, H, W) uint8 or float32 CUDA tensor, C <= 4; cameras as for ``undistort_keypoints`` (one, or one per image); out_size
    (Ho, Wo), None = (H, W); fill = the value of everything outside the source image.  Bilinear, integer coordinates being pixel centres;
    float32 is rounded once, uint8 is floor(value + 0.5) clamped.  Returns the images (B, C, Ho, Wo) of the input's type, with
    return_valid also valid (B, Ho, Wo) uint8: 1 where all four taps were inside the source.  Asynchronous."""
    who = "undistort_images"
    _twoview.tensors(who, images)
    if images.dim() != 4 or images.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f'{who}: expected images (B,C,H,W) uint8 or float32')
    B, Ch, H, W = images.shape
    Ho, Wo = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if Ho < 0 or Wo < 0:
        raise RuntimeError(f'{who}: out_size {out_size} is negative')
    if Ch > MAX_CHANNELS:
        raise _lib.XFeatHipError(f"{who}: {Ch} channels, more than {MAX_CHANNELS}")
    fill = float(fill)
    kind, params = _packed(who, cameras)
    n_cam = kind.shape[0]
    if n_cam not in (1, B) and B > 0:
        raise _lib.XFeatHipError(f"{who}: {n_cam} cameras for {B} images (one for all, or one each)")
    empty = B == 0 or Ch == 0 or Ho == 0 or Wo == 0
    no_source = H == 0 or W == 0
    if not images.is_cuda and not (empty or no_source):
        raise _lib.XFeatHipError(f"{who} works on device-resident images")
    dev = images.device
    dst = torch.empty((B, Ch, Ho, Wo), dtype=images.dtype, device=dev)
    valid = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if return_valid else None
    if empty or no_source:                    # no pixel to write, or none to read: everything is outside
        if not empty:
            dst.fill_(fill if images.dtype == torch.float32 else (min(255.0, max(0.0, math.floor(fill + 0.5))) if fill == fill else 0.0))
            if valid is not None:
                valid.zero_()
        return (dst, valid) if return_valid else dst
    src = images.contiguous()
    kind, params = kind.to(dev), params.to(dev)
    k4 = _pinhole_side(who, K_new, n_cam, dev)
    lib = load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dtype = IMAGE_F32 if images.dtype == torch.float32 else IMAGE_U8
    one = n_cam == 1
    for a in range(0, B, MAX_IMAGES):
        b = min(B, a + MAX_IMAGES)
        _lib.check(lib.xfh_undistort_images(_ptr(src[a:b]), dtype, b - a, Ch, H, W, _ptr(kind if one else kind[a:b]), _ptr(params if one else params[a:b]),
                                            1 if one else b - a, (_ptr(k4 if one else k4[a:b])) if k4 is not None else None, Ho, Wo, fill, _ptr(dst[a:b]),
                                            _ptr(valid[a:b]) if valid is not None else None, stream), "xfh_undistort_images")
    return (dst, valid) if return_valid else dst


# ---- poselib's call shape for any supported model -------------------------------------------------------------------------------------------
def _pinhole_dict(cam, params):
    return {"model": "PINHOLE", "width": cam.get("width", 0), "height": cam.get("height", 0), "params": [float(v) for v in params[:4]]}


def _one_camera(who, cam):
    if not isinstance(cam, dict):
        raise _lib.XFeatHipError(f"{who}: a camera dict expected, got {cam!r}")
    kind, params = pack_cameras(cam)
    return int(kind[0]), params[0]


def _scatter(details, keep):
    """The inlier list of the kept rows back at the input's length: dropped rows are False."""
    inl = [False] * len(keep)
    for i, v in zip(np.nonzero(keep)[0].tolist(), details["inliers"]):
        inl[i] = v
    return dict(details, inliers=inl)


def estimate_relative_pose(kpts0, kpts1, camera0, camera1, ransac_opt=None, bundle_opt=None, *, seed=0):
    """``poselib.estimate_relative_pose(kpts0, kpts1, camera0, camera1, ransac_opt, bundle_opt)`` for camera dicts of any supported model.

    Both sides are undistorted to the PINHOLE cameras of their own fx, fy, cx, cy, correspondences with a side whose status is not 0 are
    dropped, and ``pose.estimate_relative_pose`` runs on the rest (its options, its result); 'inliers' has the input's length, dropped rows
    False.  With two cameras without distortion the points go to ``pose.estimate_relative_pose`` as they are.  Synchronises (as that
    function does)."""
    from . import pose
    who = "estimate_relative_pose"
    (k0, p0), (k1, p1) = _one_camera(who, camera0), _one_camera(who, camera1)
    cam0, cam1 = _pinhole_dict(camera0, p0), _pinhole_dict(camera1, p1)
    if k0 == PINHOLE and k1 == PINHOLE:
        return pose.estimate_relative_pose(kpts0, kpts1, cam0, cam1, ransac_opt, bundle_opt, seed=seed)
    a, b = _twoview.as_points(kpts0), _twoview.as_points(kpts1)
    if a.shape != b.shape:
        raise RuntimeError('kpts0 and kpts1 must hold the same number of points')
    if a.shape[0] == 0:
        return pose.estimate_relative_pose(a, b, cam0, cam1, ransac_opt, bundle_opt, seed=seed)
    ua, ub = undistort_keypoints(a, camera0), undistort_keypoints(b, camera1)
    keep = ((ua['status'] == 0) & (ub['status'] == 0)).cpu().numpy()
    sel = torch.from_numpy(keep).to(ua['kpts'].device)
    model, details = pose.estimate_relative_pose(ua['kpts'][sel], ub['kpts'][sel], cam0, cam1, ransac_opt, bundle_opt, seed=seed)
    return model, _scatter(details, keep)


def estimate_absolute_pose(points2D, points3D, camera, ransac_opt=None, bundle_opt=None, *, seed=0):
    """``poselib.estimate_absolute_pose(points2D, points3D, camera, ransac_opt, bundle_opt)`` for a camera dict of any supported model: the
    2D points are undistorted, rows whose status is not 0 are dropped and ``absolute_pose.estimate_absolute_pose`` runs on the rest;
    'inliers' has the input's length, dropped rows False.  Synchronises (as that function does)."""
    from . import absolute_pose
    who = "estimate_absolute_pose"
    k, p = _one_camera(who, camera)
    cam = _pinhole_dict(camera, p)
    if k == PINHOLE:
        return absolute_pose.estimate_absolute_pose(points2D, points3D, cam, ransac_opt, bundle_opt, seed=seed)
    a = _twoview.as_points(points2D)
    X = torch.as_tensor(np.asarray(points3D) if not torch.is_tensor(points3D) else points3D).reshape(-1, 3)
    if a.shape[0] != X.shape[0]:
        raise RuntimeError('points2D and points3D must hold the same number of points')
    if a.shape[0] == 0:
        return absolute_pose.estimate_absolute_pose(a, X, cam, ransac_opt, bundle_opt, seed=seed)
    ua = undistort_keypoints(a, camera)
    keep = (ua['status'] == 0).cpu().numpy()
    sel = torch.from_numpy(keep).to(ua['kpts'].device)
    model, details = absolute_pose.estimate_absolute_pose(ua['kpts'][sel], X.to(sel.device)[sel], cam, ransac_opt, bundle_opt, seed=seed)
    return model, _scatter(details, keep)
