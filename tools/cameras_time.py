#!/usr/bin/env python3
"""Time the camera models (FINDINGS.md 3.24): undistort_keypoints (xfh_camera_points) at 64 images of 4096 key-points through a Brown and a
fisheye camera, and undistort_images (xfh_undistort_images) at B = 64 VGA frames of one channel, fp32 and uint8, Brown and fisheye.  Whole
calls between HIP events, 20 runs after 3 untimed ones.  The bytes a call must move over its time are given as a share of the 8 TB/s HBM
peak: whole-call figures.  There is no parent to compare with and no threshold: the figures are reported.
    python tools/cameras_time.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from accelerated_features_amd import cameras  # noqa: E402
from twoview_support import timed  # noqa: E402

HBM_PEAK = 8.0e12
WARM, RUNS = 3, 20
share = lambda b, ms: f"{b / 1e6:.1f} MB = {b / (ms * 1e-3) / 1e9:.0f} GB/s = {100 * b / (ms * 1e-3) / HBM_PEAK:.1f} % of the HBM peak"      # noqa: E731
W, H = 640, 480
CAMERAS = {"brown": {"model": "OPENCV", "width": W, "height": H, "params": [500.0, 505.0, 323.0, 238.0, -0.28, 0.07, 1e-3, -5e-4]},
           "fisheye": {"model": "OPENCV_FISHEYE", "width": W, "height": H, "params": [320.0, 317.0, 318.5, 242.5, -0.03, 0.006, -0.002, 0.0003]}}

torch.manual_seed(0)
P, K = 64, 4096
pts = torch.rand((P, K, 2), device="cuda") * torch.tensor([W, H], device="cuda")
for name, cam in CAMERAS.items():
    packed = tuple(torch.from_numpy(v).cuda() for v in cameras.pack_cameras(cam))       # on the device once: the timed call uploads nothing
    out, ms = timed(lambda: cameras.undistort_keypoints(pts, packed), WARM, RUNS)
    moved = P * K * (8 + 8 + 1)               # the points read, the points and the status written
    print(f"xfh_camera_points {name} undistort P {P} K {K}: {ms:9.4f} ms per call ({share(moved, ms)}); rows ok "
          f"{100 * (out['status'] == 0).float().mean().item():.2f} %", flush=True)

B = 64
for dtype in (torch.float32, torch.uint8):
    src = (torch.rand((B, 1, H, W), device="cuda") * 255).to(dtype)
    for name, cam in CAMERAS.items():
        packed = tuple(torch.from_numpy(v).cuda() for v in cameras.pack_cameras(cam))
        (dst, valid), ms = timed(lambda: cameras.undistort_images(src, packed, return_valid=True), WARM, RUNS)
        e = src.element_size()
        moved = B * H * W * (2 * e + 1)       # every source pixel read once (the taps of neighbours share cache lines), the image and valid written
        print(f"xfh_undistort_images {name} {str(dtype)[6:]} B {B} {W} x {H} x 1: {ms:9.4f} ms per call ({share(moved, ms)}); valid "
              f"{100 * valid.float().mean().item():.1f} %", flush=True)
