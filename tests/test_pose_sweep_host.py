"""The host side of the relative-pose threshold sweep (no GPU): the ScanNet-1500 metrics and helpers of accelerated_features_amd.pose
on values worked out by hand, the workspace planning of xfh_relpose_sweep_workspace_bytes, and the absence of a CPU path."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from accelerated_features_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_scannet_thresholds():
    from accelerated_features_amd import pose
    assert tuple(pose.SCANNET_THRESHOLDS) == (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0)
    assert len(pose.SCANNET_THRESHOLDS) <= pose.MAX_THRESHOLDS == 16


def test_pose_accuracy_by_hand():
    from accelerated_features_amd import pose
    # 8 pairs: 3 below 5 degrees, 5 below 10 (10 itself is not below 10), 6 below 20, one without a pose
    err = [1.0, 4.9, 0.0, 5.0, 9.99, 10.0, 20.0, np.inf]
    assert pose.pose_accuracy(err) == {5: 37.5, 10: 62.5, 20: 75.0}
    assert pose.pose_accuracy(err, thresholds=(1, 100)) == {1: 12.5, 100: 87.5}


def test_relative_transform_by_hand():
    from accelerated_features_amd import pose
    # camera 0 at the origin, axes = world; camera 1 at (1, 2, 3), rotated by 90 degrees about z (its x axis is the world's y).
    # X1 = R1' (X0 - c1): the relative rotation is -90 degrees about z, the translation R1' (0 - c1) = (-2, 1, -3)
    P0 = np.eye(4)
    P1 = np.eye(4)
    P1[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    P1[:3, 3] = [1, 2, 3]
    T = pose.relative_transform(P0, P1)
    assert T.shape == (3, 4)
    assert np.array_equal(T, np.array([[0.0, 1, 0, -2], [-1, 0, 0, 1], [0, 0, 1, -3]]))
    X0 = np.array([1.0, 2.0, 4.0])                # the world point one above camera 1's centre: on its z axis
    assert np.array_equal(T[:, :3] @ X0 + T[:, 3], [0.0, 0.0, 1.0])
    same = pose.relative_transform(P1, P1)
    assert np.array_equal(same, np.c_[np.eye(3), np.zeros(3)])
    batch = pose.relative_transform(np.stack([P0, P1])[:, :3], np.stack([P1, P1])[:, :3])       # (B, 3, 4) poses, batched
    assert batch.shape == (2, 3, 4) and np.array_equal(batch[0], T) and np.array_equal(batch[1], same)


def test_sweep_workspace_planning_is_host_only(lib):
    ws = lib.xfh_relpose_sweep_workspace_bytes
    for bad in ((0, 1000, 12), (-1, 1000, 12), (4, 0, 12), (4, 1000, 0), (4, 1000, 17), (4, 1000, -3)):
        assert ws(*bad) == 0, bad
    assert ws(1, 1, 1) > 0
    for P, iters, T in ((1, 1000, 1), (7, 1000, 12), (1500, 10000, 12), (3, 16384, 16)):
        assert ws(P + 1, iters, T) >= ws(P, iters, T) > 0
        assert ws(P, iters + 300, T) >= ws(P, iters, T)
        if T < 16:
            assert ws(P, iters, T + 1) >= ws(P, iters, T)
    # candidate poses once per hypothesis (10 x 12 fp64), a u64 cost and a u32 count per (candidate, threshold)
    assert ws(2, 1024, 12) >= 2 * 1024 * (960 + 12 * 120)
    assert ws(2, 1024, 12) < 12 * lib.xfh_relpose_workspace_bytes(2, 1024)
    assert ws(5, 1000, 1) >= lib.xfh_relpose_workspace_bytes(5, 1000)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_means_the_sweep_raises(lib):
    from accelerated_features_amd import _lib, pose
    K = np.eye(3)
    with pytest.raises(_lib.XFeatHipError):
        pose.estimate_relative_pose_sweep_batch(torch.zeros(1, 8, 2), torch.zeros(1, 8, 2), None, K, K, pose.SCANNET_THRESHOLDS)
    z = torch.zeros(1, 8, 2)
    i = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(_lib.XFeatHipError):
        pose.estimate_relative_pose_sweep_matches(z, z, i, i, torch.zeros(1, dtype=torch.int32), K, K, [1.0, 2.0])
    with pytest.raises(_lib.XFeatHipError):
        pose.estimate_pose(np.zeros((8, 2)), np.zeros((8, 2)), K, K, 1.0)


def test_estimate_pose_offers_no_opencv_branch():
    from accelerated_features_amd import _lib, pose
    with pytest.raises(_lib.XFeatHipError):
        pose.estimate_pose(np.zeros((8, 2)), np.zeros((8, 2)), np.eye(3), np.eye(3), 1.0, type='opencv')
