"""The sequence workload of the tools under tools/ (and of bench.py's pipeline leg, which keeps its own copy): Fusion A,
synthetic KITTI-shaped frames (mmmot_amd.synth.make_frame(7000 + t, 120000, n_det)) with 10-12 detections each.  The
package is imported inside the functions, so a caller that has put another checkout first on sys.path gets that one's."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True, appear_fpn=False,
          point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg', test_mode=2,
          neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='A', affinity_op='multiply',
          softmax_mode='none')


def detections(frames):
    """detections per frame"""
    return np.random.default_rng(5).integers(10, 13, frames)


def sequence_feeds(frames, ego=None, seed=0):
    """``frames`` FrameFeeds (pinned host copies), generated on up to 16 threads.  ``ego=seed``: the same frames seen from
    a moving camera - every feed carries a pose of mmmot_amd.synth.ego_poses(frames, seed) and a KITTI-like
    Tr_imu_to_velo, so the pipeline aligns each frame's points to the frame before it.  ``seed``: another sequence of
    the same shape (0: the one every tool has measured)."""
    from mmmot_amd.pipeline import FrameFeed
    from mmmot_amd.synth import make_frame
    ndet = detections(frames)
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        made = list(pool.map(lambda t: make_frame(7000 + 100000 * int(seed) + t, 120000, int(ndet[t])), range(frames)))
    if ego is None:
        return [FrameFeed(*f) for f in made]
    from mmmot_amd.synth import KITTI_IMU2VELO, ego_poses
    return [FrameFeed(img, sweep, dict(info, **{'calib/Tr_imu_to_velo': KITTI_IMU2VELO}), dets, pose=pose)
            for (img, sweep, info, dets), pose in zip(made, ego_poses(frames, ego))]
