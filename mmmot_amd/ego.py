"""Ego motion between the frames of a pair: the O(1)-per-frame host algebra of the reference's alignment step.

``TestSequence._generate_img_lidar`` (reference dataset/test_seq_dataset.py:199-210) moves the second frame of a pair
into the first frame's coordinates: from the two frames' ``pos`` / ``rad`` (``get_pos``, utils/data_util.py:486-494) it
forms ``R = get_rotate_mat(rad_b - rad_a, rotate_order=[1, 2, 3])`` and ``T = get_transform_mat(pos_b - pos_a,
rad_a[-1])`` and hands them to ``align_pos`` (box centres) and ``align_points`` (the extracted LiDAR points).  This module
restates those numpy float64 operations in the reference's order (utils/data_util.py:497-509,534-584 and
point_cloud/box_np_ops.py:584-611), so that the matrices - and the records the device kernel reads
(mmmot_amd.points.align_points, csrc/align_points.hip) - are the reference's.  The O(points) part runs on the device;
``align_pos`` is O(boxes), stays on the host like the plane algebra of mmmot_amd.points, and is here for drop-in
completeness: ``TrackingNet.forward`` reads only ``points`` / ``points_split``, so the pipeline does not call it.
"""
import numpy as np

MAX_CHAIN = 4   # MMMOT_ALIGN_MAX_CHAIN
RECORD = 80     # MMMOT_ALIGN_REC: doubles per transform record


def rotate_mat(delta_rad, rotate_order=(3, 2, 1)):
    """``get_rotate_mat`` (utils/data_util.py:534-575): the 3x3 rotation of (roll, pitch, yaw) = ``delta_rad``; the
    elementary rotations are multiplied from the one with the largest ``rotate_order`` entry down (default z, y, x).
    Returns a float64 ndarray (the reference returns the same values as an ``np.matrix``)."""
    rx_cos, rx_sin = np.cos(delta_rad[0]), np.sin(delta_rad[0])
    rx = np.eye(3)
    rx[1, 1], rx[1, 2], rx[2, 1], rx[2, 2] = rx_cos, -rx_sin, rx_sin, rx_cos
    ry_cos, ry_sin = np.cos(delta_rad[1]), np.sin(delta_rad[1])
    ry = np.eye(3)
    ry[0, 0], ry[0, 2], ry[2, 0], ry[2, 2] = ry_cos, ry_sin, -ry_sin, ry_cos
    rz_cos, rz_sin = np.cos(delta_rad[2]), np.sin(delta_rad[2])
    rz = np.eye(3)
    rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = rz_cos, -rz_sin, rz_sin, rz_cos
    mats = [rx, ry, rz]
    r = np.eye(3)
    for i in np.argsort(rotate_order)[::-1]:
        r = r @ mats[i]
    return r


def transform_mat(delta_pos, yaw):
    """``get_transform_mat`` (utils/data_util.py:578-584): the position difference turned by the first frame's yaw."""
    rot_sin, rot_cos = np.sin(yaw), np.cos(yaw)
    rot_mat_T = np.array([[rot_cos, -rot_sin, 0], [rot_sin, rot_cos, 0], [0, 0, 1]])
    return delta_pos @ rot_mat_T


def pair_motion(pose_a, pose_b):
    """(R, T) of the pair (a, b), poses = (pos, rad) as ``get_pos`` returns them, the way ``_generate_img_lidar`` forms
    them (dataset/test_seq_dataset.py:200-203)."""
    pos_a, rad_a = (np.asarray(v, dtype=np.float64) for v in pose_a)
    pos_b, rad_b = (np.asarray(v, dtype=np.float64) for v in pose_b)
    return rotate_mat(rad_b - rad_a, rotate_order=[1, 2, 3]), transform_mat(pos_b - pos_a, rad_a[-1])


def _hom(points):
    if points.shape[-1] == 3:
        points = np.concatenate([points, np.ones(list(points.shape[:-1]) + [1])], axis=-1)
    return points


def imu_matrices(imu2velo):
    """The two 4x4 matrices of ``lidar_to_imu`` / ``imu_to_lidar`` (box_np_ops.py:599-611): rows go to the IMU frame with
    ``inv(imu2velo.T)`` and back with ``imu2velo.T``."""
    imu2velo = np.asarray(imu2velo)
    return np.linalg.inv(imu2velo.T), imu2velo.T


def align_pos(R, T, velo2cam, imu2velo, r_rect, delta_rad, location, rotation_y):
    """``align_pos`` (utils/data_util.py:497-509): camera-frame box centres [N, 3] and yaw [N] of a pair's second frame
    in the first frame's coordinates.  The reference adds the yaw steps to ``rotation_y`` in place; this returns a new
    array and leaves the argument as it is."""
    if len(R) == 0:
        return location, rotation_y
    cam = np.asarray(r_rect) @ np.asarray(velo2cam)
    to_imu, to_velo = imu_matrices(imu2velo)
    velo_loc = (_hom(np.asarray(location)) @ np.linalg.inv(cam.T))[..., :3]        # camera_to_lidar
    imu_loc = (_hom(velo_loc) @ to_imu)[..., :3]                                   # lidar_to_imu
    rotation_y = np.array(rotation_y, copy=True)
    for i in range(len(R)):
        imu_loc = imu_loc @ np.asarray(R[-i - 1]).T + np.asarray(T[-i - 1])
        rotation_y += delta_rad[-i - 1][-1]  # [roll, pitch, yaw]: only yaw
    new_velo_loc = (_hom(imu_loc) @ to_velo)[..., :3]                              # imu_to_lidar
    return (_hom(new_velo_loc) @ cam.T)[..., :3], rotation_y                       # lidar_to_camera


def transform_record(R, T, imu2velo):
    """The float64 [RECORD] transform record of one segment of ``mmmot_align_points`` (include/mmmot_hip.h): A =
    inv(imu2velo.T), the chain steps (R, T) in the order they are APPLIED - the reference's lists from last to first,
    as ``align_points``' loop walks them - and B = imu2velo.T."""
    if len(R) != len(T):
        raise ValueError('align_points: R and T must have the same length (%d, %d)' % (len(R), len(T)))
    if not 1 <= len(R) <= MAX_CHAIN:
        raise ValueError('align_points: a chain of 1..%d (R, T) steps, got %d' % (MAX_CHAIN, len(R)))
    to_imu, to_velo = imu_matrices(imu2velo)
    if to_imu.shape != (4, 4):
        raise ValueError('align_points: imu2velo must be 4x4, got %s' % (to_imu.shape,))
    rec = np.zeros(RECORD, dtype=np.float64)
    rec[0:16] = np.asarray(to_imu, dtype=np.float64).reshape(-1)
    for c in range(len(R)):
        r = np.asarray(R[-c - 1], dtype=np.float64)
        t = np.asarray(T[-c - 1], dtype=np.float64).reshape(-1)
        if r.shape != (3, 3) or t.shape != (3,):
            raise ValueError('align_points: every R must be 3x3 and every T a 3-vector')
        rec[16 + 12 * c:25 + 12 * c] = r.reshape(-1)
        rec[25 + 12 * c:28 + 12 * c] = t
    rec[64:80] = np.asarray(to_velo, dtype=np.float64).reshape(-1)
    return rec


def box_motion(pose_p, pose_q, calib):
    """The ego motion of the pair (p, q), p the earlier frame, composed for BOX CENTRES: (C, inv C, dyaw).  C is the
    row-vector 4x4 float64 matrix that does to a camera-frame location of frame q what ``align_pos([R], [T], ..)`` does
    with (R, T) = ``pair_motion(pose_p, pose_q)``: camera -> LiDAR (``inv(cam.T)``, cam = R0_rect @ Tr_velo_to_cam) ->
    IMU (``inv(imu2velo.T)``) -> the step q @ R.T + T -> LiDAR (``imu2velo.T``) -> camera (``cam.T``), multiplied in
    that order: ``[x, y, z, 1] @ C`` is the location in frame p's coordinates.  ``inv C`` (``np.linalg.inv``) takes it
    back; ``dyaw`` = (rad_q - rad_p)[2] is what ``align_pos`` adds to ``rotation_y``.  ``calib``: the frame-info dict with
    ``calib/R0_rect``, ``calib/Tr_velo_to_cam`` and ``calib/Tr_imu_to_velo``.  The records of ``mmmot_fill_tracks``
    (tracks.pack_fill) are made of these."""
    R, T = pair_motion(pose_p, pose_q)
    cam = np.asarray(calib['calib/R0_rect'], dtype=np.float64) @ np.asarray(calib['calib/Tr_velo_to_cam'], dtype=np.float64)
    to_imu, to_velo = imu_matrices(np.asarray(calib['calib/Tr_imu_to_velo'], dtype=np.float64))
    step = np.eye(4)
    step[:3, :3] = R.T
    step[3, :3] = T
    C = np.linalg.inv(cam.T) @ to_imu @ step @ to_velo @ cam.T
    dyaw = float(np.asarray(pose_q[1], dtype=np.float64)[2] - np.asarray(pose_p[1], dtype=np.float64)[2])
    return C, np.linalg.inv(C), dyaw
