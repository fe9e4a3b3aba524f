#!/usr/bin/env python
"""Generate tests/golden/ego_align.npz by running the REFERENCE's ego-motion alignment.

    python tools/gen_golden_ego.py --reference <checkout of the reference project>

Imports ``align_points``, ``align_pos``, ``get_rotate_mat`` and ``get_transform_mat`` from the reference's
utils/data_util.py as they are.  That module imports ``pyproj`` (used by ``get_pos`` only), and its neighbours import
``numba`` and ``cv2``; where one of them is not installed a stub module takes its place in ``sys.modules`` (the way
oracle/gen_golden_points.py stubs numba): none of the four functions touches them.

The fixture holds the inputs - three poses of a synthetic drive (mmmot_amd.synth.ego_poses), the calibration matrices,
point sets of Q in {1, 63, 64, 65, 257, 1000} rows with 3 and 4 columns, each with the all-zero row an empty box is
padded with, and a few box centres - and what the reference makes of them: R, T of both pairs, the aligned fp32 points
for chains of one and two steps (computed the way dataset/test_seq_dataset.py:209 does, ``pc[:, :3] = align_points(...,
pc[:, :3])`` on the fp32 array), and the ``align_pos`` outputs.  Only data is written.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

QS = (1, 63, 64, 65, 257, 1000)


def _stub_missing(names):
    for name in names:
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            if name == 'numba':
                def _ident(*a, **k):
                    if len(a) == 1 and callable(a[0]) and not k:
                        return a[0]
                    return lambda f: f
                m.jit = m.njit = _ident
            sys.modules[name] = m


def point_set(rng, Q, F):
    """KITTI-range rows (metres; reflectivity in [0, 1]) with one all-zero row (the padding of an empty box)"""
    pts = np.stack([rng.uniform(0, 70, Q), rng.uniform(-30, 30, Q), rng.uniform(-2.5, 1.0, Q), rng.uniform(0, 1, Q)], 1)
    pts = pts[:, :F].astype(np.float32)
    pts[Q // 2] = 0.0
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference project')
    args = ap.parse_args()
    _stub_missing(['pyproj', 'numba', 'cv2'])
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils.data_util import align_points, align_pos, get_rotate_mat, get_transform_mat
    from mmmot_amd.synth import KITTI_IMU2VELO, KITTI_R0, KITTI_TR, ego_poses

    poses = ego_poses(3, seed=1)
    pos = np.stack([p for p, _ in poses])
    rad = np.stack([r for _, r in poses])
    # the lists as dataset/test_seq_dataset.py:199-203 grows them
    delta_rad, R, T = [], [], []
    for t in (1, 2):
        delta_rad.append(rad[t] - rad[t - 1])
        R.append(get_rotate_mat(delta_rad[-1], rotate_order=[1, 2, 3]))
        T.append(get_transform_mat(pos[t] - pos[t - 1], rad[t - 1][-1]))
    out = {'pos': pos, 'rad': rad, 'Tr_imu_to_velo': KITTI_IMU2VELO, 'R0_rect': KITTI_R0, 'Tr_velo_to_cam': KITTI_TR,
           'R': np.stack([np.asarray(r) for r in R]), 'T': np.stack([np.asarray(t) for t in T]),
           'delta_rad': np.stack(delta_rad),
           'rot_default_order': np.asarray(get_rotate_mat(delta_rad[0])), 'qs': np.asarray(QS)}
    rng = np.random.default_rng(20240)
    for Q in QS:
        for F in (3, 4):
            pts = point_set(rng, Q, F)
            out['pts_%d_%d' % (Q, F)] = pts
            for c in (1, 2):
                pc = pts.copy()
                pc[:, :3] = align_points(R[:c], T[:c], KITTI_IMU2VELO, pc[:, :3])
                assert pc.dtype == np.float32
                out['aligned_%d_%d_c%d' % (Q, F, c)] = pc
    # box centres in the camera frame (a few metres to tens of metres ahead) and their yaw
    N = 7
    vel = np.stack([rng.uniform(5, 60, N), rng.uniform(-15, 15, N), rng.uniform(-1.9, -1.0, N), np.ones(N)], 1)
    location = (vel @ (KITTI_R0 @ KITTI_TR).T)[:, :3]
    rotation_y = rng.uniform(-np.pi, np.pi, N)
    out['location'], out['rotation_y'] = location, rotation_y
    for c in (1, 2):
        loc, rot = align_pos(R[:c], T[:c], KITTI_TR, KITTI_IMU2VELO, KITTI_R0, delta_rad[:c], location.copy(),
                             rotation_y.copy())  # the reference adds to rotation_y in place
        out['aligned_loc_c%d' % c], out['aligned_rot_c%d' % c] = np.asarray(loc), np.asarray(rot)
    path = os.path.join(ROOT, 'tests', 'golden', 'ego_align.npz')
    np.savez_compressed(path, **out)
    moved = max(float(np.abs(out['aligned_%d_3_c1' % Q] - out['pts_%d_3' % Q]).max()) for Q in QS)
    print('%s: %d arrays, %d bytes; the alignment moves a coordinate by up to %.2f m' % (
        path, len(out), os.path.getsize(path), moved))


if __name__ == '__main__':
    main()
