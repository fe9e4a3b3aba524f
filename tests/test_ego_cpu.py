"""Ego-motion alignment without a GPU: the host algebra of mmmot_amd/ego.py and the float64 statement of the kernel's
arithmetic (tests/ego_ref.py) against what the reference itself computed (tests/golden/ego_align.npz, written by
tools/gen_golden_ego.py), the argument checks of mmmot_align_points in the cross-compiled library, the synthetic moving
sequence, and the pose checks of FrameFeed / SequencePipeline that come before any device work."""
import os
import types

import numpy as np
import pytest

import ego_ref
from mmmot_amd import ego

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ego_align.npz')
QS = (1, 63, 64, 65, 257, 1000)
# the same numpy operations as the reference on values of magnitude <= 100: a few fp64 roundings are about 1e-13, the
# factor 10 allows for another BLAS
HOST_TOL = 1e-12


@pytest.fixture(scope='module')
def z():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_contents(z):
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert tuple(z['qs'].tolist()) == QS and z['pos'].shape == (3, 3) and z['R'].shape == (2, 3, 3)
    assert 1e5 < np.abs(z['pos'][:, :2]).min() and np.abs(z['pos'][:, :2]).max() < 1e7  # web-mercator magnitude
    for Q in QS:
        for F in (3, 4):
            pts = z['pts_%d_%d' % (Q, F)]
            assert pts.shape == (Q, F) and pts.dtype == np.float32
            zero = np.flatnonzero(~pts.any(axis=1))
            assert len(zero) == 1  # the padding row of an empty box
            for c in (1, 2):
                out = z['aligned_%d_%d_c%d' % (Q, F, c)]
                assert out.shape == (Q, F) and out.dtype == np.float32
                assert np.abs(out[zero[0], :3]).max() > 0.1  # the reference aligns that row too: it does not stay zero


def test_rotate_and_transform_mat(z):
    for t in (1, 2):
        d = z['rad'][t] - z['rad'][t - 1]
        assert np.array_equal(d, z['delta_rad'][t - 1])
        R = ego.rotate_mat(d, rotate_order=[1, 2, 3])
        assert isinstance(R, np.ndarray) and R.shape == (3, 3)
        assert np.abs(R - z['R'][t - 1]).max() <= HOST_TOL
        T = ego.transform_mat(z['pos'][t] - z['pos'][t - 1], z['rad'][t - 1][-1])
        assert np.abs(T - z['T'][t - 1]).max() <= HOST_TOL
    assert np.abs(ego.rotate_mat(z['delta_rad'][0]) - z['rot_default_order']).max() <= HOST_TOL
    # the two orders are different products once two angles are non-zero
    assert np.abs(ego.rotate_mat([0.3, -0.2, 0.1]) - ego.rotate_mat([0.3, -0.2, 0.1], [1, 2, 3])).max() > 1e-3


def test_pair_motion(z):
    for t in (1, 2):
        R, T = ego.pair_motion((z['pos'][t - 1], z['rad'][t - 1]), (z['pos'][t], z['rad'][t]))
        assert np.abs(R - z['R'][t - 1]).max() <= HOST_TOL and np.abs(T - z['T'][t - 1]).max() <= HOST_TOL
        assert 0.5 < np.linalg.norm(T) < 2.0  # about a metre per frame, out of positions of 1e6


def test_align_pos(z):
    loc, rot = z['location'], z['rotation_y']
    for c in (1, 2):
        R, T, d = list(z['R'][:c]), list(z['T'][:c]), list(z['delta_rad'][:c])
        rot_in = rot.copy()
        got_loc, got_rot = ego.align_pos(R, T, z['Tr_velo_to_cam'], z['Tr_imu_to_velo'], z['R0_rect'], d, loc, rot_in)
        assert np.abs(got_loc - z['aligned_loc_c%d' % c]).max() <= HOST_TOL
        assert np.abs(got_rot - z['aligned_rot_c%d' % c]).max() <= HOST_TOL
        assert np.array_equal(rot_in, rot)  # the argument is left as it is
        assert np.abs(got_loc - loc).max() > 0.1
    same_loc, same_rot = ego.align_pos([], [], z['Tr_velo_to_cam'], z['Tr_imu_to_velo'], z['R0_rect'], [], loc, rot)
    assert same_loc is loc and same_rot is rot


def test_transform_record(z):
    rec = ego.transform_record(list(z['R']), list(z['T']), z['Tr_imu_to_velo'])
    assert rec.shape == (ego.RECORD,) and rec.dtype == np.float64
    assert np.array_equal(rec[:16].reshape(4, 4), np.linalg.inv(z['Tr_imu_to_velo'].T))
    assert np.array_equal(rec[64:].reshape(4, 4), z['Tr_imu_to_velo'].T)
    # applied from last to first: step 0 is the reference's R[-1], T[-1]
    assert np.array_equal(rec[16:25].reshape(3, 3), z['R'][1]) and np.array_equal(rec[25:28], z['T'][1])
    assert np.array_equal(rec[28:37].reshape(3, 3), z['R'][0]) and np.array_equal(rec[37:40], z['T'][0])
    assert not rec[40:64].any()
    with pytest.raises(ValueError):
        ego.transform_record([z['R'][0]] * 5, [z['T'][0]] * 5, z['Tr_imu_to_velo'])
    with pytest.raises(ValueError):
        ego.transform_record([z['R'][0]], [], z['Tr_imu_to_velo'])


def test_kernel_arithmetic_statement_against_the_reference(z):
    """tests/ego_ref.py (sequential k order, no FMA) against the reference's BLAS route: every coordinate within 1 fp32
    ulp, at most 1 in 10 000 different at all - counted over every case of the fixture"""
    pairs = []
    for Q in QS:
        for F in (3, 4):
            pts = z['pts_%d_%d' % (Q, F)]
            for c in (1, 2):
                got = ego_ref.align_points(list(z['R'][:c]), list(z['T'][:c]), z['Tr_imu_to_velo'], pts)
                want = z['aligned_%d_%d_c%d' % (Q, F, c)]
                assert got.dtype == np.float32 and got.shape == want.shape
                if F == 4:
                    assert np.array_equal(got[:, 3].view(np.uint32), pts[:, 3].view(np.uint32))
                pairs.append((got[:, :3], want[:, :3]))
    worst, ndiff, n = ego_ref.assert_close_to_reference(pairs)
    print('ego_ref vs reference: worst %.2f ulp, %d of %d coordinates differ' % (worst, ndiff, n))
    assert n == 2 * 2 * 3 * sum(QS)


def test_align_points_argument_checks():
    from mmmot_amd import _lib
    _lib.build()
    lib = _lib.load()
    assert lib.mmmot_abi_version() == 10
    f = lib.mmmot_align_points
    EINVAL = -1
    # pts, F, Q, NS, seg_row0, xf, chain, out, out_row0, ldo, stream; 8 stands for a non-null pointer: every call below
    # is answered before any launch
    assert f(8, 2, 4, 1, 8, 8, 1, 8, 0, 2, None) == EINVAL and f(8, 5, 4, 1, 8, 8, 1, 8, 0, 5, None) == EINVAL  # F
    for null in (0, 4, 5, 7):  # pts, seg_row0, xf, out
        args = [8, 3, 4, 1, 8, 8, 1, 8, 0, 3, None]
        args[null] = None
        assert f(*args) == EINVAL, null
    assert f(8, 3, 4, 1, 8, 8, 5, 8, 0, 3, None) == EINVAL   # a chain longer than 4
    assert f(8, 3, 4, 1, 8, 8, -1, 8, 0, 3, None) == EINVAL
    assert f(8, 3, -1, 1, 8, 8, 1, 8, 0, 3, None) == EINVAL  # negative sizes
    assert f(8, 3, 4, -1, 8, 8, 1, 8, 0, 3, None) == EINVAL
    assert f(8, 3, 4, 1, 8, 8, 1, 8, -1, 3, None) == EINVAL
    assert f(8, 3, 4, 0, 8, 8, 1, 8, 0, 3, None) == EINVAL   # rows without a segment
    assert f(8, 4, 4, 1, 8, 8, 1, 8, 0, 3, None) == EINVAL   # rows of 4 floats at a stride of 3
    # Q = 0: a no-op, also with null pointers; a bad F or chain is still refused
    assert f(None, 3, 0, 0, None, None, 1, None, 0, 3, None) == 0 and f(8, 4, 0, 1, 8, 8, 4, 8, 7, 4, None) == 0
    assert f(None, 2, 0, 0, None, None, 1, None, 0, 3, None) == EINVAL
    assert f(None, 3, 0, 0, None, None, 5, None, 0, 3, None) == EINVAL
    with open(os.path.join(ROOT, 'include', 'mmmot_hip.h')) as h:
        header = h.read()
    assert 'int mmmot_align_points(const float* pts, int F, int Q, int NS,' in header
    assert '#define MMMOT_ALIGN_REC %d' % ego.RECORD in header
    assert '#define MMMOT_ALIGN_MAX_CHAIN %d' % ego.MAX_CHAIN in header
    assert len(_lib.SIGNATURES['mmmot_align_points']) == 11 and 'align_points.hip' in _lib.SOURCES


def test_align_points_operator_checks_without_a_device():
    import torch
    from mmmot_amd.points import align_points, align_points_batched
    pts = torch.zeros(5, 3)
    assert align_points([], [], np.eye(4), pts) is pts  # the reference returns its argument for an empty chain
    with pytest.raises(ValueError):
        align_points([np.eye(3)], [], np.eye(4), pts)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        align_points([np.eye(3)], [np.zeros(3)], np.eye(4), pts)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        align_points_batched(pts, [0, 5], np.zeros((1, ego.RECORD)), 1)


def _same_frames(a, b):
    assert len(a) == len(b)
    for (ia, pa, fa, da), (ib, pb, fb, db) in zip(a, b):
        assert np.array_equal(ia, ib) and np.array_equal(pa, pb)
        assert fa.keys() == fb.keys() and all(np.array_equal(fa[k], fb[k]) for k in fa)
        assert da.keys() == db.keys() and all(np.array_equal(da[k], db[k]) for k in da)


def test_make_sequence_ego():
    from mmmot_amd.synth import make_frame, make_sequence
    kw = dict(seed=3, n_pts=500, det_range=(2, 3), hw=(48, 64))
    still = make_sequence(3, **kw)
    # ego=None: what make_sequence returned before it had the argument
    rng = np.random.default_rng([0x5ea, 3])
    _same_frames(still, [make_frame(3000 + t, 500, int(rng.integers(2, 4)), (48, 64)) for t in range(3)])
    _same_frames(still, make_sequence(3, ego=None, **kw))
    assert all(set(info) == {'calib/R0_rect', 'calib/Tr_velo_to_cam', 'calib/P2', 'img_shape'} for _, _, info, _ in still)
    moving = make_sequence(3, ego=0, **kw)
    for (im, pm, fm, dm), (i0, p0, f0, d0) in zip(moving, still):  # the same frames, seen from a moving camera
        assert np.array_equal(im, i0) and np.array_equal(pm, p0) and all(np.array_equal(dm[k], d0[k]) for k in d0)
        assert set(fm) == set(f0) | {'calib/Tr_imu_to_velo', 'pos', 'rad'}
        assert fm['calib/Tr_imu_to_velo'].shape == (4, 4) and fm['pos'].shape == (3,) and fm['rad'].shape == (3,)
        assert 1e5 < abs(fm['pos'][0]) < 1e7 and 1e5 < abs(fm['pos'][1]) < 1e7
    for (_, _, fa, _), (_, _, fb, _) in zip(moving, moving[1:]):
        assert 0.5 < np.linalg.norm(fb['pos'] - fa['pos']) < 2.0 and not np.array_equal(fa['rad'], fb['rad'])
        R, T = ego.pair_motion((fa['pos'], fa['rad']), (fb['pos'], fb['rad']))
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
        assert 0.5 < np.linalg.norm(T) < 2.0
    _same_frames(moving, make_sequence(3, ego=0, **kw))  # seeded
    assert not np.array_equal(make_sequence(3, ego=1, **kw)[1][2]['pos'], moving[1][2]['pos'])


def test_pose_checks_come_before_any_device_work():
    """no GPU here: a FrameFeed that got as far as pinning its image, or a pipeline that got as far as its first upload,
    would fail with another error"""
    import torch
    from mmmot_amd.pipeline import FrameFeed, SequencePipeline
    from mmmot_amd.synth import make_sequence
    img, sweep, info, dets = make_sequence(1, n_pts=200, det_range=(2, 2), hw=(48, 64), ego=0)[0]
    pose = (info['pos'], info['rad'])
    with pytest.raises(ValueError, match='not both'):
        FrameFeed(img, sweep, info, dets, point_transform=lambda p: p, pose=pose)
    with pytest.raises(ValueError, match='Tr_imu_to_velo'):
        FrameFeed(img, sweep, {k: v for k, v in info.items() if k != 'calib/Tr_imu_to_velo'}, dets, pose=pose)
    with pytest.raises(ValueError, match='pose'):
        FrameFeed(img, sweep, info, dets, pose=(info['pos'][:2], info['rad']))
    feeds = [types.SimpleNamespace(pose=pose, dets=dets), types.SimpleNamespace(pose=None, dets=dets),
             types.SimpleNamespace(pose=pose, dets=dets)]
    pipe = SequencePipeline(torch.nn.Linear(1, 1), overlap=False)
    with pytest.raises(ValueError, match='2 of 3 frames carry a pose'):
        pipe.run(feeds)
    with pytest.raises(ValueError, match='2 of 3 frames carry a pose'):
        pipe.run_offline(feeds)
    pipe = SequencePipeline(torch.nn.Linear(1, 1), overlap=False, reuse_appearance=True)
    with pytest.raises(ValueError, match='1 of 2 frames carry a pose'):
        pipe.run(feeds[:2])
