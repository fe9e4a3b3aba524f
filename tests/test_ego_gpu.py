"""Ego-motion alignment on the device: mmmot_align_points (csrc/align_points.hip) through mmmot_amd.points against what
the reference computed (tests/golden/ego_align.npz) and against the float64 statement of its arithmetic (tests/ego_ref.py),
and the routing of raw / aligned points through every order of the SequencePipeline on a moving synthetic sequence."""
import os

import numpy as np
import pytest
import torch

import ego_ref
from common import TOL
from mmmot_amd import TrackingNet, ego
from mmmot_amd.points import align_points, align_points_batched, prep_points
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (1, 63, 64, 65, 257, 1000)
KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True, appear_fpn=False,
          point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg', test_mode=2,
          neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='C', affinity_op='multiply',
          softmax_mode='none')


@pytest.fixture(scope='module')
def z():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'ego_align.npz')) as f:
        return {k: f[k] for k in f.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the kernel against the reference's results ------------------------------------------------------------------------
def test_kernel_against_the_reference(z):
    """every Q, F and chain length of the fixture; the output is a row- and column-strided slice of a NaN-filled buffer"""
    pairs = []
    for Q in QS:
        for F in (3, 4):
            pts = z['pts_%d_%d' % (Q, F)]
            d_pts = torch.from_numpy(pts).cuda()
            for c in (1, 2):
                R, T = list(z['R'][:c]), list(z['T'][:c])
                want = z['aligned_%d_%d_c%d' % (Q, F, c)]
                buf = torch.full((Q + 5, F + 2), float('nan'), device='cuda')
                view = buf[2:2 + Q, 1:1 + F]
                got = align_points(R, T, z['Tr_imu_to_velo'], d_pts, out=view)
                assert got.data_ptr() == view.data_ptr() and got.shape == (Q, F)
                h = buf.cpu().numpy()
                guard = np.ones(h.shape, dtype=bool)
                guard[2:2 + Q, 1:1 + F] = False
                assert np.isnan(h[guard]).all(), 'Q=%d F=%d chain=%d wrote outside its slice' % (Q, F, c)
                res = h[2:2 + Q, 1:1 + F]
                assert np.isfinite(res).all()
                assert np.array_equal(d_pts.cpu().numpy(), pts)  # the input is left as it is
                if F == 4:
                    assert np.array_equal(bits(res[:, 3]), bits(pts[:, 3])), 'the fourth column is a copy'
                zero = int(np.flatnonzero(~pts.any(axis=1))[0])
                assert np.array_equal(bits(res[zero, :3]), bits(want[zero, :3])) and np.abs(res[zero, :3]).max() > 0.1
                # the kernel IS the float64 statement (same operations, same order): bit for bit
                assert np.array_equal(bits(res), bits(ego_ref.align_points(R, T, z['Tr_imu_to_velo'], pts)))
                again = align_points(R, T, z['Tr_imu_to_velo'], d_pts)  # a fresh contiguous output
                assert again.is_contiguous() and np.array_equal(bits(again.cpu().numpy()), bits(res)), 'run twice'
                pairs.append((res[:, :3], want[:, :3]))
    worst, ndiff, n = ego_ref.assert_close_to_reference(pairs, 'kernel vs reference')
    print('kernel vs reference: worst %.2f ulp, %d of %d coordinates differ' % (worst, ndiff, n))


def test_empty_chain_returns_the_argument():
    pts = torch.zeros(4, 3, device='cuda')
    assert align_points([], [], np.eye(4), pts) is pts


def _random_transform(rng):
    rad = rng.uniform(-0.05, 0.05, 3)
    return ego.rotate_mat(rad, [1, 2, 3]), rng.uniform(-2, 2, 3)


def _scene(rng, Q, F):
    pts = np.stack([rng.uniform(0, 70, Q), rng.uniform(-30, 30, Q), rng.uniform(-2.5, 1.0, Q), rng.uniform(0, 1, Q)], 1)
    return pts[:, :F].astype(np.float32)


@pytest.mark.parametrize('F', [3, 4])
def test_batched_launch(z, F):
    """three segments of 0, 65 and 257 rows, each with its own transform: bit-equal to three single launches and to the
    float64 statement; the rows go to an offset of a joined buffer whose other rows stay as they were"""
    rng = np.random.default_rng(77 + F)
    imu = z['Tr_imu_to_velo']
    sizes = (0, 65, 257)
    rows = np.concatenate([[0], np.cumsum(sizes)])
    segs = [_scene(rng, q, F) for q in sizes]
    xf = [_random_transform(rng) for _ in sizes]
    rec = np.stack([ego.transform_record([R], [T], imu) for R, T in xf])
    d_all = torch.from_numpy(np.concatenate(segs)).cuda()
    joined = torch.full((10 + 322 + 3, F), 7.0, device='cuda')
    got = align_points_batched(d_all, rows, rec, 1, out=joined, out_row0=10)
    assert got.shape == (322, F) and got.data_ptr() == joined[10:].data_ptr()
    h = joined.cpu().numpy()
    assert (h[:10] == 7.0).all() and (h[332:] == 7.0).all(), 'rows outside [10, 332) were written'
    pairs = []
    for i, (seg, (R, T)) in enumerate(zip(segs, xf)):
        part = h[10 + rows[i]:10 + rows[i + 1]]
        want = ego_ref.align_points([R], [T], imu, seg)
        assert np.array_equal(bits(part), bits(want))
        if len(seg):
            single = align_points([R], [T], imu, torch.from_numpy(seg).cuda())
            assert np.array_equal(bits(single.cpu().numpy()), bits(part)), 'segment %d: batched != single launch' % i
            pairs.append((part[:, :3], want[:, :3]))
    ego_ref.assert_close_to_reference(pairs, 'batched vs float64 statement')
    fresh = align_points_batched(d_all, rows, rec, 1)  # without out: a new [Q, F] tensor
    assert np.array_equal(bits(fresh.cpu().numpy()), bits(h[10:332]))


def test_operator_refuses_what_it_cannot_write(z):
    pts = torch.zeros(8, 3, device='cuda')
    rec = ego.transform_record([np.eye(3)], [np.zeros(3)], z['Tr_imu_to_velo'])[np.newaxis]
    with pytest.raises(ValueError):
        align_points_batched(pts, [0, 8], rec, 1, out=torch.zeros(7, 3, device='cuda'))          # too few rows
    with pytest.raises(ValueError):
        align_points_batched(pts, [0, 8], rec, 1, out=torch.zeros(12, 3, device='cuda'), out_row0=5)
    with pytest.raises(ValueError):
        align_points_batched(pts, [0, 8], rec, 1, out=torch.zeros(3, 8, device='cuda').t())      # inner stride != 1
    with pytest.raises(ValueError):
        align_points_batched(pts, [0, 7], rec, 1)                                                # offsets do not end at Q
    with pytest.raises(ValueError):
        align_points_batched(pts, [0, 8], rec, 5)
    with pytest.raises(ValueError):
        align_points_batched(pts, [0, 8], rec, 1, out=pts)                                       # not a separate buffer


# ---- the pipeline on a moving sequence --------------------------------------------------------------------------------
S = 32


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


@pytest.fixture(scope='module')
def moving():
    from mmmot_amd.pipeline import FrameFeed, SequencePipeline
    from mmmot_amd.synth import make_sequence
    model = TrackingNet(**KW)
    init_module(model, seed=0)
    model.eval().cuda()
    frames = make_sequence(4, n_pts=4000, det_range=(3, 4), ego=0)
    feeds = [FrameFeed(*f, pose=(f[2]['pos'], f[2]['rad'])) for f in frames]
    runs = {
        'overlap': SequencePipeline(model, S, overlap=True).run(feeds),
        'serial': SequencePipeline(model, S, overlap=False).run(feeds),
        'reuse': SequencePipeline(model, S, reuse_appearance=True).run(feeds),
        'offline': SequencePipeline(model, S).run_offline(feeds, frames_per_encode=2, pairs_per_forward=2),
    }
    return model, frames, feeds, runs


def _direct_inputs(frames, t):
    """crops, raw points of both frames, the joined split and the counts of pair (t-1, t), by the un-batched operators"""
    from mmmot_amd.crops import crop_resize_u8
    crops, pts, split, ns = [], [], [0], []
    for img, sweep, info, dets in frames[t - 1:t + 1]:
        crops.append(crop_resize_u8(torch.from_numpy(img).cuda(), dets['bbox'], S))
        pc = prep_points(torch.from_numpy(sweep).cuda(), info, dets, without_reflectivity=True)
        pts.append(pc['points'])
        split += [split[-1] + s for s in pc['points_split'][1:]]
        ns.append(len(dets['rotation_y']))
    return crops, pts, split, ns


def _motion(frames, t):
    (_, _, fa, _), (_, _, fb, _) = frames[t - 1], frames[t]
    return ego.pair_motion((fa['pos'], fa['rad']), (fb['pos'], fb['rad'])) + (fb['calib/Tr_imu_to_velo'],)


def test_every_order_gives_the_same_scores(moving):
    _, frames, _, runs = moving
    assert all(len(r) == len(frames) - 1 for r in runs.values())
    for name in ('serial', 'reuse', 'offline'):
        for t, (a, b) in enumerate(zip(runs['overlap'], runs[name])):
            assert _same(a, b), '%s differs from the overlapped run at pair %d' % (name, t + 1)


def test_pairs_equal_direct_calls_with_the_first_frame_raw(moving):
    """per pair: model(cat(crops_a, crops_b), points = cat(raw_a, align_points(raw_b))) - frame t goes in RAW as the
    first frame of pair t + 1, although the pair before used its aligned copy"""
    from mmmot_amd.tracker_glue import scores_for_solver
    model, frames, _, runs = moving
    for t in range(1, len(frames)):
        crops, pts, split, ns = _direct_inputs(frames, t)
        R, T, imu = _motion(frames, t)
        aligned = align_points([R], [T], imu, pts[1])
        assert not torch.equal(aligned, pts[1])
        det_info = {'points': torch.cat([pts[0], aligned]).unsqueeze(0),
                    'points_split': torch.tensor(split, dtype=torch.float32).unsqueeze(0).cuda()}
        with torch.no_grad():
            det, links, new, end, _ = model(torch.cat(crops), det_info, [torch.tensor([n]) for n in ns])
        assert _same(runs['overlap'][t - 1], scores_for_solver(det, links, new, end, model.test_mode)), t


def test_without_poses_the_scores_differ(moving):
    from mmmot_amd.pipeline import FrameFeed, SequencePipeline
    model, frames, _, runs = moving
    still = SequencePipeline(model, S).run([FrameFeed(*f) for f in frames])
    for t, (a, b) in enumerate(zip(runs['overlap'], still)):
        assert not torch.equal(a[1][0], b[1][0]), 'pair %d: the alignment left the link scores as they were' % (t + 1)


def test_one_pair_against_the_cpu_oracle(moving):
    from oracle import crops_ref
    from oracle import restatement as Rst
    model, frames, _, runs = moving
    t = 2
    crops, pts, split, ns = _direct_inputs(frames, t)
    R, T, imu = _motion(frames, t)
    pts_o = np.concatenate([pts[0].cpu().numpy(), ego_ref.align_points([R], [T], imu, pts[1].cpu().numpy())])
    crops_o = np.stack([crops_ref.to_tensor_normalize(u) for u in torch.cat(crops).cpu().numpy()])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    cfg = dict(fusion='C', affinity_op='multiply', softmax_mode='none', neg_threshold=0.2, score_arch='branch_cls')
    with torch.no_grad():
        o = Rst.tracking_forward(sd, cfg, torch.from_numpy(crops_o), torch.from_numpy(pts_o).unsqueeze(0),
                                 torch.tensor(split, dtype=torch.float32).unsqueeze(0), ns)
    tm = model.test_mode
    det_s, link_s, new_s, end_s = runs['overlap'][t - 1]
    errs = [(det_s - o[0][tm]).abs().max().item(), (link_s[0] - o[1][0][tm:tm + 1]).abs().max().item(),
            (new_s - o[2][tm]).abs().max().item(), (end_s - o[3][tm]).abs().max().item()]
    print('pair %d vs oracle: max |pipeline - oracle| det/link/new/end = %s' % (t, errs))
    assert max(errs) < TOL


def test_tracks_of_the_moving_sequence(moving):
    from mmmot_amd.pipeline import SequencePipeline
    model, frames, feeds, runs = moving
    pipe = SequencePipeline(model, S, associate=True, track=True)
    res = pipe.run(feeds)
    assert len(res) == 3 and all(_same(r[0], s) for r, s in zip(res, runs['overlap']))
    assert len(pipe.tracks) == 4
    for (_, _, _, dets), ids in zip(frames, pipe.tracks):
        assert ids.dtype == np.int64 and ids.shape == (len(dets['rotation_y']),)
    off = SequencePipeline(model, S, associate=True, track=True)
    off.run_offline(feeds, frames_per_encode=2, pairs_per_forward=2)
    assert all(np.array_equal(a, b) for a, b in zip(off.tracks, pipe.tracks))
