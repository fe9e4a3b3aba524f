"""mmmot_amd/train_pipeline.py on the device: a prepared sample equals the hand-composed calls tensor by tensor, the
overlapped order equals the serial one bit for bit (losses and parameters), a step equals the loop of INTEGRATION.md
section 5, and the forms of a sample (no augmentation, three frames, partial poses)."""
import numpy as np
import pytest
import torch

import labels_ref
from common import case_kwargs, get_case
from mmmot_amd import TrackingLoss, TrackingNet, augment, build_optim, ego, labels
from mmmot_amd.crops import augment_crops, crop_resize_normalize, crop_resize_u8
from mmmot_amd.pipeline import FrameFeed
from mmmot_amd.points import align_points, align_points_batched, prep_points_batched
from mmmot_amd.synth import make_sequence
from mmmot_amd.train_pipeline import TrainingPipeline, TrainSample
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = 32
SHIFT = np.array([[2, -2, 2, -2], [-2, 2, -2, 2], [2, 2, -2, -2], [-2, -2, 2, 2]], dtype=np.float64)
OPT = dict(lr_scheduler=dict(optim='Adam', base_lr=3e-4), weight_decay=0.01, fixed_wd=True)


@pytest.fixture(scope='module')
def frames():
    return make_sequence(4, 3, n_pts=4000, det_range=(3, 4), hw=(96, 128), ego=1)


def feed(frame, pose=True):
    img, sweep, info, dets = frame
    return FrameFeed(img, sweep, info, dets, pose=(info['pos'], info['rad']) if pose else None)


def gt_of(dets):
    """the detections' own boxes as ground truth: ids n-1 .. 0 in every frame (the last one, which wins a shared
    detection, is id 0 in all of them: frames link), all cars but the first"""
    n = len(dets['bbox'])
    name = np.full(n, labels.CAR, dtype=np.int64)
    name[0] = 3
    return {'bbox': np.asarray(dets['bbox'], dtype=np.float64).copy(), 'id': np.arange(n, dtype=np.int64)[::-1].copy(), 'name': name}


def sample_of(fr, pose=True, poses=None):
    poses = [pose] * len(fr) if poses is None else poses
    return TrainSample([feed(f, p) for f, p in zip(fr, poses)], [gt_of(f[3]) for f in fr],
                       [np.asarray(f[3]['bbox'], dtype=np.float64) + SHIFT[:len(f[3]['bbox'])] for f in fr])


def make_model(use_dropout=False, seq_len=2):
    c, base = get_case('s2_C_multiply_none')
    m = TrackingNet(**dict(case_kwargs(c, base), dropblock=0, use_dropout=use_dropout, seq_len=seq_len))
    init_module(m, 0)
    return m.to(DEV).train()


def make_pipe(model, **kw):
    crit = TrackingLoss(detloss_type='bce', linkloss_type='l2', det_ratio=1.5, trans_ratio=0.001)
    kw.setdefault('augment', augment.RandomResizedCropFlip(S))
    return TrainingPipeline(model, crit, build_optim(model, OPT), size=S, seed=5, **kw)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_prepare_equals_the_hand_composed_calls(frames):
    fr = frames[:2]
    sample = sample_of(fr)
    for overlap in (False, True):
        got = make_pipe(make_model(), overlap=overlap).prepare(sample)
        torch.cuda.synchronize()
        # ---- by hand ----
        shift = sample.shift_bboxes
        sweeps = [torch.from_numpy(f[1]).to(DEV) for f in fr]
        pcs = prep_points_batched(sweeps, [f[2] for f in fr], [f[3] for f in fr], without_reflectivity=True,
                                  shift_bboxes=shift)
        R, T = ego.pair_motion((fr[0][2]['pos'], fr[0][2]['rad']), (fr[1][2]['pos'], fr[1][2]['rad']))
        second = align_points([R], [T], fr[1][2]['calib/Tr_imu_to_velo'], pcs[1]['points'])
        points = torch.cat([pcs[0]['points'], second])
        split = pcs[0]['points_split'] + [pcs[0]['points_split'][-1] + s for s in pcs[1]['points_split'][1:]]
        u8 = torch.cat([crop_resize_u8(torch.from_numpy(f[0]).to(DEV), b, S) for f, b in zip(fr, shift)])
        params = augment.RandomResizedCropFlip(S).draw(u8.shape[0], torch.Generator().manual_seed(5))
        crops = augment_crops(u8, params)
        matched = labels.match_dets_batch(shift, [g['bbox'] for g in sample.gts], [g['id'] for g in sample.gts],
                                          [g['name'] for g in sample.gts])
        # ---- tensor by tensor ----
        assert np.array_equal(got['params'], params)
        assert torch.equal(bits(got['crops']), bits(crops))
        assert got['det_info']['points'].shape[0] == 1 and torch.equal(bits(got['det_info']['points'][0]), bits(points))
        assert not got['det_info']['points_split'].is_cuda
        assert got['det_info']['points_split'].reshape(-1).tolist() == [float(s) for s in split]
        assert [int(d) for d in got['det_split']] == [len(b) for b in shift]
        for t in range(2):
            assert got['det_id'][t].is_cuda and got['det_id'][t].shape == (1, len(shift[t]), 1)
            assert torch.equal(got['det_id'][t][0].cpu(), matched[t][0].cpu())
            assert torch.equal(got['det_cls'][t][0].cpu(), matched[t][1].cpu())
        # ... and what the host restatement of the matching gives; the jittered boxes still find ground truth
        for t in range(2):
            g = sample.gts[t]
            ids, cls = labels_ref.match_dets(shift[t], g['bbox'], g['id'], g['name'])
            assert got['det_id'][t].reshape(-1).tolist() == ids.tolist() and (ids >= 0).any()
            assert got['det_cls'][t].reshape(-1).tolist() == cls.tolist() and (cls == 1).any()
        assert not torch.equal(bits(second), bits(pcs[1]['points']))  # the alignment moved the second frame


def run_three(frames, overlap, use_dropout):
    torch.manual_seed(21)
    model = make_model(use_dropout)
    pipe = make_pipe(model, overlap=overlap)
    losses = pipe.run([sample_of(frames[k:k + 2]) for k in range(3)])
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, pipe


def test_overlap_equals_serial_bit_for_bit(frames):
    la, pa, pipe = run_three(frames, True, True)
    lb, pb, _ = run_three(frames, False, True)
    assert la.shape == (3,) and not la.is_cuda and bool(torch.isfinite(la).all()) and pipe.it == 3
    assert torch.equal(bits(la), bits(lb)), (la.tolist(), lb.tolist())
    assert set(pa) == set(pb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    lc, pc, _ = run_three(frames, True, False)  # without dropout the numbers differ: the draws of the first run were used
    assert not torch.equal(bits(la), bits(lc))


def test_step_equals_the_integration_loop(frames):
    sample = sample_of(frames[1:3])
    torch.manual_seed(8)
    ma = make_model()
    pa = make_pipe(ma, overlap=True)
    loss_a = pa.step(pa.prepare(sample))
    torch.manual_seed(8)
    mb = make_model()
    pb = make_pipe(mb, overlap=False)
    p = pb.prepare(sample)
    model, criterion, optimizer = mb, pb.criterion, pb.optimizer
    det_img, det_info, det_split, det_cls, det_id = p['crops'], p['det_info'], p['det_split'], p['det_cls'], p['det_id']
    # INTEGRATION.md section 5
    det_score, link_score, new_score, end_score, trans = model(det_img, det_info, det_split)
    gt_det, gt_link, gt_new, gt_end = labels.generate_gt(det_score[0], det_cls, det_id, det_split)
    loss = criterion(det_split, gt_det, gt_link, gt_new, gt_end, det_score, link_score, new_score, end_score, trans)
    optimizer.zero_grad(); loss.backward(); optimizer.step()
    torch.cuda.synchronize()
    assert loss_a.is_cuda and loss_a.dim() == 0 and not loss_a.requires_grad
    assert torch.equal(bits(loss_a.reshape(1)), bits(loss.reshape(1)))
    sa, sb = ma.state_dict(), mb.state_dict()
    moved = 0
    init = make_model().state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        moved += int(not torch.equal(sa[k], init[k]))
    assert moved > 50  # the step trained the network


def test_no_augmentation_feeds_the_evaluation_crops(frames):
    fr = frames[:2]
    sample = sample_of(fr)
    pipe = make_pipe(make_model(), augment=None, overlap=False)
    got = pipe.prepare(sample)
    want = torch.cat([crop_resize_normalize(torch.from_numpy(f[0]).to(DEV), b, S) for f, b in zip(fr, sample.shift_bboxes)])
    assert got['params'] is None and torch.equal(bits(got['crops']), bits(want))
    assert bool(torch.isfinite(pipe.step(got)))


def test_three_frames_with_poses(frames):
    fr = frames[:3]
    sample = sample_of(fr)
    pipe = make_pipe(make_model(seq_len=3), overlap=True)
    p = pipe.prepare(sample)
    loss = pipe.step(p)
    assert bool(torch.isfinite(loss)) and len(p['det_split']) == 3
    pcs = prep_points_batched([torch.from_numpy(f[1]).to(DEV) for f in fr], [f[2] for f in fr], [f[3] for f in fr],
                              without_reflectivity=True, shift_bboxes=sample.shift_bboxes)
    poses = [(f[2]['pos'], f[2]['rad']) for f in fr]
    steps = [ego.pair_motion(poses[k - 1], poses[k]) for k in (1, 2)]
    third = align_points([s[0] for s in steps], [s[1] for s in steps], fr[2][2]['calib/Tr_imu_to_velo'], pcs[2]['points'])
    n2 = int(third.shape[0])
    assert n2 > 0 and torch.equal(bits(p['det_info']['points'][0][-n2:]), bits(third))
    n0 = int(pcs[0]['points'].shape[0])
    assert torch.equal(bits(p['det_info']['points'][0][:n0]), bits(pcs[0]['points']))  # frame 0 stays raw


def test_partial_poses_are_refused(frames):
    with pytest.raises(ValueError):
        sample_of(frames[:2], poses=[True, False])
    with pytest.raises(ValueError):
        sample_of(frames[:3], poses=[True, True, False])
    s = sample_of(frames[:2], pose=False)  # none at all: nothing is aligned
    p = make_pipe(make_model(), overlap=False).prepare(s)
    pcs = prep_points_batched([torch.from_numpy(f[1]).to(DEV) for f in frames[:2]], [f[2] for f in frames[:2]],
                              [f[3] for f in frames[:2]], without_reflectivity=True, shift_bboxes=s.shift_bboxes)
    assert torch.equal(bits(p['det_info']['points'][0]), bits(torch.cat([pc['points'] for pc in pcs])))
