"""Track IDs on the device (csrc/track_ids.hip through mmmot::track_ids / mmmot_amd.tracks) against the fixtures the
reference produced (tests/golden/track_ids_*.npz): exact IDs, frame_start and last_id after every pair, whatever the
launch size and the kernel; state and outputs written in full; the error flag; the drop-in on host and device tensors;
and SequencePipeline(track=True) in its three orders against tests/tracking_ref.py.  Every comparison is exact."""
import glob
import os

import numpy as np
import pytest
import torch

from association_ref import random_instance
from tracking_ref import Tracker, check_pair, load_fixture, tracks_of
from mmmot_amd import TrackingNet
from mmmot_amd.association import pairs_table
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import TRACK_STATE_HEAD, TRACK_STATE_INTS, track_layout
from mmmot_amd.tracks import TrackingError, TrackState, assign_ids, track_ids
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'track_ids_*.npz')))
NAMES = [os.path.basename(f)[len('track_ids_'):-4] for f in FIXTURES]


def fixture(name):
    return load_fixture(os.path.join(GOLDEN, 'track_ids_%s.npz' % name))[0]


def walk(pairs, B, max_nm=0, state=None, check=True):
    """the sequence through assign_ids in launches of B pairs; returns the state"""
    state = TrackState('cuda') if state is None else state
    for g in range(0, len(pairs), B):
        grp = pairs[g:g + B]
        blocks = torch.from_numpy(np.concatenate([p['block'] for p in grp])).cuda()
        got = assign_ids(state, blocks, [(p['N'], p['M']) for p in grp], [(p['f0'], p['f1']) for p in grp], max_nm)
        assert len(got) == len(grp)
        if check:
            for p, (ids0, ids1, start, last) in zip(grp, got):
                check_pair(p, ids0, ids1, start, last)
    return state


@pytest.mark.parametrize('variant', ['auto', 'four_waves'])
@pytest.mark.parametrize('B', [1, 8, 0], ids=['B1', 'B8', 'whole'])
@pytest.mark.parametrize('path', FIXTURES, ids=NAMES)
def test_fixture_sequences_equal_the_reference(path, B, variant):
    pairs, z = load_fixture(path)
    state = walk(pairs, B or len(pairs), 0 if variant == 'auto' else 512)
    s = state.read()
    assert s['flags'] == 0 and s['last_id'] == int(z['last_id'][-1])


@pytest.mark.parametrize('name', NAMES)
def test_state_after_one_launch_equals_state_after_single_launches(name):
    pairs = fixture(name)
    one = walk(pairs, len(pairs), check=False).buf.cpu()
    many = walk(pairs, 1, check=False).buf.cpu()
    mixed = walk(pairs, 3, 512, check=False).buf.cpu()
    assert torch.equal(one, many) and torch.equal(one, mixed)


@pytest.mark.parametrize('fill', [0xFF, 0x7B])
@pytest.mark.parametrize('max_nm', [0, 512])
def test_workspace_poison_ids_and_state_written_in_full(fill, max_nm):
    """the raw entry point over poisoned buffers: every output int and the whole state block are written"""
    ops = HipOps()
    for name in ('start', 'n12x100'):
        pairs = fixture(name)
        splits = [(p['N'], p['M']) for p in pairs]
        table, _ = pairs_table(splits)
        fidx = torch.tensor([(p['f0'], p['f1']) for p in pairs], dtype=torch.int32)
        blocks = torch.from_numpy(np.concatenate([p['block'] for p in pairs])).cuda()
        total, off, need = track_layout(table, fidx, blocks.numel())
        res = []
        for f in (0, fill):
            ids = torch.empty(total, dtype=torch.int32, device='cuda')
            state = torch.empty(TRACK_STATE_INTS, dtype=torch.int32, device='cuda')
            ids.view(torch.uint8).fill_(f)
            state.view(torch.uint8).fill_(f)
            state[:TRACK_STATE_HEAD] = torch.tensor([0, -1, 0, 0], dtype=torch.int32)  # a new sequence; the IDs stay poisoned
            ops.track_ids(blocks, table.reshape(-1).cuda(), off.to(torch.int32).cuda(), fidx.reshape(-1).cuda(), len(pairs),
                          max_nm or need, state, ids)
            torch.cuda.synchronize()
            res.append((ids.cpu(), state.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        want = walk(pairs, len(pairs)).buf.cpu()
        assert torch.equal(res[1][1], want)
        o = 0
        for p in pairs:  # and they are the reference's
            N, M = p['N'], p['M']
            r = res[1][0][o:o + N + M + 2].numpy()
            check_pair(p, r[:N], r[N:N + M], int(r[N + M]), int(r[N + M + 1]))
            o += N + M + 2
        assert o == total


def test_infeasible_assignment_sets_the_flag_and_raises():
    """an error return, not a device fault: the device stays usable and a valid pair still runs afterwards"""
    cases = [
        # a kept second-frame detection that is neither new nor linked
        (2, 1, [1, 1, 1], [1, 1, 0], np.zeros((2, 1))),
        # linked twice
        (2, 1, [1, 1, 1], [1, 1, 0], np.ones((2, 1))),
        # linked from a rejected row
        (2, 2, [0, 1, 1, 1], [0, 1, 0, 1], np.array([[1, 0], [0, 0]])),
    ]
    for N, M, det, new, link in cases:
        state = TrackState('cuda')
        block = np.concatenate([det, new, det, np.asarray(link).reshape(-1)]).astype(np.float32)
        with pytest.raises(TrackingError):
            assign_ids(state, torch.from_numpy(block).cuda(), [(N, M)], [(0, 1)])
        assert state.read()['flags'] == 1
        state.reset()
        assert torch.equal(state.buf.cpu(), TrackState('cuda').buf.cpu())
    torch.cuda.synchronize()
    walk(fixture('start'), 4)
    # the host-side drop-in raises as well
    with pytest.raises(TrackingError):
        t = lambda x: torch.tensor(x, dtype=torch.float32)
        track_ids(TrackState('cuda'), t([1, 1, 1]), [torch.zeros(1, 2, 1)], t([1, 1, 0]), t([1, 1, 1]), [2, 1], (0, 1))


def test_table_checks_come_before_any_launch():
    state = TrackState('cuda')
    blocks = torch.zeros(3 * 5 + 6, device='cuda')
    with pytest.raises(ValueError):
        assign_ids(state, blocks, [(2, 513)], [(0, 1)])
    with pytest.raises(ValueError):
        assign_ids(state, blocks[:5], [(2, 3)], [(0, 1)])       # the blocks are shorter than the table says
    with pytest.raises(ValueError):
        assign_ids(state, blocks, [(2, 3)], [(0, 1), (1, 2)])   # frame indices for another number of pairs
    with pytest.raises(ValueError):
        assign_ids(state, blocks, [(2, 3)], [(-1, 0)])
    with pytest.raises(ValueError):
        assign_ids(state, blocks, [(2, 3)], [(0, 1)], max_nm=2)
    assert torch.equal(state.buf.cpu(), TrackState('cuda').buf.cpu())


@pytest.mark.parametrize('name', ['start', 'kitti'])
def test_track_ids_host_and_device_tensors(name):
    pairs = fixture(name)
    host, dev = TrackState('cuda'), TrackState('cuda')
    t = torch.from_numpy
    for p in pairs:
        N, M = p['N'], p['M']
        args = (t(p['det']), [t(p['link']).view(1, N, M)], t(p['new']), t(p['end']))
        split = [torch.tensor([N]), torch.tensor([M])]
        a, sa = track_ids(host, *args, split, (p['f0'], p['f1']))
        cu = (args[0].cuda(), [args[1][0].cuda()], args[2].cuda(), args[3].cuda())
        b, sb = track_ids(dev, *cu, split, (p['f0'], p['f1']))
        assert sa == sb == p['frame_start'] and len(a) == len(b) == len(p['emitted']) == (1 if sa else 2)
        for x, y, w, n in zip(a, b, p['emitted'], ([M] if sa else [N, M])):
            assert x.dtype == torch.int64 and x.device.type == 'cpu' and x.shape == (n,) and torch.equal(x, y)
            assert np.array_equal(x.numpy()[x.numpy() >= 0], w)
    assert torch.equal(host.buf.cpu(), dev.buf.cpu()) and host.read()['last_id'] == pairs[-1]['last_id']


# ---- end to end: SequencePipeline(track=True) ----------------------------------------------------------------------
KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True, appear_fpn=False,
          point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg', test_mode=2,
          neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='A', affinity_op='multiply',
          softmax_mode='none')
S = 64
_FEEDS = []


def feeds():
    if not _FEEDS:
        from mmmot_amd.pipeline import FrameFeed
        from mmmot_amd.synth import make_frame
        _FEEDS.extend(FrameFeed(*make_frame(300 + t, 20000, 4 + t % 4)) for t in range(11))
    return _FEEDS


def model():
    m = TrackingNet(**KW)
    init_module(m, seed=0)
    return m.eval().cuda()


def same_results(a, b):
    assert len(a) == len(b)
    for (sa, aa), (sb, ab) in zip(a, b):
        for x, y in zip((sa[0], sa[1][0], sa[2], sa[3], aa[0], aa[1][0], aa[2], aa[3]),
                        (sb[0], sb[1][0], sb[2], sb[3], ab[0], ab[1][0], ab[2], ab[3])):
            assert torch.equal(x, y)


def ref_tracks(res, fs):
    return tracks_of([(a[0].numpy(), a[1][0].numpy(), a[2].numpy()) for _, a in res], [len(f.dets['bbox']) for f in fs])


def same_tracks(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == np.int64 and np.array_equal(x, y), (x, y)


def test_sequence_pipeline_tracks_in_three_orders():
    from mmmot_amd.pipeline import SequencePipeline
    fs, m = feeds(), model()
    runs = {
        'run': (lambda p, **k: p.run(fs, **k), {}),
        'online': (lambda p, **k: p.run(fs, **k), {'reuse_appearance': True}),
        'offline': (lambda p, **k: p.run_offline(fs, frames_per_encode=4, pairs_per_forward=8, **k), {}),
    }
    tracks = {}
    for name, (run, kw) in runs.items():
        plain = run(SequencePipeline(m, S, associate=True, **kw))
        pipe = SequencePipeline(m, S, associate=True, track=True, **kw)
        seen = []
        got = run(pipe, on_tracks=lambda t, ids: seen.append((t, ids.copy())))
        same_results(got, plain)
        assert len(pipe.tracks) == len(fs) and all(len(x) == len(f.dets['bbox']) for x, f in zip(pipe.tracks, fs))
        same_tracks(pipe.tracks, ref_tracks(got, fs))
        last = {}
        for t, ids in seen:   # the callback saw every frame, and its last emission is what stands
            last[t] = ids
        assert sorted(last) == list(range(len(fs)))
        same_tracks([last[t] for t in range(len(fs))], pipe.tracks)
        tracks[name] = pipe.tracks
        # a second run on the same pipeline starts a new sequence
        run(pipe)
        same_tracks(pipe.tracks, tracks[name])
    same_tracks(tracks['run'], tracks['online'])
    same_tracks(tracks['run'], tracks['offline'])
    assert any((x >= 0).any() for x in tracks['run'])


def test_queue_solve_with_an_empty_frame():
    """a frame without detections is answered on the host; its IDs still come from the kernel and the state"""
    from mmmot_amd.tracker_glue import queue_solve
    rng = np.random.default_rng(3)
    t = lambda x: torch.from_numpy(x).cuda()
    state, ref, counts = TrackState('cuda'), Tracker(), [4, 0, 3, 5]
    for p in range(3):
        N, M = counts[p], counts[p + 1]
        det, new, end, link = (t(x) for x in random_instance(rng, N, M, 1.0, 'eval'))
        sel = [(det, [link.view(1, N, M)], new, end)]
        plain = queue_solve(sel, [(N, M)]).fetch()[0]
        sc, asg, (ids0, ids1, start, last) = queue_solve(sel, [(N, M)], track=state, frame_idx=[(p, p + 1)]).fetch()[0]
        assert all(torch.equal(x, y) for x, y in zip((asg[0], asg[1][0], asg[2], asg[3]),
                                                     (plain[1][0], plain[1][1][0], plain[1][2], plain[1][3])))
        w0, w1, ws = ref.pair(asg[0].numpy(), asg[1][0].numpy(), asg[2].numpy(), N, M, p, p + 1)
        assert np.array_equal(ids0, w0) and np.array_equal(ids1, w1) and start == ws and last == ref.last_id


def test_queue_solve_with_a_pair_without_detections():
    """N = M = 0 between two ordinary pairs of the `start` fixture: the empty pair has no solver block at all, and its
    IDs (none), frame_start, last_id and the state still come from the kernel - an empty ``blocks`` is not a null
    pointer.  Expected: tests/tracking_ref.Tracker over the same three pairs."""
    from mmmot_amd.tracker_glue import queue_solve
    first, third = fixture('start')[:2]
    state, ref = TrackState('cuda'), Tracker()
    empty = torch.empty(0, device='cuda')
    for p in (first, None, third):
        if p is None:
            f0, f1 = 1000, 1001   # frames of their own: the stored frame has detections, this one has none
            r = queue_solve([(empty, [empty.view(1, 0, 0)], empty, empty)], [(0, 0)], track=state, frame_idx=[(f0, f1)])
            sc, asg, (ids0, ids1, start, last) = r.fetch()[0]
            assert sc[0].numel() == 0 and asg[0].numel() == 0 and asg[1][0].shape == (1, 0, 0)
            w0, w1, ws = ref.pair(np.zeros(0), np.zeros((0, 0)), np.zeros(0), 0, 0, f0, f1)
        else:
            ids0, ids1, start, last = assign_ids(state, torch.from_numpy(p['block']).cuda(), [(p['N'], p['M'])],
                                                 [(p['f0'], p['f1'])])[0]
            w0, w1, ws = ref.pair(p['det'], p['link'], p['new'], p['N'], p['M'], p['f0'], p['f1'])
        assert ids0.dtype == np.int64 and np.array_equal(ids0, w0) and np.array_equal(ids1, w1)
        assert start == ws and last == ref.last_id
    s = state.read()
    assert s['flags'] == 0 and s['last_id'] == ref.last_id and s['frame'] == ref.stored
    assert np.array_equal(s['ids'], ref.stored_ids)


def test_forced_recompute_gives_the_same_tracks():
    """rows made stale between a pair's hand-off and its check (a trunk change, the mechanism of
    tests/test_appearance_reuse_gpu.py): the pair is computed again and its IDs start from the state before it"""
    from mmmot_amd.pipeline import SequencePipeline
    fs = feeds()[:7]

    def at(m, when):
        def on_scores(t, sc):
            if t == when:
                m.set_trunk('f32')
        return on_scores
    m = model()
    calm = SequencePipeline(m, S, associate=True, track=True)
    want = calm.run(fs, on_scores=at(m, 2))   # undisturbed: the per-pair order, pairs 3.. in the new arithmetic

    m = model()
    pipe = SequencePipeline(m, S, associate=True, track=True, reuse_appearance=True)
    real, calls = pipe.finish_hand_off, []

    def finish(pending):
        r = real(pending)
        calls.append(1)
        if len(calls) == 3:   # pair 3 is on the host, its check has not run yet
            m.set_trunk('f32')
        return r
    pipe.finish_hand_off = finish
    got = pipe.run(fs)
    assert pipe.stats['recomputed_pairs'] == 1 and len(calls) == len(fs)
    same_results(got, want)
    same_tracks(pipe.tracks, calm.tracks)
    same_tracks(pipe.tracks, ref_tracks(got, fs))
