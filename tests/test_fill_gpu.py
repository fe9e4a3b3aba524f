"""Gap filling on the device (csrc/fill_tracks.hip through HipOps.fill_tracks, mmmot::fill_tracks and
mmmot_amd.tracks.fill_gaps) against the NumPy restatement tests/fill_ref.py: BIT FOR BIT on out, out_id, out_src,
fill_start and info, between NaN guard rows behind ``capacity``, and twice for bit equality of two calls.  Then the
evaluators before and after filling, and ``SequencePipeline.run_global(fill=)``."""
import numpy as np
import pytest
import torch

import fill_cases
import fill_ref
from mmmot_amd import evaluate as E
from mmmot_amd import torch_ops, tracks

pytestmark = pytest.mark.gpu

GUARD = 5
SENTINEL = -77


def device_fill(t, max_fill, xf=None, capacity=0, nulls=(), S=None):
    """one call of the entry on fresh buffers: (status, {fill_start, out, out_id, out_src, info} as host arrays, rows
    behind ``capacity`` included)"""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    L, F = len(t['ids']), len(t['frame_no'])
    S = len(t['seq_start']) - 1 if S is None else S
    a = dict(det=dev(t['det'].reshape(-1), np.float32), ids=dev(t['ids'], np.int32),
             frame_start=dev(t['frame_start'], np.int32), frame_no=dev(t['frame_no'], np.int32),
             seq_start=dev(t['seq_start'], np.int32), xf=None if xf is None else dev(xf.reshape(-1), np.float64),
             wtab=dev(fill_ref.weights().reshape(-1), np.float64),
             work=torch.empty(3 * L + 1, dtype=torch.int32, device='cuda'),
             fill_start=torch.full((F + 1,), SENTINEL, dtype=torch.int32, device='cuda'),
             out=torch.full(((capacity + GUARD) * 12,), float('nan'), dtype=torch.float32, device='cuda'),
             out_id=torch.full((capacity + GUARD,), SENTINEL, dtype=torch.int32, device='cuda'),
             out_src=torch.full(((capacity + GUARD) * 2,), SENTINEL, dtype=torch.int32, device='cuda'),
             info=torch.full((max(S, 1) * 4,), SENTINEL, dtype=torch.int32, device='cuda'))
    for k in nulls:
        a[k] = None
    st = torch_ops._ops().fill_tracks(a['det'], a['ids'], a['frame_start'], a['frame_no'], a['seq_start'], a['xf'],
                                      a['wtab'], L, F, S, max_fill, capacity, a['work'], a['fill_start'], a['out'],
                                      a['out_id'], a['out_src'], a['info'])
    torch.cuda.synchronize()
    host = {k: a[k].cpu().numpy() for k in ('fill_start', 'out', 'out_id', 'out_src', 'info') if a[k] is not None}
    return st, host


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(t, max_fill, xf=None, capacity=None):
    """the device against the restatement, bit for bit, twice; returns the restatement's result"""
    w = fill_ref.weights()
    full = fill_ref.fill(t['det'], t['ids'], t['frame_start'], t['frame_no'], t['seq_start'], xf, w, max_fill, 10 ** 9)
    capacity = int(full['fill_start'][-1]) if capacity is None else capacity
    want = fill_ref.fill(t['det'], t['ids'], t['frame_start'], t['frame_no'], t['seq_start'], xf, w, max_fill, capacity)
    n = len(want['out'])
    assert n <= capacity
    runs = [device_fill(t, max_fill, xf, capacity) for _ in range(2)]
    for st, got in runs:
        assert st == 0
        out = got['out'].reshape(-1, 12)
        assert np.array_equal(bits(out[:n]), bits(want['out'])), np.abs(out[:n] - want['out']).max()
        assert np.array_equal(got['out_id'][:n], want['out_id'])
        assert np.array_equal(got['out_src'].reshape(-1, 2)[:n], want['out_src'])
        assert np.array_equal(got['fill_start'], want['fill_start'])
        assert np.array_equal(got['info'].reshape(-1, 4), want['info'])
        # nothing behind the rows a call owes: the rest of the capacity and the guard rows are as they were
        assert np.isnan(out[n:]).all() and (got['out_id'][n:] == SENTINEL).all() and (got['out_src'][2 * n:] == SENTINEL).all()
    for k in runs[0][1]:
        assert np.array_equal(bits(runs[0][1][k]), bits(runs[1][1][k])), k
    return want


def seq(seed, n_frames=30, n_tracks=6, **kw):
    return fill_cases.random_sequence(np.random.default_rng(seed), n_frames, n_tracks, **kw)


WIDE = [(0, list(range(70))), (1, list(range(0, 70, 2)) + [-1] * 8), (3, [-1] * 3),
        (4, list(range(69, -1, -1)))]  # 70 detections a frame, 35 of them missed in frame 1, all in frame 3
SMALL = {
    'descending ids, three holes in one frame': [[(10, [7, 3, 5, -1]), (11, [-1]), (12, [5, -1, 7, 3])]],
    'unlisted frame numbers': [[(0, [1]), (3, []), (4, [-1]), (6, [1])]],
    'adjacent links a . b . . c': [[(0, [9]), (1, []), (2, [9]), (3, []), (4, []), (5, [9])]],
    'rejected and foreign ids': [[(0, [-1, 4]), (1, []), (2, [-1])], [(3, []), (4, [4])]],
    'hole in a frame without detections': [[(0, [2, 1]), (1, []), (2, []), (3, [1, 2])]],
    'more than a wave': [WIDE],
    'random': [seq(11)],
    'random, two sequences': [seq(12, 17), seq(13, 40, 8)],
}


@pytest.mark.parametrize('name', list(SMALL))
def test_against_the_restatement(name):
    want = check(fill_cases.tables(SMALL[name]), 7)
    if name != 'rejected and foreign ids':
        assert len(want['out']) > 0
    if name == 'more than a wave':
        assert want['fill_start'].tolist() == [0, 0, 35, 105, 105]


@pytest.mark.parametrize('max_fill', [1, 3, 30])
def test_max_fill_limits(max_fill):
    # links of n = 2 .. 33 frame numbers, with every frame between listed (empty): n <= max_fill + 1 are filled
    s = [(0, list(range(2, 34)))] + [(k, [k] if k >= 2 else []) for k in range(1, 34)]
    want = check(fill_cases.tables([s]), max_fill)
    filled = max_fill  # n = 2 .. max_fill + 1
    assert want['info'].tolist() == [[0, sum(range(1, max_fill + 1)), filled, 32 - filled]]


def test_standing_camera_equals_identity_records():
    t = fill_cases.tables([seq(21), seq(22, 12)])
    still = check(t, 7)
    ident = check(t, 7, fill_cases.identity_records(len(t['frame_no']), 7))
    assert len(still['out']) > 10 and all(np.array_equal(bits(still[k]), bits(ident[k])) for k in still)


@pytest.mark.parametrize('max_fill', [7, 30])
def test_moving_camera(max_fill):
    t = fill_cases.tables([seq(31, 40, p_miss=0.4), seq(32, 20)])
    xf = fill_cases.motion_records(60, max_fill, 3, t['seq_start'])
    want = check(t, max_fill, xf)
    still = fill_ref.fill(t['det'], t['ids'], t['frame_start'], t['frame_no'], t['seq_start'], None, fill_ref.weights(),
                          max_fill, 10 ** 9)
    assert len(want['out']) > 20 and np.abs(want['out'][:, 7:10] - still['out'][:, 7:10]).max() > 0.5  # it did move


def test_five_sequences_in_one_launch_equal_five_calls():
    seqs = [seq(41, 20), [], seq(42, 9), [(5, [-1, -1]), (6, []), (7, [-1])], seq(43, 33, 7)]
    t = fill_cases.tables(seqs)
    xf = fill_cases.motion_records(len(t['frame_no']), 7, 5, t['seq_start'])
    want = check(t, 7, xf)
    assert want['info'][:, 1].tolist()[1] == want['info'][:, 1].tolist()[3] == 0 and (want['info'][[0, 2, 4], 1] > 0).all()
    r = 0
    for s, one in enumerate(seqs):
        f0, f1 = t['seq_start'][s], t['seq_start'][s + 1]
        d0, d1 = t['frame_start'][f0], t['frame_start'][f1]
        sub = dict(det=t['det'][d0:d1], ids=t['ids'][d0:d1], frame_start=t['frame_start'][f0:f1 + 1] - d0,
                   frame_no=t['frame_no'][f0:f1], seq_start=np.asarray([0, f1 - f0], np.int32))
        n = int(want['info'][s, 1])
        st, got = device_fill(sub, 7, xf[f0:f1], n)
        assert st == 0
        if f1 == f0 or d1 == d0:  # nothing to launch: a no-op
            assert n == 0
            continue
        assert np.array_equal(bits(got['out'].reshape(-1, 12)[:n]), bits(want['out'][r:r + n]))
        assert np.array_equal(got['out_id'][:n], want['out_id'][r:r + n])
        assert np.array_equal(got['out_src'].reshape(-1, 2)[:n], want['out_src'][r:r + n] - d0)
        assert np.array_equal(got['fill_start'], want['fill_start'][f0:f1 + 1] - want['fill_start'][f0])
        assert np.array_equal(got['info'], want['info'][s])
        r += n


def test_status_words():
    ok = [(0, [1]), (1, []), (2, [1])]
    # a planted duplicate: that sequence only
    want = check(fill_cases.tables([ok, [(0, [2, 5, 2]), (1, []), (2, [2, 5])], ok]), 7)
    assert want['info'].tolist() == [[0, 1, 1, 0], [fill_ref.EDUP, 0, 0, 0], [0, 1, 1, 0]]
    # one row too few: the guard rows stay, the counts are reported
    t = fill_cases.tables([seq(51), seq(52, 12)])
    full = check(t, 7)
    rows = int(full['fill_start'][-1])
    want = check(t, 7, capacity=rows - 1)
    assert want['info'][:, 0].tolist() == [0, fill_ref.ECAPACITY] and np.array_equal(want['info'][:, 1:], full['info'][:, 1:])
    want = check(t, 7, capacity=0)
    assert want['info'][:, 0].tolist() == [fill_ref.ECAPACITY] * 2
    # decreasing frame numbers
    want = check(fill_cases.tables([ok, [(4, [1]), (3, []), (5, [1])], [(7, [3]), (7, []), (9, [3])]]), 7)
    assert want['info'].tolist() == [[0, 1, 1, 0], [fill_ref.ECONTRACT, 0, 0, 0], [fill_ref.ECONTRACT, 0, 0, 0]]
    # tables that are not prefixes stop the whole call, and nothing is read through them
    for key, bad in (('frame_start', [0, 2, 1, 2]), ('frame_start', [0, 1, 1, 9]), ('seq_start', [1, 3]), ('seq_start', [0, 2])):
        t = fill_cases.tables([ok])
        t[key] = np.asarray(bad, np.int32)
        want = check(t, 7)
        assert want['info'].tolist() == [[fill_ref.ECONTRACT, 0, 0, 0]] and len(want['out']) == 0
    # the Python surface raises
    d = {'bbox': np.zeros((2, 4)), 'dimensions': np.ones((2, 3)), 'location': np.ones((2, 3)), 'rotation_y': np.zeros(2)}
    with pytest.raises(tracks.TrackingError, match='sequence 1.*twice'):
        tracks.fill_gaps_batch([([d, d], [[0, 1], [1, 0]]), ([d, d], [[3, 3], [3, 4]])])
    with pytest.raises(tracks.TrackingError, match='do not increase'):
        tracks.fill_gaps([d, d], [[0, 1], [1, 0]], frame_idx=[3, 2])


def test_what_the_launcher_refuses():
    t = fill_cases.tables([[(0, [1]), (1, []), (2, [1])]])
    assert device_fill(t, 7, capacity=1)[0] == 0
    for k in ('det', 'ids', 'frame_start', 'frame_no', 'seq_start', 'wtab', 'work', 'fill_start', 'out', 'out_id',
              'out_src', 'info'):
        st, got = device_fill(t, 7, capacity=1, nulls=(k,))
        assert st == -1, k
        assert all((v == SENTINEL).all() if v.dtype == np.int32 else np.isnan(v).all() for v in got.values())  # no launch
    for max_fill in (0, 31, -1):
        assert device_fill(t, max_fill, capacity=1)[0] == -1
    assert device_fill(t, 7, capacity=1, S=0)[0] == -1
    with pytest.raises(ValueError):
        torch.ops.mmmot.fill_tracks(torch.zeros(10, dtype=torch.int32, device='cuda'), [2, 3, 1, 7, 1, 0])
    with pytest.raises(ValueError):
        torch.ops.mmmot.fill_tracks(torch.zeros(10, dtype=torch.int32, device='cuda'), [2, 3, 1, 31, 1, 0])


def test_meta_kernel_and_no_cpu_kernel():
    p = tracks.pack_fill([fill_cases.scene(True)], 3)
    out = torch.ops.mmmot.fill_tracks(torch.empty(len(p['packed']), dtype=torch.int32, device='meta'), p['sizes'])
    assert out.device.type == 'meta' and out.shape == (torch_ops.fill_layout(p['sizes'])[3],)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mmmot.fill_tracks(torch.from_numpy(p['packed']), p['sizes'])


def same_filled(a, b):
    assert a.info == b.info and len(a.frames) == len(b.frames) and (a.scores is None) == (b.scores is None)
    for t in range(len(a.frames)):
        assert set(a.frames[t]) == set(b.frames[t])
        for k in a.frames[t]:
            x, y = np.asarray(a.frames[t][k]), np.asarray(b.frames[t][k])
            assert x.dtype == y.dtype and np.array_equal(x, y), (t, k)
        assert np.array_equal(a.ids[t], b.ids[t]) and np.array_equal(a.filled[t], b.filled[t])
        assert np.array_equal(a.src[t], b.src[t])
        assert a.scores is None or np.array_equal(a.scores[t], b.scores[t])


def test_fill_gaps_and_batch_equal_the_host_route():
    from test_fill_cpu import moving_sequence
    frames, ids, frame_idx, scores, poses = moving_sequence()
    seqs = [(frames, ids, frame_idx, scores, poses, fill_cases.CALIB), fill_cases.scene(True), (frames[:9], ids[:9], frame_idx[:9]),
            dict(frames=[], ids=[])]
    want = fill_cases.host_fill(seqs)[2]
    got = tracks.fill_gaps_batch(seqs)
    assert len(got) == 4 and got[0].info['rows'] > 5 and got[3].frames == []
    for g, w in zip(got, want):
        same_filled(g, w)
    # per sequence what fill_gaps returns for it alone, bit for bit - a moving one and standing ones
    same_filled(tracks.fill_gaps(frames, ids, frame_idx, scores, poses, fill_cases.CALIB), got[0])
    same_filled(tracks.fill_gaps(*fill_cases.scene(True)), got[1])
    same_filled(tracks.fill_gaps(frames[:9], ids[:9], frame_idx[:9]), got[2])


def test_evaluators_get_the_recall_back():
    gt_frames, gt_ids = fill_cases.scene(False)
    frames, ids = fill_cases.scene(True)
    n = fill_cases.N_FRAMES
    gt = E.labels_from_tracks(gt_frames, gt_ids, ground_truth=True, box3d=True)
    ft = tracks.fill_gaps(frames, ids, max_fill=3)
    holes = sum(len(fill_cases.scene_holes(o)) for o in range(fill_cases.N_OBJ))
    assert ft.info == {'rows': holes, 'links_filled': 2 * fill_cases.N_OBJ, 'links_too_long': 0}
    for ev in (lambda tr: E.evaluate_sequences(gt, tr), lambda tr: E.evaluate_3d_sequences(gt, tr, overlap='3d').all):
        before = ev(E.labels_from_tracks(frames, ids, n_frames=n, box3d=True))
        after = ev(E.labels_from_tracks(ft.frames, ft.ids, n_frames=n, box3d=True))
        assert before.fn == holes and before.fragments > 0 and before.fp == 0 and before.MOTA < 1.0
        assert after.fn == 0 and after.fp == 0 and after.fragments == 0 and after.id_switches == 0 and after.MOTA == 1.0


def test_run_global_fill():
    from test_pipeline_gap_gpu import S, model
    from mmmot_amd.pipeline import FrameFeed, SequencePipeline
    from mmmot_amd.synth import make_sequence
    from test_lockstep_gpu import shaped
    frames = make_sequence(8, seed=23, n_pts=4000, det_range=(2, 5), hw=(120, 400), ego=1)
    feeds = [FrameFeed(img, sweep, info, shaped(dets, 0 if t == 5 else None), pose=(info['pos'], info['rad']))
             for t, (img, sweep, info, dets) in enumerate(frames)]
    plain, filled = SequencePipeline(model(), S), SequencePipeline(model(), S)
    a = plain.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=3)
    b = filled.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=3, fill=7)
    # without fill: the parent's result; with it: the same solve, and no further forward
    assert a.filled is None and plain.stats == filled.stats
    assert a.objective == b.objective and a.n_tracks == b.n_tracks and a.split == b.split
    assert all(np.array_equal(x, y) for x, y in zip(a.ids, b.ids))
    assert all(torch.equal(x, y) for x, y in zip(a.scores[0:1] + a.scores[2:], b.scores[0:1] + b.scores[2:]))
    assert all(np.array_equal(x, y) for x, y in zip(plain.tracks, filled.tracks)) and len(filled.tracks) == 8
    by_hand = tracks.fill_gaps([f.dets for f in feeds], filled.tracks, poses=[f.pose for f in feeds], calib=feeds[0].info,
                               max_fill=7)
    same_filled(b.filled, by_hand)
    assert len(b.filled.frames) == 8 and b.filled.scores is None
    assert all(len(i) == len(d['bbox']) for i, d in zip(b.filled.ids, b.filled.frames))
    # a track that crosses the emptied frame 5 has a box there now
    crossing = set(np.concatenate(filled.tracks[:5]).tolist()) & set(np.concatenate(filled.tracks[6:]).tolist()) - {-1}
    assert set(b.filled.ids[5].tolist()) >= crossing and b.filled.filled[5].all()
    with pytest.raises(ValueError, match='fill must lie in 0 .. 30'):
        plain.run_global(feeds, fill=31)
