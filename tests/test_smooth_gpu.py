"""Track smoothing on the device (csrc/smooth_tracks.hip through HipOps.smooth_tracks, mmmot::smooth_tracks and
mmmot_amd.tracks.smooth_tracks) against the NumPy restatement tests/smooth_ref.py: BIT FOR BIT on out, out_vel and info,
between NaN guard rows behind the L rows, and twice for bit equality of two calls.  Then the shared header's other user
(mmmot_fill_tracks), the 3D evaluator before and after smoothing, and ``SequencePipeline.run_global(smooth=)``."""
import numpy as np
import pytest
import torch

import fill_cases
import smooth_cases as C
import smooth_ref as R
from mmmot_amd import evaluate as E
from mmmot_amd import torch_ops, tracks

pytestmark = pytest.mark.gpu

GUARD = 3
SENTINEL = -77
bits = C.bits


def device_smooth(t, observed=None, xf0=None, nulls=(), S=None, work_offset=0, L=None, F=None, **prm):
    """one call of the entry on fresh buffers: (status, {out, vel, info} as host arrays, the guard rows included)"""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    prm = dict(R.DEFAULT, **prm)
    n = len(t['ids'])  # the buffers are those of the tables, whatever L / F / S the call claims
    L = n if L is None else L
    F = len(t['frame_no']) if F is None else F
    S = len(t['seq_start']) - 1 if S is None else S
    a = dict(det=dev(t['det'].reshape(-1), np.float32), ids=dev(t['ids'], np.int32),
             frame_start=dev(t['frame_start'], np.int32), frame_no=dev(t['frame_no'], np.int32),
             seq_start=dev(t['seq_start'], np.int32),
             observed=None if observed is None else dev(observed, np.int32),
             xf0=None if xf0 is None else dev(xf0.reshape(-1), np.float64),
             work=torch.empty(75 * n + 2 + 2, dtype=torch.int32, device='cuda')[work_offset:],
             out=torch.full(((n + GUARD) * 12,), float('nan'), dtype=torch.float32, device='cuda'),
             out_vel=torch.full(((n + GUARD) * 4,), float('nan'), dtype=torch.float32, device='cuda'),
             info=torch.full((max(S, 1) * 4,), SENTINEL, dtype=torch.int32, device='cuda'))
    for k in nulls:
        a[k] = None
    st = torch_ops._ops().smooth_tracks(a['det'], a['ids'], a['frame_start'], a['frame_no'], a['seq_start'], a['observed'],
                                        a['xf0'], L, F, S, [prm[k] for k in R.PARAMS], int(prm['yaw_flip']), a['work'],
                                        a['out'], a['out_vel'], a['info'])
    torch.cuda.synchronize()
    host = {k: a[v].cpu().numpy() for k, v in (('out', 'out'), ('vel', 'out_vel'), ('info', 'info')) if a[v] is not None}
    return st, host


def untouched(got):
    return all((v == SENTINEL).all() if v.dtype == np.int32 else np.isnan(v).all() for v in got.values())


def check(t, observed=None, xf0=None, **prm):
    """the device against the restatement, bit for bit, twice; returns the restatement's result"""
    want = C.ref(t, observed, xf0, **prm)
    L = len(t['ids'])
    runs = [device_smooth(t, observed, xf0, **prm) for _ in range(2)]
    for st, got in runs:
        assert st == 0
        out, vel = got['out'].reshape(-1, 12), got['vel'].reshape(-1, 4)
        assert np.array_equal(bits(out[:L]), bits(want['out'])), np.abs(out[:L] - want['out']).max()
        assert np.array_equal(bits(vel[:L]), bits(want['vel'])), np.abs(vel[:L] - want['vel']).max()
        assert np.array_equal(got['info'].reshape(-1, 4), want['info'])
        assert np.isnan(out[L:]).all() and np.isnan(vel[L:]).all()  # nothing behind the L rows
    for k in runs[0][1]:
        assert np.array_equal(bits(runs[0][1][k]), bits(runs[1][1][k])), k
    return want


def seq(seed, n_frames=30, n_tracks=6, **kw):
    return fill_cases.random_sequence(np.random.default_rng(seed), n_frames, n_tracks, **kw)


def long_track():
    rng = np.random.default_rng(300)
    no = np.cumsum(1 + (rng.random(300) < 0.2) * rng.integers(1, 4, 300))
    loc = np.stack([0.4 * no, 1.5 + 0 * no, 60 - 0.1 * no], 1) + rng.normal(0, 0.2, (300, 3))
    yaw = np.asarray([R.wrap(v) for v in 0.07 * no + rng.normal(0, 0.05, 300)])  # turns more than three times
    return C.single_track(no, loc=loc, yaw=yaw, dims=1.6 + rng.normal(0, 0.1, (300, 3)))


WIDE = [(0, list(range(70))), (1, list(range(0, 70, 2)) + [-1] * 8), (3, [-1] * 3),
        (4, list(range(69, -1, -1)))]  # 70 detections a frame: the 70 heads cross a wave and (x 8 lanes) a workgroup
CASES = {
    '12 frames, 5 tracks, misses and unlisted frame numbers': lambda: fill_cases.tables([seq(11, 12, 5)]),
    '70 detections a frame': lambda: fill_cases.tables([WIDE]),
    'one track of 300 rows': long_track,
    'two sequences': lambda: fill_cases.tables([seq(12, 17), seq(13, 40, 8)]),
}


@pytest.mark.parametrize('name', list(CASES))
def test_against_the_restatement(name):
    t = CASES[name]()
    want = check(t)
    assert want['info'][:, 0].tolist() == [0] * (len(t['seq_start']) - 1) and want['info'][:, 1].sum() > 0
    if name == '70 detections a frame':
        assert want['info'].tolist() == [[0, 70, 175, 11]]
    if name == 'one track of 300 rows':
        assert want['info'].tolist() == [[0, 1, 300, 0]] and np.abs(want['vel'][:, 3] - 0.07).max() < 0.05
    masked = check(t, C.random_mask(t, 5), yaw_flip=True, q_dim=0.001)
    assert not np.array_equal(bits(masked['out']), bits(want['out']))


def test_five_sequences_in_one_launch_equal_five_calls():
    seqs = [seq(41, 20), [], seq(42, 9), [(5, [-1, -1]), (6, []), (7, [-1])], seq(43, 33, 7)]
    t = fill_cases.tables(seqs)
    xf0 = C.frame_records(len(t['frame_no']), 5, t['seq_start'])
    obs = C.random_mask(t, 9, 0.2)
    want = check(t, obs, xf0)
    assert want['info'][:, 1].tolist()[1] == want['info'][:, 1].tolist()[3] == 0 and (want['info'][[0, 2, 4], 1] > 0).all()
    for s in range(len(seqs)):
        f0, f1 = t['seq_start'][s], t['seq_start'][s + 1]
        d0, d1 = t['frame_start'][f0], t['frame_start'][f1]
        sub = dict(det=t['det'][d0:d1], ids=t['ids'][d0:d1], frame_start=t['frame_start'][f0:f1 + 1] - d0,
                   frame_no=t['frame_no'][f0:f1], seq_start=np.asarray([0, f1 - f0], np.int32))
        st, got = device_smooth(sub, obs[d0:d1], xf0[f0:f1])
        assert st == 0
        if f1 == f0 or d1 == d0:  # nothing to launch: a no-op
            assert untouched(got)
            continue
        n = d1 - d0
        assert np.array_equal(bits(got['out'].reshape(-1, 12)[:n]), bits(want['out'][d0:d1]))
        assert np.array_equal(bits(got['vel'].reshape(-1, 4)[:n]), bits(want['vel'][d0:d1]))
        assert np.array_equal(got['info'], want['info'][s])


def test_observed_mask_of_a_real_fill():
    frames, ids = C.noisy_scene(True)
    filled = tracks.fill_gaps(frames, ids, max_fill=3)
    p = tracks.pack_smooth([(filled.frames, filled.ids, None, [~m for m in filled.filled])])
    assert (p['observed'] == 0).sum() == filled.info['rows'] == 24
    want = check(p, p['observed'])
    assert want['info'].tolist() == [[0, 6, 240, 0]]
    # and through the operator and the surface: what the host route gives
    got = tracks.smooth_tracks(filled.frames, filled.ids, observed=[~m for m in filled.filled])
    from test_smooth_cpu import same_smoothed
    same_smoothed(got, C.host_smooth([(filled.frames, filled.ids, None, [~m for m in filled.filled])])[2][0])


def test_standing_camera_equals_identity_records():
    t = fill_cases.tables([seq(21), seq(22, 12)])
    obs = C.random_mask(t, 1)
    still = check(t, obs)
    ident = check(t, obs, C.identity_records(len(t['frame_no'])))
    assert still['info'][:, 1].sum() >= 8 and all(np.array_equal(bits(still[k]), bits(ident[k])) for k in still)


def test_moving_camera():
    t = fill_cases.tables([seq(31, 40, p_miss=0.4), seq(32, 20)])
    xf0 = C.frame_records(60, 3, t['seq_start'])
    want = check(t, C.random_mask(t, 2), xf0)
    still = C.ref(t, C.random_mask(t, 2))
    assert np.abs(want['out'][:, 7:10] - still['out'][:, 7:10]).max() > 1e-3  # it did move
    # the records of synth.ego_poses through ego.box_motion, as tracks.pack_smooth builds them
    from mmmot_amd import synth
    poses = synth.ego_poses(12, 4)
    frames, ids = C.noisy_scene(True)
    p = tracks.pack_smooth([(frames[:12], ids[:12], None, None, poses, fill_cases.CALIB)])
    assert np.array_equal(p['xf0'], C.frame_records(12, 4))
    check(p, None, p['xf0'])


def test_yaw_through_pi_and_yaw_flip():
    no = np.arange(0, 40, 2)
    rng = np.random.default_rng(6)
    yaw = np.asarray([R.wrap(v) for v in 2.6 + 0.06 * no + rng.normal(0, 0.03, 20)])
    assert yaw.min() < -2.5 and yaw.max() > 2.5
    want = check(C.single_track(no, yaw=yaw))
    turn = lambda a, b: np.abs([R.wrap(float(x) - float(y)) for x, y in zip(a, b)]).max()
    assert turn(want['out'][:, 10], yaw) < 0.1 and (np.abs(want['out'][:, 10]) <= np.float32(np.pi)).all()
    flipped = yaw.copy()
    flipped[7] = R.wrap(flipped[7] + np.pi)
    flipped[13:] = [R.wrap(v + np.pi) for v in flipped[13:]]
    on = check(C.single_track(no, yaw=flipped), yaw_flip=True)
    off = check(C.single_track(no, yaw=flipped))
    assert turn(on['out'][:, 10], want['out'][:, 10]) < 1e-5 and turn(off['out'][:, 10], want['out'][:, 10]) > 0.3


def test_what_is_copied_through():
    from test_smooth_cpu import copied_case
    t, obs = copied_case()
    want = check(t, obs)
    assert want['info'].tolist() == [[0, 2, 6, 6]]
    for kw in (dict(r_loc=0.0), dict(r_yaw=0.0), dict(r_dim=0.0), dict(r_loc=0.0, v0_loc=0.0, r_dim=0.0)):
        assert check(t, obs, **kw)['info'].tolist() == [[0, 2, 6, 6]]
    none = check(t, obs, r_loc=0.0, r_yaw=0.0, r_dim=0.0)
    assert none['info'].tolist() == [[0, 0, 0, 12]] and np.array_equal(bits(none['out']), bits(t['det']))
    # leading and trailing unobserved rows of one track
    no = np.asarray([3, 4, 6, 7, 8, 9, 12, 13])
    loc = np.stack([0.5 * no, 0 * no, 20 - 0.25 * no], 1) + np.random.default_rng(5).normal(0, 0.1, (8, 3))
    obs = np.asarray([0, 0, 1, 1, 1, 1, 0, 0], np.int32)
    want = check(C.single_track(no, loc=loc), obs)
    assert want['info'].tolist() == [[0, 1, 6, 2]] and np.array_equal(want['vel'][6], want['vel'][5])
    assert check(C.single_track(no, loc=loc), np.zeros(8, np.int32))['info'].tolist() == [[0, 0, 0, 8]]


def test_status_words():
    ok = [(0, [1]), (1, []), (2, [1])]
    want = check(fill_cases.tables([ok, [(0, [2, 5, 2]), (1, []), (2, [2, 5])], ok]))
    assert want['info'].tolist() == [[0, 1, 2, 0], [R.EDUP, 0, 0, 5], [0, 1, 2, 0]]
    want = check(fill_cases.tables([ok, [(4, [1]), (3, []), (5, [1])], [(7, [3]), (7, []), (9, [3])]]))
    assert want['info'].tolist() == [[0, 1, 2, 0], [R.ECONTRACT, 0, 0, 2], [R.ECONTRACT, 0, 0, 2]]
    # tables that are not prefixes stop the whole call: every row copied, and nothing is read through them
    for key, bad in (('frame_start', [0, 2, 1, 2]), ('frame_start', [0, 1, 1, 9]), ('seq_start', [1, 3]), ('seq_start', [0, 2])):
        t = fill_cases.tables([ok])
        t[key] = np.asarray(bad, np.int32)
        want = check(t)
        assert want['info'].tolist() == [[R.ECONTRACT, 0, 0, 0]] and np.array_equal(bits(want['out']), bits(t['det']))
    # the Python surface raises
    d = {'bbox': np.zeros((2, 4)), 'dimensions': np.ones((2, 3)), 'location': np.ones((2, 3)), 'rotation_y': np.zeros(2)}
    with pytest.raises(tracks.TrackingError, match='sequence 1.*twice'):
        tracks.smooth_tracks_batch([([d, d], [[0, 1], [1, 0]]), ([d, d], [[3, 3], [3, 4]])])
    with pytest.raises(tracks.TrackingError, match='do not increase'):
        tracks.smooth_tracks([d, d], [[0, 1], [1, 0]], frame_idx=[3, 2])


def test_what_the_launcher_refuses():
    t = fill_cases.tables([[(0, [1]), (1, []), (2, [1])]])
    assert device_smooth(t)[0] == 0
    for k in ('det', 'ids', 'frame_start', 'frame_no', 'seq_start', 'work', 'out', 'info'):
        st, got = device_smooth(t, nulls=(k,))
        assert st == -1 and untouched(got), k  # no launch
    bad = [dict(S=0), dict(S=-1), dict(L=-1), dict(F=-1), dict(yaw_flip=2), dict(work_offset=1),
           dict(L=2 ** 31 // 75 + 1)]  # 75 L + 2 >= 2^31: refused; one row less would still index in 32 bits
    bad += [{k: v} for k in R.PARAMS for v in (-1.0, float('nan'), float('inf'))]
    bad += [dict(v0_loc=0.0), dict(v0_yaw=0.0), dict(r_loc=1e-300, v0_loc=0.0)]
    for kw in bad:
        st, got = device_smooth(t, **kw)
        assert st == -1 and untouched(got), kw
    assert device_smooth(t, r_loc=0.0, v0_loc=0.0)[0] == 0  # a group that is left alone needs no v0
    for kw in (dict(L=0), dict(F=0)):  # a no-op that returns 0
        st, got = device_smooth(t, nulls=('det', 'work', 'out', 'info'), **kw)
        assert st == 0 and untouched(got)
    with pytest.raises(ValueError):
        torch.ops.mmmot.smooth_tracks(torch.zeros(10, dtype=torch.int32, device='cuda'), [2, 3, 1, 0, 0, 0] + [0] * 8)
    with pytest.raises(ValueError):
        torch.ops.mmmot.smooth_tracks(torch.zeros(10, dtype=torch.int32, device='cuda'), [2, 3, 1, 0, 0, 0])
    p = tracks.pack_smooth([fill_cases.scene(True)])
    sizes = p['sizes'][:6] + torch_ops.smooth_param_bits([-1.0] + list(p['smoother'].params()[1:]))
    with pytest.raises(RuntimeError, match='MMMOT_EINVAL'):
        torch.ops.mmmot.smooth_tracks(torch.from_numpy(p['packed']).cuda(), sizes)


def test_without_the_velocity_output():
    t = fill_cases.tables([seq(61, 15)])
    xf0 = C.frame_records(15, 7)
    want = check(t, None, xf0)
    st, got = device_smooth(t, None, xf0, nulls=('out_vel',))
    assert st == 0 and np.array_equal(bits(got['out'].reshape(-1, 12)[:len(t['ids'])]), bits(want['out']))
    assert np.array_equal(got['info'].reshape(-1, 4), want['info'])


def test_meta_kernel_and_no_cpu_kernel():
    p = tracks.pack_smooth([C.noisy_scene(True)])
    out = torch.ops.mmmot.smooth_tracks(torch.empty(len(p['packed']), dtype=torch.int32, device='meta'), p['sizes'])
    assert out.device.type == 'meta' and out.shape == (torch_ops.smooth_layout(p['sizes'])[3],)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mmmot.smooth_tracks(torch.from_numpy(p['packed']), p['sizes'])


def test_fill_tracks_still_equals_its_restatement():
    # mmmot_fill_tracks shares csrc/track_links.h with the smoother
    from test_fill_gpu import check as fill_check
    t = fill_cases.tables([seq(12, 17), seq(13, 40, 8)])
    want = fill_check(t, 7, fill_cases.motion_records(len(t['frame_no']), 7, 3, t['seq_start']))
    assert len(want['out']) > 20


def test_batch_equals_single_calls():
    from test_smooth_cpu import same_smoothed
    from test_fill_cpu import moving_sequence
    frames, ids, frame_idx, scores, poses = moving_sequence()
    sm = tracks.TrackSmoother(q_dim=0.001, yaw_flip=True)
    seqs = [(frames, ids, frame_idx, None, poses, fill_cases.CALIB, scores), C.noisy_scene(True),
            dict(frames=frames[:9], ids=ids[:9], frame_idx=frame_idx[:9]), dict(frames=[], ids=[])]
    got = tracks.smooth_tracks_batch(seqs, sm)
    want = C.host_smooth(seqs, sm)[2]
    assert len(got) == 4 and got[0].info['tracks'] > 2 and got[3].frames == []
    for g, w in zip(got, want):
        same_smoothed(g, w)
    same_smoothed(tracks.smooth_tracks(frames, ids, frame_idx, None, poses, fill_cases.CALIB, sm, scores=scores), got[0])
    same_smoothed(tracks.smooth_tracks(*C.noisy_scene(True), smoother=sm), got[1])
    same_smoothed(tracks.smooth_tracks(frames[:9], ids[:9], frame_idx[:9], smoother=sm), got[2])


def test_evaluation_before_and_after_smoothing():
    gt = E.labels_from_tracks(*fill_cases.scene(False), ground_truth=True, box3d=True)
    frames, ids = C.noisy_scene(True)
    st = tracks.smooth_tracks(frames, ids)
    lab = lambda f, i: E.labels_from_tracks(f, i, n_frames=fill_cases.N_FRAMES, box3d=True)
    before = E.evaluate_3d_sequences(gt, lab(frames, ids), overlap='3d').all
    after = E.evaluate_3d_sequences(gt, lab(st.frames, st.ids), overlap='3d').all
    for k in ('tp', 'fn', 'fp', 'id_switches', 'fragments', 'MT', 'PT', 'ML', 'n_gt'):
        assert getattr(before, k) == getattr(after, k), k
    print('MOTP (mean 3D IoU of the matches): %.4f before, %.4f after' % (before.MOTP, after.MOTP))
    assert before.tp == 216 and after.MOTP >= before.MOTP  # the mean overlap: larger is better


def test_run_global_smooth():
    from test_fill_gpu import same_filled
    from test_lockstep_gpu import shaped
    from test_pipeline_gap_gpu import S, model
    from test_smooth_cpu import same_smoothed
    from mmmot_amd.pipeline import FrameFeed, SequencePipeline
    from mmmot_amd.synth import make_sequence
    frames = make_sequence(8, seed=23, n_pts=4000, det_range=(2, 5), hw=(120, 400), ego=1)
    feeds = [FrameFeed(img, sweep, info, shaped(dets, 0 if t == 5 else None), pose=(info['pos'], info['rad']))
             for t, (img, sweep, info, dets) in enumerate(frames)]
    plain, smoothed = SequencePipeline(model(), S), SequencePipeline(model(), S)
    sm = tracks.TrackSmoother()
    a = plain.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=3, fill=7)
    b = smoothed.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=3, fill=7, smooth=sm)
    assert a.smoothed is None and plain.stats == smoothed.stats
    assert a.objective == b.objective and all(np.array_equal(x, y) for x, y in zip(plain.tracks, smoothed.tracks))
    same_filled(a.filled, b.filled)
    poses = [f.pose for f in feeds]
    filled = tracks.fill_gaps([f.dets for f in feeds], smoothed.tracks, poses=poses, calib=feeds[0].info, max_fill=7)
    by_hand = tracks.smooth_tracks(filled.frames, filled.ids, observed=[~m for m in filled.filled], poses=poses,
                                   calib=feeds[0].info, smoother=sm)
    same_smoothed(b.smoothed, by_hand)
    # the test model's random weights link nothing (every detection is a track of its own), so every row is a chain of
    # one row here: this test covers the hand-off; the smoothing behind it is covered by the tests above
    n = sum(len(i) for i in filled.ids)
    assert len(b.smoothed.frames) == 8 and b.smoothed.info['rows_changed'] + b.smoothed.info['rows_copied'] == n
    # without fill the solved sequence is smoothed
    c = SequencePipeline(model(), S).run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=3, smooth=sm)
    same_smoothed(c.smoothed, tracks.smooth_tracks([f.dets for f in feeds], smoothed.tracks, poses=poses,
                                                   calib=feeds[0].info, smoother=sm))
    assert c.filled is None
    with pytest.raises(ValueError, match='TrackSmoother'):
        plain.run_global(feeds, smooth=dict(q_loc=1.0))
