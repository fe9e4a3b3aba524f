"""Tracklet stitching on the device (csrc/stitch_tracks.hip through HipOps.stitch_tracks, mmmot::stitch_tracks and
mmmot_amd.tracks.stitch_tracks) against the NumPy restatement tests/stitch_ref.py: BIT FOR BIT on out_ids, next, links
and info, between guard words behind every output, and twice for bit equality of two calls; the objective against the
restatement's fp64 sum to 1e-9 relative.  Then the shared header's other users (mmmot_fill_tracks, mmmot_smooth_tracks)
and the scene with one long hole per object, end to end on the device."""
import numpy as np
import pytest
import torch

import fill_cases
import smooth_cases
import stitch_cases as C
import stitch_ref as R
from mmmot_amd import evaluate as E
from mmmot_amd import torch_ops, tracks

pytestmark = pytest.mark.gpu

GUARD = 5
SENTINEL = -77
bits = C.bits
OUTS = ('out_ids', 'next', 'links', 'objective', 'info')


def device_stitch(t, vel=True, xf0=None, k_start=None, pairs=None, nulls=(), work_offset=0, **over):
    """one call of the entry on fresh buffers: (status, the outputs as host arrays, the guard words included).  ``over``:
    TrackStitcher's arguments, and L / F / S / n_tracks / n_link / max_k in place of what the tables hold"""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    prm = dict(C.PARAMS, **{k: v for k, v in over.items() if k in C.PARAMS})
    r2, inv_r2 = R.tables(prm['drift'], prm['max_speed'], prm['slack'], min(max(prm['max_dt'], 1), R.MAX_DT))
    ks, pr = C.track_tables(t)
    ks, pr = ks if k_start is None else np.asarray(k_start, np.int32), pr if pairs is None else np.asarray(pairs, np.int32)
    K = np.diff(C.track_tables(t)[0] if k_start is None else ks).astype(np.int64)
    n, S0 = len(t['ids']), len(t['seq_start']) - 1
    T, n_link = int(np.abs(K).sum()), int((K * K).sum())
    z = dict(L=n, F=len(t['frame_no']), S=S0, n_tracks=T, n_link=n_link, max_k=int(K.max()))
    z.update({k: v for k, v in over.items() if k in z})
    # the buffers hold what the tables and what the call claims need (a claim the entry refuses allocates nothing more)
    T, n_link = (max(own, z[k]) if 0 <= z[k] < 10 ** 6 else own for own, k in ((T, 'n_tracks'), (n_link, 'n_link')))
    vel = t['vel'] if vel is True else vel
    a = dict(det=dev(t['det'].reshape(-1), np.float32), ids=dev(t['ids'], np.int32),
             frame_start=dev(t['frame_start'], np.int32), frame_no=dev(t['frame_no'], np.int32),
             seq_start=dev(t['seq_start'], np.int32), vel=None if vel is None else dev(vel.reshape(-1), np.float32),
             xf0=None if xf0 is None else dev(xf0.reshape(-1), np.float64), k_start=dev(ks, np.int32),
             pairs=dev(pr.reshape(-1), np.int32), r2=dev(r2.reshape(-1), np.float64), inv_r2=dev(inv_r2.reshape(-1), np.float64),
             work=torch.empty((torch_ops.stitch_work(n, len(t['frame_no']), S0, T, n_link) + 3) // 2, dtype=torch.int64,
                              device='cuda').view(torch.int32)[work_offset:],
             out_ids=torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device='cuda'),
             next=torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device='cuda'),
             links=torch.full((n_link + GUARD,), float(SENTINEL), dtype=torch.float32, device='cuda'),
             objective=torch.full((S0 + GUARD,), float(SENTINEL), dtype=torch.float64, device='cuda'),
             info=torch.full((S0 * 4 + GUARD,), SENTINEL, dtype=torch.int32, device='cuda'))
    for k in nulls:
        a[k] = None
    st = torch_ops._ops().stitch_tracks(a['det'], a['ids'], a['frame_start'], a['frame_no'], a['seq_start'], a['vel'], a['xf0'],
                                        a['k_start'], a['pairs'], a['r2'], a['inv_r2'], z['L'], z['F'], z['S'], z['n_tracks'],
                                        z['n_link'], z['max_k'], prm['min_dt'], prm['max_dt'], prm['min_rows'],
                                        prm['mode'] if isinstance(prm['mode'], int) else R.MODES[prm['mode']],
                                        prm['max_size_ratio'], prm['gap_penalty'], a['work'], a['out_ids'], a['next'],
                                        a['links'], a['objective'], a['info'])
    torch.cuda.synchronize()
    return st, {k: a[k].cpu().numpy() for k in OUTS if a[k] is not None}


def untouched(got):
    return all((v == SENTINEL).all() for v in got.values())


def check(t, vel=True, xf0=None, k_start=None, pairs=None, **prm):
    """the device against the restatement, bit for bit, twice; returns the restatement's result"""
    want = C.ref(t, vel, xf0, k_start, pairs, **prm)
    runs = [device_stitch(t, vel, xf0, k_start, pairs, **prm) for _ in range(2)]
    for st, got in runs:
        assert st == 0
        for k in ('out_ids', 'next', 'links', 'info'):
            w = want[k].reshape(-1)
            assert np.array_equal(bits(got[k][:len(w)]), bits(w)), (k, np.flatnonzero(bits(got[k][:len(w)]) != bits(w))[:8])
            assert (got[k][len(w):] == SENTINEL).all(), k  # nothing behind the output
        obj, w = got['objective'], want['objective']
        assert np.array_equal(np.isnan(obj[:len(w)]), np.isnan(w)) and (obj[len(w):] == SENTINEL).all()
        ok = ~np.isnan(w)
        assert (np.abs(obj[:len(w)][ok] - w[ok]) <= 1e-9 * np.abs(w[ok])).all()
    for k in OUTS:
        assert np.array_equal(bits(runs[0][1][k]), bits(runs[1][1][k])), k
    return want


# K = 1, 2: the smallest; 64 / 65: a wave edge; 128 / 129: the solver's one-wave / four-wave switch; 256 / 257: one K past
# the cost kernel's LDS tile of 256 heads; 512: the limit
@pytest.mark.parametrize('K', [1, 2, 64, 65, 128, 129, 256, 257, 512])
def test_against_the_restatement(K):
    t = C.with_k(K, K, holey=K in (65, 129), stray=K // 8, spread=4.0, sigma=0.3)
    want = check(t, max_dt=12)
    assert want['info'][0].tolist()[:2] == [0, K]
    if K > 1:
        assert want['info'][0, 2] >= K // 3 and want['info'][0, 3] > 0
        assert 0 < np.isfinite(want['links']).sum() < K * K
    check(t, max_dt=12, min_rows=2, mode='3d', gap_penalty=0.01)


def test_too_many_tracks():
    t = C.with_k(9, 513)
    want = check(t)
    assert want['info'].tolist() == [[R.ETOOMANY, 0, 0, 0]] and (bits(want['links']) == 0x7fc00000).all()
    # beside a sequence that is solved
    both = C.concat([C.with_k(5, 6), t, C.with_k(6, 7)])
    want = check(both)
    assert want['info'][:, 0].tolist() == [0, R.ETOOMANY, 0] and want['info'][[0, 2], 2].sum() > 0
    # a max_k below the tracks a sequence holds: the solver's launch does not serve it
    want = check(C.with_k(5, 6), max_k=5)
    assert want['info'].tolist() == [[R.ECONTRACT, 0, 0, 0]]


def long_track():
    """one track of 300 rows, then a second one behind a hole: the walk from the head to the tail"""
    rng = np.random.default_rng(300)
    no = np.concatenate([np.arange(300), np.arange(310, 315)])
    t = smooth_cases.single_track(no, loc=np.stack([0.1 * no, 1.5 + 0 * no, 60 - 0.1 * no], 1) + rng.normal(0, 0.05, (305, 3)))
    t['ids'][300:] = 4
    t['vel'] = np.tile(np.asarray([0.1, 0, -0.1, 0], np.float32), (305, 1))
    return t


def test_one_track_of_300_rows():
    want = check(long_track())
    assert want['info'].tolist() == [[0, 2, 1, 5]] and want['next'][299] == 300 and (want['out_ids'] == 3).all()


def sub_table(t, s):
    f0, f1 = t['seq_start'][s], t['seq_start'][s + 1]
    d0, d1 = t['frame_start'][f0], t['frame_start'][f1]
    return dict(det=t['det'][d0:d1], ids=t['ids'][d0:d1], vel=t['vel'][d0:d1], frame_start=t['frame_start'][f0:f1 + 1] - d0,
                frame_no=t['frame_no'][f0:f1], seq_start=np.asarray([0, f1 - f0], np.int32)), (d0, d1, f0, f1)


def test_five_sequences_in_one_launch_equal_five_calls():
    empty = dict(det=np.zeros((0, 12), np.float32), ids=np.zeros(0, np.int32), vel=np.zeros((0, 4), np.float32),
                 frame_start=np.zeros(1, np.int32), frame_no=np.zeros(0, np.int32))
    stray = C.with_k(44, 3)
    stray['ids'][:] = -1  # frames and rows, no track
    t = C.concat([C.with_k(41, 20, holey=True), empty, C.with_k(42, 9, stray=4), stray, C.with_k(43, 33)])
    xf0 = smooth_cases.frame_records(len(t['frame_no']), 5, t['seq_start'])
    want = check(t, xf0=xf0)
    assert want['info'][:, 1].tolist() == [20, 0, 9, 0, 33] and (want['info'][[0, 2, 4], 2] > 0).all()
    assert np.isnan(want['objective'][[1, 3]]).all()
    lo = np.concatenate([[0], np.cumsum(want['info'][:, 1].astype(np.int64) ** 2)])
    for s in range(5):
        sub, (d0, d1, f0, f1) = sub_table(t, s)
        st, got = device_stitch(sub, xf0=xf0[f0:f1])
        assert st == 0
        if f1 == f0 or d1 == d0:  # nothing to launch: a no-op
            assert untouched(got)
            continue
        n, K = d1 - d0, int(want['info'][s, 1])
        assert np.array_equal(got['out_ids'][:n], want['out_ids'][d0:d1])
        assert np.array_equal(np.where(got['next'][:n] >= 0, got['next'][:n] + d0, -1), want['next'][d0:d1])
        assert np.array_equal(bits(got['links'][:K * K]), bits(want['links'][lo[s]:lo[s + 1]]))
        assert np.array_equal(got['info'][:4], want['info'][s])
        a, b = got['objective'][0], want['objective'][s]
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9 * abs(b)


def test_moving_camera():
    from mmmot_amd import synth
    t = C.concat([C.with_k(31, 30, holey=True), C.with_k(32, 12)])
    xf0 = smooth_cases.frame_records(len(t['frame_no']), 3, t['seq_start'])
    want = check(t, xf0=xf0)
    still = C.ref(t)
    assert not np.array_equal(bits(want['links']), bits(still['links']))  # it did move
    # objects that stand in the world, seen from the moving camera: only with the records do the tracklets meet
    n = 40
    poses = synth.ego_poses(n, 4)
    rec = smooth_cases.frame_records(n, 4)
    world = np.asarray([[-6.0, 1.5, 25.0], [5.0, 1.6, 40.0], [0.5, 1.4, 60.0]])
    spec = {0: (range(0, 6), range(20, 26)), 1: (range(2, 9), range(24, 30)), 2: (range(5, 10), range(30, 36))}
    rows = []
    for o, segs in spec.items():
        for k, seg in enumerate(segs):
            for f in seg:
                inv = rec[f, 16:32].reshape(4, 4)
                rows.append((f, 2 * o + k, np.concatenate([world[o], [1.0]]) @ inv))
    rows.sort(key=lambda r: (r[0], r[1]))
    det = np.zeros((len(rows), 12), np.float32)
    det[:, 2:4], det[:, 4:7], det[:, 11] = 50.0, 1.6, 0.5
    det[:, 7:10] = [r[2][:3] for r in rows]
    counts = np.bincount([r[0] for r in rows], minlength=n)
    t = dict(det=det, ids=np.asarray([r[1] for r in rows], np.int32), vel=np.zeros((len(rows), 4), np.float32),
             frame_start=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), frame_no=np.arange(n, dtype=np.int32),
             seq_start=np.asarray([0, n], np.int32))
    moved = check(t, xf0=rec, drift=0.0, slack=0.5, max_speed=0.0)
    assert moved['info'].tolist() == [[0, 6, 3, sum(len(s[1]) for s in spec.values())]]
    assert check(t, drift=0.0, slack=0.5, max_speed=0.0)['info'][0, 2] < 3  # without them the camera's way is in between
    assert np.array_equal(smooth_cases.frame_records(n, 4), tracks.pack_stitch(
        [([dict(bbox=np.zeros((0, 4)), dimensions=np.zeros((0, 3)), location=np.zeros((0, 3)), rotation_y=np.zeros(0))] * n,
          [[]] * n, None, None, poses, fill_cases.CALIB)])['xf0'])


def test_standing_camera_equals_identity_records():
    t = C.with_k(21, 40, stray=6)
    still = check(t)
    ident = check(t, xf0=smooth_cases.identity_records(len(t['frame_no'])))
    assert still['info'][0, 2] > 8 and all(np.array_equal(bits(still[k]), bits(ident[k])) for k in still)


def test_without_velocities_3d_mode_size_gate_and_gap_penalty():
    t = C.with_k(51, 48, spread=4.0, sigma=0.3)
    plain = check(t)
    static = check(t, vel=None)
    assert static['info'][0, 2] > 0 and not np.array_equal(bits(static['links']), bits(plain['links']))
    solid = check(t, mode='3d')
    assert not np.array_equal(bits(solid['links']), bits(plain['links']))
    sized = check(t, max_size_ratio=1.02)  # the dimensions carry 0.02 m of noise: some pairs of one object fail
    assert 0 < np.isfinite(sized['links']).sum() < np.isfinite(plain['links']).sum()
    # a penalty that turns passing scores negative: the links stay in the block, the solver leaves them
    pen = check(t, gap_penalty=0.2)
    neg = np.isfinite(pen['links']) & (pen['links'] < 0)
    assert neg.sum() > 0 and np.isfinite(pen['links']).sum() == np.isfinite(plain['links']).sum()
    assert pen['info'][0, 2] < plain['info'][0, 2]
    nan_v = t['vel'].copy()
    nan_v[::7, 0] = np.nan
    nan_t = dict(t, det=t['det'].copy(), vel=nan_v)
    nan_t['det'][3::11, 9] = np.nan
    nan_t['det'][5::13, 4] = np.nan
    lost = check(nan_t, max_size_ratio=3.0)
    assert np.isfinite(lost['links']).sum() < np.isfinite(plain['links']).sum()


def test_status_words_and_broken_tables():
    ok = C.with_k(61, 6)
    dup = C.with_k(62, 5)
    ks_dup = C.track_tables(dup)[0]
    f = int(np.flatnonzero(np.diff(dup['frame_start']) >= 2)[0])
    dup['ids'][dup['frame_start'][f] + 1] = dup['ids'][dup['frame_start'][f]]  # an ID twice in a frame
    back = C.with_k(63, 4)
    back['frame_no'] = back['frame_no'].copy()
    back['frame_no'][3] = back['frame_no'][2]  # frame numbers that do not increase
    t = C.concat([ok, dup, back, C.with_k(64, 7)])
    K = np.asarray([6, 5, 4, 7], np.int64)
    ks = np.concatenate([[0], np.cumsum(K)]).astype(np.int32)
    pr = np.stack([K, K, 2 * ks[:-1], np.concatenate([[0], np.cumsum(K * K)])[:-1]], 1).astype(np.int32)
    want = check(t, k_start=ks, pairs=pr)
    assert want['info'][:, 0].tolist() == [0, R.EDUP, R.ECONTRACT, 0] and want['info'][1:3, 1:].tolist() == [[0, 0, 0]] * 2
    assert np.isnan(want['objective'][1:3]).all() and not np.isnan(want['objective'][[0, 3]]).any()
    assert (bits(want['links'][36:36 + 25 + 16]) == 0x7fc00000).all() and (want['next'][len(ok['ids']):][:len(dup['ids'])] == -1).all()
    # a k_start that counts another number of tracks than the device finds (with the pairs table that follows it)
    K2 = np.asarray([6, 5, 4, 6], np.int64)
    ks2 = np.concatenate([[0], np.cumsum(K2)]).astype(np.int32)
    pr2 = np.stack([K2, K2, 2 * ks2[:-1], np.concatenate([[0], np.cumsum(K2 * K2)])[:-1]], 1).astype(np.int32)
    want = check(t, k_start=ks2, pairs=pr2)
    assert want['info'][:, 0].tolist() == [0, R.EDUP, R.ECONTRACT, R.ECONTRACT]
    # tables that are not prefixes stop the whole call, and nothing is read through them
    quiet = lambda w, tt: (w['info'].tolist() == [[R.ECONTRACT, 0, 0, 0]] * (len(tt['seq_start']) - 1)
                           and np.array_equal(w['out_ids'], tt['ids']) and (w['next'] == -1).all()
                           and (bits(w['links']) == 0x7fc00000).all() and np.isnan(w['objective']).all())
    ks1, pr1 = C.track_tables(ok)
    F, L = len(ok['frame_no']), len(ok['ids'])
    assert ok['frame_start'][2] < L
    fs_dec = ok['frame_start'].copy()
    fs_dec[1] = L  # inside [0, L], and above the entry behind it
    fs_far = ok['frame_start'].copy()
    fs_far[-1] = L + 900
    for key, bad in (('frame_start', fs_dec), ('frame_start', fs_far), ('seq_start', np.asarray([1, F])),
                     ('seq_start', np.asarray([0, F - 1]))):
        tt = dict(ok)
        tt[key] = np.asarray(bad, np.int32)
        assert quiet(check(tt, k_start=ks1, pairs=pr1), tt), key
    for bad_ks, bad_pr in ((np.asarray([1, 6]), pr1), (np.asarray([0, 5]), pr1), (ks1, [[6, 6, 0, 1]]), (ks1, [[6, 5, 0, 0]]),
                           (ks1, [[6, 6, 2, 0]]), (ks1, [[6, 6, 0, -36]]), (ks1, [[6, 6, 0, 2 ** 31 - 40]])):
        st, got = device_stitch(ok, k_start=bad_ks, pairs=bad_pr, n_tracks=6, n_link=36, max_k=6)
        assert st == 0 and got['info'][:4].tolist() == [R.ECONTRACT, 0, 0, 0] and np.isnan(got['objective'][0])
        assert np.array_equal(got['out_ids'][:L], ok['ids']) and (got['next'][:L] == -1).all()
        assert (bits(got['links'][:36]) == 0x7fc00000).all()
        assert all((got[k][n:] == SENTINEL).all() for k, n in (('out_ids', L), ('next', L), ('links', 36), ('info', 4)))
    # the Python surface raises
    d = {'bbox': np.zeros((2, 4)), 'dimensions': np.ones((2, 3)), 'location': np.ones((2, 3)), 'rotation_y': np.zeros(2)}
    with pytest.raises(tracks.TrackingError, match='sequence 1.*twice'):
        tracks.stitch_tracks_batch([([d, d], [[0, 1], [1, 0]]), ([d, d], [[3, 3], [3, 4]])])
    with pytest.raises(tracks.TrackingError, match='do not increase'):
        tracks.stitch_tracks([d, d], [[0, 1], [1, 0]], frame_idx=[3, 2])


def test_what_the_launcher_refuses():
    t = C.with_k(71, 4)
    assert device_stitch(t)[0] == 0
    for k in ('det', 'ids', 'frame_start', 'frame_no', 'seq_start', 'k_start', 'pairs', 'r2', 'inv_r2', 'work', 'out_ids',
              'next', 'links', 'objective', 'info'):
        st, got = device_stitch(t, nulls=(k,))
        assert st == -1 and untouched(got), k  # no launch
    assert device_stitch(t, nulls=('vel', 'xf0'))[0] == 0
    bad = [dict(S=0), dict(S=-1), dict(L=-1), dict(F=-1), dict(n_tracks=-1), dict(n_link=-1), dict(max_k=-1),
           dict(work_offset=1), dict(L=2 ** 29), dict(n_link=2 ** 31 - 1), dict(n_tracks=2 ** 31 - 1),
           dict(min_dt=0), dict(min_dt=-3), dict(min_dt=31), dict(max_dt=257), dict(max_dt=0), dict(mode=2), dict(mode=-1),
           dict(min_rows=0), dict(min_rows=-1)]
    bad += [{k: v} for k in ('max_size_ratio', 'gap_penalty') for v in (-1.0, float('nan'), -1e-300)]
    for kw in bad:
        st, got = device_stitch(t, **kw)
        assert st == -1 and untouched(got), kw
    assert device_stitch(t, min_dt=256, max_dt=256)[0] == 0  # the limits themselves
    for kw in (dict(L=0), dict(F=0)):  # a no-op that returns 0
        st, got = device_stitch(t, nulls=('det', 'work', 'out_ids', 'info'), **kw)
        assert st == 0 and untouched(got)
    with pytest.raises(ValueError):
        torch.ops.mmmot.stitch_tracks(torch.zeros(10, dtype=torch.int32, device='cuda'), [2, 3, 1, 2, 4, 2, 0, 0, 1, 30, 3, 0, 0, 0])
    p = tracks.pack_stitch([fill_cases.scene(True)])
    with pytest.raises(ValueError):
        torch.ops.mmmot.stitch_tracks(torch.from_numpy(p['packed']).cuda(), p['sizes'][:12])
    sizes = p['sizes'][:12] + torch_ops.stitch_param_bits(0.0, -1.0)
    with pytest.raises(RuntimeError, match='MMMOT_EINVAL'):
        torch.ops.mmmot.stitch_tracks(torch.from_numpy(p['packed']).cuda(), sizes)


def test_fill_and_smooth_still_equal_their_restatements():
    # mmmot_fill_tracks and mmmot_smooth_tracks share csrc/track_links.h with the stitcher
    from test_fill_gpu import check as fill_check
    from test_smooth_gpu import check as smooth_check, seq
    t = fill_cases.tables([seq(12, 17), seq(13, 40, 8)])
    want = fill_check(t, 7, fill_cases.motion_records(len(t['frame_no']), 7, 3, t['seq_start']))
    assert len(want['out']) > 20
    want = smooth_check(t, smooth_cases.random_mask(t, 5), smooth_cases.frame_records(len(t['frame_no']), 3, t['seq_start']))
    assert want['info'][:, 1].sum() > 8


def same_stitched(a, b):
    assert len(a.ids) == len(b.ids) and all(np.array_equal(x, y) for x, y in zip(a.ids, b.ids))
    assert np.array_equal(a.pairs, b.pairs) and np.array_equal(bits(a.links), bits(b.links)) and a.info == b.info
    assert (np.isnan(a.objective) and np.isnan(b.objective)) or abs(a.objective - b.objective) <= 1e-9 * abs(b.objective)


def test_batch_equals_single_calls_and_the_host_route():
    from test_stitch_cpu import frames_of
    from mmmot_amd import synth
    parts = [C.with_k(81, 14, holey=True, stray=3), C.with_k(82, 1), C.with_k(83, 30)]
    seqs = [frames_of(p) for p in parts]
    seqs[0] = seqs[0] + (synth.ego_poses(len(seqs[0][0]), 6), fill_cases.CALIB)
    seqs.append(dict(frames=[], ids=[], velocity=[]))
    k = tracks.TrackStitcher(max_dt=12, min_rows=2, gap_penalty=0.001, max_size_ratio=2.0)
    got = tracks.stitch_tracks_batch(seqs, k)
    want = C.host_stitch(seqs, k)[2]
    assert len(got) == 4 and got[0].info['stitches'] > 2 and got[3].ids == [] and np.isnan(got[3].objective)
    for g, w in zip(got, want):
        same_stitched(g, w)
    for s in range(3):
        same_stitched(tracks.stitch_tracks(*seqs[s], stitcher=k), got[s])
    none = tracks.stitch_tracks_batch([dict(frames=[], ids=[])])[0]  # no rows at all: nothing is launched
    assert none.ids == [] and none.info == {'tracks': 0, 'stitches': 0, 'rows_changed': 0} and np.isnan(none.objective)


def test_the_scene_end_to_end():
    """the scene with one long hole per object through fill_gaps, smooth_tracks and stitch_tracks on the device, the 3D
    evaluator before and after"""
    n = fill_cases.N_OBJ
    gt = E.labels_from_tracks(*fill_cases.scene(False), ground_truth=True, box3d=True)
    frames, ids = C.broken_scene(True)
    filled = tracks.fill_gaps(frames, ids, max_fill=3)
    sm = tracks.smooth_tracks(filled.frames, filled.ids, observed=[~m for m in filled.filled])
    st = tracks.stitch_tracks(sm.frames, sm.ids, velocity=sm.velocity)
    same_stitched(st, C.host_stitch([(sm.frames, sm.ids, None, sm.velocity)])[2][0])
    assert st.info['tracks'] == 2 * n and st.info['stitches'] == n
    assert all(np.array_equal(i, np.asarray(w) % n) for i, w in zip(st.ids, sm.ids))
    again = tracks.fill_gaps(filled.frames, st.ids, max_fill=14)
    obs = [np.concatenate([~m, np.zeros(len(m2) - len(m), bool)]) for m, m2 in zip(filled.filled, again.filled)]
    sm2 = tracks.smooth_tracks(again.frames, again.ids, observed=obs)
    lab = lambda f, i: E.labels_from_tracks(f, i, n_frames=fill_cases.N_FRAMES, box3d=True)
    before = E.evaluate_3d_sequences(gt, lab(sm.frames, sm.ids), overlap='3d').all
    after = E.evaluate_3d_sequences(gt, lab(sm2.frames, sm2.ids), overlap='3d').all
    print('3D evaluation: before fn %d, fragments %d, switches %d, MOTA %.4f; after fn %d, fragments %d, switches %d, MOTA %.4f'
          % (before.fn, before.fragments, before.id_switches, before.MOTA, after.fn, after.fragments, after.id_switches,
             after.MOTA))
    assert before.fragments == n and before.fn > 0 and before.fp == 0
    assert after.fragments == 0 and after.id_switches == 0 and after.fn == 0 and after.fp == 0 and after.MOTA == 1.0
