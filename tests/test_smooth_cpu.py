"""The smoothing of DESIGN section 12b on the host: the restatement tests/smooth_ref.py against an independent batch solve
and its exact properties, the status words, ``tracks.pack_smooth`` / ``unpack_smooth`` with the restatement standing in
for the launches, ``tracks.TrackSmoother``, and the benefit on a noisy scene.  No GPU.

Batch solve: the smoothed means are the minimiser of the model's quadratic form over all states of a track; the normal
equations are solved with ``numpy.linalg.solve``.  The two routes differ in fp64 rounding only.  Measured largest
difference over the cases of ``BATCH_CASES`` (positions and velocities, both filters): 1.52e-10 (a 40-row track; at most 1.7e-13 on the tracks of 2 and 3 rows); asserted at ten
times that, ``BATCH_TOL``."""
import numpy as np
import pytest

import fill_cases
import smooth_cases as C
import smooth_ref as R
from mmmot_amd import torch_ops, tracks

BATCH_TOL = 1.52e-9
DIFFUSE = 1e8


def batch_cv(z, obs, d, q, r, v0):
    """the posterior mean of all 2m states: prior p0 ~ N(z0, r), v0 ~ N(0, v0); x_k - F x_{k-1} ~ N(0, Q(d_k));
    z_k - p_k ~ N(0, r) at the observed rows k >= 1"""
    m = len(z)
    H, g = np.zeros((2 * m, 2 * m)), np.zeros(2 * m)
    H[0, 0] += 1 / r
    g[0] += z[0] / r
    H[1, 1] += 1 / v0
    for k in range(1, m):
        dk = float(d[k])
        F = np.array([[1.0, dk], [0.0, 1.0]])
        Qi = np.linalg.inv(q * np.array([[dk ** 3 / 3, dk ** 2 / 2], [dk ** 2 / 2, dk]]))
        J = np.zeros((2, 2 * m))
        J[:, 2 * k:2 * k + 2] = np.eye(2)
        J[:, 2 * k - 2:2 * k] = -F
        H += J.T @ Qi @ J
        if obs[k]:
            H[2 * k, 2 * k] += 1 / r
            g[2 * k] += z[k] / r
    x = np.linalg.solve(H, g)
    return x[0::2], x[1::2]


def batch_walk(z, obs, d, q, r):
    m = len(z)
    H, g = np.zeros((m, m)), np.zeros(m)
    H[0, 0] += 1 / r
    g[0] += z[0] / r
    for k in range(1, m):
        w = 1 / (q * float(d[k]))
        H[k, k] += w
        H[k - 1, k - 1] += w
        H[k, k - 1] -= w
        H[k - 1, k] -= w
        if obs[k]:
            H[k, k] += 1 / r
            g[k] += z[k] / r
    return np.linalg.solve(H, g)


def batch_case(m, seed):
    rng = np.random.default_rng(seed)
    d = np.concatenate([[0], 1 + (rng.random(m - 1) < 0.3) * rng.integers(1, 4, m - 1)])  # gaps in the frame numbers
    no = np.cumsum(d)
    z = 0.7 * no + rng.normal(0, 0.3, m) + 5.0
    obs = np.concatenate([[True], rng.random(m - 1) >= 0.25])
    if m > 3:
        obs[-2:] = False  # trailing unobserved rows
    return z, obs, d


BATCH_CASES = [(2, 1), (2, 2), (3, 3), (3, 4), (40, 5), (40, 6)]


def batch_differences():
    worst = 0.0
    for m, seed in BATCH_CASES:
        z, obs, d = batch_case(m, seed)
        for q, r, v0 in ((0.01, 0.04, 1.0), (0.5, 0.09, 0.25)):
            ps, vs = R.smooth_cv(z, obs, d, q, r, v0)
            bp, bv = batch_cv(z, obs, d, q, r, v0)
            worst = max(worst, np.abs(np.asarray(ps) - bp).max(), np.abs(np.asarray(vs) - bv).max())
            pw = R.smooth_walk(z, obs, d, q, r)
            worst = max(worst, np.abs(np.asarray(pw) - batch_walk(z, obs, d, q, r)).max())
    return worst


def test_smoothed_means_equal_the_batch_solution():
    worst = batch_differences()
    print('largest difference to the batch solve: %.3e' % worst)
    assert worst <= BATCH_TOL
    z, obs, d = batch_case(40, 5)
    assert (~obs).sum() >= 3 and d.max() > 1  # the cases do hold unobserved rows and gaps
    # and the smoother is no identity: the check would notice a filter that returns its measurements
    assert np.abs(np.asarray(R.smooth_cv(z, obs, d, 0.01, 0.04, 1.0)[0]) - z)[obs].max() > 0.05


def test_constant_velocity_and_yaw_rate_through_pi_are_reproduced():
    no = np.asarray([0, 1, 2, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16], np.int64)
    d = np.concatenate([[0], np.diff(no)])
    obs = [True] * len(no)
    # A track starts with v ~ N(0, v0), which pulls a short track's velocity towards 0 by (posterior variance / v0): the
    # property is that of the model a noise-free track comes from - no process noise, q = 0 - with a diffuse start,
    # v0 = 1e8 (a pull of 3e-12 on the position and 3e-13 on the velocity of these 14 rows).
    # fp64 level: a line, and a yaw of rate 0.125 from 2.5 that crosses pi, to 1e-9
    ps, vs = R.smooth_cv(3.0 + 0.3 * no, obs, d, 0.0, 0.04, DIFFUSE)
    assert np.abs(np.asarray(ps) - (3.0 + 0.3 * no)).max() < 1e-9 and np.abs(np.asarray(vs) - 0.3).max() < 1e-9
    true = 2.5 + 0.125 * no
    y = [R.wrap(v) for v in true]
    assert min(y) < -2.5 and max(y) > 2.5  # it does cross
    u = R.unwrap(y, obs, False)
    ps, vs = R.smooth_cv(u, obs, d, 0.0, 0.01, DIFFUSE)
    assert np.abs(np.asarray(ps) - true).max() < 1e-9 and np.abs(np.asarray(vs) - 0.125).max() < 1e-9
    assert np.abs(np.asarray([R.wrap_loop(v) for v in ps]) - y).max() < 1e-9
    # through the tables, with values fp32 holds exactly: the stored location IS the input, the velocity the true one
    loc = np.stack([-14.0 + 0.0625 * no, 1.5 + 0.015625 * no, 12.0 + 0.125 * no], 1)
    t = C.single_track(no, loc=loc, yaw=np.asarray(y), dims=np.tile([1.5, 1.75, 4.0], (len(no), 1)))
    res = C.ref(t, q_loc=0.0, q_yaw=0.0, v0_loc=DIFFUSE, v0_yaw=DIFFUSE)
    assert np.array_equal(res['out'][:, 7:10], t['det'][:, 7:10]) and np.array_equal(res['out'][:, 4:7], t['det'][:, 4:7])
    assert np.abs(res['vel'][:, 0:3].astype(np.float64) - [0.0625, 0.015625, 0.125]).max() < 1e-9
    # the yaw went through fp32 (2e-7 on these values): the smoothed line stays within that of the stored one
    assert np.abs(res['out'][:, 10] - t['det'][:, 10]).max() < 5e-7 and np.abs(res['vel'][:, 3] - 0.125).max() < 5e-7
    assert res['info'].tolist() == [[0, 1, len(no), 0]]


def test_constant_size_is_the_mean_of_the_observed_sizes():
    rng = np.random.default_rng(3)
    z = 1.6 + rng.normal(0, 0.1, 25)
    obs = np.concatenate([[True], rng.random(24) > 0.3])
    d = np.concatenate([[0], rng.integers(1, 4, 24)])
    ps = np.asarray(R.smooth_walk(z, obs, d, 0.0, 0.01))
    assert np.abs(ps - z[obs].mean()).max() < 1e-12
    dims = np.stack([z, z + 0.25, z + 2.0], 1)
    t = C.single_track(np.cumsum(d), dims=dims)
    res = C.ref(t, observed=obs.astype(np.int32))
    mean = t['det'][obs, 4:7].astype(np.float64).mean(0)
    assert np.abs(res['out'][:, 4:7] - mean).max() < 2e-7 and (np.ptp(res['out'][:, 4:7], 0) == 0).all()


def copied_case():
    seq = [(2, [5, -1, 7, 9]), (3, [7, 5]), (5, [-1, 5, 7]), (6, [8, 7]), (9, [5])]
    t = fill_cases.tables([seq])
    obs = np.ones(len(t['ids']), np.int32)
    obs[[0, 5]] = 0  # ID 5 in frames 2 and 3... its rows: 0 (frame 2), 5 (frame 3), 7 (frame 5), 11 (frame 9)
    return t, obs


def test_what_is_copied_bit_for_bit():
    t, obs = copied_case()
    assert t['ids'].tolist() == [5, -1, 7, 9, 7, 5, -1, 5, 7, 8, 7, 5]
    res = C.ref(t, observed=obs)
    out, det = res['out'], t['det']
    same = lambda rows, cols=slice(None): np.array_equal(C.bits(out[rows][:, cols]), C.bits(det[rows][:, cols]))
    # ID -1, the one-row chains of IDs 9 and 8, the two leading unobserved rows of ID 5: as they came, velocity 0
    copied = [1, 6, 3, 9, 0, 5]
    assert same(copied) and (res['vel'][copied] == 0).all()
    changed = [2, 4, 8, 10, 7, 11]
    assert (out[changed, 4:11] != det[changed, 4:11]).all() and same(changed, [0, 1, 2, 3, 11])
    assert res['info'].tolist() == [[0, 2, 6, 6]]
    # a group whose r is 0 is copied, with velocity 0, and the other groups do not notice
    for grp, cols, vcols in (('r_loc', [7, 8, 9], [0, 1, 2]), ('r_yaw', [10], [3]), ('r_dim', [4, 5, 6], [])):
        part = C.ref(t, observed=obs, **{grp: 0.0})
        assert np.array_equal(C.bits(part['out'][:, cols]), C.bits(det[:, cols])) and (part['vel'][:, vcols] == 0).all()
        rest = [c for c in range(12) if c not in cols]
        assert np.array_equal(C.bits(part['out'][:, rest]), C.bits(out[:, rest]))
        assert part['info'].tolist() == [[0, 2, 6, 6]]
    none = C.ref(t, observed=obs, r_loc=0.0, r_yaw=0.0, r_dim=0.0)
    assert np.array_equal(C.bits(none['out']), C.bits(det)) and (none['vel'] == 0).all()
    assert none['info'].tolist() == [[0, 0, 0, 12]]


def test_trailing_unobserved_rows_continue_the_last_velocity():
    no = np.asarray([0, 1, 2, 3, 4, 6, 7, 10])
    rng = np.random.default_rng(5)
    loc = np.stack([0.5 * no, 0.1 * no, 20 - 0.25 * no], 1) + rng.normal(0, 0.1, (8, 3))
    obs = np.asarray([1, 1, 1, 1, 1, 0, 0, 0], np.int32)
    loc[5:] = 99.0  # what an unobserved row holds is not read
    res = C.ref(C.single_track(no, loc=loc, yaw=0.02 * no), observed=obs)
    out, vel = res['out'].astype(np.float64), res['vel'].astype(np.float64)
    for k in (5, 6, 7):
        assert np.array_equal(vel[k], vel[4])
        assert np.abs(out[k, 7:10] - (out[4, 7:10] + (no[k] - no[4]) * vel[4, 0:3])).max() < 1e-5
        assert abs(out[k, 10] - (out[4, 10] + (no[k] - no[4]) * vel[4, 3])) < 1e-6
    assert abs(vel[4, 0] - 0.5) < 0.15


def test_yaw_flip_removes_a_planted_pi():
    no = np.arange(12)
    rng = np.random.default_rng(8)
    yaw = 2.9 + 0.05 * no + rng.normal(0, 0.02, 12)
    clean = np.asarray([R.wrap(v) for v in yaw])
    planted = clean.copy()
    planted[6] = R.wrap(planted[6] + np.pi)
    want = C.ref(C.single_track(no, yaw=clean), yaw_flip=True)['out'][:, 10]
    assert np.array_equal(want, C.ref(C.single_track(no, yaw=clean))['out'][:, 10])  # no step beyond pi/2: no effect
    got = C.ref(C.single_track(no, yaw=planted), yaw_flip=True)['out'][:, 10]
    off = C.ref(C.single_track(no, yaw=planted))['out'][:, 10]
    diff = lambda a, b: np.abs([R.wrap(float(x) - float(y)) for x, y in zip(a, b)]).max()
    assert diff(got, want) < 1e-5 and diff(off, want) > 0.3
    # a detector that stays turned from row 6 on: the track keeps its heading
    turned = clean.copy()
    turned[6:] = [R.wrap(v + np.pi) for v in turned[6:]]
    assert diff(C.ref(C.single_track(no, yaw=turned), yaw_flip=True)['out'][:, 10], want) < 1e-5


def test_identity_records_give_the_standing_camera_result():
    t = fill_cases.tables([fill_cases.random_sequence(np.random.default_rng(21), 30, 6),
                           fill_cases.random_sequence(np.random.default_rng(22), 12, 6)])
    obs = C.random_mask(t, 1)
    still = C.ref(t, observed=obs)
    ident = C.ref(t, observed=obs, xf0=C.identity_records(len(t['frame_no'])))
    assert still['info'][:, 1].sum() >= 8 and all(np.array_equal(C.bits(still[k]), C.bits(ident[k])) for k in still)
    moved = C.ref(t, observed=obs, xf0=C.frame_records(len(t['frame_no']), 3, t['seq_start']))
    assert np.abs(moved['out'][:, 7:10] - still['out'][:, 7:10]).max() > 1e-3
    assert np.array_equal(moved['info'], still['info'])


def test_status_words():
    ok = [(0, [1]), (1, []), (2, [1])]
    res = C.ref(fill_cases.tables([ok, [(0, [2, 5, 2]), (1, []), (2, [2, 5])], ok]))
    assert res['info'].tolist() == [[0, 1, 2, 0], [R.EDUP, 0, 0, 5], [0, 1, 2, 0]]
    t = fill_cases.tables([ok, [(4, [1]), (3, []), (5, [1])], [(7, [3]), (7, []), (9, [3])]])
    res = C.ref(t)
    assert res['info'].tolist() == [[0, 1, 2, 0], [R.ECONTRACT, 0, 0, 2], [R.ECONTRACT, 0, 0, 2]]
    assert np.array_equal(C.bits(res['out'][2:]), C.bits(t['det'][2:])) and (res['vel'][2:] == 0).all()
    assert (res['out'][:2, 7:10] != t['det'][:2, 7:10]).all()
    for key, bad in (('frame_start', [0, 2, 1, 2]), ('frame_start', [0, 1, 1, 9]), ('seq_start', [1, 3]), ('seq_start', [0, 2])):
        t = fill_cases.tables([ok])
        t[key] = np.asarray(bad, np.int32)
        res = C.ref(t)
        assert res['info'].tolist() == [[R.ECONTRACT, 0, 0, 0]] and np.array_equal(C.bits(res['out']), C.bits(t['det']))


def test_track_smoother_validates():
    s = tracks.TrackSmoother()
    assert dict(zip(R.PARAMS, s.params()), yaw_flip=s.yaw_flip) == R.DEFAULT and 'q_loc=0.01' in repr(s)
    for kw in (dict(q_loc=-1), dict(r_yaw=float('nan')), dict(r_dim=float('inf')), dict(v0_loc=0.0), dict(v0_yaw=-0.0),
               dict(q_dim=-1e-300)):
        with pytest.raises(ValueError, match='TrackSmoother'):
            tracks.TrackSmoother(**kw)
    assert tracks.TrackSmoother(r_loc=0.0, v0_loc=0.0).v0_loc == 0.0  # a group that is left alone needs no v0
    with pytest.raises(ValueError, match='TrackSmoother'):
        tracks.pack_smooth([fill_cases.scene(True)], smoother=dict(q_loc=1))
    with pytest.raises(ValueError, match='sizes'):
        torch_ops.smooth_layout([1, 1, 0, 0, 0, 0])
    with pytest.raises(ValueError, match='sizes'):
        torch_ops.smooth_layout([1, 1, 1, 2, 0, 0])


def same_smoothed(a, b):
    assert a.info == b.info and len(a.frames) == len(b.frames) and (a.scores is None) == (b.scores is None)
    for t in range(len(a.frames)):
        assert set(a.frames[t]) == set(b.frames[t])
        for k in a.frames[t]:
            x, y = np.asarray(a.frames[t][k]), np.asarray(b.frames[t][k])
            assert x.dtype == y.dtype and np.array_equal(x, y), (t, k)
        assert np.array_equal(a.ids[t], b.ids[t]) and np.array_equal(a.velocity[t], b.velocity[t])
        assert a.scores is None or np.array_equal(a.scores[t], b.scores[t])


def test_pack_and_unpack_round_trip():
    from test_fill_cpu import moving_sequence
    frames, ids, frame_idx, scores, poses = moving_sequence()
    filled = fill_cases.host_fill([(frames, ids, frame_idx, scores, poses, fill_cases.CALIB)])[2][0]
    observed = [~m for m in filled.filled]
    seqs = [(filled.frames, filled.ids, frame_idx, observed, poses, fill_cases.CALIB, filled.scores),
            C.noisy_scene(True), dict(frames=frames[:9], ids=ids[:9], frame_idx=frame_idx[:9]), dict(frames=[], ids=[])]
    p, res, got = C.host_smooth(seqs, tracks.TrackSmoother(yaw_flip=True))
    assert p['sizes'][:6] == [len(p['ids']), len(p['frame_no']), 4, 1, 1, 1] and p['xf0'].shape == (len(p['frame_no']), 33)
    assert p['observed'].sum() == len(p['ids']) - sum(int(m.sum()) for m in filled.filled)
    lay = torch_ops.smooth_layout(p['sizes'])
    assert lay[0]['xf0'][0] == 0 and len(p['packed']) == lay[2] and len(R.block_of(res, p['sizes'])) == lay[3]
    a = got[0]
    assert len(got) == 4 and got[3].frames == [] and a.info['tracks'] > 2 and a.info['rows_changed'] > 10
    assert a.info['rows_changed'] + a.info['rows_copied'] == sum(len(i) for i in filled.ids)
    n = 0
    for t, d in enumerate(a.frames):
        m = len(filled.ids[t])
        rows = res['out'][n:n + m].astype(np.float64)
        assert np.array_equal(d['dimensions'], rows[:, [6, 4, 5]]) and np.array_equal(d['location'], rows[:, 7:10])
        assert np.array_equal(d['rotation_y'], rows[:, 10]) and np.array_equal(a.velocity[t], res['vel'][n:n + m])
        assert np.array_equal(d['bbox'], filled.frames[t]['bbox']) and np.array_equal(a.scores[t], filled.scores[t])
        assert np.array_equal(a.ids[t], filled.ids[t])
        n += m
    assert got[1].scores is None
    # the inputs are not modified, and a sequence alone gives what it gives in the batch
    assert all(np.array_equal(x['location'], y['location']) for x, y in zip(filled.frames, seqs[0][0]))
    for k in range(3):
        same_smoothed(C.host_smooth([seqs[k]], tracks.TrackSmoother(yaw_flip=True))[2][0], got[k])
    with pytest.raises(tracks.TrackingError, match='sequence 1.*twice'):
        d = {'bbox': np.zeros((2, 4)), 'dimensions': np.ones((2, 3)), 'location': np.ones((2, 3)), 'rotation_y': np.zeros(2)}
        C.host_smooth([([d, d], [[0, 1], [1, 0]]), ([d, d], [[3, 3], [3, 4]])])
    with pytest.raises(ValueError, match='mask'):
        C.host_smooth([([d, d], [[0, 1], [1, 0]], None, [[1, 1], [1]])])


def test_the_writer_and_the_labels_take_the_result(tmp_path):
    from mmmot_amd import evaluate as E
    frames, ids = C.noisy_scene(True)
    st = C.host_smooth([(frames, ids)])[2][0]
    tracks.write_kitti_tracks(str(tmp_path / 'a.txt'), st.frames, st.ids)
    assert len(open(str(tmp_path / 'a.txt')).read().splitlines()) == sum(len(i) for i in ids)
    E.labels_from_tracks(st.frames, st.ids, n_frames=fill_cases.N_FRAMES, box3d=True)


def test_smoothing_helps_on_the_noisy_scene():
    frames, ids = C.noisy_scene(True)
    filled = fill_cases.host_fill([(frames, ids)], 3)[2][0]
    st = C.host_smooth([(filled.frames, filled.ids, None, [~m for m in filled.filled])])[2][0]
    before, n = C.location_error(filled.frames, filled.ids)
    after, _ = C.location_error(st.frames, st.ids)
    holes = sum(len(fill_cases.scene_holes(o)) for o in range(fill_cases.N_OBJ))
    assert n == fill_cases.N_FRAMES * fill_cases.N_OBJ and st.info == {'tracks': 6, 'rows_changed': n, 'rows_copied': 0}
    print('mean location error: %.4f before, %.4f after' % (before, after))
    assert after < before
    lin, k = C.location_error(filled.frames, filled.ids, filled.filled)
    smo, _ = C.location_error(st.frames, st.ids, filled.filled)
    print('filled rows (%d): %.4f by linear interpolation, %.4f smoothed' % (k, lin, smo))
    assert k == holes and smo < lin


def test_motp_gains_on_the_noisy_scene():
    # the 3D evaluator's host restatement: MOTP is the mean 3D IoU of the matches, so larger is better
    import mot3d_ref
    from mmmot_amd import evaluate as E
    gt = E.labels_from_tracks(*fill_cases.scene(False), ground_truth=True, box3d=True)
    frames, ids = C.noisy_scene(True)
    st = C.host_smooth([(frames, ids)])[2][0]
    lab = lambda f, i: E.labels_from_tracks(f, i, n_frames=fill_cases.N_FRAMES, box3d=True)
    before, after = mot3d_ref.evaluate(gt, lab(frames, ids), '3d'), mot3d_ref.evaluate(gt, lab(st.frames, st.ids), '3d')
    for k in ('tp', 'fn', 'fp', 'id_switches', 'fragments'):
        assert before[k] == after[k], k
    print('MOTP %.4f before, %.4f after' % (before['total_cost'] / before['tp'], after['total_cost'] / after['tp']))
    assert before['tp'] == 216 and after['total_cost'] > before['total_cost']
