"""Tracklet stitching without a GPU: the NumPy restatement tests/stitch_ref.py at the boundaries
the section names, its matching against scipy's assignment solver, the chains, the host sides ``tracks.pack_stitch`` /
``unpack_stitch`` with the restatement standing in for the launches, the Meta kernel of mmmot::stitch_tracks, and what
stitching is for: on the scene with one long hole per object every object gets one ID again."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import clear_mot_ref
import fill_cases
import smooth_cases
import stitch_cases as C
import stitch_ref
from mmmot_amd import ego, synth, torch_ops, tracks
from mmmot_amd import evaluate as E


def hand(spec, stray=()):
    """tables of hand-made tracks: ``spec[k]`` = list of (frame number, (x, y, z)[, (vx, vy, vz)[, (h, w, l)]]) rows of
    track k (ID 10 + k); the listed frames are the numbers that occur, in order"""
    nos = sorted({r[0] for t in spec for r in t} | set(stray))
    rows = sorted((r[0], k, r) for k, t in enumerate(spec) for r in t)
    det, ids, vel, counts = [], [], [], [0] * len(nos)
    for no, k, r in rows:
        d = np.zeros(12)
        d[2:4], d[11] = 50.0, 0.5
        d[4:7] = r[3] if len(r) > 3 else (1.5, 1.6, 4.0)
        d[7:10] = r[1]
        det.append(d)
        ids.append(10 + k)
        vel.append(tuple(r[2] if len(r) > 2 else (0, 0, 0)) + (0,))
        counts[nos.index(no)] += 1
    return dict(det=np.asarray(det).reshape(-1, 12).astype(np.float32), ids=np.asarray(ids, np.int32),
                vel=np.asarray(vel, np.float64).reshape(-1, 4).astype(np.float32),
                frame_start=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), frame_no=np.asarray(nos, np.int32),
                seq_start=np.asarray([0, len(nos)], np.int32))


def link(t, i=0, j=1, **prm):
    r = C.ref(t, **prm)
    K = int(r['info'][0, 1])
    return r['links'].reshape(K, K)[i, j], r


def line(k, frames, p0, v, dims=None):
    return [(no, tuple(np.asarray(p0, np.float64) + np.asarray(v, np.float64) * no), tuple(v)) + (() if dims is None else (dims,))
            for no in frames]


def test_tables_are_the_stitchers():
    k = tracks.TrackStitcher(max_dt=17, drift=0.3, max_speed=3.0, slack=1.5)
    r2, inv = stitch_ref.tables(0.3, 3.0, 1.5, 17)
    assert np.array_equal(C.bits(k.r2), C.bits(r2)) and np.array_equal(C.bits(k.inv_r2), C.bits(inv))
    assert np.isnan(k.r2[:, 0]).all() and np.isnan(k.inv_r2[:, 0]).all() and k.r2.shape == (2, 18)
    assert k.r2[0, 2] == (0.3 * 2 + 1.5) ** 2 or abs(k.r2[0, 2] - 4.41) < 1e-12
    assert k.r2[1, 3] == 110.25


def test_radius_is_inclusive_and_the_next_location_is_not():
    # two one-row tracks three frames apart: no velocity, row 1 of the table, r = 4 * 3 + 2 = 14, d2 = 196 = r2 exactly
    t = hand([[(0, (0, 0, 0))], [(3, (14, 0, 0))]])
    s, r = link(t)
    assert np.isfinite(s) and r['info'][0].tolist()[:2] == [0, 2]
    want = np.float32(np.float64(1.0) - np.float64(196.0) * (np.float64(1.0) / np.float64(196.0)))
    assert C.bits(np.float32(s)) == C.bits(want)
    t = hand([[(0, (0, 0, 0))], [(3, (float(np.nextafter(np.float32(14), np.float32(15))), 0, 0))]])
    s, _ = link(t)
    assert C.bits(np.float32(s)) == 0x7fc00000
    # the y distance counts in '3d' only
    t = hand([[(0, (0, 0, 0))], [(3, (14, 1, 0))]])
    assert np.isfinite(link(t)[0]) and np.isnan(link(t, mode='3d')[0])


def test_dt_bounds():
    two = lambda dt: hand([[(5, (0, 0, 0))], [(5 + dt, (0.5, 0, 0))]])
    for dt, present in ((2, False), (3, True), (7, True), (8, False)):
        s, r = link(two(dt), min_dt=3, max_dt=7)
        assert np.isfinite(s) == present, dt
        assert r['info'][0, 2] == int(present)
    # a track is no candidate of itself, and a head in front of a tail is none
    s, r = link(two(3), 0, 0)
    assert np.isnan(s) and np.isnan(link(two(3), 1, 0)[0]) and np.isnan(link(two(3), 1, 1)[0])


def test_frame_numbers_not_positions_give_dt():
    # listed frames 0, 1, 2 carry the numbers 0, 1, 6: the hole is 5 frame numbers long
    t = hand([[(0, (0, 0, 0)), (1, (0.1, 0, 0))], [(6, (0.6, 0, 0))]])
    assert np.isnan(link(t, max_dt=4)[0]) and np.isfinite(link(t, max_dt=5)[0])
    r = C.ref(t, max_dt=5, gap_penalty=0.01)
    d2 = np.float64(np.float32(0.6) - np.float32(0.1)) ** 2
    r2 = np.float64(4.0 * 5 + 2.0) ** 2
    want = np.float32((1.0 - d2 * (1.0 / r2)) - np.float64(0.01) * 4.0)
    assert C.bits(r['links'].reshape(2, 2)[0, 1]) == C.bits(want)


@pytest.mark.parametrize('what', ['location', 'velocity', 'dimension'])
def test_nan_removes_the_link(what):
    a = line(0, [0, 1, 2], (0, 0, 0), (0.2, 0, 0), (1.5, 1.6, 4.0))
    b = line(1, [5, 6, 7], (0, 0, 0), (0.2, 0, 0), (1.5, 1.6, 4.0))
    prm = dict(max_size_ratio=1.5)
    assert np.isfinite(link(hand([a, b]), **prm)[0])
    for side in (0, 1):
        t = hand([a, b])
        row = 2 if side == 0 else 3  # the tail of track 0, the head of track 1
        if what == 'location':
            t['det'][row, 7] = np.nan
        elif what == 'velocity':
            t['vel'][row, 2] = np.nan
        else:
            t['det'][row, 5] = np.nan
        s, r = link(t, **prm)
        assert C.bits(np.float32(s)) == 0x7fc00000 and r['info'][0].tolist() == [0, 2, 0, 0]


@pytest.mark.parametrize('rows_tail,rows_head', [(3, 3), (3, 2), (2, 3), (2, 2)])
def test_the_four_velocity_cases(rows_tail, rows_head):
    """min_rows = 3: a track of two rows has no velocity.  The tail track's velocity is exact, the head track's is off
    by 0.1 in x, so ef and eb differ and each case has its own score"""
    v = (0.25, 0.0, 0.125)
    a = line(0, range(3 - rows_tail, 3), (1, 1.5, 20), v)
    b = [(no, p, (0.35, 0.0, 0.125)) for no, p, _ in line(1, range(8, 8 + rows_head), (1, 1.5, 20), v)]
    s, r = link(hand([a, b]))
    d = np.float64(6.0)
    Pt, Ph = (np.asarray(x[-1 if k == 0 else 0][1], np.float32).astype(np.float64) for k, x in enumerate((a, b)))
    Vt, Vh = np.asarray(v, np.float32).astype(np.float64), np.asarray((0.35, 0.0, 0.125), np.float32).astype(np.float64)
    g = lambda e: e[0] * e[0] + e[2] * e[2]
    ef, eb, es = g(Ph - (Pt + d * Vt)), g(Pt - (Ph - d * Vh)), g(Ph - Pt)
    tv, hv = rows_tail >= 3, rows_head >= 3
    d2 = max(ef, eb) if tv and hv else (ef if tv else (eb if hv else es))
    r2 = np.float64((0.5 if tv or hv else 4.0) * 6 + 2.0) ** 2
    assert ef < eb < es
    assert C.bits(np.float32(s)) == C.bits(np.float32(1.0 - d2 * (1.0 / r2)))
    assert np.isnan(link(hand([a, b]), vel=None)[0]) == (es > (4.0 * 6 + 2.0) ** 2)
    # without velocities every case is the static one
    assert C.bits(np.float32(link(hand([a, b]), vel=None)[0])) == C.bits(np.float32(1.0 - es * (1.0 / np.float64(26.0) ** 2)))


def test_both_velocities_need_both_errors_inside():
    # the head track's velocity is so wrong that eb leaves the radius while ef stays inside
    a = line(0, [0, 1, 2], (0, 0, 0), (0.2, 0, 0))
    b = [(no, p, (2.0, 0, 0)) for no, p, _ in line(1, [6, 7, 8], (0, 0, 0), (0.2, 0, 0))]
    assert np.isnan(link(hand([a, b]))[0])
    assert np.isfinite(link(hand([a, b[:2]]))[0])  # two rows: the head has no velocity, ef alone decides


def test_identity_records_equal_none_bit_for_bit():
    t = C.with_k(3, 24, holey=True, stray=5)
    a, b = C.ref(t), C.ref(t, xf0=smooth_cases.identity_records(len(t['frame_no'])))
    for k in a:
        assert np.array_equal(C.bits(a[k]), C.bits(b[k])), k
    assert a['info'][0, 2] > 0


def test_composed_record_moves_a_centre_like_align_pos():
    """words 0..15 of the xf0 record ``pack_stitch`` stores for frame p, applied by the restatement, against
    ``ego.align_pos`` with (R, T) of (frame 0, frame p): 1e-11 m, the bound of tests/test_fill_cpu.py for the same
    composed matrix"""
    n = 9
    poses = synth.ego_poses(n, 3)
    t = C.with_k(4, 6)
    frames = [dict(bbox=np.zeros((0, 4)), dimensions=np.zeros((0, 3)), location=np.zeros((0, 3)), rotation_y=np.zeros(0))] * n
    p = tracks.pack_stitch([(frames, [np.zeros(0, np.int64)] * n, None, None, poses, fill_cases.CALIB)])
    assert np.array_equal(p['xf0'], smooth_cases.frame_records(n, 3))
    loc = t['det'][:, 7:10]
    for q in range(1, n):
        R, T = ego.pair_motion(poses[0], poses[q])
        want, _ = ego.align_pos([R], [T], synth.KITTI_TR, synth.KITTI_IMU2VELO, synth.KITTI_R0,
                                [poses[q][1] - poses[0][1]], loc.astype(np.float64), np.zeros(len(loc)))
        got = np.asarray([stitch_ref.record(row, None, p['xf0'][q, 0:16])[0] for row in t['det']])
        assert np.abs(got - want).max() < 1e-11
    # a velocity turns with the record and is not shifted
    P0, V = stitch_ref.record(t['det'][0], np.asarray([1, 2, 3, 0], np.float32), p['xf0'][5, 0:16])
    z = np.zeros(12, np.float32)
    z[7:10] = (1, 2, 3)
    assert np.allclose(V, stitch_ref.record(z, None, p['xf0'][5, 0:16])[0] - p['xf0'][5, 12:15], atol=1e-12)


def test_no_track_one_track_and_one_row_tracks():
    t = hand([[(0, (0, 0, 0))]])
    t['ids'][:] = -1
    r = C.ref(t)
    assert r['info'].tolist() == [[0, 0, 0, 0]] and np.isnan(r['objective'][0]) and len(r['links']) == 0
    assert r['out_ids'].tolist() == [-1] and r['next'].tolist() == [-1]
    r = C.ref(hand([[(0, (0, 0, 0)), (1, (0, 0, 0))]]))
    assert r['info'].tolist() == [[0, 1, 0, 0]] and r['objective'][0] == 0.0 and np.isnan(r['links']).all()
    r = C.ref(hand([[(0, (0, 0, 0))], [(2, (0.1, 0, 0))], [(4, (0.2, 0, 0))]]))
    assert r['info'].tolist() == [[0, 3, 2, 2]] and r['out_ids'].tolist() == [10, 10, 10] and r['next'].tolist() == [1, 2, -1]


def test_statuses():
    t = hand([[(0, (0, 0, 0))], [(0, (5, 0, 0))], [(3, (0, 0, 0))]])
    ok = C.ref(t)
    assert ok['info'][0, 0] == 0 and ok['info'][0, 2] == 1
    quiet = lambda r, ids=t['ids']: (np.array_equal(r['out_ids'], ids) and (r['next'] == -1).all() and np.isnan(r['objective']).all()
                       and (C.bits(r['links']) == 0x7fc00000).all() and len(r['links']) == 9)
    dup = dict(t, ids=np.asarray([10, 10, 12], np.int32))
    ks, pr = C.track_tables(t)
    r = C.ref(dup, k_start=ks, pairs=pr)
    assert r['info'].tolist() == [[stitch_ref.EDUP, 0, 0, 0]] and quiet(r, dup['ids'])
    r = C.ref(dict(t, frame_no=np.asarray([3, 3], np.int32)))
    assert r['info'].tolist() == [[stitch_ref.ECONTRACT, 0, 0, 0]] and quiet(r)
    r = C.ref(dict(t, frame_start=np.asarray([0, 3, 2], np.int32)), k_start=ks, pairs=pr)
    assert r['info'].tolist() == [[stitch_ref.ECONTRACT, 0, 0, 0]] and quiet(r)
    # a k_start that counts another number of tracks than the sequence holds, with a pairs table that follows it
    r = C.ref(dict(t, ids=np.asarray([10, 11, 10], np.int32)), k_start=ks, pairs=pr)
    assert r['info'].tolist() == [[stitch_ref.ECONTRACT, 0, 0, 0]] and quiet(r, np.asarray([10, 11, 10]))
    # a pairs table that is not the one of k_start
    bad = pr.copy()
    bad[0, 3] = 1
    r = C.ref(t, pairs=bad)
    assert r['info'].tolist() == [[stitch_ref.ECONTRACT, 0, 0, 0]] and quiet(r)


def test_too_many_tracks():
    t = C.with_k(9, 513)
    r = C.ref(t)
    assert r['info'].tolist() == [[stitch_ref.ETOOMANY, 0, 0, 0]] and np.isnan(r['objective'][0])
    assert len(r['links']) == 513 * 513 and (C.bits(r['links']) == 0x7fc00000).all()
    assert np.array_equal(r['out_ids'], t['ids']) and (r['next'] == -1).all()
    assert C.ref(C.with_k(9, 512))['info'][0].tolist()[:2] == [0, 512]


def lsa(blk):
    """scipy on the gains padded with K zero-gain dummies per side: (column per row or -1, objective, margin to the best
    assignment that differs in one row's choice)"""
    K = len(blk)
    g = np.where(blk > 0, blk.astype(np.float64), 0.0)
    pad = np.zeros((2 * K, 2 * K))
    pad[:K, :K] = g
    rows, cols = linear_sum_assignment(pad, maximize=True)
    obj = pad[rows, cols].sum()
    match = np.asarray([c if c < K and g[r, c] > 0 else -1 for r, c in zip(rows[:K], cols[:K])])
    margin = np.inf
    for i in range(K):  # forbid row i's choice (a link, or staying unmatched) and solve again
        alt = pad.copy()
        if match[i] >= 0:
            alt[i, match[i]] = -1e9
        else:
            alt[i, K:] = -1e9
            alt[i, :K] = np.where(g[i] > 0, g[i], -1e9)
        r2, c2 = linear_sum_assignment(alt, maximize=True)
        margin = min(margin, obj - alt[r2, c2].sum())
    return match, obj, margin


MATCH_CASES = [(seed, K) for seed, K in ((1, 2), (2, 3), (3, 5), (4, 8), (5, 13), (6, 21), (7, 30), (8, 40), (9, 40))]


@pytest.mark.parametrize('seed,K', MATCH_CASES)
def test_matching_against_scipy(seed, K):
    """crowded objects (2.5 m apart, 0.4 m of noise, up to 13 frames of hole), so that tails compete for heads"""
    t = C.with_k(seed, K, spread=2.5, sigma=0.4)
    r = C.ref(t)
    blk = r['links'].reshape(K, K)
    match, obj, margin = lsa(blk)
    print('K %d: %d links, %d stitches, objective %.9f, margin %.3g' % (K, np.isfinite(blk).sum(), (match >= 0).sum(), obj, margin))
    assert abs(r['objective'][0] - obj) <= 1e-9
    assert margin > 1e-6  # the optimum is unique: the generator's seeds are chosen so
    heads = np.asarray([np.flatnonzero(t['ids'] == i)[0] for i in sorted(set(t['ids'].tolist()), key=lambda i: np.flatnonzero(t['ids'] == i)[0])])
    tails = np.asarray([np.flatnonzero(t['ids'] == t['ids'][h])[-1] for h in heads])
    got = np.asarray([-1 if r['next'][tl] < 0 else int(np.flatnonzero(heads == r['next'][tl])[0]) for tl in tails])
    assert np.array_equal(got, match)
    assert r['info'][0, 2] == (match >= 0).sum()
    if K >= 13:
        assert any(np.isfinite(blk[i]).sum() > 1 for i in range(K))  # a tail with a choice


def test_solver_ties_go_to_the_smallest_index():
    blk = np.full((3, 3), stitch_ref.QNAN, np.float32)
    blk[0, 1] = blk[0, 2] = blk[1, 2] = 0.5
    match, obj = stitch_ref.solve(blk)
    assert match.tolist() == [1, 2, -1] and obj == 1.0
    blk[:] = 0.25
    assert stitch_ref.solve(blk)[0].tolist() == [0, 1, 2]
    blk[:] = -0.25  # nothing gains
    assert stitch_ref.solve(blk)[0].tolist() == [-1, -1, -1]


def test_a_chain_takes_the_roots_id():
    v = (0.2, 0, 0.1)
    spec = [line(0, [0, 1, 2], (0, 1, 10), v), line(1, [9, 10, 11], (0, 1, 10), v), line(2, [20, 21, 22, 23], (0, 1, 10), v),
            line(3, [0, 1, 2, 3], (30, 1, 30), v)]
    t = hand(spec)
    r = C.ref(t)
    assert r['info'].tolist() == [[0, 4, 2, 7]]
    want = np.where(np.isin(t['ids'], (10, 11, 12)), 10, t['ids'])
    assert np.array_equal(r['out_ids'], want)
    tail = lambda k: np.flatnonzero(t['ids'] == 10 + k)[-1]
    head = lambda k: np.flatnonzero(t['ids'] == 10 + k)[0]
    assert r['next'][tail(0)] == head(1) and r['next'][tail(1)] == head(2) and (r['next'] >= 0).sum() == 2
    for f in range(len(t['frame_no'])):  # no ID twice in a frame
        ids = r['out_ids'][t['frame_start'][f]:t['frame_start'][f + 1]]
        assert len(set(ids.tolist())) == len(ids)


def test_gap_penalty_turns_a_link_down():
    a, b = line(0, [0, 1, 2], (0, 0, 0), (0.2, 0, 0)), line(1, [12, 13, 14], (0, 0, 0), (0.2, 0, 0))
    s, r = link(hand([a, b]))
    assert s > 0.99 and r['info'][0, 2] == 1
    s, r = link(hand([a, b]), gap_penalty=0.2)
    assert s < 0 and r['info'][0].tolist() == [0, 2, 0, 0] and r['objective'][0] == 0.0 and (r['next'] == -1).all()


def frames_of(t, s=0):
    fs, a, b = t['frame_start'], int(t['seq_start'][s]), int(t['seq_start'][s + 1])
    frames, ids, vel = [], [], []
    for f in range(a, b):
        d = t['det'][fs[f]:fs[f + 1]].astype(np.float64)
        frames.append(dict(bbox=d[:, 0:4], dimensions=d[:, [6, 4, 5]], location=d[:, 7:10], rotation_y=d[:, 10]))
        ids.append(t['ids'][fs[f]:fs[f + 1]].astype(np.int64))
        vel.append(t['vel'][fs[f]:fs[f + 1]].astype(np.float64))
    return frames, ids, t['frame_no'][a:b].astype(np.int64), vel


def test_pack_and_unpack_with_the_restatement():
    parts = [C.with_k(11, 9, holey=True, stray=3), C.with_k(12, 1), C.with_k(13, 16)]
    seqs = [frames_of(p) for p in parts]
    k = tracks.TrackStitcher(max_dt=12, min_rows=2, gap_penalty=0.001)
    p, res, out = C.host_stitch(seqs, k)
    both = C.concat(parts)
    for name in ('ids', 'frame_start', 'frame_no', 'seq_start', 'vel'):
        assert np.array_equal(p[name], both[name]), name
    assert np.array_equal(C.bits(p['det'][:, :11]), C.bits(both['det'][:, :11])) and p['xf0'] is None
    assert p['k_start'].tolist() == [0, 9, 10, 26] and p['pairs'].tolist() == [[9, 9, 0, 0], [1, 1, 18, 81], [16, 16, 20, 82]]
    assert p['sizes'][:12] == [len(both['ids']), len(both['frame_no']), 3, 26, 338, 16, 0, 1, 1, 12, 2, 0]
    assert p['packed'].dtype == np.int32 and len(p['packed']) == torch_ops.stitch_layout(p['sizes'])[2]
    assert res['info'][:, 0].tolist() == [0, 0, 0] and res['info'][:, 2].sum() > 0
    for s, (part, st) in enumerate(zip(parts, out)):
        alone = C.host_stitch([seqs[s]], k)[2][0]  # the batch is, per sequence, the single call
        assert all(np.array_equal(a, b) for a, b in zip(alone.ids, st.ids)) and np.array_equal(alone.pairs, st.pairs)
        assert np.array_equal(C.bits(alone.links), C.bits(st.links)) and alone.info == st.info
        assert alone.objective == st.objective or (np.isnan(alone.objective) and np.isnan(st.objective))
        one = C.ref(part, max_dt=12, min_rows=2, gap_penalty=0.001)
        assert np.array_equal(np.concatenate(st.ids), one['out_ids'])
        assert st.links.shape == (part['K'], part['K']) and np.array_equal(C.bits(st.links.reshape(-1)), C.bits(one['links']))
        assert st.info == {'tracks': part['K'], 'stitches': int(one['info'][0, 2]), 'rows_changed': int(one['info'][0, 3])}
        assert st.pairs.dtype == np.int64 and st.pairs.shape == (st.info['stitches'], 4)
        fs = part['frame_start']
        for ta, ja, tb, jb in st.pairs:
            assert one['next'][fs[ta] + ja] == fs[tb] + jb and st.ids[ta][ja] == st.ids[tb][jb]
        assert st.filled is None and st.smoothed is None
    # without velocities; with poses the records of pack_smooth
    frames, ids, no, _ = seqs[0]
    poses = synth.ego_poses(len(frames), 4)
    p2 = tracks.pack_stitch([(frames, ids, no, None, poses, fill_cases.CALIB)])
    assert p2['vel'] is None and p2['sizes'][6:8] == [1, 0]
    assert np.array_equal(p2['xf0'], smooth_cases.frame_records(len(frames), 4))
    with pytest.raises(ValueError):
        tracks.pack_stitch([seqs[0], seqs[1][:3]])  # velocities for one sequence only
    with pytest.raises(ValueError):
        tracks.pack_stitch(seqs, stitcher='no')
    bad = res.copy()
    bad['info'] = res['info'].copy()
    bad['info'][1, 0] = stitch_ref.ETOOMANY
    with pytest.raises(tracks.TrackingError, match='sequence 1'):
        tracks.unpack_stitch(p, stitch_ref.block_of(bad, p['sizes']))


def test_stitcher_validates():
    for kw in (dict(max_dt=0), dict(max_dt=257), dict(min_dt=0), dict(min_dt=5, max_dt=4), dict(max_dt=2.5), dict(drift=-1),
               dict(slack=float('nan')), dict(max_speed=float('inf')), dict(drift=0, slack=0), dict(min_rows=0),
               dict(mode='bev'), dict(max_size_ratio=0.5), dict(gap_penalty=-0.1), dict(gap_penalty=float('nan'))):
        with pytest.raises(ValueError):
            tracks.TrackStitcher(**kw)
    assert 'none of them was tuned' in ' '.join(tracks.TrackStitcher.__doc__.split())
    k = tracks.TrackStitcher()
    assert (k.max_dt, k.min_dt, k.drift, k.max_speed, k.slack, k.min_rows, k.mode, k.max_size_ratio, k.gap_penalty) == \
        (30, 1, 0.5, 4.0, 2.0, 3, 'ground', 0.0, 0.0)


def test_operator_is_registered_with_a_meta_kernel_and_no_cpu_one():
    p = tracks.pack_stitch([frames_of(C.with_k(5, 6))])
    n_out = torch_ops.stitch_layout(p['sizes'])[3]
    out = torch.ops.mmmot.stitch_tracks(torch.empty(len(p['packed']), dtype=torch.int32, device='meta'), p['sizes'])
    assert out.shape == (n_out,) and out.dtype == torch.int32 and out.device.type == 'meta'
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mmmot.stitch_tracks(torch.from_numpy(p['packed']), p['sizes'])
    with pytest.raises(ValueError):
        torch_ops.stitch_layout(p['sizes'][:5])
    lay = torch_ops.stitch_layout(p['sizes'])
    assert list(lay[0])[:3] == ['xf0', 'r2', 'inv_r2'] and list(lay[1])[0] == 'objective'  # the fp64 sections first


def test_abi_entry_is_declared_with_hip_stream():
    from mmmot_amd import _lib
    prm = _lib.PARAMS['mmmot_stitch_tracks']
    assert prm[-1].name == 'hip_stream' and 'mmmot_stitch_tracks' not in _lib.TAKES_STREAM and len(prm) == 30
    assert 'stitch_tracks.hip' in _lib.SOURCES


# ---- the scene --------------------------------------------------------------------------------------------------------
def run_scene(broken):
    frames, ids = C.broken_scene(broken)
    filled = fill_cases.host_fill([(frames, ids)], 3)[2][0]
    sm = smooth_cases.host_smooth([(filled.frames, filled.ids, None, [~m for m in filled.filled])])[2][0]
    return frames, ids, filled, sm


def switches(gt, frames, ids):
    r = clear_mot_ref.evaluate(gt, E.labels_from_tracks(frames, ids, n_frames=fill_cases.N_FRAMES))
    return r['id_switches'], r['fragments'], r['fn']


def test_every_object_gets_one_id_again():
    n = fill_cases.N_OBJ
    gt = E.labels_from_tracks(*fill_cases.scene(False), ground_truth=True)
    frames, ids, filled, sm = run_scene(True)
    assert sorted(set(np.concatenate(ids).tolist())) == list(range(2 * n))
    st = C.host_stitch([(sm.frames, sm.ids, None, sm.velocity)])[2][0]
    assert st.info == {'tracks': 2 * n, 'stitches': n, 'rows_changed': sum((np.asarray(i) >= n).sum() for i in sm.ids)}
    for t, (i, was) in enumerate(zip(st.ids, sm.ids)):
        assert np.array_equal(i, np.asarray(was) % n), t  # object o again under ID o, in every row
    for ta, ja, tb, jb in st.pairs:
        hole = C.scene_long_hole(int(st.ids[ta][ja]))  # a short hole of the scene may touch it: 10 .. 14 frames in all
        assert ta < hole[0] and tb > hole[-1] and len(hole) + 1 <= tb - ta <= 15
    # the evaluation against the hole-free truth, behind one more filling that may close the long holes (max_fill 14):
    # the broken run keeps them - two IDs are not joined - and the stitched run equals the unbroken one.  The CLEAR-MOT
    # restatement counts an ID switch only between two frames an object is tracked in one after the other, so a broken
    # track behind misses shows as a fragment, not as a switch: the switches are equal, the fragments drop
    _, _, filled1, _ = run_scene(False)
    refill = lambda f, i: fill_cases.host_fill([(f, i)], 14)[2][0]
    runs = [refill(filled.frames, filled.ids), refill(filled.frames, st.ids), refill(filled1.frames, filled1.ids)]
    before, after, unbroken = (switches(gt, r.frames, r.ids) for r in runs)
    print('ID switches, fragments, misses: broken %s, stitched %s, unbroken %s' % (before, after, unbroken))
    left = 0  # the frames of an object's long hole and of the short holes that touch it
    for o in range(n):
        missed, hole = fill_cases.scene_holes(o) | set(C.scene_long_hole(o)), C.scene_long_hole(o)
        a, b = hole[0], hole[-1]
        while a - 1 in missed:
            a -= 1
        while b + 1 in missed:
            b += 1
        left += b - a + 1
    assert before == (0, n, left)
    assert after == unbroken == (0, 0, 0)
    assert runs[0].info['links_filled'] == 0 and runs[1].info['links_filled'] == n and runs[1].info['links_too_long'] == 0


def test_without_velocities_the_scene_is_stitched_by_the_static_radius():
    n = fill_cases.N_OBJ
    frames, ids, filled, sm = run_scene(True)
    st = C.host_stitch([(filled.frames, filled.ids)])[2][0]
    assert st.info['stitches'] == n and all(np.array_equal(i, np.asarray(w) % n) for i, w in zip(st.ids, filled.ids))
