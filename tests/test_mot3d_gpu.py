"""3D MOT evaluation on the device (csrc/mot3d.hip through mmmot::mot3d / mmmot_amd.evaluate) against the serial
restatement tests/mot3d_ref.py and, in '2d' mode, against the 2D evaluator on the records of the reference's evaluator.

Overlap table: 1e-12 absolute.  Both sides are fp64 without contraction in one written operation order, values are at
most 1, and a clip is a few dozen operations at 1.1e-16 each on scenes kept away from degenerate contacts
(tests/mot3d_cases.py).  Worst difference observed: 0.0 - the device and the restatement agree bit for bit on every
table of this module.
Counters: exact.  total_cost and MODP: 1e-9 relative (sums of fewer than 1e4 terms in [0, 1] taken in another order).
thr and the reachable mask: exact.  AMOTA, sAMOTA, AMOTP: 1e-12."""
import dataclasses

import numpy as np
import pytest
import torch

import mot3d_cases
import mot3d_ref as R
from test_clear_mot_cpu import CASES, golden
from mmmot_amd import evaluate as E
from mmmot_amd.torch_ops import mot3d_layout

pytestmark = pytest.mark.gpu

TOTALS = ('tp', 'itp', 'fn', 'ifn', 'fp', 'n_itr', 'id_switches', 'fragments', 'n_mt', 'n_pt', 'n_ml',
          'n_ignored_trajectories', 'n_gt', 'n_igt', 'n_tr')
LISTS = ('tps', 'itps', 'fps', 'fns', 'ifns', 'n_itrs', 'seq_id_switches', 'seq_fragments')
TWIN_FREE = ('tp', 'itp', 'fn', 'ifn', 'fp', 'n_itr', 'n_gt', 'n_igt', 'n_tr')  # do not depend on which twin is matched
_ref = {}


def ref_sweep(name, mode, L=40):
    """the restatement's answer for a scene of tests/mot3d_cases.py; computed once"""
    if (name, mode, L) not in _ref:
        gts, trs, _, _ = mot3d_cases.build(name)
        _ref[(name, mode, L)] = R.sweep(E.concat(gts), E.concat(trs), mode, L=L)
    return _ref[(name, mode, L)]


def close(a, b, tol=1e-9):
    return abs(float(a) - float(b)) <= tol * max(1., abs(float(b)))


def check_point(m, want, twins=False):
    """a ClearMot against the restatement's counters of one operating point"""
    for k in (TWIN_FREE if twins else TOTALS):
        assert int(getattr(m, k)) == int(want[k]), (k, getattr(m, k), want[k])
    print('total_cost', m.total_cost, want['total_cost'], 'MODP', m.MODP, want['MODP'])
    assert close(m.total_cost, want['total_cost']) and close(m.MODP, want['MODP'])
    assert np.all(np.abs(m.MODP_t - want['MODP_t']) <= 1e-9)
    if twins:
        return
    for k in LISTS:
        assert list(getattr(m, k)) == list(want[k]), k
    assert all(close(a, b) for a, b in zip(m.seq_costs, want['seq_costs']))
    assert np.array_equal(m.traj_key, want['traj_key'])
    assert np.array_equal(m.gt_tracker, want['gt_tracker']) and np.array_equal(m.gt_ignored, want['gt_ignored'])


@pytest.fixture(scope='module')
def shapes():
    """one sequence whose frames hold every (G, T) of {0, 1, 2, 65, 128}^2, with the restatement's pass A"""
    n = (0, 1, 2, 65, 128)
    gt, tr = mot3d_cases.shape_frames(np.random.default_rng(77), [(g, t) for g in n for t in n])
    return gt, tr, R.evaluate(gt, tr, '3d', 0.75, min_height=0)


def test_overlap_table_and_frame_shapes(shapes):
    gt, tr, want = shapes
    got = E.overlap_tables(gt, tr, '3d')
    assert [t.shape for t in got] == [t.shape for t in want['tables']] and len(got) == 25
    worst = max([float(np.max(np.abs(a - b))) for a, b in zip(got, want['tables']) if a.size] + [0.])
    print('worst |c_device - c_restatement| (3d):', worst)
    assert worst <= 1e-12
    hit = sum(int(np.sum(t < 1.0)) for t in got)
    assert hit > 2000 and sum(int(np.sum(t <= 0.75)) for t in got) > 50  # overlapping cells, and cells inside the gate
    # empty sides, the transposed branch (G > T), the second column per lane (65) and the cap (128), all in one call
    m = E.evaluate_3d_sequences(gt, tr, overlap='3d', levels=0, min_height=0)
    check_point(m.all, want)
    assert m.all.tp > 50 and m.levels == 0 and m.best is None and m.AMOTA == 0.0


def test_bev_table_and_special_headings():
    gts, trs, _, _ = mot3d_cases.build('three')
    gt, tr = E.concat(gts), E.concat(trs)
    for h in mot3d_cases.RY_SPECIAL:
        assert np.any(gt.box3d[:, E.B3_RY] == h)
    for mode in ('bev', '3d'):
        got, want = E.overlap_tables(gt, tr, mode), ref_sweep('three', mode)['all']['tables']
        worst = max(float(np.max(np.abs(a - b))) for a, b in zip(got, want) if a.size)
        print('worst |c_device - c_restatement| (%s):' % mode, worst)
        assert worst <= 1e-12


@pytest.mark.parametrize('fixture,ev', [c for c in CASES if c[0] in ('kitti_car', 'kitti_ped', 'edges')],
                         ids=['%s-%s' % c for c in CASES if c[0] in ('kitti_car', 'kitti_ped', 'edges')])
def test_2d_mode_equals_the_2d_evaluator_bit_for_bit(fixture, ev):
    gt, tr, d = golden(fixture, ev)
    a = E.evaluate_sequences(gt, tr, cls=str(d['cls']))
    b = E.evaluate_3d_sequences(gt, tr, cls=str(d['cls']), overlap='2d', levels=0).all
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), f.name
        else:
            assert type(x) is type(y) and x == y, (f.name, x, y)
    assert a.stats_line() == b.stats_line()


@pytest.mark.parametrize('name', ['one', 'three'])
@pytest.mark.parametrize('mode', ['3d', 'bev'])
def test_operating_points_equal_the_restatement(name, mode):
    gts, trs, _, _ = mot3d_cases.build(name)
    want = ref_sweep(name, mode)
    m = E.evaluate_3d_sequences(gts, trs, overlap=mode, levels=0)
    check_point(m.all, want['all'])
    assert len(m.all.tps) == len(gts) and m.all.fp > 0 and m.all.fn > 0 and m.all.n_itr > 0 and m.all.n_igt > 0


def check_sweep(m, want, L):
    assert m.levels == L and np.array_equal(m.reachable, want['reachable'])
    assert np.array_equal(m.thr, want['thr'])  # +inf where unreachable, on both sides
    for k in range(L):
        if not want['reachable'][k]:
            assert m.MOTA_k[k] == 0. and m.sMOTA_k[k] == 0. and m.MOTP_k[k] == 0.
            continue
        w = want['levels'][k]
        got = dict(zip(('tp', 'itp', 'fn', 'ifn', 'fp', 'n_itr', 'id_switches', 'fragments', 'n_mt', 'n_pt', 'n_ml',
                        'n_ignored_trajectories'), m.counters[k].tolist()))
        assert got == {key: int(w[key]) for key in got}, (k, got)
        assert int(m.n_gt_k[k]) == w['n_gt'] and close(m.cost_k[k], w['total_cost'])
    for key in ('MOTA_k', 'sMOTA_k', 'MOTP_k'):
        assert np.all(np.abs(getattr(m, key) - want[key]) <= 1e-12), key
    print('AMOTA', m.AMOTA, want['AMOTA'], 'sAMOTA', m.sAMOTA, want['sAMOTA'], 'AMOTP', m.AMOTP, want['AMOTP'])
    assert abs(m.AMOTA - want['AMOTA']) <= 1e-12 and abs(m.sAMOTA - want['sAMOTA']) <= 1e-12
    assert abs(m.AMOTP - want['AMOTP']) <= 1e-12
    assert m.best_level == want['best']
    check_point(m.all, want['all'])
    if want['best'] >= 0:
        check_point(m.best, dict(want['levels'][want['best']]))
        smax = max(want['sMOTA_k'][want['reachable']])
        assert m.best_level == min(k for k in range(L) if want['reachable'][k] and want['sMOTA_k'][k] == smax)  # lowest k
    else:
        assert m.best is None


@pytest.mark.parametrize('name,mode', [('few_tp', '3d'), ('tied', '3d'), ('reachable', '3d'), ('three', '3d'),
                                       ('three', 'bev')])
def test_sweep_equals_the_restatement(name, mode):
    gts, trs, _, _ = mot3d_cases.build(name)
    want = ref_sweep(name, mode)
    m = E.evaluate_3d_sequences(gts, trs, overlap=mode, levels=40)
    check_sweep(m, want, 40)
    reach = want['reachable']
    if name == 'few_tp':  # fewer true positives than levels: some thresholds repeat, the upper levels are out of reach
        assert want['all']['n_gt'] < 40 and reach.any() and not reach.all() and len(set(m.thr[reach].tolist())) < reach.sum()
    if name == 'tied':  # tracks tied at a threshold are all kept: the level holds more rows than it needs
        assert len(set(m.thr[reach].tolist())) <= 3
        k = int(np.flatnonzero(reach)[0])
        assert int(m.counters[k][0]) > (k + 1) * want['all']['n_gt'] // 40 + 1
    if name == 'reachable':
        assert reach.all()
    assert m.all.n_tr >= max(int(c[0] + c[4]) for c in m.counters[reach])


def test_other_level_counts():
    gts, trs, _, _ = mot3d_cases.build('one')
    for L in (1, 7):
        check_sweep(E.evaluate_3d_sequences(gts, trs, levels=L), ref_sweep('one', '3d', L), L)


def same_bits(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, E.ClearMot):
            same_bits(x, y)
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), f.name
        else:
            assert x == y, (f.name, x, y)


def test_two_calls_are_bit_equal_and_the_sequence_order_does_not_matter():
    gts, trs, _, _ = mot3d_cases.build('three')
    a, b = E.evaluate_3d_sequences(gts, trs), E.evaluate_3d_sequences(gts, trs)
    same_bits(a, b)
    r = E.evaluate_3d_sequences(gts[::-1], trs[::-1])
    # every integer, the thresholds and what is formed from integers alone: equal; the per-sequence values: reversed,
    # bitwise; the sums over sequences are taken in sequence order, so they may differ in the last bits
    assert np.array_equal(r.counters, a.counters) and np.array_equal(r.thr, a.thr) and np.array_equal(r.reachable, a.reachable)
    assert r.AMOTA == a.AMOTA and r.sAMOTA == a.sAMOTA and r.best_level == a.best_level and abs(r.AMOTP - a.AMOTP) <= 1e-12
    for x, y in ((r.all, a.all), (r.best, a.best)):
        for k in LISTS + ('seq_costs', 'seq_modp', 'n_gts', 'n_trs'):
            assert list(getattr(x, k)) == list(getattr(y, k))[::-1], k
        for k in TOTALS:
            assert getattr(x, k) == getattr(y, k), k
        assert close(x.total_cost, y.total_cost, 1e-12)


def test_planted_twins():
    gts, trs, _, _ = mot3d_cases.build('twins')
    gt, tr = E.concat(gts), E.concat(trs)
    twins = sum(len(rows) - len(np.unique(rows, axis=0)) for rows in
                [tr.box3d[tr.rows[:, E.FRAME] == f][:, :7] for f in range(int(gt.length[0]))])
    assert twins >= 8
    for mode in ('3d', 'bev'):
        want = R.evaluate(gt, tr, mode, 0.75)
        check_point(E.evaluate_3d_sequences(gt, tr, overlap=mode, levels=0).all, want, twins=True)


def test_refusals():
    gts, trs, _, _ = mot3d_cases.build('few_tp')
    gt, tr = gts[0], trs[0]
    strip = lambda lb: E.Labels(lb.rows, lb.n_frames, lb.length, lb.n_traj, lb.cls, lb.ground_truth)
    with pytest.raises(ValueError, match='box3d'):
        E.evaluate_3d_sequences(strip(gt), tr)
    with pytest.raises(ValueError, match='sequences'):
        E.evaluate_3d_sequences([gt, gt], [tr])
    with pytest.raises(ValueError, match='levels'):
        E.evaluate_3d_sequences(gt, tr, levels=-1)
    bad = E.Labels(tr.rows, tr.n_frames, tr.length, tr.n_traj, tr.cls, False, tr.box3d.copy())
    bad.box3d[1, E.B3_W] = 0.
    with pytest.raises(ValueError, match='dimension'):
        E.evaluate_3d_sequences(gt, bad)
    many = mot3d_cases.labels([[0, 0, i, E.MAIN, 0, 0, i, 10, i + 40, 90] for i in range(129)],
                              [[1.5, 1.6, 4., 3. * i, 1.6, 20., 0., 0.5] for i in range(129)], 1, False)
    one = mot3d_cases.labels([[0, 0, 0, E.MAIN, 0, 0, 0, 10, 40, 90]], [[1.5, 1.6, 4., 0., 1.6, 20., 0., 0.]], 1, True)
    with pytest.raises(ValueError, match='more than 128'):
        E.evaluate_3d_sequences(one, many)
    dc = mot3d_cases.labels([[0, 0, -1, E.DONTCARE, -1, -1, i, 10, i + 40, 90] for i in range(65)],
                            [[-1, -1, -1, -1000, -1000, -1000, -10, 0]] * 65, 1, True)
    with pytest.raises(ValueError, match='DontCare'):
        E.evaluate_3d_sequences(dc, many)
    # the operator raises on a wrongly sized block
    p = E.pack_3d(gt, tr)
    sizes = list(p['sizes']) + [p['cells'], 40, 0]
    n_in = mot3d_layout(sizes)[2]
    for block in (torch.zeros(n_in + 1, dtype=torch.int32, device='cuda'), torch.zeros(n_in, dtype=torch.int64, device='cuda')):
        with pytest.raises(ValueError, match='packed'):
            torch.ops.mmmot.mot3d(block, sizes, [0.75, 25., 0., 2.])
    with pytest.raises(ValueError, match='params'):
        torch.ops.mmmot.mot3d(torch.zeros(n_in, dtype=torch.int32, device='cuda'), sizes, [0.75])


def test_end_to_end_from_files_equals_from_memory(tmp_path):
    """SequencePipeline(associate=True, track=True) on the synthetic workload of tests/test_tracks_gpu.py: the result
    file with scores through evaluate_3d equals labels_from_tracks through evaluate_3d_sequences; the ground truth is
    the detections themselves under their own indices"""
    from mmmot_amd.pipeline import SequencePipeline
    from mmmot_amd.tracks import write_kitti_tracks
    from test_tracks_gpu import S, feeds, model
    fs = feeds()[:8]
    pipe = SequencePipeline(model(), S, associate=True, track=True)
    pipe.run(fs)
    dets = [f.dets for f in fs]
    rng = np.random.default_rng(5)
    scores = [rng.uniform(0.1, 1.0, len(d['bbox'])) for d in dets]
    n = len(fs)
    root, gt_path = tmp_path / 'res', tmp_path / 'gt'
    (root / 'run' / 'val').mkdir(parents=True)
    (gt_path / 'label_02').mkdir(parents=True)
    (gt_path / 'evaluate_tracking.seqmap').write_text('0005 empty 000000 %06d\n' % (n - 1))
    write_kitti_tracks(str(root / 'run' / 'val' / '0005.txt'), dets, pipe.tracks, scores=scores)
    gt_ids = [np.arange(len(d['bbox'])) for d in dets]
    gt_dets = [dict(d, truncated=np.zeros(len(d['bbox'])), occluded=np.zeros(len(d['bbox']), np.int64)) for d in dets]
    write_kitti_tracks(str(gt_path / 'label_02' / '0005.txt'), gt_dets, gt_ids)
    a = E.evaluate_3d('run', str(root), 'val', gt_path=str(gt_path), cls='car')
    gt = E.labels_from_tracks(gt_dets, gt_ids, n_frames=n, ground_truth=True, box3d=True)
    tr = E.labels_from_tracks(dets, pipe.tracks, n_frames=n, box3d=True, scores=scores)
    b = E.evaluate_3d_sequences(gt, tr)
    same_bits(a, b)
    assert a.all.tp > 0 and a.all.tp == a.all.n_tr and a.all.fp == 0 and a.all.MOTP > 0.999 and a.reachable.any()
    with open(str(root / 'run' / 'val' / 'eval' / 'car' / 'stats3d_car.txt')) as f:
        assert f.read() == a.summary_line() + '\n'
