"""CLEAR-MOT evaluation, host side (mmmot_amd/evaluate.py, tests/clear_mot_ref.py) against the fixtures the reference's
evaluator produced (tests/golden/clear_mot_*.npz, tools/gen_golden_clear_mot.py): the loaders reproduce the stored
tables, the file-less route equals the file route, the serial restatement reproduces every golden record exactly, the
refusals raise, the Meta kernel gives the operator's shape.  No GPU."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import clear_mot_ref
from mmmot_amd import evaluate as E
from mmmot_amd.torch_ops import clear_mot_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FILES = os.path.join(GOLDEN, 'clear_mot_files')
INTS = ('tp', 'fp', 'fn', 'id_switches', 'fragments', 'n_gt', 'n_gt_trajectories', 'n_tr', 'n_tr_trajectories', 'itp',
        'ifn', 'n_igt', 'n_itr')
RATIOS = ('MOTA', 'MOTAL', 'MODA', 'recall', 'precision', 'F1', 'FAR', 'MT', 'PT', 'ML')
SUMS = ('total_cost', 'MOTP', 'MODP')
LISTS = ('tps', 'itps', 'fps', 'fns', 'ifns', 'n_gts', 'n_trs', 'n_igts', 'n_itrs')


def golden_cases():
    """[(fixture, evaluation)] of every stored evaluation"""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'clear_mot_*.npz'))):
        with np.load(path) as z:
            out += [(os.path.basename(path)[len('clear_mot_'):-4], e) for e in sorted({k.split('.')[0] for k in z.files})]
    return out


CASES = golden_cases()
_cache = {}


def golden(fixture, ev):
    """(ground-truth Labels, tracker Labels, the reference's record as a dict) of one stored evaluation; loaded once"""
    if (fixture, ev) not in _cache:
        with np.load(os.path.join(GOLDEN, 'clear_mot_%s.npz' % fixture)) as z:
            d = {k[len(ev) + 1:]: z[k] for k in z.files if k.startswith(ev + '.')}
        cls = str(d['cls'])
        lab = lambda s, gt: E.Labels(d[s + '_rows'], d[s + '_n_frames'], d[s + '_length'], d[s + '_n_traj'], cls, gt)
        _cache[(fixture, ev)] = (lab('gt', True), lab('tr', False), d)
    return _cache[(fixture, ev)]


def check_record(get, d, exact_sums):
    """a result (``get(name)``) against a golden record: integers, lists, trajectories and one-division ratios equal;
    the fp64 sums equal (``exact_sums``: the serial restatement) or within 1e-9 relative (another summation order)"""
    for k in INTS:
        assert int(get(k)) == int(d[k]), k
    for k in LISTS:
        assert list(get(k)) == d[k].tolist(), k
    assert np.array_equal(get('traj_key'), d['traj_key'])
    assert np.array_equal(get('gt_tracker'), d['gt_tracker']) and np.array_equal(get('gt_ignored'), d['gt_ignored'])
    for k in RATIOS:
        assert float(get(k)) == float(d[k]), k
    for k in SUMS:
        a, b = float(get(k)), float(d[k])
        assert a == b if (exact_sums or np.isinf(b)) else abs(a - b) <= 1e-9 * abs(b), (k, a, b)
    a, b = np.asarray(get('MODP_t')), d['MODP_t']
    assert a.shape == b.shape
    assert np.array_equal(a, b) if exact_sums else np.all(np.abs(a - b) <= 1e-9 * np.abs(b))


def test_fixtures_cover_the_cases_and_are_small():
    assert {f for f, _ in CASES} == {'kitti_car', 'kitti_ped', 'files', 'edges'}
    paths = glob.glob(os.path.join(GOLDEN, 'clear_mot_*.npz')) + glob.glob(os.path.join(FILES, '**', '*.txt'), recursive=True)
    assert len(paths) >= 8
    for p in paths:
        assert os.path.getsize(p) < 2 ** 20, p
    _, _, d = golden('edges', 'all')
    g = E.pack(*golden('edges', 'all')[:2])
    sizes = {(int(a), int(b)) for a, b in zip(g['g_cnt'], g['t_cnt'])}
    assert {(0, 0), (0, 2), (2, 0), (1, 1), (3, 5), (5, 3), (65, 64), (128, 128)} <= sizes
    assert np.any(d['tr_length'] > d['gt_length'])  # a tracker that runs past its sequence
    assert float(golden('edges', 'nogt')[2]['MOTA']) == -np.inf and float(golden('edges', 'notp')[2]['MOTP']) == np.inf
    assert int(golden('kitti_car', 'car')[2]['itp']) > 0 and int(golden('kitti_car', 'car')[2]['n_itr']) > 0


@pytest.mark.parametrize('cls', ['car', 'pedestrian'])
def test_load_kitti_reproduces_the_stored_tables(cls):
    names, n_frames = E.sequences_of('train', FILES)
    assert names == ['0001', '0013'] and n_frames == [60, 60]
    gt, tr, _ = golden('files', cls)
    for lab, sub, is_gt in ((gt, 'label_02', True), (tr, os.path.join('results', 'golden', 'train'), False)):
        got = E.concat([E.load_kitti(os.path.join(FILES, sub, '%s.txt' % s), cls, n, is_gt) for s, n in zip(names, n_frames)])
        assert np.array_equal(got.rows, lab.rows) and len(got.rows) > 100
        for k in ('n_frames', 'length', 'n_traj'):
            assert np.array_equal(getattr(got, k), getattr(lab, k)), k


def test_labels_from_tracks_equals_load_kitti_of_the_written_file(tmp_path):
    from test_tracks_cpu import kitti_dets
    from tracking_ref import Tracker
    from mmmot_amd.tracks import write_kitti_tracks
    pairs, frames, dets = kitti_dets()
    slot = {f: i for i, f in enumerate(frames)}
    tr = Tracker()
    ids = [np.full(len(d['bbox']), -1, np.int64) for d in dets]
    for p in pairs:
        ids0, ids1, start = tr.pair(p['det'], p['link'], p['new'], p['N'], p['M'], p['f0'], p['f1'])
        if not start:
            ids[slot[p['f0']]] = ids0
        ids[slot[p['f1']]] = ids1
    out = tmp_path / '0001.txt'
    write_kitti_tracks(str(out), dets, ids, frame_idx=frames)
    with open(os.path.join(GOLDEN, 'tracks_kitti_0001.txt'), 'rb') as f:
        assert out.read_bytes() == f.read()
    n = max(frames) + 1
    for cls in ('car', 'pedestrian'):
        a = E.load_kitti(str(out), cls, n, False)
        b = E.labels_from_tracks(dets, ids, frame_idx=frames, cls=cls)
        assert len(a.rows) > 0 and np.array_equal(a.rows, b.rows)
        assert np.array_equal(a.length, b.length) and np.array_equal(a.n_traj, b.n_traj) and int(b.n_frames[0]) == n


@pytest.mark.parametrize('fixture,ev', CASES, ids=['%s-%s' % c for c in CASES])
def test_serial_restatement_reproduces_the_golden_record_exactly(fixture, ev):
    gt, tr, d = golden(fixture, ev)
    r = clear_mot_ref.evaluate(gt, tr)
    check_record(lambda k: r[k], d, exact_sums=True)


def test_refusals(tmp_path):
    row = lambda f, i, box='10 10 50 90': '%d %d Car -1 -1 -10 %s -1 -1 -1 -1000 -1000 -1000 -10 0.9' % (f, i, box)
    p = tmp_path / 'dup.txt'
    p.write_text('\n'.join([row(0, 1), row(1, 1), row(1, 1)]))
    with pytest.raises(ValueError, match='not unique'):
        E.load_kitti(str(p), 'car', 3, False)
    assert len(E.load_kitti(str(p), 'car', 3, True).rows) == 3  # the ground-truth loader does not check
    p.write_text('\n'.join(row(0, i, '%d 10 %d 90' % (i, i + 40)) for i in range(129)))
    many, one = E.load_kitti(str(p), 'car', 1, False), E.load_kitti(str(p), 'car', 1, True)
    one.rows = one.rows[:1]
    with pytest.raises(ValueError, match='more than 128'):
        E.pack(one, many)
    with pytest.raises(ValueError, match='more than 128'):
        E.evaluate_sequences(E.load_kitti(str(p), 'car', 1, True), many, device='meta')  # refused before any device work
    p.write_text('\n'.join(['0 -1 DontCare -1 -1 -10 %d 10 %d 90 -1 -1 -1 -1000 -1000 -1000 -10' % (i, i + 40)
                            for i in range(65)] + [row(0, 0).rsplit(' ', 1)[0]]))
    with pytest.raises(ValueError, match='DontCare'):
        E.pack(E.load_kitti(str(p), 'car', 1, True), one)
    p.write_text('0 -1 Car 0 0 -10 1 1 5 5 -1 -1 -1 -1000 -1000 -1000 -10\n1 3 Truck 0 0 -10 1 1 5 5 -1 -1 -1 -1000 -1000 -1000 -10')
    assert len(E.load_kitti(str(p), 'car', 2, True).rows) == 0  # ID -1 dropped, other classes not loaded
    p.write_text(row(3, 1))
    assert int(E.load_kitti(str(p), 'car', 2, False).length[0]) == 502  # frames beyond n_frames extend the table


def test_meta_kernel_shape_and_layout():
    gt, tr, _ = golden('edges', 'all')
    p = E.pack(gt, tr)
    inp, out, n_in, n_out = clear_mot_layout(p['sizes'])
    nG, nT, nD, NF, NTr, S = p['sizes']
    assert n_in == 8 * (nG + nT + nD) + 6 * NF + 3 * nG + 2 * nT + NTr + 1 + nG + 2 * (S + 1)
    assert n_out == 4 * NF + 4 * (S + 1) + 6 * NF + 2 * nG + 4 * NTr + 12 * (S + 1)
    assert inp['boxes'][0] == 0 and out['frame_d'][0] == 0 and out['seq_d'][0] % 2 == 0
    res = torch.ops.mmmot.clear_mot(torch.empty(n_in, dtype=torch.int32, device='meta'), p['sizes'], [0.5, 25., 0., 2.])
    assert res.shape == (n_out,) and res.dtype == torch.int32 and res.device.type == 'meta'
    with pytest.raises(ValueError):
        clear_mot_layout([1, 1, 0, 1, 1, 0])
    with pytest.raises(NotImplementedError):  # no CPU kernel, no fallback
        torch.ops.mmmot.clear_mot(torch.zeros(n_in, dtype=torch.int32), p['sizes'], [0.5, 25., 0., 2.])


def test_library_exports_clear_mot_and_header_declares_it():
    from mmmot_amd import _lib
    path = _lib.build()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', path]).decode()
    assert re.search(r'\bT mmmot_clear_mot\b', syms)
    with open(os.path.join(ROOT, 'include', 'mmmot_hip.h')) as f:
        assert re.search(r'\bint mmmot_clear_mot\(const double\* boxes, int nG,', f.read())
    assert len(_lib.SIGNATURES['mmmot_clear_mot']) == 24 and 'clear_mot.hip' in _lib.SOURCES
    lib = _lib.load()
    assert lib.mmmot_clear_mot(None, 0, 0, 0, None, 0, None, None, None, None, 0, None, 0, 0.5, 25., 0., 2., None, None, None,
                               None, None, None, None) == -1  # S < 1: refused before any launch
