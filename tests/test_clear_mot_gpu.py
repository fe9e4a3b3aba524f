"""CLEAR-MOT evaluation on the device (csrc/clear_mot.hip through mmmot::clear_mot / mmmot_amd.evaluate) against the
records the reference's evaluator produced (tests/golden/clear_mot_*.npz) and, for random instances, against the serial
restatement tests/clear_mot_ref.py.

Equal: every integer statistic, every per-sequence list, the MT / PT / ML counts, per trajectory the matched tracker
IDs and ignored flags, and the ratios that are one division of equal integers (bitwise).  total_cost, MOTP, MODP and
each MODP_t: within 1e-9 relative - sums of fewer than 1e5 fp64 terms in [0.5, 1] taken in another order than the
reference's running sum; reordering is bounded by n * 2^-53 ~ 1e-11, so the tolerance leaves two decades."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clear_mot_ref
import hota_cases
from test_clear_mot_cpu import CASES, FILES, GOLDEN, ROOT, check_record, golden
from mmmot_amd import evaluate as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fixture,ev', CASES, ids=['%s-%s' % c for c in CASES])
def test_golden_records(fixture, ev):
    gt, tr, d = golden(fixture, ev)
    m = E.evaluate_sequences(gt, tr, cls=str(d['cls']))
    check_record(lambda k: getattr(m, k), d, exact_sums=False)
    assert m.stats_line() + '\n' == str(d['stats_txt'])  # six decimals: far above the tolerance of the sums


def split_sequences(lab):
    out = []
    for s in range(lab.n_sequences):
        rows = lab.rows[lab.rows[:, E.SEQ] == s].copy()
        rows[:, E.SEQ] = 0
        out.append(E.Labels(rows, lab.n_frames[s:s + 1], lab.length[s:s + 1], lab.n_traj[s:s + 1], lab.cls, lab.ground_truth))
    return out


def test_batch_invariance_of_the_per_sequence_values():
    gt, tr, _ = golden('edges', 'all')
    whole = E.evaluate_sequences(gt, tr)
    per = ('tps', 'itps', 'fps', 'fns', 'ifns', 'n_gts', 'n_trs', 'n_igts', 'n_itrs', 'seq_costs', 'seq_modp',
           'seq_id_switches', 'seq_fragments')
    fo = np.concatenate([[0], np.cumsum(gt.length)])
    assert gt.n_sequences >= 6
    for s, (g1, t1) in enumerate(zip(split_sequences(gt), split_sequences(tr))):
        one = E.evaluate_sequences(g1, t1)
        for k in per:
            a, b = getattr(one, k)[0], getattr(whole, k)[s]
            assert a == b and type(a) is type(b), (s, k, a, b)  # fp64 sums included: bitwise
        assert np.array_equal(one.MODP_t, whole.MODP_t[fo[s]:fo[s + 1]])
        sel = whole.traj_key[:, 0] == s
        assert np.array_equal(one.traj_key[:, 1:], whole.traj_key[sel][:, 1:])


def random_labels(rng, sizes, span):
    """one sequence with len(sizes) frames of (G, T) boxes: the tracker = jittered ground truth in shuffled order plus
    false boxes, with vans, truncated / occluded objects, DontCare areas and small boxes mixed in"""
    g, t = [], []
    for f, (G, T) in enumerate(sizes):
        n = max(G, T)
        x, y = rng.uniform(0, span, n), rng.uniform(0, span, n)
        b = np.stack([x, y, x + rng.uniform(20, 160, n), y + rng.uniform(15, 120, n)], axis=1)
        for k in range(G):
            g.append([0, f, int(rng.integers(0, 24)) if G <= 24 else k, rng.random() < 0.15, int(rng.integers(0, 3) * (rng.random() < 0.3)),
                      int(rng.integers(0, 4)), *b[k]])
        ids = rng.permutation(200)[:T] if T <= 24 else rng.permutation(T)
        for j, k in enumerate(rng.permutation(n)[:T]):
            bb = b[k] + rng.uniform(-12, 12, 4) if rng.random() < 0.8 else b[k] + rng.uniform(-60, 60, 4)
            t.append([0, f, int(ids[j]), rng.random() < 0.15, -1, -1, *bb])
        for _ in range(int(rng.integers(0, 3))):
            x, y = rng.uniform(0, span, 2)
            g.append([0, f, -1, E.DONTCARE, -1, -1, x, y, x + rng.uniform(50, 300), y + rng.uniform(50, 300)])
    # a ground-truth ID may repeat within a frame (the loader does not refuse it there); the tracker's are unique
    mk = lambda rows, gt_side: E.Labels(np.asarray(rows, np.float64).reshape(-1, 10), np.array([len(sizes)]),
                                        np.array([len(sizes)]),
                                        np.array([len({r[2] for r in rows if r[3] != E.DONTCARE})]), 'car', gt_side)
    return mk(g, True), mk(t, False)


@pytest.fixture(scope='module')
def random_cases():
    """200 frames with G, T in [0, 16] and a dozen at 64 / 65 / 128, with the serial restatement's answer (computed once)"""
    rng = np.random.default_rng(20240)
    small = [(int(a), int(b)) for a, b in rng.integers(0, 17, (200, 2))]
    big = [(64, 64), (65, 64), (64, 65), (65, 65), (128, 128), (128, 64), (64, 128), (128, 127), (127, 128), (65, 128),
           (128, 65), (128, 128)]
    cases = []
    for sizes, span in ((small[:100], 500.0), (small[100:], 250.0), (big[:6], 1500.0), (big[6:], 1000.0)):
        gt, tr = random_labels(rng, sizes, span)
        cases.append((gt, tr, clear_mot_ref.evaluate(gt, tr)))
    return cases


def test_random_instances_equal_the_serial_restatement(random_cases):
    frames = 0
    for gt, tr, want in random_cases:
        m = E.evaluate_sequences(gt, tr)
        check_record(lambda k: getattr(m, k), {k: np.asarray(v) for k, v in want.items()}, exact_sums=False)
        frames += len(m.MODP_t)
        assert m.tp > 0 and m.fp > 0 and m.fn > 0
    assert frames == 212
    # all of them as ONE call of four sequences: the same per-sequence numbers
    whole = E.evaluate_sequences([c[0] for c in random_cases], [c[1] for c in random_cases])
    assert whole.tps == [c[2]['tps'][0] for c in random_cases] and whole.fps == [c[2]['fps'][0] for c in random_cases]
    assert whole.id_switches == sum(c[2]['id_switches'] for c in random_cases)


def test_transposed_rows_equal_columns_and_an_empty_side():
    """hota_cases.twin_sequence (70 x 3, 3 x 70 with the same tracker box in two columns, 0 x 2) against the serial
    restatement; of the two equal columns the device takes the smaller one, the restatement either"""
    gt, tr = hota_cases.twin_sequence(np.random.default_rng(600))
    want = {k: np.asarray(v) for k, v in clear_mot_ref.evaluate(gt, tr).items()}
    twin = np.isin(want['gt_tracker'], hota_cases.TWIN_IDS)
    assert twin.sum() == 1
    want['gt_tracker'] = np.where(twin, hota_cases.TWIN_IDS[0], want['gt_tracker'])
    m = E.evaluate_sequences(gt, tr)
    check_record(lambda k: getattr(m, k), want, exact_sums=False)
    assert (m.tp, m.fp, m.fn) == (6, 69, 67)


def test_drop_in_returns_the_golden_tuple_and_writes_the_stats_file(tmp_path):
    shutil.copytree(os.path.join(FILES, 'results'), str(tmp_path / 'res'))
    got = E.evaluate('golden', str(tmp_path / 'res'), 'train', gt_path=FILES)
    _, _, d = golden('files', 'pedestrian')  # the last class evaluated
    want = [d[k] for k in ('MOTA', 'MOTP', 'recall', 'precision', 'F1', 'fp', 'fn', 'id_switches')]
    assert len(got) == 8
    for k, (a, b) in enumerate(zip(got, want)):
        assert (abs(a - float(b)) <= 1e-9 * abs(float(b))) if k == 1 else a == float(b), (k, a, b)
    for cls in ('car', 'pedestrian'):
        with open(str(tmp_path / 'res' / 'golden' / 'train' / 'eval' / cls / ('stats_%s.txt' % cls))) as f:
            assert f.read() == str(golden('files', cls)[2]['stats_txt'])
    only = E.evaluate('golden', str(tmp_path / 'res'), 'train', gt_path=FILES, cls='car')
    assert only[5] == int(golden('files', 'car')[2]['fp'])


def test_pipeline_tracks_against_themselves():
    """labels_from_tracks of the track_ids_kitti fixture's detections and IDs, evaluated against itself"""
    from test_tracks_cpu import kitti_dets
    from tracking_ref import Tracker
    pairs, frames, dets = kitti_dets()
    slot = {f: i for i, f in enumerate(frames)}
    tr = Tracker()
    ids = [np.full(len(d['bbox']), -1, np.int64) for d in dets]
    for p in pairs:
        ids0, ids1, start = tr.pair(p['det'], p['link'], p['new'], p['N'], p['M'], p['f0'], p['f1'])
        if not start:
            ids[slot[p['f0']]] = ids0
        ids[slot[p['f1']]] = ids1
    for d in dets:  # as ground truth every object counts: nothing truncated or occluded away
        d['truncated'] = np.zeros(len(d['bbox']))
        d['occluded'] = np.zeros(len(d['bbox']), np.int64)
    for cls in ('car', 'pedestrian'):
        gt = E.labels_from_tracks(dets, ids, frame_idx=frames, cls=cls, ground_truth=True)
        tk = E.labels_from_tracks(dets, ids, frame_idx=frames, cls=cls)
        m = E.evaluate_sequences(gt, tk, cls=cls, min_height=0)
        main = int(np.sum(gt.rows[:, E.CLS] == E.MAIN))
        assert main > 0 and m.n_gt == main and m.tp == len(gt.rows)
        assert m.MOTA == 1.0 and m.MOTP == 1.0 and m.fp == 0 and m.fn == 0 and m.id_switches == 0 and m.fragments == 0


def test_library_resolves_the_new_symbol():
    from mmmot_amd import _lib
    syms = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert re.search(r'\bT mmmot_clear_mot\b', syms)
    assert _lib.load().mmmot_clear_mot.argtypes == _lib.SIGNATURES['mmmot_clear_mot']
