"""Generate tests/golden/clear_mot_*.npz and tests/golden/clear_mot_files/ with the REFERENCE's evaluator:

    python tools/gen_golden_clear_mot.py --reference /path/to/mmMOT

imports kitti_devkit.evaluate_tracking.trackingEvaluation from the reference checkout (nothing of it is copied), runs it
on ground-truth and tracker files written here, and stores tables and results as data: per evaluation ``<name>.*`` the
label rows of both sides (mmmot_amd.evaluate.Labels: sequence, frame, ID, class code, truncation, occlusion, box),
everything compute3rdPartyMetrics left on the object, MODP_t, per ground-truth trajectory (sorted by sequence and track
ID) the matched tracker IDs and ignored flags, and the text of stats_<cls>.txt.

Fixtures: kitti_car / kitti_ped - 60-frame excerpts of KITTI training sequences 0001 and 0013, the tracker = the ground
truth with seeded box jitter, dropped boxes, ID changes and added false boxes; files - both excerpts in one call, the
label and result files themselves under tests/golden/clear_mot_files/ (the drop-in's input); edges - synthetic
sequences (empty sides, wave boundary, the frame limit, ignore thresholds, trajectory corner cases, infinite totals).

Per frame the reference's association is asserted equal to scipy's linear_sum_assignment on the same gated matrix: the
fixtures hold no tie between equal-cost matchings.  A fixture that fails is regenerated with another --seed."""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mmmot_amd.evaluate import concat, load_kitti  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SCALARS = ('MOTA', 'MOTP', 'MOTAL', 'MODA', 'MODP', 'recall', 'precision', 'F1', 'FAR', 'MT', 'PT', 'ML', 'tp', 'fp', 'fn',
           'id_switches', 'fragments', 'n_gt', 'n_gt_trajectories', 'n_tr', 'n_tr_trajectories', 'itp', 'ifn', 'n_igt',
           'n_itr', 'total_cost')
LISTS = ('tps', 'itps', 'fps', 'fns', 'ifns', 'n_gts', 'n_trs', 'n_igts', 'n_itrs')


def line(frame, tid, name, trunc, occ, box, score=None):
    f = [str(frame), str(tid), name, str(trunc), str(occ), '-10'] + ['%.6f' % v for v in box] + \
        ['-1', '-1', '-1', '-1000', '-1000', '-1000', '-10']
    return ' '.join(f + ([] if score is None else ['%.4f' % score]))


def excerpt(path, start, n):
    """rows of frames [start, start + n) of a label file, frames renumbered from 0: (frame, id, name, trunc, occ, box)"""
    rows = []
    with open(path) as f:
        for ln in f:
            p = ln.split()
            if start <= int(p[0]) < start + n:
                rows.append((int(p[0]) - start, int(p[1]), p[2], int(p[3]), int(p[4]), [float(v) for v in p[6:10]]))
    return rows


def best_window(path, n, wanted):
    """start frame of the n-frame window that holds the most of its rarest wanted kind of row"""
    with open(path) as f:
        rows = [ln.split() for ln in f]
    last = max(int(p[0]) for p in rows)
    kinds = [np.zeros(last + 1) for _ in wanted]
    for p in rows:
        for k, w in zip(kinds, wanted):
            k[int(p[0])] += w(p)
    score = [min(k[s:s + n].sum() for k in kinds) for s in range(max(1, last + 2 - n))]
    return int(np.argmax(score))


def jitter_tracker(rows, rng, names, jitter=8.0, drop=0.10, swap=0.05, extra=0.05):
    """a tracker from ground-truth rows: jittered boxes, dropped boxes, changed IDs, added false boxes"""
    out, remap, next_id = [], {}, 1000
    for frame, tid, name, trunc, occ, box in rows:
        if name == 'DontCare' or name not in names or rng.random() < drop:
            continue
        if rng.random() < swap:
            remap[tid] = next_id
            next_id += 1
        b = np.asarray(box) + rng.uniform(-jitter, jitter, 4)
        out.append((frame, remap.get(tid, tid), name, -1, -1, b.tolist()))
        if rng.random() < extra:
            x, y = rng.uniform(0, 1100), rng.uniform(100, 300)
            out.append((frame, next_id, name, -1, -1, [x, y, x + rng.uniform(20, 120), y + rng.uniform(15, 90)]))
            next_id += 1
    return out


def write_rows(path, rows, score=None):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write('\n'.join(line(*r, score=score) for r in rows) + ('\n' if rows else ''))


def run_reference(ET, work, names, n_frames, cls, part='all'):
    """the reference's evaluator over work/gt/label_02 and work/res/golden/<part>; returns it after saveToStats"""
    e = ET.trackingEvaluation(t_sha='golden', root=os.path.join(work, 'res'), part=part,
                              gt_path=os.path.join(work, 'gt'), mail=ET.mailpy.Mail(''), cls=cls)
    e.sequence_name, e.n_frames, e.n_sequences = list(names), list(n_frames), len(names)
    e.gt_trajectories = [[] for _ in names]
    e.ign_trajectories = [[] for _ in names]
    if not e.loadTracker():
        return None
    assert e.loadGroundtruth()
    assert e.compute3rdPartyMetrics()
    for s in range(len(names)):  # no ties: the association equals linear_sum_assignment's on the same gated matrix
        for f in range(len(e.groundtruth[s])):
            g, t = e.groundtruth[s][f], e.tracker[s][f]
            if not g or not t:
                continue
            c = np.array([[1 - e.boxoverlap(gg, tt) for tt in t] for gg in g])
            m = np.where(c <= e.min_overlap, c, 1e9)
            want = [-1] * len(g)
            for i, j in zip(*linear_sum_assignment(m)):
                if m[i, j] < 1e9:
                    want[i] = t[j].track_id
            assert want == [gg.tracker for gg in g], 'tie or disagreement in sequence %s frame %d' % (names[s], f)
    e.createEvalDir()
    e.saveToStats()
    return e


def record(e, names, n_frames, work, cls, part='all'):
    gt = concat([load_kitti(os.path.join(work, 'gt', 'label_02', '%s.txt' % s), cls, n, True)
                 for s, n in zip(names, n_frames)])
    tr = concat([load_kitti(os.path.join(work, 'res', 'golden', part, '%s.txt' % s), cls, n, False)
                 for s, n in zip(names, n_frames)])
    d = {'cls': np.array(cls), 'names': np.array(names)}
    for side, lb in (('gt', gt), ('tr', tr)):
        d[side + '_rows'], d[side + '_n_frames'], d[side + '_length'], d[side + '_n_traj'] = \
            lb.rows, lb.n_frames, lb.length, lb.n_traj
    for k in SCALARS:
        d[k] = np.array(getattr(e, k), np.float64)
    for k in LISTS:
        d[k] = np.array(getattr(e, k), np.int64)
    d['MODP_t'] = np.array(e.MODP_t, np.float64)
    flat_g, flat_i, keys = [], [], []
    for s in range(len(names)):
        for tid in sorted(e.gt_trajectories[s]):
            flat_g += e.gt_trajectories[s][tid]
            flat_i += e.ign_trajectories[s][tid]
            keys.append((s, tid, len(e.gt_trajectories[s][tid])))
    d['gt_tracker'], d['gt_ignored'] = np.array(flat_g, np.int64), np.array(flat_i, bool)
    d['traj_key'] = np.array(keys, np.int64).reshape(-1, 3)
    with open(os.path.join(e.eval_dir, 'stats_%s.txt' % cls)) as f:
        d['stats_txt'] = np.array(f.read())
    return d


def fixture(ET, out, evals):
    """evals: {name: (files {sequence: (gt rows, tracker rows, n_frames)}, cls)} -> one npz"""
    data = {}
    for name, (files, cls) in evals.items():
        work = tempfile.mkdtemp()
        try:
            names = sorted(files)
            for s in names:
                write_rows(os.path.join(work, 'gt', 'label_02', '%s.txt' % s), files[s][0])
                write_rows(os.path.join(work, 'res', 'golden', 'all', '%s.txt' % s), files[s][1], score=0.9)
            n_frames = [files[s][2] for s in names]
            e = run_reference(ET, work, names, n_frames, cls)
            if e is None:  # the tracker holds no trajectory of the class: the devkit skips it, and so does the fixture
                print('%s: no %s in the tracker, skipped' % (name, cls))
                continue
            for k, v in record(e, names, n_frames, work, cls).items():
                data['%s.%s' % (name, k)] = v
        finally:
            shutil.rmtree(work)
    np.savez_compressed(out, **data)
    assert os.path.getsize(out) < 2 ** 20, out
    print(out, os.path.getsize(out), 'bytes')


def edge_sequences(rng):
    """synthetic sequences: {name: (gt rows, tracker rows, n_frames)}"""
    def boxes(n, span=4000.0):
        x, y = rng.uniform(0, span, n), rng.uniform(0, span, n)
        return np.stack([x, y, x + rng.uniform(40, 200, n), y + rng.uniform(40, 200, n)], axis=1)

    def jit(b, j=6.0):
        return b + rng.uniform(-j, j, b.shape)

    seqs = {}
    # 0000: empty sides, 1 x 1, 3 x 5 and 5 x 3
    g, t = [], []
    b = boxes(2); t += [(1, 10 + k, 'Car', -1, -1, b[k].tolist()) for k in range(2)]
    b = boxes(2); g += [(2, k, 'Car', 0, 0, b[k].tolist()) for k in range(2)]
    b = boxes(1); g += [(3, 0, 'Car', 0, 0, b[0].tolist())]; t += [(3, 10, 'Car', -1, -1, jit(b)[0].tolist())]
    b = boxes(5); tb = jit(b)
    g += [(4, k, 'Car', 0, 0, b[k].tolist()) for k in range(3)]
    t += [(4, 10 + k, 'Car', -1, -1, tb[k].tolist()) for k in (3, 1, 4, 0, 2)]
    b = boxes(5); tb = jit(b)
    g += [(5, k, 'Car', 0, 0, b[k].tolist()) for k in range(5)]
    t += [(5, 10 + k, 'Car', -1, -1, tb[k].tolist()) for k in (4, 0, 2)]
    seqs['0000'] = (g, t, 6)
    # 0001: 65 x 64, 128 x 128 (crowded: many valid cells per row), no valid cell
    g, t = [], []
    b = boxes(65, 900.0); tb = jit(b, 15.0); p = rng.permutation(64)
    g += [(0, k, 'Car', 0, 0, b[k].tolist()) for k in range(65)]
    t += [(0, 200 + int(k), 'Car', -1, -1, tb[k].tolist()) for k in p]
    b = boxes(128, 1200.0); tb = jit(b, 15.0); p = rng.permutation(128)
    g += [(1, k, 'Car', 0, 0, b[k].tolist()) for k in range(128)]
    t += [(1, 200 + int(k), 'Car', -1, -1, tb[k].tolist()) for k in p]
    b = boxes(3)
    g += [(2, k, 'Car', 0, 0, b[k].tolist()) for k in range(3)]
    t += [(2, 200 + k, 'Car', -1, -1, (b[k] + 500).tolist()) for k in range(3)]
    seqs['0002'] = (g, t, 3)
    # 0003: the ignore thresholds
    g, t = [], []
    for f in range(3):
        g += [(f, -1, 'DontCare', -1, -1, [100, 100, 150, 200]), (f, -1, 'DontCare', -1, -1, [300, 100, 350.01, 200]),
              (f, 0, 'Car', 0, 0, [500, 100, 600, 180]), (f, 1, 'Car', 1, 0, [700, 100, 800, 180]),
              (f, 2, 'Car', 0, 3, [900, 100, 1000, 180]), (f, 3, 'Van', 0, 0, [1100, 100, 1200, 180]),
              (f, 4, 'Car', 1, 0, [500, 250, 600, 330]), (f, 5, 'Van', 0, 0, [700, 250, 800, 330])]
        t += [(f, 20, 'Car', -1, -1, [100, 100, 200, 200]),       # DontCare coverage exactly 0.5: a false positive
              (f, 21, 'Car', -1, -1, [300, 100, 400, 200]),       # just above: ignored
              (f, 22, 'Car', -1, -1, [10, 100, 60, 125]),         # height exactly 25: ignored
              (f, 23, 'Car', -1, -1, [10, 200, 60, 225.5]),       # above: a false positive
              (f, 24, 'Van', -1, -1, [10, 300, 90, 360]),         # unmatched van: ignored
              (f, 25, 'Car', -1, -1, jit(np.array([[500., 100, 600, 180]]), 3)[0].tolist()),
              (f, 26, 'Car', -1, -1, jit(np.array([[700., 100, 800, 180]]), 3)[0].tolist()),   # truncated GT: ignored TP
              (f, 27, 'Car', -1, -1, jit(np.array([[900., 100, 1000, 180]]), 3)[0].tolist()),  # occluded GT
              (f, 28, 'Van', -1, -1, jit(np.array([[1100., 100, 1200, 180]]), 3)[0].tolist()),  # van on van
              (f, 29, 'Car', -1, -1, [640, 120, 680, 140])]       # height 20 but it matches nothing: ignored
    seqs['0003'] = (g, t, 3)
    # 0004: trajectories - ignored in every frame, one object, ID switches, fragments, gaps, a switch in the last frame
    g, t = [], []
    plan = {0: [50, 50, 51, 51, -1, 51, 52, 52],      # switches and a gap
            1: [60, -1, -1, 60, 60, -1, 61, 60],      # fragments
            2: [-1, -1, -1, -1, -1, -1, -1, 70],      # mostly lost
            3: [80, 80, 80, 80, 80, 80, 80, 81]}      # a switch in the last frame
    for f in range(8):
        for k, ids in plan.items():
            bx = np.array([[100. + 250 * k + 5 * f, 100, 200 + 250 * k + 5 * f, 190]])
            g.append((f, k, 'Car', 0, 0, bx[0].tolist()))
            if ids[f] >= 0:
                t.append((f, ids[f], 'Car', -1, -1, jit(bx, 4)[0].tolist()))
        bx = np.array([[100. + 5 * f, 250, 200 + 5 * f, 340]])
        g.append((f, 9, 'Car', 2, 0, bx[0].tolist()))  # truncated in every frame
        if f % 2:
            t.append((f, 90, 'Car', -1, -1, jit(bx, 4)[0].tolist()))
    g.append((5, 7, 'Car', 0, 0, [900, 250, 1000, 340]))  # a trajectory of one object
    t.append((5, 97, 'Car', -1, -1, [902, 251, 1001, 342]))
    seqs['0004'] = (g, t, 8)
    # 0005: the tracker runs past the sequence
    g = [(f, 0, 'Car', 0, 0, [100. + f, 100, 220 + f, 200]) for f in range(3)]
    t = [(f, 5, 'Car', -1, -1, [103. + f, 98, 221 + f, 203]) for f in range(3)] + \
        [(f, 6, 'Car', -1, -1, [100., 100, 220, 200]) for f in (5, 7)]
    seqs['0005'] = (g, t, 3)
    # 0006: pedestrians with the neighbouring class
    g, t = [], []
    for f in range(4):
        g += [(f, 0, 'Pedestrian', 0, 0, [100. + 3 * f, 100, 140 + 3 * f, 200]),
              (f, 1, 'Person_sitting', 0, 0, [300, 100, 350, 170]), (f, 2, 'Pedestrian', 0, 1, [500, 100, 540, 210]),
              (f, -1, 'DontCare', -1, -1, [700, 100, 900, 300])]
        t += [(f, 40, 'Pedestrian', -1, -1, [102. + 3 * f, 101, 141 + 3 * f, 203]),
              (f, 41, 'Person_sitting', -1, -1, [301, 102, 349, 171]), (f, 42, 'Person_sitting', -1, -1, [10, 10, 60, 90]),
              (f, 43, 'Pedestrian', -1, -1, [720, 120, 760, 220])]
        if f != 2:
            t.append((f, 44 + (f == 3), 'Pedestrian', -1, -1, [501, 99, 542, 212]))
    seqs['0006'] = (g, t, 4)
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference (its kitti_devkit and data/tracking)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--frames', type=int, default=60)
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    sys.path[:0] = [ref, os.path.join(ref, 'kitti_devkit')]  # kitti_devkit.mailpy, and munkres as the devkit imports it
    os.chdir(ref)  # the evaluator's constructor opens ./data/tracking/evaluate_tracking.seqmap
    import kitti_devkit.evaluate_tracking as ET
    rng = np.random.default_rng(a.seed)
    labels = os.path.join(ref, 'data', 'tracking', 'label_02')
    n = a.frames

    car = os.path.join(labels, '0001.txt')
    s0 = best_window(car, n, [lambda p: p[2] == 'Van', lambda p: p[2] == 'DontCare',
                              lambda p: p[2] == 'Car' and int(p[4]) > 2, lambda p: p[2] == 'Car' and int(p[3]) > 0])
    ped = os.path.join(labels, '0013.txt')
    s1 = best_window(ped, n, [lambda p: p[2] == 'Pedestrian', lambda p: p[2] == 'DontCare',
                              lambda p: p[2] == 'Pedestrian' and int(p[3]) > 0, lambda p: p[2] == 'Person'])
    print('excerpts: 0001 from frame %d, 0013 from frame %d' % (s0, s1))
    names = ('Car', 'Van', 'Pedestrian', 'Person_sitting', 'Person')
    g1 = excerpt(car, s0, n)
    g13 = excerpt(ped, s1, n)
    f1 = (g1, jitter_tracker(g1, rng, names), n)
    f13 = (g13, jitter_tracker(g13, rng, names), n)
    fixture(ET, os.path.join(GOLDEN, 'clear_mot_kitti_car.npz'), {'car': ({'0001': f1}, 'car'),
                                                                 'pedestrian': ({'0001': f1}, 'pedestrian')})
    fixture(ET, os.path.join(GOLDEN, 'clear_mot_kitti_ped.npz'), {'car': ({'0013': f13}, 'car'),
                                                                 'pedestrian': ({'0013': f13}, 'pedestrian')})
    both = {'0001': f1, '0013': f13}
    fixture(ET, os.path.join(GOLDEN, 'clear_mot_files.npz'), {'car': (both, 'car'), 'pedestrian': (both, 'pedestrian')})
    files = os.path.join(GOLDEN, 'clear_mot_files')
    shutil.rmtree(files, ignore_errors=True)
    for s, (g, t, _) in both.items():
        write_rows(os.path.join(files, 'label_02', '%s.txt' % s), g)
        write_rows(os.path.join(files, 'results', 'golden', 'train', '%s.txt' % s), t, score=0.9)
    with open(os.path.join(files, 'evaluate_tracking.seqmap'), 'w') as f:
        f.write(''.join('%s empty %06d %06d\n' % (s, 0, n - 1) for s in sorted(both)))

    edges = edge_sequences(rng)
    nogt = {'0000': ([(0, -1, 'DontCare', -1, -1, [100, 100, 300, 300])],
                     [(0, 1, 'Car', -1, -1, [500, 100, 600, 200]), (1, 1, 'Car', -1, -1, [505, 100, 605, 200])], 2)}
    notp = {'0000': ([(0, 0, 'Car', 0, 0, [100, 100, 200, 200]), (1, 0, 'Car', 0, 0, [105, 100, 205, 200])],
                     [(0, 1, 'Car', -1, -1, [500, 100, 600, 200]), (1, 1, 'Car', -1, -1, [505, 100, 605, 200])], 2)}
    fixture(ET, os.path.join(GOLDEN, 'clear_mot_edges.npz'),
            {'all': (edges, 'car'), 'pedestrian': ({'0006': edges['0006']}, 'pedestrian'), 'nogt': (nogt, 'car'),
             'notp': (notp, 'car')})


if __name__ == '__main__':
    main()
