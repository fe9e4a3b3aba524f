"""3D MOT evaluation, host side: the restatement tests/mot3d_ref.py against closed forms and an independent area
computation, the labels with 3D boxes and scores through the file and the file-less route, the sweep arithmetic, the
generator's conditions, the refusals and the operator's Meta kernel.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import clear_mot_ref
import mot3d_cases
import mot3d_ref as R
from mmmot_amd import evaluate as E
from mmmot_amd.torch_ops import mot3d_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def box(x=0., z=10., ry=0., h=1.5, w=2., l=4., y=1.6):
    return [h, w, l, x, y, z, ry, 0.]


def test_closed_forms():
    # axis-aligned boxes against the min / max formula
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, b = box(rng.uniform(-3, 3), rng.uniform(8, 12), 0., *rng.uniform(1, 3, 3), rng.uniform(1, 2)), \
            box(rng.uniform(-3, 3), rng.uniform(8, 12), 0., *rng.uniform(1, 3, 3), rng.uniform(1, 2))
        ox = max(0., min(a[3] + a[2] / 2, b[3] + b[2] / 2) - max(a[3] - a[2] / 2, b[3] - b[2] / 2))
        oz = max(0., min(a[5] + a[1] / 2, b[5] + b[1] / 2) - max(a[5] - a[1] / 2, b[5] - b[1] / 2))
        oy = max(0., min(a[4], b[4]) - max(a[4] - a[0], b[4] - b[0]))
        A, I = ox * oz, ox * oz * oy
        assert abs(R.iou_boxes(a, b, True) - A / (a[1] * a[2] + b[1] * b[2] - A)) <= 1e-12
        assert abs(R.iou_boxes(a, b) - I / (a[0] * a[1] * a[2] + b[0] * b[1] * b[2] - I)) <= 1e-12
    # identical boxes, at any heading
    for ry in (0., 0.3, math.pi / 2, math.pi, -math.pi, 2.5):
        assert abs(R.iou_boxes(box(ry=ry), box(ry=ry)) - 1.) <= 1e-12 and abs(R.iou_boxes(box(ry=ry), box(ry=ry), True) - 1.) <= 1e-12
    # a box against itself turned by pi is itself; by pi / 2 with w = l too
    assert abs(R.iou_boxes(box(ry=0.4), box(ry=0.4 + math.pi)) - 1.) <= 1e-12
    assert abs(R.iou_boxes(box(ry=0.4, w=3., l=3.), box(ry=0.4 + math.pi / 2, w=3., l=3.)) - 1.) <= 1e-12
    # disjoint and height-disjoint
    assert R.iou_boxes(box(0.), box(30.)) == 0. and R.iou_boxes(box(0.), box(30.), True) == 0.
    assert R.iou_boxes(box(y=1.6), box(y=-2.)) == 0. and abs(R.iou_boxes(box(y=1.6), box(y=-2.), True) - 1.) <= 1e-12
    # containment: the small box inside the large one, turned
    small, large = box(0.2, 10.1, 0.7, h=1., w=1., l=1.5, y=1.5), box(0., 10., 0.2, h=2., w=4., l=6., y=1.8)
    assert abs(R.iou_boxes(small, large, True) - 1.5 / 24.) <= 1e-12 and abs(R.iou_boxes(large, small, True) - 1.5 / 24.) <= 1e-12
    assert abs(R.iou_boxes(small, large) - 1.5 / 48.) <= 1e-12
    # the unit square against itself turned by 45 degrees: the regular octagon, A = 2 (sqrt 2 - 1)
    sq, sq45 = R.footprints([box(0., 0., 0., 1., 1., 1.)])[0], R.footprints([box(0., 0., math.pi / 4, 1., 1., 1.)])[0]
    assert abs(R.clip_area(sq, sq45) - 2 * (math.sqrt(2.) - 1.)) <= 1e-12 and len(R.clip(sq, sq45)) == 8
    assert abs(R.clip_area(sq45, sq) - 2 * (math.sqrt(2.) - 1.)) <= 1e-12


def random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        a = box(rng.uniform(-2, 2), rng.uniform(8, 12), rng.uniform(-math.pi, math.pi), *rng.uniform(1, 4, 3), rng.uniform(1, 2))
        b = box(rng.uniform(-2, 2), rng.uniform(8, 12), rng.uniform(-math.pi, math.pi), *rng.uniform(1, 4, 3), rng.uniform(1, 2))
        out.append((a, b))
    return out


def test_symmetry_and_invariance_under_a_common_motion():
    hit = 0
    for n, (a, b) in enumerate(random_pairs(100, 5)):
        v3, vb = R.iou_boxes(a, b), R.iou_boxes(a, b, True)
        hit += v3 > 0
        assert abs(R.iou_boxes(b, a) - v3) <= 1e-12 and abs(R.iou_boxes(b, a, True) - vb) <= 1e-12
        th, dx, dz = 0.37 * n, 3.0 - n, 0.5 * n
        moved = []
        for q in (a, b):  # rotate the scene by th about the y axis, then translate
            c, s = math.cos(th), math.sin(th)
            m = list(q)
            m[3], m[5], m[6] = c * q[3] + s * q[5] + dx, -s * q[3] + c * q[5] + dz, q[6] + th
            moved.append(m)
        assert abs(R.iou_boxes(*moved) - v3) <= 1e-9 and abs(R.iou_boxes(*moved, True) - vb) <= 1e-9
    assert hit > 50


def test_area_against_the_convex_hull_of_inside_vertices_and_edge_crossings():
    from scipy.spatial import ConvexHull

    def inside(p, poly):  # poly runs clockwise in (x, z): inside is to the right of every edge
        return all((poly[(e + 1) % 4][0] - poly[e][0]) * (p[1] - poly[e][1]) -
                   (poly[(e + 1) % 4][1] - poly[e][1]) * (p[0] - poly[e][0]) <= 0 for e in range(4))

    def crossing(p, q, r, s):
        d = (q[0] - p[0]) * (s[1] - r[1]) - (q[1] - p[1]) * (s[0] - r[0])
        if d == 0:
            return None
        t = ((r[0] - p[0]) * (s[1] - r[1]) - (r[1] - p[1]) * (s[0] - r[0])) / d
        u = ((r[0] - p[0]) * (q[1] - p[1]) - (r[1] - p[1]) * (q[0] - p[0])) / d
        return (p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])) if 0 <= t <= 1 and 0 <= u <= 1 else None

    hit = 0
    for a, b in random_pairs(200, 9):
        fa, fb = R.footprints([a])[0], R.footprints([b])[0]
        pa, pb = [(fa[2 * k], fa[2 * k + 1]) for k in range(4)], [(fb[2 * k], fb[2 * k + 1]) for k in range(4)]
        pts = [p for p in pa if inside(p, pb)] + [p for p in pb if inside(p, pa)]
        for i in range(4):
            for j in range(4):
                x = crossing(pa[i], pa[(i + 1) % 4], pb[j], pb[(j + 1) % 4])
                if x is not None:
                    pts.append(x)
        want = ConvexHull(np.asarray(pts)).volume if len(pts) >= 3 else 0.  # .volume of a 2D hull is its area
        hit += want > 0
        assert abs(R.clip_area(fa, fb) - want) <= 1e-9
    assert hit > 100


def test_footprints_of_the_package_and_the_restatement_are_the_same_bits():
    b3 = np.asarray([p for pair in random_pairs(20, 1) for p in pair])
    assert np.array_equal(E.footprints(b3), R.footprints(b3))
    f = R.footprints([box(1., 10., 0., 1.5, 2., 4., 1.6)])[0]  # l along x at heading 0, clockwise from (+, +)
    assert f.tolist() == [3., 11., 3., 9., -1., 9., -1., 11., 1.6 - 1.5, 1.6, 8., 12.]


def tracked_fixture():
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
    return frames, dets, ids


def test_labels_with_box3d_and_scores_through_the_file_and_without(tmp_path):
    from mmmot_amd.tracks import write_kitti_tracks
    frames, dets, ids = tracked_fixture()
    rng = np.random.default_rng(0)
    scores = [rng.uniform(0, 1, len(d['bbox'])).astype(np.float32) for d in dets]
    n = max(frames) + 1
    # the defaults are unchanged: the golden file byte for byte, ten columns, no box3d
    out = tmp_path / 'plain.txt'
    write_kitti_tracks(str(out), dets, ids, frame_idx=frames)
    with open(os.path.join(GOLDEN, 'tracks_kitti_0001.txt'), 'rb') as f:
        assert out.read_bytes() == f.read()
    plain = E.load_kitti(str(out), 'car', n, False)
    assert plain.box3d is None and plain.rows.shape[1] == 10
    assert E.labels_from_tracks(dets, ids, frame_idx=frames).box3d is None
    default3 = E.load_kitti(str(out), 'car', n, False, box3d=True)
    assert np.array_equal(default3.rows, plain.rows) and np.all(default3.box3d[:, E.B3_SCORE] == 0.9)
    assert np.array_equal(default3.box3d, E.labels_from_tracks(dets, ids, frame_idx=frames, box3d=True).box3d)
    # with scores
    out = tmp_path / 'scored.txt'
    write_kitti_tracks(str(out), dets, ids, frame_idx=frames, scores=scores)
    for cls in ('car', 'pedestrian'):
        a = E.load_kitti(str(out), cls, n, False, box3d=True)
        b = E.labels_from_tracks(dets, ids, frame_idx=frames, cls=cls, box3d=True, scores=scores)
        assert len(a.rows) > 0 and np.array_equal(a.rows, b.rows) and np.array_equal(a.box3d, b.box3d)
        assert a.box3d.shape == (len(a.rows), 8) and len(np.unique(a.box3d[:, E.B3_SCORE])) > 3
        assert np.array_equal(a.rows, E.load_kitti(str(out), cls, n, False).rows)
        g = E.load_kitti(str(out), cls, n, True, box3d=True)  # read as ground truth: the score is 0
        assert np.all(g.box3d[:, E.B3_SCORE] == 0.) and np.array_equal(g.box3d[:, :7], a.box3d[:, :7])
        assert np.all(E.labels_from_tracks(dets, ids, frame_idx=frames, cls=cls, ground_truth=True, box3d=True,
                                           scores=scores).box3d[:, E.B3_SCORE] == 0.)
    # dimensions lhw -> hwl, as the file has them
    from mmmot_amd.tracks import KITTI_NAMES
    t0 = next(t for t in range(len(dets)) if np.any(ids[t] >= 0))
    k = int(np.flatnonzero(ids[t0] >= 0)[0])
    name = dets[t0]['name'][k] if 'name' in dets[t0] else 0
    name = name if isinstance(name, str) else KITTI_NAMES[int(name)]
    first = E.labels_from_tracks(dets[t0:t0 + 1], ids[t0:t0 + 1], cls=name.lower(), box3d=True)
    lhw = np.asarray(dets[t0]['dimensions'][k], np.float32)
    assert np.allclose(first.box3d[0, :3], [lhw[1], lhw[2], lhw[0]], atol=6e-5, rtol=0)
    assert np.allclose(first.box3d[0, 3:6], np.asarray(dets[t0]['location'][k], np.float32), atol=6e-5, rtol=0)
    # a ground-truth file without the score column
    p = tmp_path / 'gt.txt'
    p.write_text('0 1 Car 0 0 -10 10 10 50 90 1.5 1.6 3.9 2.0 1.7 20.0 0.1\n0 -1 DontCare -1 -1 -10 1 1 5 5 -1 -1 -1 -1000 -1000 -1000 -10')
    g = E.load_kitti(str(p), 'car', 1, True, box3d=True)
    assert g.box3d.tolist() == [[1.5, 1.6, 3.9, 2.0, 1.7, 20.0, 0.1, 0.], [-1, -1, -1, -1000, -1000, -1000, -10, 0.]]
    t = E.load_kitti(str(p), 'car', 1, False, box3d=True)  # a result file without the column: 0
    assert t.box3d[0, E.B3_SCORE] == 0.
    # concat carries the field, for all or for none
    both = E.concat([g, g])
    assert both.box3d.shape == (4, 8) and np.array_equal(both.box3d[2:], g.box3d)
    assert E.concat([plain, plain]).box3d is None
    with pytest.raises(ValueError, match='box3d'):
        E.concat([g, E.load_kitti(str(p), 'car', 1, True)])


def test_sweep_arithmetic():
    # need_k with n_gt no multiple of 40; every object matched: every level reachable
    s = [0.9 - 0.01 * i for i in range(37)]
    thr, reach = R.thresholds(list(reversed(s)), 37, 40)
    assert reach.all()
    need = [(k * 37 + 39) // 40 for k in range(1, 41)]
    assert need[0] == 1 and need[-1] == 37 and need[1] == 2 and need[20] == 20 and sorted(set(need)) == list(range(1, 38))
    assert thr.tolist() == [s[n - 1] for n in need]
    # fewer matches than objects: the upper levels are unreachable
    thr, reach = R.thresholds(s[:10], 37, 40)
    assert reach.tolist() == [n <= 10 for n in need] and np.all(np.isinf(thr[~reach])) and thr[reach][-1] == s[9]
    # equal scores at a threshold: the threshold is that score and `>=` keeps them all
    thr, reach = R.thresholds([0.5] * 6 + [0.25] * 4, 10, 5)
    assert thr.tolist() == [0.5, 0.5, 0.5, 0.25, 0.25] and int(np.sum(np.asarray([0.5] * 6 + [0.25] * 4) >= thr[2])) == 6
    # no ground truth: nothing is reachable, the averages are 0
    thr, reach = R.thresholds([], 0, 40)
    assert not reach.any() and R.averages([None] * 40, reach)[:3] == (0., 0., 0.) and R.averages([None] * 40, reach)[6] == -1
    # the metrics of a hand-made counter table, L = 4: levels 1, 2, 3 reachable
    tab = [dict(fn=7, fp=1, id_switches=0, n_gt=10, tp=3, total_cost=2.4), dict(fn=5, fp=2, id_switches=1, n_gt=10, tp=5, total_cost=3.5),
           dict(fn=2, fp=6, id_switches=2, n_gt=10, tp=8, total_cost=6.0), None]
    am, sm, ap, mota, smota, motp, best = R.averages(tab, np.array([True, True, True, False]))
    assert mota.tolist() == [1 - 8 / 10., 1 - 8 / 10., 1 - 10 / 10., 0.]
    assert smota.tolist() == [max(0., 1 - (8 - 0.75 * 10) / (0.25 * 10)), max(0., 1 - (8 - 0.5 * 10) / (0.5 * 10)),
                              max(0., 1 - (10 - 0.25 * 10) / (0.75 * 10)), 0.]
    assert motp.tolist() == [2.4 / 3, 3.5 / 5, 6.0 / 8, 0.]
    assert am == sum(mota.tolist()) / 4. and sm == sum(smota.tolist()) / 4. and ap == sum(motp.tolist()) / 4.
    assert best == 0 and smota[0] == 0.8
    # the lowest level wins a tie
    tie = [dict(fn=5, fp=0, id_switches=0, n_gt=10, tp=5, total_cost=4.), dict(fn=5, fp=0, id_switches=0, n_gt=10, tp=5, total_cost=4.)]
    assert R.averages(tie + tie, np.array([False, True, True, False]))[6] == 1
    # the package's host arithmetic is the same
    tot_i = np.array([[3, 0, 7, 0, 1, 0, 0], [5, 0, 5, 0, 2, 0, 1], [8, 0, 2, 0, 6, 0, 2], [0, 0, 0, 0, 0, 0, 0]])
    got = E.sweep_metrics(tot_i, np.array([2.4, 3.5, 6.0, 0.]), 10, np.array([True, True, True, False]))
    assert got[:3] == (am, sm, ap) and got[3].tolist() == mota.tolist() and got[4].tolist() == smota.tolist()
    assert got[5].tolist() == motp.tolist()


def test_track_scores_are_means_in_file_order():
    gts, trs, _, _ = mot3d_cases.build('one')
    tr, gt = trs[0], gts[0]
    want = R.track_scores(tr, gt.length)
    got = E.track_scores(tr.rows, tr.box3d[:, E.B3_SCORE])
    assert np.array_equal(got, want) and len(np.unique(got)) < len(got)
    p = E.pack_3d(gt, tr)
    assert np.array_equal(p['sigma'], want[p['t_idx']]) and p['box3d'].shape == (p['sizes'][0] + p['sizes'][1], 12)
    assert p['cells'] == int((p['g_cnt'] * p['t_cnt']).sum()) and np.array_equal(p['box3d'][:p['sizes'][0]],
                                                                                 R.footprints(gt.box3d[p['g_idx']]))


@pytest.mark.parametrize('name', sorted(mot3d_cases.specs()))
def test_generator_conditions_and_rejection_share(name):
    gts, trs, drawn, rejected = mot3d_cases.build(name)
    assert rejected <= 0.1 * drawn, (drawn, rejected)
    r = R.sweep(E.concat(gts), E.concat(trs), '3d', L=40)
    a = r['all']
    assert a['tp'] > 0 and a['n_gt'] > 0
    if name in ('one', 'three'):
        assert a['fp'] > 0 and a['fn'] > 0 and a['itp'] + a['ifn'] > 0 and a['n_itr'] > 0
        assert np.any(E.concat(gts).rows[:, E.CLS] == E.DONTCARE) and np.any(E.concat(trs).rows[:, E.CLS] == E.NEIGHBOUR)
    if name == 'few_tp':
        assert a['n_gt'] < 40 and not r['reachable'].all() and r['reachable'].any()
    if name == 'tied':
        assert len(set(r['thr'][r['reachable']].tolist())) <= 3 < int(r['reachable'].sum())
    if name == 'reachable':
        assert r['reachable'].all() and a['fn'] == 0
    # sMOTA_k is clamped below only: need_k rounds up, so a level can hold more recall than r_k and exceed 1
    assert 0. <= r['sAMOTA'] and 0. <= r['AMOTP'] <= 1. and r['AMOTA'] <= 1.


def test_2d_mode_of_the_restatement_is_the_2d_restatement():
    from test_clear_mot_cpu import golden
    gt, tr, d = golden('files', 'car')
    want = clear_mot_ref.evaluate(gt, tr)
    ev = np.array([r[E.FRAME] < gt.length[int(r[E.SEQ])] for r in tr.rows], bool)
    got = R.evaluate(gt, tr, '2d', 0.5, keep=ev)
    for k in ('tp', 'itp', 'fn', 'ifn', 'fp', 'n_itr', 'id_switches', 'fragments', 'n_mt', 'n_pt', 'n_ml', 'n_gt',
              'n_ignored_trajectories', 'tps', 'fps', 'fns'):
        assert got[k] == want[k], k
    assert np.array_equal(got['gt_tracker'], want['gt_tracker']) and abs(got['total_cost'] - want['total_cost']) < 1e-9


def test_refusals(tmp_path):
    gts, trs, _, _ = mot3d_cases.build('few_tp')
    gt, tr = gts[0], trs[0]
    strip = lambda lb: E.Labels(lb.rows, lb.n_frames, lb.length, lb.n_traj, lb.cls, lb.ground_truth)
    with pytest.raises(ValueError, match='box3d'):
        E.pack_3d(strip(gt), tr)
    with pytest.raises(ValueError, match='box3d'):
        E.evaluate_3d_sequences(gt, strip(tr), device='meta')
    assert E.pack_3d(strip(gt), strip(tr), need_3d=False)['box3d'].shape[1] == 12  # the '2d' mode takes them
    with pytest.raises(ValueError, match='sequences'):
        E.pack_3d([gt, gt], tr)
    with pytest.raises(ValueError, match='levels'):
        E.evaluate_3d_sequences(gt, tr, levels=-1, device='meta')
    with pytest.raises(ValueError, match='overlap'):
        E.evaluate_3d_sequences(gt, tr, overlap='4d', device='meta')
    for col, v in ((E.B3_H, 0.), (E.B3_W, -1.), (E.B3_L, float('nan'))):
        bad = E.Labels(tr.rows, tr.n_frames, tr.length, tr.n_traj, tr.cls, False, tr.box3d.copy())
        bad.box3d[0, col] = v
        with pytest.raises(ValueError, match='dimension'):
            E.pack_3d(gt, bad)
    # 129 boxes on a side, 65 DontCare areas: refused before any device work
    many = mot3d_cases.labels([[0, 0, i, E.MAIN, 0, 0, i, 10, i + 40, 90] for i in range(129)],
                              [[1.5, 1.6, 4., 3. * i, 1.6, 20., 0., 0.5] for i in range(129)], 1, False)
    one = mot3d_cases.labels([[0, 0, 0, E.MAIN, 0, 0, 0, 10, 40, 90]], [[1.5, 1.6, 4., 0., 1.6, 20., 0., 0.]], 1, True)
    with pytest.raises(ValueError, match='more than 128'):
        E.evaluate_3d_sequences(one, many, device='meta')
    dc = mot3d_cases.labels([[0, 0, -1, E.DONTCARE, -1, -1, i, 10, i + 40, 90] for i in range(65)],
                            [[-1, -1, -1, -1000, -1000, -1000, -10, 0]] * 65, 1, True)
    with pytest.raises(ValueError, match='DontCare'):
        E.evaluate_3d_sequences(dc, many, device='meta')


def test_meta_kernel_shape_and_layout():
    gts, trs, _, _ = mot3d_cases.build('three')
    p = E.pack_3d(gts, trs)
    nG, nT, nD, NF, NTr, S = p['sizes']
    sizes = p['sizes'] + [p['cells'], 40, 0]
    inp, out, n_in, n_out = mot3d_layout(sizes)
    assert n_in == 8 * (nG + nT + nD) + 24 * (nG + nT) + 2 * nT + 6 * NF + NF + 3 * nG + 2 * nT + NTr + 1 + nG + 2 * (S + 1)
    assert n_out == 41 * (4 * NF + 4 * (S + 1) + 6 * NF + 2 * nG + 4 * NTr + 12 * (S + 1)) + 2 * 40 + 40
    assert all(inp[k][0] % 2 == 0 for k in ('boxes', 'box3d', 'sigma')) and all(out[k][0] % 2 == 0 for k in ('frame_d', 'seq_d', 'thr'))
    res = torch.ops.mmmot.mot3d(torch.empty(n_in, dtype=torch.int32, device='meta'), sizes, [0.75, 25., 0., 2.])
    assert res.shape == (n_out,) and res.dtype == torch.int32 and res.device.type == 'meta'
    for bad in ([1, 1, 0, 1, 1, 0, 1, 40, 0], [1, 1, 0, 1, 1, 1, 1, 40, 3], [1, 1, 0, 1, 1, 1, 1, 2000, 0],
                [1, 1, 0, 1, 1, 1, 2 ** 31, 40, 0], [1, 1, 0, 1, 1, 1, 1, 40]):
        with pytest.raises(ValueError):
            mot3d_layout(bad)
    with pytest.raises(NotImplementedError):  # no CPU kernel, no fallback
        torch.ops.mmmot.mot3d(torch.zeros(n_in, dtype=torch.int32), sizes, [0.75, 25., 0., 2.])


def test_library_exports_mot3d_and_header_declares_it():
    from mmmot_amd import _lib
    path = _lib.build()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', path]).decode()
    assert re.search(r'\bT mmmot_mot3d\b', syms)
    with open(os.path.join(ROOT, 'include', 'mmmot_hip.h')) as f:
        assert re.search(r'\bint mmmot_mot3d\(const double\* boxes, const double\* box3d,', f.read())
    assert len(_lib.SIGNATURES['mmmot_mot3d']) == 35 and 'mot3d.hip' in _lib.SOURCES
    lib = _lib.load()
    args = [None, None, None, 0, 0, 0, None, None, 0, None, None, None, None, 0, None, 0, 0, 40, 0, 0.75, 25., 0., 2., None,
            0, None, None, None, None, None, None, None, None, None, None]
    assert lib.mmmot_mot3d(*args) == -1  # S < 1: refused before any launch
