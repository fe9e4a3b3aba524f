"""Seeded random scenes of the 3D MOT tests and the conditions they have to meet (checked on the CPU by
tests/test_mot3d_cpu.py, used on the device by tests/test_mot3d_gpu.py).

A drawn sequence is rejected and drawn again from the next seed when, in '3d' or 'bev' mode,
  - any c lies within 1e-9 of the gate 1 - 0.25,
  - any vertex met while clipping lies within 1e-6 of the clip line it is tested against,
  - (frames of at most 6 boxes a side, by brute force) two matchings of a frame take the same number of valid cells at
    costs less than 1e-9 apart.
``build`` reports how many draws were rejected.  Scenes with planted twins (``twins``) admit the tie on purpose and
skip the last two conditions."""
import numpy as np

import mot3d_ref
from hota_cases import distinct_totals
from mmmot_amd import evaluate as E

GATE = 0.75
FOCAL, CX, CY = 720.0, 620.0, 180.0
RY_SPECIAL = (0.0, np.pi / 2, np.pi, -np.pi)


def labels(rows, b3, n_frames, ground_truth):
    """ONE sequence from rows [0, frame, track ID, class code, truncation, occlusion, x1, y1, x2, y2] and box3d rows"""
    rows = np.asarray(rows, np.float64).reshape(-1, 10)
    ids = {r[E.TID] for r in rows if r[E.CLS] != E.DONTCARE}
    return E.Labels(rows, np.array([n_frames]), np.array([n_frames]), np.array([len(ids)]), 'car', bool(ground_truth),
                    np.asarray(b3, np.float64).reshape(-1, 8))


def project(b):
    """a rough image-plane box of a 3D box (h, w, l, x, y, z, ..): enough for min_height and the DontCare areas"""
    h, w, l, x, y, z = (float(v) for v in b[:6])
    z = max(z, 2.0)
    half = 0.5 * max(w, l) * FOCAL / z
    u, v = CX + FOCAL * x / z, CY + FOCAL * y / z
    return [u - half, v - FOCAL * h / z, u + half, v]


def random_sequence(rng, counts, n_gid, kitti=True, all_matched=False, tied=False, twins=False):
    """counts: (G, T) of every frame.  n_gid ground-truth identities drive over the ground plane; a tracker box follows
    a ground-truth box with jitter in position, size and heading (sometimes turned by pi) under an ID that changes half
    way; the tracker boxes beyond min(G, T) are strays far away, some under a DontCare area.  kitti: neighbour-class,
    occluded and truncated rows.  all_matched: tight jitter and nothing ignored, so that every object is a true positive.
    tied: track scores from {0.25, 0.5, 0.75} only.  twins: every tracker box of a frame's first object is planted
    twice (an identical twin under another ID)."""
    F = len(counts)
    pos = np.stack([rng.uniform(-25, 25, n_gid), rng.uniform(6, 70, n_gid)], axis=1)
    vel = rng.uniform(-0.6, 0.6, (n_gid, 2))
    dim = np.stack([rng.uniform(1.3, 2.0, n_gid), rng.uniform(1.5, 2.0, n_gid), rng.uniform(3.2, 5.0, n_gid)], axis=1)
    ry = rng.uniform(-np.pi, np.pi, n_gid)
    ry[:min(4, n_gid)] = RY_SPECIAL[:min(4, n_gid)]
    kind = np.where(rng.random(n_gid) < 0.15, E.NEIGHBOUR, E.MAIN) if kitti and not all_matched else np.full(n_gid, E.MAIN)
    perm = [rng.permutation(n_gid), rng.permutation(n_gid)]
    n_tid = 2 * n_gid + 40
    score_of = rng.choice([0.25, 0.5, 0.75], n_tid) if tied else rng.uniform(0.05, 0.95, n_tid)
    g, g3, t, t3 = [], [], [], []
    for f, (G, T) in enumerate(counts):
        ids = rng.permutation(n_gid)[:G]
        boxes = []
        for i in ids:
            x, z = pos[i] + f * vel[i]
            b = [dim[i, 0], dim[i, 1], dim[i, 2], x, 1.65 + 0.01 * (i % 7), z, ry[i], 0.0]
            boxes.append(b)
            occ = int(rng.integers(0, 4)) if kitti and not all_matched else 0
            trunc = int(rng.random() < 0.1) if kitti and not all_matched else 0
            g.append([0, f, int(i), kind[i], trunc, occ, *project(b)])
            g3.append(b)
        m = min(G, T - (1 if twins and T > G else 0)) if twins else min(G, T)
        order = rng.permutation(G)[:m]
        for n, k in enumerate(order):
            b = list(boxes[k])
            wide = (not all_matched) and rng.random() < 0.2
            b[3] += rng.uniform(-1.6, 1.6) if wide else rng.uniform(-0.15, 0.15)
            b[5] += rng.uniform(-1.6, 1.6) if wide else rng.uniform(-0.15, 0.15)
            b[4] += rng.uniform(-0.1, 0.1)
            b[0:3] = [v * rng.uniform(0.93, 1.07) for v in b[0:3]]
            b[6] += rng.uniform(-0.08, 0.08) + (np.pi if rng.random() < 0.2 else 0.0)
            tid = int(perm[f >= (F + 1) // 2][ids[k]])
            b[7] = float(np.clip(score_of[tid] + (0.0 if tied else rng.uniform(-0.04, 0.04)), 0.0, 1.0))
            cls = E.NEIGHBOUR if kitti and not all_matched and rng.random() < 0.08 else E.MAIN
            t.append([0, f, tid, cls, -1, -1, *project(b)])
            t3.append(b)
            if twins and n == 0 and len(order) < T:
                t.append([0, f, n_tid + 1, cls, -1, -1, *project(b)])
                t3.append(list(b))
        have = len(order) + (1 if twins and len(order) and len(order) < T else 0)
        used = set()
        for k in range(T - have):
            sid = n_gid + int(rng.integers(0, n_gid + 40))
            while sid in used:
                sid = n_gid + int(rng.integers(0, n_gid + 40))
            used.add(sid)
            b = [rng.uniform(1.3, 2.0), rng.uniform(1.5, 2.0), rng.uniform(3.2, 5.0), 200.0 + 12.0 * k + rng.uniform(0, 2),
                 1.7, rng.uniform(20, 90), rng.uniform(-np.pi, np.pi), float(score_of[sid])]
            box = project(b)
            t.append([0, f, sid, E.MAIN, -1, -1, *box])
            t3.append(b)
            if kitti and rng.random() < 0.5:  # a DontCare area over a part of the stray
                c = rng.uniform(0.1, 0.9)
                g.append([0, f, -1, E.DONTCARE, -1, -1, box[0] - 5, box[1] - 5, box[0] + c * (box[2] - box[0]), box[3] + 5])
                g3.append([-1, -1, -1, -1000, -1000, -1000, -10, 0])
    return labels(g, g3, F, True), labels(t, t3, F, False)


def conditions_met(gt, tr, matchings, twins=False):
    for mode in ('3d', 'bev'):
        margin = []
        G3, T3 = mot3d_ref.footprints(gt.box3d), mot3d_ref.footprints(tr.box3d)
        for f in range(int(gt.length[0])):
            gs = np.flatnonzero((gt.rows[:, E.FRAME] == f) & (gt.rows[:, E.CLS] != E.DONTCARE))
            ts = np.flatnonzero(tr.rows[:, E.FRAME] == f)
            c = mot3d_ref.cost_table(gt.rows[gs], tr.rows[ts], mode, G3[gs], T3[ts])
            if c.size and np.any(np.abs(c - GATE) <= 1e-9):
                return False
            if twins:
                continue
            if mode == '3d':
                for i in gs:
                    for j in ts:
                        mot3d_ref.clip(G3[i], T3[j], margin)
            if matchings and c.size:
                if max(c.shape) > 6:
                    raise ValueError('brute force over the matchings of a %d x %d frame' % c.shape)
                tot = distinct_totals(np.where(c <= GATE, 128.0 - c, 0.0))
                if len(tot) > 1 and tot[0] - tot[1] <= 1e-9:
                    return False
        if margin and min(margin) <= 1e-6:
            return False
    return True


def _counts(rng, n, choices):
    return [tuple(int(v) for v in rng.choice(choices, 2)) for _ in range(n)]


# name -> (first seed, matchings checked, [per sequence: kwargs of random_sequence])
def specs():
    rng = np.random.default_rng(11)
    return {
        # S = 1 and S = 3, about 20 frames, DontCare areas, occluded / truncated objects, neighbour-class rows
        'one': (100, True, [dict(counts=_counts(rng, 20, [0, 1, 4, 6]), n_gid=8)]),
        'three': (200, True, [dict(counts=[(5, 6)], n_gid=8), dict(counts=_counts(rng, 19, [0, 1, 5, 6]), n_gid=8),
                              dict(counts=_counts(rng, 21, [2, 3, 6]), n_gid=9)]),
        # the sweep: fewer true positives than levels; tied track scores; every level reachable
        'few_tp': (300, True, [dict(counts=[(3, 3), (2, 3), (3, 2), (3, 4)], n_gid=4, kitti=False)]),
        'tied': (400, True, [dict(counts=_counts(rng, 20, [4, 5, 6]), n_gid=8, tied=True)]),
        'reachable': (500, True, [dict(counts=[(5, 5)] * 12 + [(5, 6)] * 4, n_gid=7, all_matched=True)]),
        # planted twins: the admitted tie
        'twins': (600, False, [dict(counts=[(3, 5), (4, 6), (2, 4), (5, 6)] * 3, n_gid=8, kitti=False, twins=True)]),
    }


_built = {}


def build(name):
    """(ground-truth Labels per sequence, tracker Labels per sequence, drawn, rejected); built once"""
    if name in _built:
        return _built[name]
    seed, matchings, seqs = specs()[name]
    gts, trs, drawn, rejected = [], [], 0, 0
    for kw in seqs:
        while True:
            gt, tr = random_sequence(np.random.default_rng(seed), **kw)
            seed += 1
            drawn += 1
            if conditions_met(gt, tr, matchings, kw.get('twins', False)):
                break
            rejected += 1
            if rejected > 20:
                raise RuntimeError('mot3d_cases.%s: the generator keeps breaking its conditions' % name)
        gts.append(gt)
        trs.append(tr)
    _built[name] = (gts, trs, drawn, rejected)
    return _built[name]


def shape_frames(rng, sizes):
    """one sequence for the overlap-table test: frame f holds sizes[f] = (G, T) boxes scattered over a small patch of
    ground (so that many cells overlap), headings 0, pi / 2, pi and -pi among them"""
    g, g3, t, t3 = [], [], [], []
    for f, (G, T) in enumerate(sizes):
        for rows, b3s, n in ((g, g3, G), (t, t3, T)):
            for k in range(n):
                ry = RY_SPECIAL[k % 4] if k % 3 == 0 else rng.uniform(-np.pi, np.pi)
                b = [rng.uniform(1.3, 2.0), rng.uniform(1.5, 2.2), rng.uniform(3.0, 5.0), rng.uniform(-9, 9),
                     rng.uniform(1.2, 2.2), rng.uniform(10, 28), ry, rng.uniform(0, 1)]
                rows.append([0, f, k, E.MAIN, 0, 0, *project(b)])
                b3s.append(b)
    return labels(g, g3, len(sizes), True), labels(t, t3, len(sizes), False)
