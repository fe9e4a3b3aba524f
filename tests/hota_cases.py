"""Seeded random inputs of the HOTA / IDF1 tests and the conditions they have to meet (checked on the CPU by
tests/test_hota_cpu.py, used on the device by tests/test_hota_gpu.py).

A drawn sequence that breaks a condition is drawn again from the next seed; ``build`` reports how many were."""
import itertools

import numpy as np

import hota_ref
from mmmot_amd import evaluate as E

GAP = 1e-9


def labels(rows, n_frames, ground_truth):
    """ONE sequence from rows [sequence 0, frame, track ID, class code, truncation, occlusion, x1, y1, x2, y2]"""
    rows = np.asarray(rows, np.float64).reshape(-1, 10)
    ids = {r[E.TID] for r in rows if r[E.CLS] != E.DONTCARE}
    return E.Labels(rows, np.array([n_frames]), np.array([n_frames]), np.array([len(ids)]), 'car', bool(ground_truth))


def random_sequence(rng, counts, n_gid, n_stray, kitti=True, cyclic=0):
    """counts: (G, T) of every frame.  n_gid ground-truth identities drift over the image; a tracker box follows a
    ground-truth box with jitter under an ID that is a permutation of the gt ID and changes to another permutation half
    way; the tracker boxes beyond min(G, T) are strays far from every gt box with IDs of their own (n_stray of them).
    kitti: neighbour-class, occluded and truncated gt rows, small boxes and DontCare areas over some strays.
    cyclic > 0: frame f holds the gt IDs cyclic * f + k instead of a random draw (every ID gets its turn)."""
    F = len(counts)
    pos = np.stack([rng.uniform(0, 1100, n_gid), rng.uniform(0, 300, n_gid)], axis=1)
    size = np.stack([rng.uniform(40, 160, n_gid), rng.uniform(28, 120, n_gid)], axis=1)
    vel = rng.uniform(-4, 4, (n_gid, 2))
    kind = np.where(rng.random(n_gid) < 0.15, E.NEIGHBOUR, E.MAIN) if kitti else np.full(n_gid, E.MAIN)
    perm = [rng.permutation(n_gid), rng.permutation(n_gid)]
    if cyclic:  # every tracker ID gets its turn too
        perm = [np.arange(n_gid), np.roll(np.arange(n_gid), 1)]
    g, t = [], []
    for f, (G, T) in enumerate(counts):
        ids = (cyclic * f + np.arange(G)) % n_gid if cyclic else rng.permutation(n_gid)[:G]
        boxes = []
        for i in ids:
            x, y = pos[i] + f * vel[i]
            b = np.array([x, y, x + size[i, 0], y + size[i, 1]])
            boxes.append(b)
            occ = int(rng.integers(0, 4)) if kitti else 0
            trunc = int(rng.random() < 0.1) if kitti else 0
            g.append([0, f, int(i), kind[i], trunc, occ, *b])
        m = min(G, T)
        for k in rng.permutation(G)[:m]:
            w, h = boxes[k][2] - boxes[k][0], boxes[k][3] - boxes[k][1]
            j = rng.uniform(-0.08, 0.08, 4) if rng.random() < 0.85 else rng.uniform(-0.35, 0.35, 4)
            t.append([0, f, int(perm[f >= (F + 1) // 2][ids[k]]), E.MAIN, -1, -1, *(boxes[k] + j * np.array([w, h, w, h]))])
        for k, sid in enumerate(((cyclic * f + np.arange(T - m)) % n_stray if cyclic else rng.permutation(n_stray)[:T - m])):
            x, y = rng.uniform(0, 1100), 5000 + 200 * k + rng.uniform(0, 20)
            w, h = rng.uniform(40, 160), rng.uniform(12, 40) if kitti and rng.random() < 0.5 else rng.uniform(28, 120)
            t.append([0, f, n_gid + int(sid), E.MAIN, -1, -1, x, y, x + w, y + h])
            if kitti and rng.random() < 0.5:  # a DontCare area over a part of the stray
                c = rng.uniform(0.1, 0.9)
                g.append([0, f, -1, E.DONTCARE, -1, -1, x - 5, y - 5, x + c * w, y + h + 5])
    return labels(g, F, True), labels(t, F, False)


TWIN_COLUMNS, TWIN_IDS = (1, 66), (301, 300)  # the twin in the smaller column carries the larger ID


def twin_sequence(rng):
    """One sequence of three frames for the per-frame search where the drawn frames do not take it: 70 x 3 (the rows are
    the tracker side, and ground-truth columns in a lane's second slot), 3 x 70 with the SAME box in the tracker columns
    TWIN_COLUMNS (equal costs in two lanes, one of them in the second slot), and 0 x 2 (no row).  Boxes sit on a grid
    and overlap their partner only; plain main-class rows, every ID in one frame only, so that apart from which twin
    is taken nothing depends on the choice among equal matchings."""
    def spot(k, y0=0.):
        x, y = 20. + 150 * (k % 10), y0 + 20. + 110 * (k // 10)
        return np.array([x, y, x + 100, y + 80])

    near = lambda b: b + rng.uniform(-6, 6, 4)
    g = [[0, 0, k, E.MAIN, 0, 0, *spot(k)] for k in range(70)] + [[0, 1, 200 + k, E.MAIN, 0, 0, *spot(k)] for k in range(3)]
    t = [[0, 0, 100 + n, E.MAIN, -1, -1, *near(spot(k))] for n, k in enumerate((10, 40, 69))]
    twin = near(spot(1))
    partner = {5: near(spot(0)), 69: near(spot(2)), TWIN_COLUMNS[0]: twin, TWIN_COLUMNS[1]: twin}
    ids = dict(zip(TWIN_COLUMNS, TWIN_IDS))
    for j in range(70):
        t.append([0, 1, ids.get(j, 400 + j), E.MAIN, -1, -1, *partner.get(j, spot(j, 3000))])
    t += [[0, 2, 500 + j, E.MAIN, -1, -1, *spot(j)] for j in range(2)]
    return labels(g, 3, True), labels(t, 3, False)


def distinct_totals(m):
    """totals of all assignments of the smaller side of matrix m, one per set of non-zero cells, descending"""
    m = np.asarray(m, np.float64)
    if m.shape[0] > m.shape[1]:
        m = m.T
    R, C = m.shape
    if R == 0:
        return [0.0]
    seen = {}
    for cols in itertools.permutations(range(C), R):
        v = m[np.arange(R), cols]
        seen.setdefault(frozenset((r, c) for r, c in enumerate(cols) if v[r] != 0.0), float(v.sum()))
    return sorted(seen.values(), reverse=True)


def near(values, marks):
    values = np.asarray(values, np.float64).reshape(-1, 1)
    return bool(values.size and np.any(np.abs(values - np.asarray(marks, np.float64).reshape(1, -1)) <= GAP))


def conditions_met(gt, tr, prepare, matchings):
    """the generator conditions for one sequence; ``matchings``: also the gap between the best and the next-best total of
    both per-frame assignments, by brute force (frames of at most 6 boxes a side)"""
    marks = np.r_[hota_ref.ALPHAS - hota_ref.EPS, 0.5]
    r = hota_ref.hota(gt, tr, prepare=prepare)['seq'][0]
    for (g, t) in hota_ref.frames_of(gt, tr, 0):
        dc, cand = g[g[:, E.CLS] == E.DONTCARE], g[g[:, E.CLS] != E.DONTCARE]
        if near(hota_ref.iou_matrix(cand[:, E.X1:], t[:, E.X1:]), marks):
            return False
        if prepare is not None and (near(hota_ref.iou_matrix(t[:, E.X1:], dc[:, E.X1:], True), [0.5]) or
                                    near(t[:, E.X1 + 3] - t[:, E.X1 + 1], [25.0])):
            return False
    if not matchings:
        return True
    for m in [x for x in r['gated'] if x is not None] + r['scores']:
        if max(m.shape) > 6:
            raise ValueError('brute force over the matchings of a %d x %d frame' % m.shape)
        tot = distinct_totals(m)
        if len(tot) > 1 and tot[0] - tot[1] <= GAP:
            return False
    return True


# name -> (first seed, prepare, matchings checked, [per sequence: kwargs of random_sequence with the frame counts, or
# make = another generator])
def _counts(rng, n, choices):
    return [tuple(int(v) for v in rng.choice(choices, 2)) for _ in range(n)]


def specs():
    rng = np.random.default_rng(7)
    small = dict(n_gid=8, n_stray=6)
    return {
        # sequences of 1, 2 and 37 frames with 0, 1 and 5 (at most 6) boxes a side, G != T both ways
        'small_kitti': (100, 'kitti', True, [dict(counts=[(5, 6)], **small), dict(counts=[(6, 1), (1, 5)], **small),
                                             dict(counts=_counts(rng, 37, [0, 1, 5, 6]), **small)]),
        'small_plain': (200, None, True, [dict(counts=[(1, 0)], **small), dict(counts=[(0, 5), (5, 5)], **small),
                                          dict(counts=_counts(rng, 37, [0, 1, 5]), kitti=False, **small)]),
        # 12 boxes a side
        'mid_kitti': (300, 'kitti', False, [dict(counts=_counts(rng, 37, [0, 1, 5, 12]), n_gid=14, n_stray=12)]),
        # one frame at exactly CLEAR_MOT_MAX_BOXES boxes on both sides, one on either side
        'full_frame': (400, 'kitti', False, [dict(counts=[(128, 128), (12, 5), (128, 60), (70, 128)], n_gid=128,
                                                   n_stray=128)]),
        # more IDs than a wave has lanes: G = 70, T = 90, a few boxes a frame
        'wide_ids': (500, None, False, [dict(counts=[(4, 5)] * 40, n_gid=70, n_stray=20, kitti=False, cyclic=3)]),
        # the tracker side as rows with 70 columns, two equal columns, an empty side
        'transposed_twins': (600, 'kitti', False, [dict(make=twin_sequence)]),
    }


def build(name):
    """(ground-truth Labels per sequence, tracker Labels per sequence, prepare, matchings checked, drawn, replaced)"""
    seed, prepare, matchings, seqs = specs()[name]
    gts, trs, drawn, replaced = [], [], 0, 0
    for kw in seqs:
        kw = dict(kw)
        make = kw.pop('make', random_sequence)
        while True:
            gt, tr = make(np.random.default_rng(seed), **kw)
            seed += 1
            drawn += 1
            if conditions_met(gt, tr, prepare, matchings):
                break
            replaced += 1
            if replaced > 20:
                raise RuntimeError('hota_cases.%s: the generator keeps breaking its conditions' % name)
        gts.append(gt)
        trs.append(tr)
    return gts, trs, prepare, matchings, drawn, replaced
