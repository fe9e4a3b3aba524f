"""Serial numpy restatement of the CLEAR-MOT evaluator (reference kitti_devkit/evaluate_tracking.py:393-792): the host
oracle of tests/test_clear_mot_*.py and the host stand-in for timing.  One Python loop over sequences, frames and
trajectories on the label tables of mmmot_amd.evaluate.Labels (rows: sequence, frame, track ID, class code, truncation,
occlusion, x1, y1, x2, y2); the per-frame matching is scipy's linear_sum_assignment on the gated cost matrix.

evaluate(gt, tracker) returns a dict with the reference's names: the totals, the per-sequence lists, MODP_t, and per
ground-truth trajectory - sorted by (sequence, track ID), objects in frame order - the matched tracker IDs and ignored
flags, flat (``gt_tracker``, ``gt_ignored``) with ``traj_key`` rows (sequence, track ID, objects)."""
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

INVALID = 1000.0  # cost of a gated-out cell: above any sum of valid costs of a frame (<= 64), small enough to keep them


def overlap(a, b, over_a=False):
    """boxoverlap (:364-391): a, b = (x1, y1, x2, y2)"""
    x1, y1, x2, y2 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    w, h = x2 - x1, y2 - y1
    if w <= 0. or h <= 0.:
        return 0.
    inter = w * h
    aarea = (a[2] - a[0]) * (a[3] - a[1])
    if over_a:
        return inter / aarea
    barea = (b[2] - b[0]) * (b[3] - b[1])
    return inter / (aarea + barea - inter)


def cost_matrix(g, t, min_overlap=0.5):
    """(c [G, T] with c = 1 - IoU, valid [G, T]) of two float [n, 4] box arrays"""
    c = np.ones((len(g), len(t)))
    for i in range(len(g)):
        for j in range(len(t)):
            c[i, j] = 1 - overlap(g[i], t[j])
    return c, c <= min_overlap


def match(c, valid):
    """the valid cells of a minimum-cost assignment of min(G, T) pairs: {row: column}"""
    if c.size == 0:
        return {}
    rows, cols = linear_sum_assignment(np.where(valid, c, INVALID))
    return {int(r): int(k) for r, k in zip(rows, cols) if valid[r, k]}


def scan_trajectory(g, ign):
    """(ignored, ID switches, fragments, 'MT' / 'PT' / 'ML' / None) of one trajectory (:698-743)"""
    if all(ign):
        return True, 0, 0, None
    if all(v == -1 for v in g):
        return False, 0, 0, 'ML'
    ids = frag = 0
    last_id = g[0]
    tracked = 1 if g[0] >= 0 else 0
    f = 0
    for f in range(1, len(g)):
        if ign[f]:
            last_id = -1
            continue
        if last_id != g[f] and last_id != -1 and g[f] != -1 and g[f - 1] != -1:
            ids += 1
        if f < len(g) - 1 and g[f - 1] != g[f] and last_id != -1 and g[f] != -1 and g[f + 1] != -1:
            frag += 1
        if g[f] != -1:
            tracked += 1
            last_id = g[f]
    if len(g) > 1 and g[f - 1] != g[f] and last_id != -1 and g[f] != -1 and not ign[f]:
        frag += 1
    ratio = tracked / float(len(g) - sum(ign))
    return False, ids, frag, 'MT' if ratio > 0.8 else ('ML' if ratio < 0.2 else 'PT')


def evaluate(gt, tracker, min_overlap=0.5, max_truncation=0, min_height=25, max_occlusion=2):
    S = len(gt.n_frames)
    r = dict(n_gt=0, n_tr=0, tp=0, itp=0, fn=0, ifn=0, fp=0, n_igt=0, n_itr=0, total_cost=0., id_switches=0, fragments=0,
             n_mt=0, n_pt=0, n_ml=0, n_ignored_trajectories=0)
    lists = {k: [] for k in ('tps', 'itps', 'fps', 'fns', 'ifns', 'n_gts', 'n_trs', 'n_igts', 'n_itrs', 'seq_costs',
                             'seq_id_switches', 'seq_fragments')}
    modp_t, flat_g, flat_i, keys = [], [], [], []
    for s in range(S):
        G = gt.rows[gt.rows[:, 0] == s]
        T = tracker.rows[tracker.rows[:, 0] == s]
        traj, tign = {}, {}
        q = dict(tp=0, itp=0, fp=0, fn=0, ifn=0, igt=0, itr=0, n_gts=0, n_trs=0, cost=0.)
        for f in range(int(gt.length[s])):
            rows = G[G[:, 1] == f]
            g, dc, t = rows[rows[:, 3] != 2], rows[rows[:, 3] == 2], T[T[:, 1] == f]
            c, valid = cost_matrix(g[:, 6:], t[:, 6:], min_overlap)
            m = match(c, valid)
            for i in range(len(g)):
                traj.setdefault(int(g[i, 2]), []).append(int(t[m[i], 2]) if i in m else -1)
            matched_t = set(m.values())
            t_ign = []
            for j in range(len(t)):
                ig = False
                if j not in matched_t:
                    ig = t[j, 3] == 1 or abs(t[j, 7] - t[j, 9]) <= min_height or \
                        any(overlap(t[j, 6:], d[6:], True) > 0.5 for d in dc)
                t_ign.append(bool(ig))
            ifn = itp = pairs = 0
            tmpc = 0
            for i, j in sorted(m.items()):  # the reference's running sums, match by match in row order
                r['total_cost'] += 1 - c[i, j]
                tmpc += 1 - c[i, j]
            q['cost'] += tmpc
            for i in range(len(g)):
                cond = bool(g[i, 5] > max_occlusion or g[i, 4] > max_truncation or g[i, 3] == 1)
                tign.setdefault(int(g[i, 2]), []).append(cond)
                tid = int(t[m[i], 2]) if i in m else -1
                if tid < 0:
                    ifn += cond
                else:
                    itp += cond
                    if cond:
                        pairs += t_ign[m[i]]
                        tmpc -= 1 - c[i, m[i]]
            tmptp = len(m) - itp
            fn = len(g) - len(m) - ifn
            fp = len(t) - tmptp - sum(t_ign) - itp + pairs
            assert tmptp >= 0 and fn >= 0 and fp >= 0
            modp_t.append(tmpc / float(tmptp) if tmptp != 0 else 1)
            for k, v in (('tp', tmptp), ('itp', itp), ('fp', fp), ('fn', fn), ('ifn', ifn), ('igt', ifn + itp),
                         ('itr', sum(t_ign)), ('n_gts', len(g)), ('n_trs', len(t))):
                q[k] += v
            r['tp'] += len(m)
        for k, v in (('n_gt', q['n_gts'] - q['igt']), ('n_tr', q['n_trs']), ('itp', q['itp']), ('fn', q['fn']),
                     ('ifn', q['ifn']), ('fp', q['fp']), ('n_igt', q['igt']), ('n_itr', q['itr'])):
            r[k] += v
        for k, v in (('tps', 'tp'), ('itps', 'itp'), ('fps', 'fp'), ('fns', 'fn'), ('ifns', 'ifn'), ('n_gts', 'n_gts'),
                     ('n_trs', 'n_trs'), ('n_igts', 'igt'), ('n_itrs', 'itr'), ('seq_costs', 'cost')):
            lists[k].append(q[v])
        sid = sfr = 0
        for tid in sorted(traj):
            ig, ids, frag, cat = scan_trajectory(traj[tid], tign[tid])
            r['n_ignored_trajectories'] += ig
            r['id_switches'] += ids
            r['fragments'] += frag
            sid, sfr = sid + ids, sfr + frag
            if cat:
                r['n_' + cat.lower()] += 1
            flat_g += traj[tid]
            flat_i += tign[tid]
            keys.append((s, tid, len(traj[tid])))
        lists['seq_id_switches'].append(sid)
        lists['seq_fragments'].append(sfr)
    r.update(lists)
    r['n_gt_trajectories'], r['n_tr_trajectories'] = int(gt.n_traj.sum()), int(tracker.n_traj.sum())
    den = r['n_gt_trajectories'] - r['n_ignored_trajectories']
    r['MT'], r['PT'], r['ML'] = (0., 0., 0.) if den == 0 else tuple(r[k] / float(den) for k in ('n_mt', 'n_pt', 'n_ml'))
    if (r['fp'] + r['tp']) == 0 or (r['tp'] + r['fn']) == 0:
        r['recall'] = r['precision'] = 0.
    else:
        r['recall'], r['precision'] = r['tp'] / float(r['tp'] + r['fn']), r['tp'] / float(r['fp'] + r['tp'])
    pr = r['recall'] + r['precision']
    r['F1'] = 0. if pr == 0 else 2. * (r['precision'] * r['recall']) / pr
    nf = int(np.sum(gt.n_frames))
    r['FAR'] = 'n/a' if nf == 0 else r['fp'] / float(nf)
    if r['n_gt'] == 0:
        r['MOTA'] = r['MODA'] = r['MOTAL'] = -float('inf')
    else:
        r['MOTA'] = 1 - (r['fn'] + r['fp'] + r['id_switches']) / float(r['n_gt'])
        r['MODA'] = 1 - (r['fn'] + r['fp']) / float(r['n_gt'])
        r['MOTAL'] = r['MOTA'] if r['id_switches'] == 0 else \
            1 - (r['fn'] + r['fp'] + math.log10(r['id_switches'])) / float(r['n_gt'])
    r['MOTP'] = float('inf') if r['tp'] == 0 else r['total_cost'] / float(r['tp'])
    r['MODP'] = 'n/a' if nf == 0 else sum(modp_t) / float(nf)
    r['MODP_t'] = np.asarray(modp_t, np.float64)
    r['gt_tracker'], r['gt_ignored'] = np.asarray(flat_g, np.int64), np.asarray(flat_i, bool)
    r['traj_key'] = np.asarray(keys, np.int64).reshape(-1, 3)
    return r
