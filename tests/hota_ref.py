"""HOTA and IDF1 of tracked sequences, restated in NumPy + scipy.optimize.linear_sum_assignment from the rules of
DESIGN.md section 13 ("HOTA / IDF1").  This file is the executable specification mmmot_amd.evaluate.hota_sequences is
checked against; it was written from those rules, not from any published toolkit, and no agreement with one is claimed.

    r = hota(gt, tracker, prepare='kitti')     # gt / tracker: mmmot_amd.evaluate.Labels (or lists of them)

returns a dict: the per-alpha arrays TP, FN, FP, LocSum, HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA (suffix
'_alpha' for the ratios), their scalar means, IDTP / IDFN / IDFP / IDF1 / IDR / IDP, 'seq' (one dict per sequence) and
'frame_values' [frames, 2] (value of the preparation assignment, value of the pass-2 assignment).  A sequence's dict
also keeps the matrices both assignments were taken on ('gated', 'scores') and the similarities ('sims'), for checks
of the test inputs.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

from mmmot_amd.evaluate import CLS, DONTCARE, FRAME, MAIN, NEIGHBOUR, OCC, SEQ, TID, TRUNC, X1, concat

EPS = np.finfo(float).eps
ALPHAS = 0.05 * np.arange(1, 20)


def iou_matrix(a, b, over_a=False):
    """IoU (or intersection / area of a) of every box of a [n, 4] with every box of b [m, 4]: fm_overlap's operation
    order, every operation rounded on its own"""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    x1 = np.maximum(a[:, None, 0], b[None, :, 0])
    y1 = np.maximum(a[:, None, 1], b[None, :, 1])
    x2 = np.minimum(a[:, None, 2], b[None, :, 2])
    y2 = np.minimum(a[:, None, 3], b[None, :, 3])
    w, h = x2 - x1, y2 - y1
    inter = w * h
    aarea = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    barea = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        r = inter / aarea if over_a else inter / (aarea + barea - inter)
    return np.where((w <= 0.0) | (h <= 0.0), 0.0, r)


def prepare_frame(g, t, prepare, min_height=25, max_truncation=0, max_occlusion=2):
    """rows of one frame (ground truth with DontCare, tracker) -> (kept gt rows, kept tracker rows, assignment value,
    the gated similarity matrix the assignment was taken on - None without preparation)"""
    dc = g[g[:, CLS] == DONTCARE]
    g = g[g[:, CLS] != DONTCARE]
    if prepare is None:
        return g[g[:, CLS] == MAIN], t, 0.0, None
    s = iou_matrix(g[:, X1:], t[:, X1:])
    s = np.where(s < 0.5 - EPS, 0.0, s)
    rows, cols = linear_sum_assignment(-s)
    hit = s[rows, cols] > EPS
    rows, cols = rows[hit], cols[hit]
    value = float(s[rows, cols].sum())
    bad_gt = (g[:, CLS] == NEIGHBOUR) | (g[:, OCC] > max_occlusion) | (g[:, TRUNC] > max_truncation)
    remove = np.zeros(len(t), bool)
    remove[cols] = bad_gt[rows]
    unmatched = np.ones(len(t), bool)
    unmatched[cols] = False
    small = (t[:, X1 + 3] - t[:, X1 + 1]) <= min_height + EPS
    cover = iou_matrix(t[:, X1:], dc[:, X1:], over_a=True)
    in_dc = np.any(cover > 0.5 + EPS, axis=1) if len(dc) else np.zeros(len(t), bool)
    remove |= unmatched & (small | in_dc)
    return g[(g[:, CLS] == MAIN) & ~bad_gt], t[~remove], value, s


def frames_of(gt, tracker, s):
    """per frame of sequence s: (ground-truth rows, tracker rows), file order within a frame"""
    g = gt.rows[gt.rows[:, SEQ] == s]
    t = tracker.rows[tracker.rows[:, SEQ] == s]
    return [(g[g[:, FRAME] == f], t[t[:, FRAME] == f]) for f in range(int(gt.length[s]))]


def hota_sequence(frames):
    """frames: per frame (kept gt rows, kept tracker rows) of ONE sequence -> dict of its values"""
    gids = np.unique(np.concatenate([g[:, TID] for g, _ in frames] + [np.zeros(0)]))
    tids = np.unique(np.concatenate([t[:, TID] for _, t in frames] + [np.zeros(0)]))
    G, T, A = len(gids), len(tids), len(ALPHAS)
    fr = [(np.searchsorted(gids, g[:, TID]), np.searchsorted(tids, t[:, TID]), iou_matrix(g[:, X1:], t[:, X1:]))
          for g, t in frames]
    gt_count, tr_count = np.zeros(G), np.zeros(T)
    pot, pm = np.zeros((G, T)), np.zeros((G, T), np.int64)
    for gi, ti, s in fr:
        gt_count[gi] += 1
        tr_count[ti] += 1
        d = s.sum(0)[None, :] + s.sum(1)[:, None] - s
        ok = d > EPS
        pot[gi[:, None], ti[None, :]] += np.where(ok, s / np.where(ok, d, 1.0), 0.0)
        pm[gi[:, None], ti[None, :]] += s >= 0.5
    align = pot / (gt_count[:, None] + tr_count[None, :] - pot)
    TP, FN, FP = (np.zeros(A, np.int64) for _ in range(3))
    LocSum, mc, values, scores = np.zeros(A), np.zeros((A, G, T), np.int64), [], []
    for gi, ti, s in fr:
        score = align[gi[:, None], ti[None, :]] * s
        scores.append(score)
        if len(gi) == 0 or len(ti) == 0:
            FN += len(gi)
            FP += len(ti)
            values.append(0.0)
            continue
        rows, cols = linear_sum_assignment(-score)
        values.append(float(score[rows, cols].sum()))
        for a, alpha in enumerate(ALPHAS):
            hit = s[rows, cols] >= alpha - EPS
            n = int(hit.sum())
            TP[a] += n
            FN[a] += len(gi) - n
            FP[a] += len(ti) - n
            LocSum[a] += s[rows[hit], cols[hit]].sum()
            mc[a, gi[rows[hit]], ti[cols[hit]]] += 1
    den = np.maximum(1, TP)
    Aa = mc / np.maximum(1, gt_count[None, :, None] + tr_count[None, None, :] - mc)
    r = {'TP': TP, 'FN': FN, 'FP': FP, 'LocSum': LocSum, 'G': G, 'T': T,
         'AssA': (mc * Aa).sum((1, 2)) / den,
         'AssRe': (mc * (mc / np.maximum(1, gt_count[None, :, None]))).sum((1, 2)) / den,
         'AssPr': (mc * (mc / np.maximum(1, tr_count[None, None, :]))).sum((1, 2)) / den,
         'values': values, 'scores': scores, 'sims': [f[2] for f in fr]}
    # IDF1: the literal (G + T) x (G + T) program
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fn[:G, T:] = 1e10
    fp[G:, :T] = 1e10
    fn[np.arange(G), T + np.arange(G)] = gt_count
    fp[G + np.arange(T), np.arange(T)] = tr_count
    fn[:G, :T] = gt_count[:, None] - pm
    fp[:G, :T] = tr_count[None, :] - pm
    rows, cols = linear_sum_assignment(fn + fp)
    r['IDFN'] = int(round(fn[rows, cols].sum()))
    r['IDFP'] = int(round(fp[rows, cols].sum()))
    r['IDTP'] = int(round(gt_count.sum())) - r['IDFN']
    r['n_gt'], r['n_tr'] = int(round(gt_count.sum())), int(round(tr_count.sum()))
    return r


def ratios(r):
    """steps 3 / 4: Det*, LocA, HOTA from the counts and the association values of r (in place), and the means"""
    TP, FN, FP = r['TP'], r['FN'], r['FP']
    r['LocA_alpha'] = np.where(TP == 0, 1.0, r['LocSum'] / np.maximum(1e-10, TP))
    r['DetRe_alpha'] = TP / np.maximum(1, TP + FN)
    r['DetPr_alpha'] = TP / np.maximum(1, TP + FP)
    r['DetA_alpha'] = TP / np.maximum(1, TP + FN + FP)
    for k in ('AssA', 'AssRe', 'AssPr'):
        r[k + '_alpha'] = r[k]
    r['HOTA_alpha'] = np.sqrt(r['DetA_alpha'] * r['AssA_alpha'])
    for k in ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA'):
        r[k] = float(np.mean(r[k + '_alpha']))
    r['IDF1'] = r['IDTP'] / max(1.0, r['IDTP'] + 0.5 * r['IDFP'] + 0.5 * r['IDFN'])
    r['IDR'] = r['IDTP'] / max(1.0, float(r['IDTP'] + r['IDFN']))
    r['IDP'] = r['IDTP'] / max(1.0, float(r['IDTP'] + r['IDFP']))
    return r


def combine(seqs):
    """step 4 over the per-sequence dicts of hota_sequence"""
    out = {k: sum(s[k] for s in seqs) for k in ('TP', 'FN', 'FP', 'LocSum', 'IDTP', 'IDFN', 'IDFP', 'n_gt', 'n_tr')}
    den = np.maximum(1, out['TP'])
    for k in ('AssA', 'AssRe', 'AssPr'):
        out[k] = sum(s[k] * s['TP'] for s in seqs) / den
    return ratios(out)


def hota(gt, tracker, prepare='kitti', min_height=25, max_truncation=0, max_occlusion=2):
    gt = concat(gt) if isinstance(gt, (list, tuple)) else gt
    tracker = concat(tracker) if isinstance(tracker, (list, tuple)) else tracker
    seqs, values = [], []
    for s in range(gt.n_sequences):
        prepared = [prepare_frame(g, t, prepare, min_height, max_truncation, max_occlusion)
                    for g, t in frames_of(gt, tracker, s)]
        r = hota_sequence([p[:2] for p in prepared])
        values += [[p[2], w] for p, w in zip(prepared, r.pop('values'))]
        r['gated'] = [p[3] for p in prepared]
        seqs.append(r)
    out = combine(seqs)
    out['seq'] = [ratios(dict(s)) for s in seqs]
    out['frame_values'] = np.asarray(values, np.float64).reshape(-1, 2)
    return out
