"""Serial NumPy / Python float64 restatement of the 3D MOT evaluation (DESIGN.md section 13 "3D / AMOTA"): the host
oracle of tests/test_mot3d_*.py and the host stand-in for timing.  The rules were written for this project; no agreement
with any published 3D evaluator is claimed.

Overlap, in this operation order (every product, sum and quotient rounded on its own - Python floats):
  footprint corners  (x + c dx + s dz, z - s dx + c dz), (dx, dz) = (l/2, w/2), (l/2, -w/2), (-l/2, -w/2), (-l/2, w/2)
  clip               the subject polygon (ground truth) against the edges e = 0..3 of the clip polygon (tracker), edge e
                     from corner A = e to corner B = (e + 1) % 4:  side(P) = ex (Pz - Az) - ez (Px - Ax) with (ex, ez) =
                     B - A, inside where side <= 0; walking S -> E over the polygon starting with S = the last vertex:
                     where the two sides differ emit S + t (E - S), t = dS / (dS - dE); then emit E where E is inside
  area               0.5 |sum_{k=1}^{n-2} (u_k x u_{k+1})|, u_k = P_k - P_0, the terms added in order from 0.0
  H                  min(y_a, y_b) - max(y_a - h_a, y_b - h_b)
  IoU3D              I / ((vol_a + vol_b) - I), I = A H, 0 unless A > 0 and H > 0;  IoUbev = A / ((wl_a + wl_b) - A)
  c                  1 - IoU

One operating point: tests/clear_mot_ref.py's evaluation (its matching, trajectory scan and 2D overlap are imported)
with c from the table; the sweep: ``sweep``."""
import numpy as np

import clear_mot_ref
from mmmot_amd import evaluate as E

CORNERS = ((1., 1.), (1., -1.), (-1., -1.), (-1., 1.))


def footprints(b3):
    """box3d rows [n, 8] -> [n, 12]: corners (x, z) x 4, y - h, y, w l, h w l (NumPy float64)"""
    b3 = np.asarray(b3, np.float64).reshape(-1, 8)
    h, w, l, x, y, z, ry = (b3[:, k] for k in range(7))
    c, s = np.cos(ry), np.sin(ry)
    out = np.empty((len(b3), 12))
    for k, (sx, sz) in enumerate(CORNERS):
        dx, dz = sx * (l / 2), sz * (w / 2)
        out[:, 2 * k] = x + c * dx + s * dz
        out[:, 2 * k + 1] = z - s * dx + c * dz
    out[:, 8], out[:, 9], out[:, 10], out[:, 11] = y - h, y, w * l, h * w * l
    return out


def clip(a, b, margin=None):
    """the vertices [(x, z)] of footprint a (8 floats) clipped by footprint b.  margin: a list that receives |side| of
    every vertex against every clip line it is tested on (the generator's degeneracy check)"""
    poly = [(float(a[2 * k]), float(a[2 * k + 1])) for k in range(4)]
    for e in range(4):
        ax, az = float(b[2 * e]), float(b[2 * e + 1])
        ex, ez = float(b[2 * ((e + 1) & 3)]) - ax, float(b[2 * ((e + 1) & 3) + 1]) - az
        out = []
        if poly:
            sx, sz = poly[-1]
            ds = ex * (sz - az) - ez * (sx - ax)
            for qx, qz in poly:
                de = ex * (qz - az) - ez * (qx - ax)
                if margin is not None:
                    margin.append(abs(de) / max(1e-300, (ex * ex + ez * ez) ** 0.5))
                if (de <= 0.) != (ds <= 0.) and len(out) < 8:
                    t = ds / (ds - de)
                    out.append((sx + t * (qx - sx), sz + t * (qz - sz)))
                if de <= 0. and len(out) < 8:
                    out.append((qx, qz))
                sx, sz, ds = qx, qz, de
        poly = out
    return poly


def area(poly):
    if len(poly) < 3:
        return 0.
    x0, z0 = poly[0]
    s = 0.
    for k in range(1, len(poly) - 1):
        ux, uz = poly[k][0] - x0, poly[k][1] - z0
        vx, vz = poly[k + 1][0] - x0, poly[k + 1][1] - z0
        s = s + (ux * vz - vx * uz)
    return 0.5 * abs(s)


def clip_area(a, b):
    return area(clip(a, b))


def iou(g, t, bev=False):
    """IoU3D (bev: IoUbev) of two packed boxes (12 floats each, ``footprints``)"""
    A = clip_area(g, t)
    if not A > 0.:
        return 0.
    if bev:
        return A / ((float(g[10]) + float(t[10])) - A)
    H = min(float(g[9]), float(t[9])) - max(float(g[8]), float(t[8]))
    if not H > 0.:
        return 0.
    I = A * H
    return I / ((float(g[11]) + float(t[11])) - I)


def iou_boxes(a, b, bev=False):
    """IoU of two box3d rows (h, w, l, x, y, z, rotation_y[, score])"""
    fa, fb = footprints(np.r_[np.asarray(a, np.float64)[:7], 0.]), footprints(np.r_[np.asarray(b, np.float64)[:7], 0.])
    return iou(fa[0], fb[0], bev)


def cost_table(g, t, mode, g3=None, t3=None, cache=None, keys=None):
    """c [G, T] of one frame: g, t rows of Labels.rows; g3, t3 their packed 3D boxes ('3d' / 'bev').  cache: a dict that
    keeps the cells between calls under (mode, keys[0][i], keys[1][j]) - a cell does not depend on the level"""
    c = np.ones((len(g), len(t)))
    for i in range(len(g)):
        for j in range(len(t)):
            k = None if cache is None else (mode, int(keys[0][i]), int(keys[1][j]))
            if k is not None and k in cache:
                c[i, j] = cache[k]
                continue
            if mode == '2d':
                c[i, j] = 1 - clear_mot_ref.overlap(g[i, 6:], t[j, 6:])
            else:
                c[i, j] = 1. - iou(g3[i], t3[j], mode == 'bev')
            if k is not None:
                cache[k] = c[i, j]
    return c


def track_scores(tracker, gt_length):
    """per tracker row the mean score of its track over the evaluated rows (frame < the ground truth's length), summed in
    file order; NaN on rows that are not evaluated"""
    acc = {}
    ev = [r[E.FRAME] < gt_length[int(r[E.SEQ])] for r in tracker.rows]
    for k, r in enumerate(tracker.rows):
        if ev[k]:
            a = acc.setdefault((int(r[E.SEQ]), int(r[E.TID])), [0., 0])
            a[0] = a[0] + float(tracker.box3d[k, 7])
            a[1] += 1
    return np.array([acc[(int(r[E.SEQ]), int(r[E.TID]))][0] / acc[(int(r[E.SEQ]), int(r[E.TID]))][1] if ev[k] else np.nan
                     for k, r in enumerate(tracker.rows)], np.float64).reshape(-1)


def evaluate(gt, tracker, mode='3d', gate=0.75, keep=None, sigma=None, max_truncation=0, min_height=25, max_occlusion=2,
             cache=None):
    """One operating point: clear_mot_ref.evaluate with c from ``cost_table`` and the tracker rows ``keep`` (a mask;
    default all).  Returns the counters the device returns: totals, per-sequence lists, MODP_t, total_cost, the flat
    trajectories, ``tables`` (c of every frame) and ``matched`` (sigma of the partner of every true positive that is
    not ignored, in frame order)."""
    S = len(gt.n_frames)
    keep = np.ones(len(tracker.rows), bool) if keep is None else np.asarray(keep, bool)
    g3all = footprints(gt.box3d) if mode != '2d' else np.zeros((len(gt.rows), 12))
    t3all = footprints(tracker.box3d) if mode != '2d' else np.zeros((len(tracker.rows), 12))
    r = dict(tp=0, itp=0, fn=0, ifn=0, fp=0, n_itr=0, total_cost=0., id_switches=0, fragments=0, n_mt=0, n_pt=0, n_ml=0,
             n_ignored_trajectories=0, n_obj=0, n_tr=0)
    lists = {k: [] for k in ('tps', 'itps', 'fps', 'fns', 'ifns', 'n_itrs', 'seq_costs', 'seq_id_switches', 'seq_fragments')}
    modp_t, flat_g, flat_i, keys, tables, matched = [], [], [], [], [], []
    for s in range(S):
        gi = np.flatnonzero(gt.rows[:, 0] == s)
        ti = np.flatnonzero((tracker.rows[:, 0] == s) & keep)
        traj, tign = {}, {}
        q = dict(tp=0, itp=0, fp=0, fn=0, ifn=0, itr=0, cost=0.)
        for f in range(int(gt.length[s])):
            fi = gi[gt.rows[gi, 1] == f]
            gsel, dsel = fi[gt.rows[fi, 3] != 2], fi[gt.rows[fi, 3] == 2]
            tsel = ti[tracker.rows[ti, 1] == f]
            g, dc, t = gt.rows[gsel], gt.rows[dsel], tracker.rows[tsel]
            c = cost_table(g, t, mode, g3all[gsel], t3all[tsel], cache, (gsel, tsel))
            tables.append(c)
            m = clear_mot_ref.match(c, c <= gate)
            matched_t = set(m.values())
            t_ign = []
            for j in range(len(t)):
                ig = False
                if j not in matched_t:
                    ig = t[j, 3] == 1 or abs(t[j, 7] - t[j, 9]) <= min_height or \
                        any(clear_mot_ref.overlap(t[j, 6:], d[6:], True) > 0.5 for d in dc)
                t_ign.append(bool(ig))
            ifn = itp = pairs = 0
            cost = kept = 0.
            for i in range(len(g)):
                cond = bool(g[i, 5] > max_occlusion or g[i, 4] > max_truncation or g[i, 3] == 1)
                tid = int(t[m[i], 2]) if i in m else -1
                traj.setdefault(int(g[i, 2]), []).append(tid)
                tign.setdefault(int(g[i, 2]), []).append(cond)
                if i in m:
                    cost += 1 - c[i, m[i]]
                if tid < 0:
                    ifn += cond
                else:
                    itp += cond
                    pairs += cond and t_ign[m[i]]
                if i in m and not (tid >= 0 and cond):
                    kept += 1 - c[i, m[i]]
                    if sigma is not None:
                        matched.append(float(sigma[tsel[m[i]]]))
            tmptp = len(m) - itp
            q['cost'] += cost
            r['total_cost'] += cost
            modp_t.append(kept / float(tmptp) if tmptp != 0 else 1.)
            for k, v in (('tp', len(m)), ('itp', itp), ('fn', len(g) - len(m) - ifn), ('ifn', ifn),
                         ('fp', len(t) - tmptp - sum(t_ign) - itp + pairs), ('itr', sum(t_ign))):
                q[k] += v
            r['n_obj'] += len(g)
            r['n_tr'] += len(t)
        for k, v in (('tp', 'tp'), ('itp', 'itp'), ('fn', 'fn'), ('ifn', 'ifn'), ('fp', 'fp'), ('n_itr', 'itr')):
            r[k] += q[v]
        for k, v in (('tps', q['tp'] - q['itp']), ('itps', q['itp']), ('fps', q['fp']), ('fns', q['fn']),
                     ('ifns', q['ifn']), ('n_itrs', q['itr']), ('seq_costs', q['cost'])):
            lists[k].append(v)
        sid = sfr = 0
        for tid in sorted(traj):
            ig, ids, frag, cat = clear_mot_ref.scan_trajectory(traj[tid], tign[tid])
            r['n_ignored_trajectories'] += ig
            sid, sfr = sid + ids, sfr + frag
            if cat:
                r['n_' + cat.lower()] += 1
            flat_g += traj[tid]
            flat_i += tign[tid]
            keys.append((s, tid, len(traj[tid])))
        r['id_switches'] += sid
        r['fragments'] += sfr
        lists['seq_id_switches'].append(sid)
        lists['seq_fragments'].append(sfr)
    r.update(lists)
    r['n_igt'] = r['ifn'] + r['itp']
    r['n_gt'] = r['n_obj'] - r['n_igt']
    nf = int(np.sum(gt.n_frames))
    r['MODP'] = 'n/a' if nf == 0 else sum(modp_t) / float(nf)
    r['MODP_t'] = np.asarray(modp_t, np.float64)
    r['gt_tracker'], r['gt_ignored'] = np.asarray(flat_g, np.int64), np.asarray(flat_i, bool)
    r['traj_key'] = np.asarray(keys, np.int64).reshape(-1, 3)
    r['tables'], r['matched'] = tables, matched
    return r


def thresholds(matched, n_gt, L):
    """(thr [L] with +inf where unreachable, reachable [L]) from the matched scores of pass A"""
    s = sorted(matched, reverse=True)
    thr, reach = np.full(L, np.inf), np.zeros(L, bool)
    for k in range(1, L + 1):
        need = (k * n_gt + L - 1) // L
        if n_gt > 0 and need <= len(s):
            thr[k - 1], reach[k - 1] = s[need - 1], True
    return thr, reach


def level_metrics(c, r_k):
    """(MOTA_k, sMOTA_k, MOTP_k) of one level's counters (a dict with fn, fp, id_switches, n_gt, tp, total_cost)"""
    n_gt, err = c['n_gt'], c['fn'] + c['fp'] + c['id_switches']
    return (1 - err / float(n_gt), max(0., 1 - (err - (1 - r_k) * n_gt) / (r_k * n_gt)),
            c['total_cost'] / float(c['tp']) if c['tp'] else 0.)


def averages(levels, reach):
    """(AMOTA, sAMOTA, AMOTP, MOTA_k, sMOTA_k, MOTP_k, best level index or -1): ``levels`` = the counters of every level
    (None where unreachable)"""
    L = len(reach)
    cols = np.zeros((3, L))
    for k in range(L):
        if reach[k]:
            cols[:, k] = level_metrics(levels[k], (k + 1) / float(L))
    best = -1
    for k in range(L):
        if reach[k] and (best < 0 or cols[1, k] > cols[1, best]):
            best = k
    mean = lambda v: sum(float(x) for x in v) / float(L) if L else 0.
    return mean(cols[0]), mean(cols[1]), mean(cols[2]), cols[0], cols[1], cols[2], best


def sweep(gt, tracker, mode='3d', min_iou=0.25, L=40, min_overlap=0.5, **kw):
    """the whole evaluation: dict with all (pass A), thr, reachable, levels (per level the counters or None), the three
    averages, the per-level arrays and best (level index or -1)"""
    gate = min_overlap if mode == '2d' else 1.0 - min_iou
    if tracker.box3d is not None:
        sigma = track_scores(tracker, gt.length)
    else:
        sigma = np.zeros(len(tracker.rows))
    ev = np.array([r[E.FRAME] < gt.length[int(r[E.SEQ])] for r in tracker.rows], bool).reshape(-1)
    cache = {}
    a = evaluate(gt, tracker, mode, gate, keep=ev, sigma=sigma, cache=cache, **kw)
    thr, reach = thresholds(a['matched'], a['n_gt'], L)
    levels = [evaluate(gt, tracker, mode, gate, keep=ev & (np.nan_to_num(sigma, nan=-np.inf) >= thr[k]),
                       cache=cache, **kw)
              if reach[k] else None for k in range(L)]
    am, sm, ap, mota, smota, motp, best = averages(levels, reach)
    return dict(all=a, thr=thr, reachable=reach, levels=levels, AMOTA=am, sAMOTA=sm, AMOTP=ap, MOTA_k=mota,
                sMOTA_k=smota, MOTP_k=motp, best=best, sigma=sigma)
