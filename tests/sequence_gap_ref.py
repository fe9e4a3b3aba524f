"""Host statements of the whole-sequence association WITH SKIP LINKS (mmmot_amd.association.associate_sequence_gaps,
csrc/assign_sequence.hip), shared by the CPU and the GPU suite.  ``links[g - 1][t]`` is the n_t x n_{t+g} block of
gap g, g = 1 .. G; the flat order is [det | new | end | all g = 1 blocks in frame order | all g = 2 blocks | ..].

* ``milp_gap_route`` / ``lp_gap_route``: the literal program - for every detection v of frame t
  det_v = new_v + sum_g sum_j link^g_{t-g}[j][v] = end_v + sum_g sum_k link^g_t[v][k], all variables 0 / 1, maximise the
  scored sum - through scipy.optimize.milp and its LP relaxation through linprog, in the style of
  association_chain_ref;
* ``ssp_gap_route``: a serial fp64 restatement of the search the kernel runs - ``sequence_ref.ssp_route`` with the
  forward sweep relaxing in(k) over the source and over out(j) of the G frames before (ascending detection index: the
  earlier frame wins a tie), the same bounds;
* ``ids_of_gaps``: trajectory numbers from an assignment; ``assemble_gaps``: the flat layout from rows;
* ``planted_gap_sequence``: ``sequence_ref.planted_sequence`` with missed detections.
"""
import numpy as np
from scipy.optimize import Bounds, LinearConstraint, linprog, milp
from scipy.sparse import coo_matrix

from sequence_ref import _cost, _np


def assemble_gaps(det, new, end, links):
    """the flat fp32 scores [det | new | end | g = 1 blocks | g = 2 blocks | ..] of nested ``links``"""
    f = lambda x: np.asarray(_np(x), np.float32).reshape(-1)
    return np.concatenate([f(det), f(new), f(end)] + [f(l) for row in links for l in row])


def _offsets(split, G):
    """lo[g - 1][t]: the offset of block (g, t) among the variables, behind det / new / end"""
    lo, o = [], 3 * sum(split)
    for g in range(1, G + 1):
        row = []
        for t in range(len(split) - g):
            row.append(o)
            o += split[t] * split[t + g]
        lo.append(row)
    return lo, o


def _program(det, new, end, links, split, gt=None):
    split = [int(n) for n in split]
    T, L, G = len(split), sum(split), len(links)
    assert 1 <= G < T and all(len(links[g - 1]) == T - g for g in range(1, G + 1))
    w = assemble_gaps(det, new, end, links).astype(np.float64)
    const = 0.0
    if gt is not None:  # sum of gt - y * gt_eff with gt_eff = gt + (gt == 0) * -1
        g_ = assemble_gaps(gt[0], gt[1], gt[2], gt[3]).astype(np.float64)
        w = w - (g_ + (g_ == 0) * -1.0)
        const = float(g_.sum())
    lo, nvar = _offsets(split, G)
    assert w.size == nvar, 'scores do not match the split'
    st = np.concatenate([[0], np.cumsum(split)])
    ri, ci, va = [], [], []

    def add(r, cols, val):
        cols = np.atleast_1d(cols)
        ri.extend([r] * len(cols))
        ci.extend(cols.tolist())
        va.extend([val] * len(cols))

    r = 0
    for t in range(T):
        for j in range(split[t]):
            d = st[t] + j
            add(r, 2 * L + d, 1.0)  # end + successors of every gap = det
            add(r, d, -1.0)
            for g in range(1, G + 1):
                if t + g < T:
                    add(r, lo[g - 1][t] + j * split[t + g] + np.arange(split[t + g]), 1.0)
            r += 1
            add(r, L + d, 1.0)  # new + predecessors of every gap = det
            add(r, d, -1.0)
            for g in range(1, G + 1):
                if t - g >= 0:
                    add(r, lo[g - 1][t - g] + j + split[t] * np.arange(split[t - g]), 1.0)
            r += 1
    A = coo_matrix((va, (ri, ci)), shape=(r, w.size)).tocsr()
    return -w, const, A, L, lo, split, G


def _result(x, c, const, L, lo, split, G):
    x = np.round(x)
    links = [[x[lo[g - 1][t]:lo[g - 1][t] + split[t] * split[t + g]].reshape(split[t], split[t + g])
              for t in range(len(split) - g)] for g in range(1, G + 1)]
    return (x[0:L], links, x[L:2 * L], x[2 * L:3 * L]), float(np.dot(-c, x)) + const


def milp_gap_route(det, new, end, links, split, gt=None):
    """((det L, [[link n_t x n_{t+g} ...] per gap], new L, end L) float64 0 / 1, objective)"""
    c, const, A, L, lo, split, G = _program(det, new, end, links, split, gt)
    res = milp(c, constraints=LinearConstraint(A, 0, 0), integrality=np.ones(c.size), bounds=Bounds(0, 1),
               options={'mip_rel_gap': 0})
    assert res.status == 0, res.message
    return _result(res.x, c, const, L, lo, split, G)


def lp_gap_route(det, new, end, links, split, gt=None):
    """the LP relaxation: the matrix is the node-arc matrix of the layered network with skip arcs, totally unimodular"""
    c, const, A, L, lo, split, G = _program(det, new, end, links, split, gt)
    res = linprog(c, A_eq=A, b_eq=np.zeros(A.shape[0]), bounds=(0, 1), method='highs-ds')
    assert res.status == 0, res.message
    assert np.abs(res.x - np.round(res.x)).max() <= 1e-9, 'the LP vertex is not integral'
    return _result(res.x, c, const, L, lo, split, G)


def flat_links(links):
    return [l for row in links for l in row]


def gap_objective(assign, det, new, end, links):
    """the program's objective at an assignment (det, [[link ...] per gap], new, end)"""
    a = assemble_gaps(assign[0], assign[2], assign[3], assign[1]).astype(np.float64)
    return float(np.dot(a, assemble_gaps(det, new, end, links).astype(np.float64)))


def gap_feasible(assign, split):
    """every flow constraint holds, all values are 0 / 1"""
    split = [int(n) for n in split]
    det, links, new, end = assign
    T, G = len(split), len(links)
    det, new, end = (np.asarray(_np(x), np.float64).reshape(-1) for x in (det, new, end))
    if det.size != sum(split) or any(len(links[g - 1]) != T - g for g in range(1, G + 1)):
        return False
    links = [[np.asarray(_np(l), np.float64).reshape(split[t], split[t + g]) for t, l in enumerate(links[g - 1])]
             for g in range(1, G + 1)]
    if not all(np.all((x == 0) | (x == 1)) for x in [det, new, end] + flat_links(links)):
        return False
    st = np.concatenate([[0], np.cumsum(split)])
    for t in range(T):
        d = slice(st[t], st[t + 1])
        out = sum(links[g - 1][t].sum(1) for g in range(1, G + 1) if t + g < T)
        inn = sum(links[g - 1][t - g].sum(0) for g in range(1, G + 1) if t - g >= 0)
        if not (np.all(end[d] + out == det[d]) and np.all(new[d] + inn == det[d])):
            return False
    return True


def same_gap_assignment(a, b):
    fl = lambda r: [r[0], r[2], r[3]] + flat_links(r[1])
    return len(fl(a)) == len(fl(b)) and all(np.array_equal(np.asarray(_np(x)).reshape(-1), np.asarray(_np(y)).reshape(-1))
                                             for x, y in zip(fl(a), fl(b)))


def ids_of_gaps(assignment, split):
    """per frame the int64 trajectory numbers of an assignment (det, [[link ...] per gap], new, end): trajectories
    numbered 0, 1, .. in the order of (first frame, detection index), -1 where det = 0"""
    split = [int(n) for n in split]
    det, links, new, _ = assignment
    det, new = _np(det).reshape(-1), _np(new).reshape(-1)
    G = len(links)
    links = [[_np(l).reshape(split[t], split[t + g]) for t, l in enumerate(links[g - 1])] for g in range(1, G + 1)]
    st = np.concatenate([[0], np.cumsum(split)])
    out, nxt = [], 0
    for t, n in enumerate(split):
        ids = np.full(n, -1, np.int64)
        for k in range(n):
            if det[st[t] + k] != 1:
                continue
            if new[st[t] + k] == 1:
                ids[k] = nxt
                nxt += 1
            else:
                src = [(g, j) for g in range(1, G + 1) if t - g >= 0 for j in np.nonzero(links[g - 1][t - g][:, k] == 1)[0]]
                assert len(src) == 1, 'a kept detection that is not new needs exactly one predecessor'
                ids[k] = out[t - src[0][0]][src[0][1]]
        out.append(ids)
    return out


def ssp_gap_route(det, new, end, links, split, gt=None, ranges=False):
    """Returns ((det L, [[link ...] per gap], new L, end L) float64 0 / 1, objective, info) with info = {'status',
    'tracks', 'augmentations', 'passes'}; status as include/mmmot_hip.h (0 ok, 2 / 3 / 4 a bound hit).  Every sweep is a
    full one; with ``ranges`` a sweep visits only the frames the kernel visits (those whose inputs the sweep before
    lowered, widened by the gap), which must give the same labels."""
    split = [int(n) for n in split]
    T, L, G = len(split), sum(split), len(links)
    f32 = lambda x: np.asarray(_np(x), dtype=np.float32).reshape(-1)
    det, new, end = f32(det), f32(new), f32(end)
    links = [[f32(l).reshape(split[t], split[t + g]) for t, l in enumerate(links[g - 1])] for g in range(1, G + 1)]
    const = 0.0
    if gt is not None:  # the loss-augmented scores, in fp32 as association._flat_scores forms them
        eff = lambda g: (f32(g) + (f32(g) == 0).astype(np.float32) * np.float32(-1)).astype(np.float32)
        const = float(sum(f32(g).astype(np.float64).sum() for g in (gt[0], gt[1], gt[2], *flat_links(gt[3]))))
        det, new, end = det - eff(gt[0]), new - eff(gt[1]), end - eff(gt[2])
        links = [[l - eff(g).reshape(l.shape) for l, g in zip(row, grow)] for row, grow in zip(links, gt[3])]
    st = np.concatenate([[0], np.cumsum(split)]).astype(int)
    frame = np.repeat(np.arange(T), split)
    cdet, cnew, cend = ([_cost(x) for x in v] for v in (det, new, end))

    def score(pj, k):  # the fp32 score of the link pj -> k
        f, t = frame[pj], frame[k]
        return links[t - f - 1][f][pj - st[f], k - st[t]]

    # clink[k]: the costs of the links into k from the detections [st[t - G], st[t]) of the G frames before, in order
    clink = [[_cost(score(pj, k)) for pj in range(st[max(frame[k] - G, 0)], st[frame[k]])] for k in range(L)]
    used, pred, succ, inl = [False] * L, [-1] * L, [-1] * L, [0.0] * L
    INF = np.inf
    status, naug, npass = 0, 0, 0
    max_pass = 2 * L + 2
    for aug in range(L + 1):
        din, dout, pin, pout, pls = [INF] * L, [INF] * L, [-2] * L, [-2] * L, [0.0] * L
        settled = False
        flo, fhi = 0, T - 1  # the frames a forward sweep has to visit; it goes on while it lowers something
        for _ in range(max_pass):
            npass += 1
            blo, bhi = T, -1
            for t in range(flo, T):
                a0, c = st[max(t - G, 0)], False
                for k in range(st[t], st[t + 1]):
                    best, bp, bs = INF, -2, 0.0
                    if cnew[k] < INF and not (used[k] and pred[k] < 0):
                        best, bp = cnew[k], -1
                    bv, bj = INF, -1
                    ck = clink[k]
                    for pj in range(a0, st[t]):  # ascending: the earlier frame, then the smaller index, wins a tie
                        if dout[pj] < INF and not (used[pj] and succ[pj] == k):
                            cand = dout[pj] + ck[pj - a0]
                            if cand < bv:
                                bv, bj = cand, pj
                    if bv < best:
                        best, bp, bs = bv, L + bj, ck[bj - a0]
                    if best < din[k]:
                        din[k], pin[k], pls[k], c = best, bp, bs, True
                    if not used[k]:
                        co = din[k] + cdet[k]
                        if co < dout[k]:
                            dout[k], pout[k], c = co, k, True
                if c:  # dout of frame t may be lower: the frames t + 1 .. t + G read it
                    blo, bhi, fhi = min(blo, t), t, max(fhi, t + G)
                elif ranges and t >= fhi:
                    break
            chg = False
            flo, fhi = (T, -1) if ranges else (0, T - 1)
            if naug > 0:
                for t in range(bhi if ranges else T - 1, -1, -1):
                    c = False
                    for k in range(st[t], st[t + 1]):
                        if used[k]:
                            ci = dout[k] - cdet[k]
                            if ci < din[k]:
                                din[k], pin[k], c = ci, L + k, True
                            pk = pred[k]
                            if pk >= 0:
                                c2 = din[k] - inl[k]
                                if c2 < dout[pk]:
                                    dout[pk], pout[pk], c = c2, k, True
                    if c:  # dout of the frames t - G .. t - 1 may be lower: the frames t - G + 1 .. t + G - 1 read them
                        chg = True
                        if ranges:
                            fhi, flo, blo = max(fhi, min(T - 1, t + G - 1)), max(0, t - G + 1), min(blo, t - G)
                    elif ranges and t <= blo:
                        break
            if not chg:
                settled = True
                break
        if not settled:
            status = 3
            break
        bv, bj = INF, -1
        for v in range(L):
            if not (used[v] and succ[v] < 0):
                c = dout[v] + cend[v]
                if c < bv:
                    bv, bj = c, v
        if not bv < 0.0:
            break
        if aug == L:
            status = 2
            break
        w, q, SINK, done = 2 * L, L + bj, 2 * L, False
        for _ in range(max_pass):
            if w != SINK:
                q = pin[w] if w < L else pout[w - L]
            if q < -1:
                break
            if q < 0:
                pred[w] = -1
                done = True
                break
            if w == SINK:
                succ[q - L] = -1
            elif w >= L and q == w - L:
                used[q] = True
            elif w < L and q == w + L:
                used[w], pred[w], succ[w] = False, -1, -1
            elif w < L:
                pred[w], succ[q - L], inl[w] = q - L, w, pls[w]
            w = q
        if not done:
            status = 4
            break
        naug += 1
    a_det = np.array([1.0 if u else 0.0 for u in used])
    a_new = np.array([1.0 if used[v] and pred[v] < 0 else 0.0 for v in range(L)])
    a_end = np.array([1.0 if used[v] and succ[v] < 0 else 0.0 for v in range(L)])
    a_links = [[np.zeros((split[t], split[t + g])) for t in range(T - g)] for g in range(1, G + 1)]
    obj = 0.0
    for v in range(L):
        if used[v]:
            obj += float(det[v]) + (float(new[v]) if pred[v] < 0 else 0.0)
            if succ[v] < 0:
                obj += float(end[v])
            else:
                f, t = frame[v], frame[succ[v]]
                a_links[t - f - 1][f][v - st[f], succ[v] - st[t]] = 1.0
                obj += float(score(v, succ[v]))
    info = {'status': status, 'tracks': int(a_new.sum()), 'augmentations': naug, 'passes': npass}
    return (a_det, a_links, a_new, a_end), (obj + const if status == 0 else float('nan')), info


def random_gap_sequence(rng, split, G, kind='normal'):
    """(det, new, end, links nested) fp32: 'normal' standard normal, 'eval' with the first-frame new and the last-frame
    end zeroed, 'dense' all scores in [0.5, 1.5] (every detection kept, long trajectories, many reroutes), 'ties'
    integers in -2 .. 2"""
    split = [int(n) for n in split]
    L = sum(split)
    if kind == 'ties':
        f = lambda *s: rng.integers(-2, 3, s).astype(np.float32)
    elif kind == 'dense':
        f = lambda *s: rng.uniform(0.5, 1.5, s).astype(np.float32)
    else:
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
    det, new, end = f(L), f(L), f(L)
    links = [[f(split[t], split[t + g]) for t in range(len(split) - g)] for g in range(1, G + 1)]
    if kind == 'eval':
        new[:split[0]] = 0
        end[L - split[-1]:] = 0
    return det, new, end, links


def planted_gap_sequence(rng, T=30, max_n=6, G=3, p_miss=0.15):
    """``sequence_ref.planted_sequence`` with misses: hidden tracks are born and die mid-sequence; the detection of a
    live track is dropped with probability ``p_miss``, never in the track's first or last frame and never for more than
    G - 1 consecutive frames; a frame may end up empty.  Scores: det in [5, 6]; the link of every (t, t + g) pair of
    detections of one hidden track, g <= G, in [5, 6], all other links in [-6, -5]; new / end in [-1, 0] with the eval
    zeros in the first and the last frame.  Every bridge gains at least 5 over the end + new it replaces and every
    other link loses at least 5, so the optimum is one trajectory per hidden track, through all of its detections -
    unless two interleaved trajectories of one hidden track, picking the better links, gain more than the link they give
    up (at least 5, for less than 1 per link: possible only for tracks of more than 7 detections, and it takes long
    ones).  The CPU suite asserts on every seed the GPU suite uses that the optimum is the hidden tracks.
    Returns (split, (det, new, end, links nested by gap) fp32, per frame the hidden track of every detection, misses)."""
    live, nxt, alive = [0, 1], 2, []
    for t in range(T):
        if t > 0:
            keep = [h for h in live if rng.random() > 0.12]
            live = keep if keep else live[:1]
            while len(live) < max_n and rng.random() < 0.3:
                live.append(nxt)
                nxt += 1
        alive.append(list(live))
    first, last = {}, {}
    for t, hs in enumerate(alive):
        for h in hs:
            first.setdefault(h, t)
            last[h] = t
    run, frames, misses = {}, [], 0
    for t, hs in enumerate(alive):
        seen = []
        for h in hs:
            if first[h] < t < last[h] and run.get(h, 0) < G - 1 and rng.random() < p_miss:
                run[h] = run.get(h, 0) + 1
                misses += 1
            else:
                run[h] = 0
                seen.append(h)
        frames.append([seen[i] for i in rng.permutation(len(seen))])
    split = [len(f) for f in frames]
    L = sum(split)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)
    det, new, end = u(5, 6, L), u(-1, 0, L), u(-1, 0, L)
    new[:split[0]] = 0
    end[L - split[-1]:] = 0
    links = []
    for g in range(1, G + 1):
        row = []
        for t in range(T - g):
            l = u(-6, -5, split[t], split[t + g])
            for j, h in enumerate(frames[t]):
                if h in frames[t + g]:
                    l[j, frames[t + g].index(h)] = u(5, 6)
            row.append(l)
        links.append(row)
    return split, (det, new, end, links), frames, misses
