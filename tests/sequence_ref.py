"""NumPy restatement of the whole-sequence association (mmmot_amd.association.associate_sequence), written from its
rules and shared by the CPU and the GPU suite:

* ``assemble(pair_rows, counts)``: the scores of a sequence from the selected rows of its consecutive pair forwards, by
  the convention of ``SequencePipeline.run_global`` ("Sequences");
* ``ids_of(assignment, split)``: trajectory numbers from an assignment - trajectories numbered 0, 1, .. in the order of
  (first frame, detection index), -1 where det = 0;
* ``ssp_route(det, new, end, links, split, gt=None)``: a serial fp64 restatement of the search the kernel runs -
  successive shortest paths, each from a label-correcting search that alternates a forward sweep over the frames with a
  backward sweep along the trajectories, the same bounds, the same tie rule (strict decrease; inside one minimum the
  smallest node index, the source first).
"""
import numpy as np


def _np(x):
    return np.asarray(x.detach().cpu() if hasattr(x, 'detach') else x)


def assemble(pair_rows, counts):
    """``pair_rows[p]`` = (det [n_p + n_{p+1}], [link 1 x n_p x n_{p+1}], new, end) of pair p = (frame p, frame p + 1),
    ``counts`` = [n_0 .. n_{K-1}].  Returns (det L, [link n_t x n_{t+1} ...], new L, end L):
    det / new of frame 0 from pair 0's first half, of frame t >= 1 from pair t-1's second half; end of frame t <= K-2 from
    pair t's first half, of frame K-1 from pair K-2's second half; link_t = pair t's block."""
    counts = [int(n) for n in counts]
    K = len(counts)
    assert K >= 2 and len(pair_rows) == K - 1
    rows = [(_np(d).reshape(-1), _np(l[0]).reshape(counts[p], counts[p + 1]), _np(n).reshape(-1), _np(e).reshape(-1))
            for p, (d, l, n, e) in enumerate(pair_rows)]
    det, new, end, links = [], [], [], []
    for t in range(K):
        if t == 0:
            det.append(rows[0][0][:counts[0]])
            new.append(rows[0][2][:counts[0]])
        else:
            det.append(rows[t - 1][0][counts[t - 1]:])
            new.append(rows[t - 1][2][counts[t - 1]:])
        end.append(rows[t][3][:counts[t]] if t <= K - 2 else rows[K - 2][3][counts[K - 2]:])
        if t <= K - 2:
            links.append(rows[t][1])
    return np.concatenate(det), links, np.concatenate(new), np.concatenate(end)


def ids_of(assignment, split):
    """per frame the int64 trajectory numbers of an assignment (det, [link ...], new, end)"""
    split = [int(n) for n in split]
    det, links, new, _ = assignment
    det, new = _np(det).reshape(-1), _np(new).reshape(-1)
    links = [_np(l).reshape(split[t], split[t + 1]) for t, l in enumerate(links)]
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
                j = np.nonzero(links[t - 1][:, k] == 1)[0]
                assert j.size == 1, 'a kept detection that is not new needs exactly one predecessor'
                ids[k] = out[t - 1][j[0]]
        out.append(ids)
    return out


def _cost(s):
    s = np.float32(s)
    if s != s:
        return np.inf
    return -float(np.float32(min(max(s, np.float32(-1e30)), np.float32(1e30))))


def ssp_route(det, new, end, links, split, gt=None):
    """Returns ((det L, [link n_t x n_{t+1} ...], new L, end L) float64 0 / 1, objective, info) with info = {'status',
    'tracks', 'augmentations', 'passes'}; status as include/mmmot_hip.h (0 ok, 2 / 3 / 4 a bound hit)."""
    split = [int(n) for n in split]
    T, L = len(split), sum(split)
    f32 = lambda x: np.asarray(_np(x), dtype=np.float32).reshape(-1)
    det, new, end = f32(det), f32(new), f32(end)
    links = [f32(l).reshape(split[t], split[t + 1]) for t, l in enumerate(links)]
    const = 0.0
    if gt is not None:  # the loss-augmented scores, in fp32 as association._flat_scores forms them
        eff = lambda g: (f32(g) + (f32(g) == 0).astype(np.float32) * np.float32(-1)).astype(np.float32)
        const = float(sum(f32(g).astype(np.float64).sum() for g in (gt[0], gt[1], gt[2], *gt[3])))
        det, new, end = det - eff(gt[0]), new - eff(gt[1]), end - eff(gt[2])
        links = [l - eff(g).reshape(l.shape) for l, g in zip(links, gt[3])]
    st = np.concatenate([[0], np.cumsum(split)]).astype(int)
    cdet, cnew, cend = ([_cost(x) for x in v] for v in (det, new, end))
    clink = [[[_cost(x) for x in row] for row in l] for l in links]
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
                a, n = st[t], split[t]
                a0, n0 = (st[t - 1], split[t - 1]) if t > 0 else (0, 0)
                c = False
                for kk in range(n):
                    k = a + kk
                    best, bp, bs = INF, -2, 0.0
                    if cnew[k] < INF and not (used[k] and pred[k] < 0):
                        best, bp = cnew[k], -1
                    bv, bj = INF, -1
                    for j in range(n0):
                        pj = a0 + j
                        if not (used[pj] and succ[pj] == k):
                            cand = dout[pj] + clink[t - 1][j][kk]
                            if cand < bv:
                                bv, bj = cand, j
                    if bv < best:
                        best, bp, bs = bv, L + a0 + bj, clink[t - 1][bj][kk]
                    if best < din[k]:
                        din[k], pin[k], pls[k], c = best, bp, bs, True
                    if not used[k]:
                        co = din[k] + cdet[k]
                        if co < dout[k]:
                            dout[k], pout[k], c = co, k, True
                if c:
                    blo, bhi = min(blo, t), t
                elif t >= fhi:
                    break
            chg = False
            flo, fhi = T, -1
            if naug > 0:
                for t in range(bhi, -1, -1):
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
                    if c:
                        fhi, flo, chg = max(fhi, t), t, True
                    elif t <= blo:
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
    a_links = [np.zeros((split[t], split[t + 1])) for t in range(T - 1)]
    obj = 0.0
    for t in range(T):
        for v in range(st[t], st[t + 1]):
            if used[v]:
                obj += float(det[v]) + (float(new[v]) if pred[v] < 0 else 0.0)
                if succ[v] < 0:
                    obj += float(end[v])
                else:
                    a_links[t][v - st[t], succ[v] - st[t + 1]] = 1.0
                    obj += float(links[t][v - st[t], succ[v] - st[t + 1]])
    info = {'status': status, 'tracks': int(a_new.sum()), 'augmentations': naug, 'passes': npass}
    return (a_det, a_links, a_new, a_end), (obj + const if status == 0 else float('nan')), info


def planted_sequence(rng, T=30, max_n=6):
    """A decisive instance with hidden tracks that are born and die mid-sequence, every frame holding 1 .. ``max_n``
    detections in shuffled order: det in [5, 6]; the planted links in [5, 6], all others in [-6, -5]; new / end in [-1, 0]
    with the eval zeros in the first and the last frame.  Returns (split, (det, new, end, links) fp32, per frame the
    hidden track of every detection)."""
    live, nxt, frames = [0, 1], 2, []
    for t in range(T):
        if t > 0:
            keep = [h for h in live if rng.random() > 0.12]
            live = keep if keep else live[:1]
            while len(live) < max_n and rng.random() < 0.3:
                live.append(nxt)
                nxt += 1
        frames.append([live[i] for i in rng.permutation(len(live))])
    split = [len(f) for f in frames]
    L = sum(split)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)
    det, new, end = u(5, 6, L), u(-1, 0, L), u(-1, 0, L)
    new[:split[0]] = 0
    end[L - split[-1]:] = 0
    links = []
    for t in range(T - 1):
        l = u(-6, -5, split[t], split[t + 1])
        for j, h in enumerate(frames[t]):
            if h in frames[t + 1]:
                l[j, frames[t + 1].index(h)] = u(5, 6)
        links.append(l)
    return split, (det, new, end, links), frames
