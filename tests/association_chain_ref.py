"""Host oracle of the chain association (the program of ``ortools_solve`` for any ``len(det_split) >= 2``), two
independent routes to its optimum:

* ``milp_route``: the literal binary program - y_det / y_new / y_end per detection, y_link per adjacent frame pair, the
  flow constraints of solvers.py:83-111, maximise the scored sum - through scipy.optimize.milp (HiGHS, mip_rel_gap = 0);
* ``lp_route``: its LP relaxation through scipy.optimize.linprog (HiGHS dual simplex): the constraint matrix is the
  node-arc matrix of a layered flow network, totally unimodular, so the vertex the simplex returns is integral.

Both return (det L, [link n_t x n_{t+1} ...], new L, end L) as float64 numpy 0 / 1 arrays and the fp64 objective.
``gt=(gt_det, gt_new, gt_end, [gt_link ...])`` is the loss-augmented objective of solvers.py:50-81 (the constant term
included in the objective value).
"""
import numpy as np
from scipy.optimize import Bounds, LinearConstraint, linprog, milp
from scipy.sparse import coo_matrix


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1)


def _program(det, new, end, links, split, gt=None):
    """(c to minimise, constant of the objective, sparse A with A y = 0, L, link offsets) - variable order:
    det [0, L), new [L, 2L), end [2L, 3L), then the link blocks row-major"""
    split = [int(n) for n in split]
    T, L = len(split), sum(split)
    assert T >= 2 and len(links) == T - 1
    w = np.concatenate([_f64(det), _f64(new), _f64(end)] + [_f64(l) for l in links])
    const = 0.0
    if gt is not None:  # sum of gt - y * gt_eff with gt_eff = gt + (gt == 0) * -1
        g = np.concatenate([_f64(gt[0]), _f64(gt[1]), _f64(gt[2])] + [_f64(l) for l in gt[3]])
        w = w - (g + (g == 0) * -1.0)
        const = float(g.sum())
    st = np.concatenate([[0], np.cumsum(split)])
    sizes = [split[t] * split[t + 1] for t in range(T - 1)]
    lo = 3 * L + np.concatenate([[0], np.cumsum(sizes)])
    assert w.size == lo[-1], 'scores do not match the split'
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
            # end + successors = det  (the last frame: end = det)
            add(r, 2 * L + d, 1.0)
            add(r, d, -1.0)
            if t < T - 1:
                add(r, lo[t] + j * split[t + 1] + np.arange(split[t + 1]), 1.0)
            r += 1
            # new + predecessors = det  (the first frame: new = det)
            add(r, L + d, 1.0)
            add(r, d, -1.0)
            if t > 0:
                add(r, lo[t - 1] + j + split[t] * np.arange(split[t - 1]), 1.0)
            r += 1
    A = coo_matrix((va, (ri, ci)), shape=(r, w.size)).tocsr()
    return -w, const, A, L, lo, split


def _result(x, c, const, L, lo, split):
    x = np.round(x)
    links = [x[lo[t]:lo[t + 1]].reshape(split[t], split[t + 1]) for t in range(len(split) - 1)]
    return (x[0:L], links, x[L:2 * L], x[2 * L:3 * L]), float(np.dot(-c, x)) + const


def milp_route(det, new, end, links, split, gt=None):
    c, const, A, L, lo, split = _program(det, new, end, links, split, gt)
    res = milp(c, constraints=LinearConstraint(A, 0, 0), integrality=np.ones(c.size), bounds=Bounds(0, 1),
               options={'mip_rel_gap': 0})
    assert res.status == 0, res.message
    return _result(res.x, c, const, L, lo, split)


def lp_route(det, new, end, links, split, gt=None):
    c, const, A, L, lo, split = _program(det, new, end, links, split, gt)
    res = linprog(c, A_eq=A, b_eq=np.zeros(A.shape[0]), bounds=(0, 1), method='highs-ds')
    assert res.status == 0, res.message
    assert np.abs(res.x - np.round(res.x)).max() <= 1e-9, 'the LP vertex is not integral'
    return _result(res.x, c, const, L, lo, split)


def objective(assign, det, new, end, links):
    """the program's objective at an assignment (det, [link ...], new, end)"""
    a = np.concatenate([np.asarray(assign[0], np.float64).reshape(-1), np.asarray(assign[2], np.float64).reshape(-1),
                        np.asarray(assign[3], np.float64).reshape(-1)] +
                       [np.asarray(l, np.float64).reshape(-1) for l in assign[1]])
    w = np.concatenate([_f64(det), _f64(new), _f64(end)] + [_f64(l) for l in links])
    return float(np.dot(a, w))


def feasible(assign, split):
    """every flow constraint of the chain program holds, all values are 0 / 1"""
    split = [int(n) for n in split]
    det, links, new, end = assign
    det, new, end = (np.asarray(x, np.float64).reshape(-1) for x in (det, new, end))
    links = [np.asarray(l, np.float64).reshape(split[t], split[t + 1]) for t, l in enumerate(links)]
    if len(links) != len(split) - 1 or det.size != sum(split):
        return False
    if not all(np.all((x == 0) | (x == 1)) for x in [det, new, end] + links):
        return False
    st = np.concatenate([[0], np.cumsum(split)])
    for t in range(len(split)):
        d = slice(st[t], st[t + 1])
        out = links[t].sum(1) if t < len(split) - 1 else 0.0
        inn = links[t - 1].sum(0) if t > 0 else 0.0
        if not (np.all(end[d] + out == det[d]) and np.all(new[d] + inn == det[d])):
            return False
    return True


def same_assignment(a, b):
    return all(np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1))
               for x, y in zip([a[0], a[2], a[3]] + list(a[1]), [b[0], b[2], b[3]] + list(b[1])))


def random_chain(rng, split, scale=1.0, kind='normal'):
    """(det L, new L, end L, [link n_t x n_{t+1} ...]) fp32, the kinds of association_ref.random_instance carried over
    to chains: 'eval' zeroes new in the first frame and end in the last (what the eval forward hands over), 'masked'
    sets det = -1 on 30 % of the detections (the neg_threshold mask)."""
    split = [int(n) for n in split]
    L = sum(split)
    f = lambda *s: (rng.standard_normal(s) * scale).astype(np.float32)
    det, new, end = f(L), f(L), f(L)
    links = [f(split[t], split[t + 1]) for t in range(len(split) - 1)]
    if kind == 'eval':
        new[:split[0]] = 0
        end[L - split[-1]:] = 0
    elif kind == 'masked':
        det[rng.random(L) < 0.3] = -1
    else:
        assert kind == 'normal', kind
    return det, new, end, links
