"""Host oracle of the frame-pair association (the two-frame program of ``ortools_solve``), two independent routes:

* ``milp_route``: the literal binary program - variables y_det / y_new / y_end per detection and y_link per pair, the
  flow constraints of the two frames, maximise the scored sum - solved by scipy.optimize.milp (HiGHS, mip_rel_gap = 0);
* ``lsa_route``: the maximum-weight matching it reduces to ("Frame-pair association"), in fp64 through
  scipy.optimize.linear_sum_assignment.

Both return (det L, link N x M, new L, end L) as float64 numpy 0 / 1 arrays and the objective.
"""
import numpy as np
from scipy.optimize import Bounds, LinearConstraint, linear_sum_assignment, milp


def _f64(*xs):
    return [np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1) for x in xs]


def milp_route(det, new, end, link, N, M):
    det, new, end, link = _f64(det, new, end, link)
    L = N + M
    # variable order: det [0, L), new [L, 2L), end [2L, 3L), link [3L, 3L + N M) row-major
    nv = 3 * L + N * M
    c = -np.concatenate([det, new, end, link])
    rows = []
    for i in range(N):  # frame 0: end_i + sum_j link_ij - det_i = 0, new_i - det_i = 0
        r = np.zeros(nv)
        r[2 * L + i] = 1
        r[3 * L + i * M:3 * L + (i + 1) * M] = 1
        r[i] = -1
        rows.append(r)
        r = np.zeros(nv)
        r[L + i] = 1
        r[i] = -1
        rows.append(r)
    for j in range(M):  # frame 1: new_j + sum_i link_ij - det_j = 0, end_j - det_j = 0
        d = N + j
        r = np.zeros(nv)
        r[L + d] = 1
        r[3 * L + j:3 * L + N * M:M] = 1
        r[d] = -1
        rows.append(r)
        r = np.zeros(nv)
        r[2 * L + d] = 1
        r[d] = -1
        rows.append(r)
    res = milp(c, constraints=LinearConstraint(np.array(rows), 0, 0), integrality=np.ones(nv), bounds=Bounds(0, 1),
               options={'mip_rel_gap': 0})
    assert res.status == 0, res.message
    x = np.round(res.x)
    return (x[0:L], x[3 * L:].reshape(N, M), x[L:2 * L], x[2 * L:3 * L]), float(np.dot(-c, x))


def gains(det, new, end, link, N, M):
    """(g [N, M], ua [N], vb [M]) in fp64 from the fp32 scores"""
    det, new, end, link = _f64(det, new, end, link)
    a = det[:N] + new[:N]
    ua = np.maximum(0.0, a + end[:N])
    b = det[N:] + end[N:]
    vb = np.maximum(0.0, b + new[N:])
    g = (link.reshape(N, M) + (a - ua)[:, None]) + (b - vb)[None, :]
    return g, ua, vb


def lsa_route(det, new, end, link, N, M):
    g, ua, vb = gains(det, new, end, link, N, M)
    r, c = linear_sum_assignment(-np.maximum(g, 0.0))
    keep = g[r, c] > 0
    r, c = r[keep], c[keep]
    L = N + M
    lk = np.zeros((N, M))
    lk[r, c] = 1
    m0, m1 = lk.sum(1) > 0, lk.sum(0) > 0
    x0, x1 = (ua > 0).astype(np.float64), (vb > 0).astype(np.float64)
    det_a = np.concatenate([np.where(m0, 1.0, x0), np.where(m1, 1.0, x1)])
    new_a = np.concatenate([np.where(m0, 1.0, x0), np.where(m1, 0.0, x1)])
    end_a = np.concatenate([np.where(m0, 0.0, x0), np.where(m1, 1.0, x1)])
    obj = float(ua.sum() + vb.sum() + g[r, c].sum())
    assert det_a.shape == (L,)
    return (det_a, lk, new_a, end_a), obj


def objective(assign, det, new, end, link):
    """the program's objective at an assignment (det, link, new, end)"""
    det, new, end, link = _f64(det, new, end, link)
    a = [np.asarray(x, dtype=np.float64).reshape(-1) for x in assign]
    return float(np.dot(a[0], det) + np.dot(a[1], link) + np.dot(a[2], new) + np.dot(a[3], end))


def feasible(assign, N, M):
    """every flow constraint of the two-frame program holds, all values are 0 / 1"""
    det, link, new, end = [np.asarray(x, dtype=np.float64) for x in assign]
    link = link.reshape(N, M)
    if not all(np.all((x == 0) | (x == 1)) for x in (det, link, new, end)):
        return False
    ok = np.all(end[:N] + link.sum(1) == det[:N]) and np.all(new[:N] == det[:N])
    ok = ok and np.all(new[N:] + link.sum(0) == det[N:]) and np.all(end[N:] == det[N:])
    return bool(ok)


def random_instance(rng, N, M, scale=1.0, kind='normal'):
    L = N + M
    f = lambda *s: (rng.standard_normal(s) * scale).astype(np.float32)
    det, new, end, link = f(L), f(L), f(L), f(N, M)
    if kind == 'eval':  # what the eval forward hands over: new[:N] = 0, end[N:] = 0
        new[:N] = 0
        end[N:] = 0
    elif kind == 'negative':  # every gain <= 0
        link = -np.abs(link) - 10 * scale
    elif kind == 'masked':  # det = -1 rows (the neg_threshold mask)
        det[rng.random(L) < 0.3] = -1
    return det, new, end, link
