"""NumPy restatement of the track smoothing of DESIGN.md section 12b (mmmot_smooth_tracks), written from the text:
float64 scalars, every product, sum and quotient rounded on its own in the stated order, one rounding to fp32 at the end.
Python / NumPy float64 scalar arithmetic never fuses a multiply with an add and divides with correct rounding, so the
bits are those of the stated order."""
import numpy as np

from fill_ref import ECONTRACT, EDUP, affine, wrap

f64 = np.float64
PI, TWO_PI, HALF_PI = f64(3.141592653589793), f64(6.283185307179586), f64(1.5707963267948966)
WRAP_STEPS = 4096
PARAMS = ('q_loc', 'r_loc', 'v0_loc', 'q_yaw', 'r_yaw', 'v0_yaw', 'q_dim', 'r_dim')
DEFAULT = dict(q_loc=0.01, r_loc=0.04, v0_loc=1.0, q_yaw=0.001, r_yaw=0.01, v0_yaw=0.04, q_dim=0.0, r_dim=0.01,
               yaw_flip=False)


def predict(p, v, P00, P01, P11, d, q):
    """the prediction lines of the constant-velocity filter: (pp, vp, A, B, C, t1, t2)"""
    d2 = d * d
    d3 = d2 * d
    q00 = q * (d3 / f64(3.0))
    q01 = q * (d2 / f64(2.0))
    q11 = q * d
    t1 = d * P01
    t2 = d * P11
    pp = p + d * v
    A = (((P00 + t1) + t1) + d * t2) + q00
    B = (P01 + t2) + q01
    C = P11 + q11
    return pp, v, A, B, C, t1, t2


def smooth_cv(z, obs, d, q, r, v0):
    """z[k] (read where obs[k]), d[k] = no[k] - no[k-1] (d[0] unused) -> smoothed (ps[k], vs[k])"""
    q, r = f64(q), f64(r)
    m = len(z)
    filt = []
    p, v, P00, P01, P11 = f64(z[0]), f64(0.0), r, f64(0.0), f64(v0)
    filt.append((p, v, P00, P01, P11))
    for k in range(1, m):
        pp, vp, A, B, C, _, _ = predict(p, v, P00, P01, P11, f64(d[k]), q)
        if obs[k]:
            s = A + r
            k0 = A / s
            k1 = B / s
            e = f64(z[k]) - pp
            p = pp + k0 * e
            v = vp + k1 * e
            P00 = A - k0 * A
            P01 = B - k0 * B
            P11 = C - k1 * B
        else:
            p, v, P00, P01, P11 = pp, vp, A, B, C
        filt.append((p, v, P00, P01, P11))
    ps, vs = [None] * m, [None] * m
    ps[m - 1], vs[m - 1] = filt[m - 1][0], filt[m - 1][1]
    for k in range(m - 2, -1, -1):
        p, v, P00, P01, P11 = filt[k]
        pp, vp, A, B, C, t1, t2 = predict(p, v, P00, P01, P11, f64(d[k + 1]), q)
        c00 = P00 + t1
        c10 = P01 + t2
        det = A * C - B * B
        g00 = (c00 * C - P01 * B) / det
        g01 = (P01 * A - c00 * B) / det
        g10 = (c10 * C - P11 * B) / det
        g11 = (P11 * A - c10 * B) / det
        ep = ps[k + 1] - pp
        ev = vs[k + 1] - vp
        ps[k] = p + (g00 * ep + g01 * ev)
        vs[k] = v + (g10 * ep + g11 * ev)
    return ps, vs


def smooth_walk(z, obs, d, q, r):
    """the one-state random walk of h, w, l -> smoothed ps[k]"""
    q, r = f64(q), f64(r)
    m = len(z)
    p, P = f64(z[0]), r
    filt = [(p, P)]
    for k in range(1, m):
        A = P + q * f64(d[k])
        if obs[k]:
            s = A + r
            k0 = A / s
            p = p + k0 * (f64(z[k]) - p)
            P = A - k0 * A
        else:
            P = A
        filt.append((p, P))
    ps = [None] * m
    ps[m - 1] = filt[m - 1][0]
    for k in range(m - 2, -1, -1):
        p, P = filt[k]
        A = P + q * f64(d[k + 1])
        g = P / A
        ps[k] = p + g * (ps[k + 1] - p)
    return ps


def unwrap(y, obs, yaw_flip):
    """the yaw measurement u[k] at the observed rows (elsewhere None)"""
    u, prev = [None] * len(y), None
    for k in range(len(y)):
        if not obs[k]:
            continue
        if prev is None:
            u[k] = f64(y[k])
        else:
            w = wrap(f64(y[k]) - f64(y[prev]))
            if yaw_flip and (w > HALF_PI or w < -HALF_PI):
                w = wrap(w + PI)
            u[k] = u[prev] + w
        prev = k
    return u


def wrap_loop(y):
    for _ in range(WRAP_STEPS):
        if not y >= PI:
            break
        y = y - TWO_PI
    for _ in range(WRAP_STEPS):
        if not y < -PI:
            break
        y = y + TWO_PI
    return y


def smooth(det, ids, frame_start, frame_no, seq_start, observed=None, xf0=None, **params):
    """-> dict(out fp32 [L, 12], vel fp32 [L, 4], info int32 [S, 4]); xf0: [F, REC] or None; params: PARAMS + yaw_flip"""
    prm = dict(DEFAULT, **params)
    det = np.asarray(det, np.float32).reshape(-1, 12)
    ids = np.asarray(ids).reshape(-1)
    fs, no, ss = (np.asarray(v).astype(np.int64).reshape(-1) for v in (frame_start, frame_no, seq_start))
    L, F, S = len(ids), len(no), len(ss) - 1
    obs_all = np.ones(L, bool) if observed is None else np.asarray(observed).reshape(-1) != 0
    out, vel, info = det.copy(), np.zeros((L, 4), np.float32), np.zeros((S, 4), np.int32)
    shape_ok = lambda t, n: t[0] == 0 and t[-1] == n and (np.diff(t) >= 0).all()
    if not (shape_ok(ss, F) and shape_ok(fs, L)):
        info[:, 0] = ECONTRACT
        return dict(out=out, vel=vel, info=info)
    r_loc, r_yaw, r_dim = (f64(prm[k]) for k in ('r_loc', 'r_yaw', 'r_dim'))
    any_r = r_loc > 0 or r_yaw > 0 or r_dim > 0
    for s in range(S):
        b, e = int(ss[s]), int(ss[s + 1])
        rows = int(fs[e] - fs[b])
        status = 0
        if any(no[p] >= no[p + 1] for p in range(b, e - 1)):
            status |= ECONTRACT
        tracks = {}
        for p in range(b, e):
            kept = ids[fs[p]:fs[p + 1]]
            kept = kept[kept >= 0]
            if len(np.unique(kept)) != len(kept):
                status |= EDUP
            for i in range(int(fs[p]), int(fs[p + 1])):
                if ids[i] >= 0:
                    tracks.setdefault(int(ids[i]), []).append((p, i))
        if status:
            info[s] = (status, 0, 0, rows)
            continue
        changed = 0
        for tid, chain in tracks.items():
            first = next((k for k, (_, i) in enumerate(chain) if obs_all[i]), None)
            if first is None:
                continue
            chain = chain[first:]
            if len(chain) < 2 or not any_r:
                continue
            info[s, 1] += 1
            changed += len(chain)
            obs = [bool(obs_all[i]) for _, i in chain]
            d = [0] + [int(no[chain[k][0]] - no[chain[k - 1][0]]) for k in range(1, len(chain))]
            rec = [None if xf0 is None else np.asarray(xf0[p], np.float64) for p, _ in chain]
            row = [det[i].astype(np.float64) for _, i in chain]
            if r_loc > 0:
                z = [(a[7], a[8], a[9]) if m is None else affine(a[7], a[8], a[9], m[0:16]) for a, m in zip(row, rec)]
                sm = [smooth_cv([zz[j] for zz in z], obs, d, prm['q_loc'], r_loc, prm['v0_loc']) for j in range(3)]
                for k, (p, i) in enumerate(chain):
                    x, y, zz = (sm[j][0][k] for j in range(3))
                    vx, vy, vz = (sm[j][1][k] for j in range(3))
                    if rec[k] is not None:
                        M = rec[k][16:32]
                        x, y, zz = affine(x, y, zz, M)
                        vx, vy, vz = [(vx * M[0 + j] + vy * M[4 + j]) + vz * M[8 + j] for j in range(3)]
                    out[i, 7:10] = np.asarray([x, y, zz], np.float64).astype(np.float32)
                    vel[i, 0:3] = np.asarray([vx, vy, vz], np.float64).astype(np.float32)
            if r_yaw > 0:
                y = [a[10] if m is None else a[10] + m[32] for a, m in zip(row, rec)]
                ps, vs = smooth_cv(unwrap(y, obs, bool(prm['yaw_flip'])), obs, d, prm['q_yaw'], r_yaw, prm['v0_yaw'])
                for k, (p, i) in enumerate(chain):
                    yy = ps[k] if rec[k] is None else ps[k] - rec[k][32]
                    out[i, 10] = np.float32(wrap_loop(yy))
                    vel[i, 3] = np.float32(vs[k])
            if r_dim > 0:
                for c in (4, 5, 6):
                    ps = smooth_walk([a[c] for a in row], obs, d, prm['q_dim'], r_dim)
                    for k, (p, i) in enumerate(chain):
                        out[i, c] = np.float32(ps[k])
        info[s, 2], info[s, 3] = changed, rows - changed
    return dict(out=out, vel=vel, info=info)


def block_of(res, sizes):
    """the restatement's result as the int32 block mmmot::smooth_tracks returns for ``sizes``, so that it can stand in
    for the launches in front of ``tracks.unpack_smooth``"""
    from mmmot_amd import torch_ops
    lay, n = torch_ops.smooth_layout(sizes)[1::2]
    block = np.zeros(n, np.int32)
    for name in ('out', 'vel', 'info'):
        v = np.ascontiguousarray(res[name]).reshape(-1).view(np.int32)
        block[lay[name][0]:lay[name][0] + len(v)] = v
    return block
