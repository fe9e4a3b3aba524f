"""NumPy restatement of the gap filling of DESIGN.md section 12a (mmmot_fill_tracks), written from the text: float64
scalars, every product and sum rounded on its own, sums in the stated order, one rounding to fp32 at the end.  Python /
NumPy float64 scalar arithmetic never fuses a multiply with an add, so the bits are those of the stated order."""
import numpy as np

FILL_MAX, REC, WT = 30, 33, 32
EDUP, ECAPACITY, ECONTRACT = 1, 2, 4
PI, TWO_PI = np.float64(3.141592653589793), np.float64(6.283185307179586)


def weights():
    """wtab[n][k] = k / n in fp64 (row 0 unused)"""
    w = np.zeros((WT, WT), np.float64)
    for n in range(1, WT):
        for k in range(WT):
            w[n, k] = np.float64(k) / np.float64(n)
    return w


def wrap(d):
    """into [-pi, pi) by at most four compare-and-add / subtract steps of 2 pi"""
    d = np.float64(d)
    for _ in range(4):
        if d >= PI:
            d = d - TWO_PI
        elif d < -PI:
            d = d + TWO_PI
    return d


def affine(x, y, z, M):
    """(x, y, z, 1) times the row-major 4x4 M (16 doubles), columns 0..2, summed in k order"""
    r = []
    for j in range(3):
        s = x * M[0 + j] + y * M[4 + j]
        s = s + z * M[8 + j]
        r.append(s + M[12 + j])
    return r


def blend(a, b, w):
    return (np.float64(1.0) - w) * a + w * b


def blend_row(a, b, w, rec_b=None, rec_p=None):
    """One new row [12] fp32 from the fp32 rows a (earlier) and b (later) at weight w (fp64).  rec_b: the record
    C[pa<-pb] | inv | dyaw that brings b into a's coordinates, rec_p: the record of (pa, hole frame); both None for a
    standing camera."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    w = np.float64(w)
    out = np.zeros(12, np.float64)
    for v in (0, 1, 2, 3, 4, 5, 6, 11):
        out[v] = blend(a64[v], b64[v], w)
    bx, by, bz = b64[7], b64[8], b64[9]
    dyb = dyp = np.float64(0.0)
    if rec_b is not None:
        bx, by, bz = affine(bx, by, bz, rec_b[0:16])
        dyb, dyp = np.float64(rec_b[32]), np.float64(rec_p[32])
    x, y, z = blend(a64[7], bx, w), blend(a64[8], by, w), blend(a64[9], bz, w)
    if rec_p is not None:
        x, y, z = affine(x, y, z, rec_p[16:32])
    out[7], out[8], out[9] = x, y, z
    ya = a64[10]
    yb = b64[10] + dyb
    d = wrap(yb - ya)
    yy = ya + w * d
    out[10] = wrap(yy - dyp)
    return out.astype(np.float32)


def fill(det, ids, frame_start, frame_no, seq_start, xf, wtab, max_fill, capacity):
    """-> dict(fill_start int32 [F+1], out fp32 [n, 12], out_id int32 [n], out_src int32 [n, 2], info int32 [S, 4]) with
    n = min(rows, capacity) the rows a call writes; xf: [F, max_fill + 1, REC] or None."""
    det = np.asarray(det, np.float32).reshape(-1, 12)
    ids = np.asarray(ids).reshape(-1)
    fs, no, ss = (np.asarray(v).astype(np.int64).reshape(-1) for v in (frame_start, frame_no, seq_start))
    L, F, S = len(ids), len(no), len(ss) - 1
    info = np.zeros((S, 4), np.int32)
    per_frame = [[] for _ in range(F)]
    shape_ok = lambda t, n: t[0] == 0 and t[-1] == n and (np.diff(t) >= 0).all()
    if not (shape_ok(ss, F) and shape_ok(fs, L)):
        info[:, 0] = ECONTRACT
        return dict(fill_start=np.zeros(F + 1, np.int32), out=np.zeros((0, 12), np.float32), out_id=np.zeros(0, np.int32),
                    out_src=np.zeros((0, 2), np.int32), info=info)
    for s in range(S):
        b, e = int(ss[s]), int(ss[s + 1])
        status = 0
        if any(no[p] >= no[p + 1] for p in range(b, e - 1)):
            status |= ECONTRACT
        for p in range(b, e):
            kept = ids[fs[p]:fs[p + 1]]
            kept = kept[kept >= 0]
            if len(np.unique(kept)) != len(kept):
                status |= EDUP
        info[s, 0] = status
        if status:
            continue
        last = {}
        for p in range(b, e):
            for i in range(int(fs[p]), int(fs[p + 1])):
                tid = int(ids[i])
                if tid < 0:
                    continue
                if tid in last:
                    pa, ia = last[tid]
                    n = int(no[p] - no[pa])
                    if 2 <= n <= max_fill + 1:
                        info[s, 2] += 1
                        for q in range(pa + 1, p):
                            per_frame[q].append((tid, ia, i, pa, p))
                    elif n > max_fill + 1:
                        info[s, 3] += 1
                last[tid] = (p, i)
    fill_start = np.zeros(F + 1, np.int64)
    fill_start[1:] = np.cumsum([len(r) for r in per_frame])
    for s in range(S):
        if info[s, 0] == 0:
            info[s, 1] = fill_start[ss[s + 1]] - fill_start[ss[s]]
            if info[s, 1] > 0 and fill_start[ss[s + 1]] > capacity:
                info[s, 0] = ECAPACITY
    n_out = int(min(fill_start[-1], capacity))
    out = np.zeros((n_out, 12), np.float32)
    out_id, out_src = np.zeros(n_out, np.int32), np.zeros((n_out, 2), np.int32)
    for p in range(F):
        for rank, (tid, ia, ib, pa, pb) in enumerate(sorted(per_frame[p])):
            r = int(fill_start[p]) + rank
            if r >= capacity:
                continue
            n, k = int(no[pb] - no[pa]), int(no[p] - no[pa])
            rec_b = rec_p = None
            if xf is not None:
                rec_b, rec_p = xf[pa, pb - pa - 1], xf[pa, p - pa - 1]
            out[r] = blend_row(det[ia], det[ib], wtab[n, k], rec_b, rec_p)
            out_id[r], out_src[r] = tid, (ia, ib)
    return dict(fill_start=fill_start.astype(np.int32), out=out, out_id=out_id, out_src=out_src, info=info)


def block_of(res, sizes):
    """the restatement's result as the int32 block mmmot::fill_tracks returns for ``sizes`` (rows that a call leaves
    unwritten are zero), so that it can stand in for the launches in front of ``tracks.unpack_fill``"""
    from mmmot_amd import torch_ops
    lay, n = torch_ops.fill_layout(sizes)[1::2]
    block = np.zeros(n, np.int32)
    for name in ('out', 'out_id', 'out_src', 'fill_start', 'info'):
        v = np.ascontiguousarray(res[name]).reshape(-1).view(np.int32)
        block[lay[name][0]:lay[name][0] + len(v)] = v
    return block
