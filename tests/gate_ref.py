"""NumPy float64 restatement of the motion gate ("Sequences: motion gate"; mmmot_gate_links in
include/mmmot_hip.h), operation by operation: every product and sum below is one NumPy operation and so rounded on its
own, in the kernel's order.  ``gate`` takes the tables of the entry and returns (out_link or None, kept)."""
import numpy as np

REC = 33
MAX_DT = 64
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]


def tables(max_speed, slack, max_dt):
    """(r2, inv_r2) [max_dt + 1] as the host makes them: r2[dt] = (max_speed * dt + slack)^2, inv_r2[0] = 0"""
    r = np.float64(max_speed) * np.arange(max_dt + 1, dtype=np.float64) + np.float64(slack)
    r2 = r * r
    inv = np.zeros_like(r2)
    inv[1:] = np.float64(1.0) / r2[1:]
    return r2, inv


def moved(loc, C):
    """rows (x, y, z, 1) x C, columns 0..2: ((x*C0j + y*C1j) + z*C2j) + C3j; ``C`` the 16 words of a record"""
    x, y, z = (loc[:, i].astype(np.float64) for i in range(3))
    out = np.empty((len(loc), 3), np.float64)
    for j in range(3):
        s = x * C[0 + j] + y * C[4 + j]
        s = s + z * C[8 + j]
        out[:, j] = s + C[12 + j]
    return out


def size_ok(a, b, ratio):
    """max(a, b) <= ratio * min(a, b) with max / min by a > b, so that a NaN on either side fails"""
    gt = a > b
    hi, lo = np.where(gt, a, b).astype(np.float64), np.where(gt, b, a).astype(np.float64)
    return hi <= np.float64(ratio) * lo


def broken(blk, frame_start, frame_no, L, F, rec_gaps, n_link, moving):
    a, b, off = (int(v) for v in blk[:3])
    if a < 0 or b >= F or a >= b or off < 0 or (moving and b - a > rec_gaps):
        return True
    a0, a1, b0, b1 = (int(frame_start[i]) for i in (a, a + 1, b, b + 1))
    if a0 < 0 or a1 < a0 or a1 > L or b0 < 0 or b1 < b0 or b1 > L or int(frame_no[b]) - int(frame_no[a]) <= 0:
        return True
    return off + (a1 - a0) * (b1 - b0) > n_link


def gate(det, frame_start, frame_no, blocks, xf, r2, inv_r2, link, mode=0, max_dt=8, max_size_ratio=0.0, weight=0.0,
         n_link=None):
    """``link`` None: count only.  Returns (out_link - a copy of ``link`` with the blocks' words rewritten - or None,
    kept int32 [NB])."""
    det = np.asarray(det, np.float32).reshape(-1, 12)
    blocks = np.asarray(blocks, np.int64).reshape(-1, 4)
    L, F = len(det), len(frame_no)
    n_link = (0 if link is None else len(link)) if n_link is None else n_link
    rec_gaps = 0 if xf is None else xf.shape[1]
    out = None if link is None else np.array(link, np.float32, copy=True)
    kept = np.zeros(len(blocks), np.int32)
    with np.errstate(invalid='ignore', over='ignore'):
        for i, blk in enumerate(blocks):
            if broken(blk, frame_start, frame_no, L, F, rec_gaps, n_link, xf is not None):
                kept[i] = -1
                continue
            a, b, off = (int(v) for v in blk[:3])
            A, B = det[frame_start[a]:frame_start[a + 1]], det[frame_start[b]:frame_start[b + 1]]
            dt = int(frame_no[b]) - int(frame_no[a])
            rr, inv = (r2[dt], inv_r2[dt]) if dt <= max_dt else (np.float64('nan'), np.float64(0.0))
            pb = B[:, 7:10].astype(np.float64) if xf is None else moved(B[:, 7:10], xf[a, b - a - 1, 0:16])
            d = A[:, None, 7:10].astype(np.float64) - pb[None, :, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 2] * d[..., 2]
            if mode == 1:
                d2 = d2 + d[..., 1] * d[..., 1]
            ok = d2 <= rr
            if max_size_ratio > 0:
                for c in (4, 5, 6):
                    ok = ok & size_ok(A[:, None, c], B[None, :, c], max_size_ratio)
            if out is None:
                kept[i] = ok.sum()
                continue
            s = out[off:off + ok.size].reshape(ok.shape)  # a view: written in place
            live = ok & ~np.isnan(s)
            kept[i] = live.sum()
            if weight > 0:
                v = (s.astype(np.float64) - np.float64(weight) * (d2 * inv)).astype(np.float32)
                s[live] = v[live]
            s[~ok] = QNAN
    return out, kept
