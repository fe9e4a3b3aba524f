"""The tracker's ID bookkeeping (reference tracking_model.py assign_det_id + align_id) restated by detection index in
plain numpy - the host oracle of the tests.  Serial loops on purpose: nothing here is shared with mmmot_amd.tracks or
csrc/track_ids.hip, and tests/golden/track_ids_*.npz (made by the reference itself) arbitrate."""
import numpy as np


class Tracker:
    def __init__(self):
        self.last_id = 0
        self.stored = None       # frame index of the stored frame
        self.stored_ids = None   # its per-detection IDs, -1 where the detection was not kept

    def pair(self, det, link, new, N, M, f0, f1):
        """One pair's assignment (det [N + M], link [N, M], new [N + M], 0 / 1) -> (ids0 [N], ids1 [M], frame_start);
        -1 marks a rejected detection.  Raises on an assignment no solver returns."""
        det, new = np.asarray(det).reshape(-1), np.asarray(new).reshape(-1)
        link = np.asarray(link).reshape(N, M)
        same = self.stored is not None and self.stored == f0
        nxt = 0 if self.stored is None else self.last_id + 1
        ids0 = np.full(N, -1, np.int64)
        for i in range(N):
            if det[i] != 1:
                continue
            if same and self.stored_ids[i] >= 0:
                ids0[i] = self.stored_ids[i]
            else:
                ids0[i] = nxt
                nxt += 1
        ids1 = np.full(M, -1, np.int64)
        for j in range(M):
            if det[N + j] != 1:
                continue
            if new[N + j] == 1:
                ids1[j] = nxt
                nxt += 1
            else:
                rows = np.flatnonzero(link[:, j] == 1)
                if len(rows) != 1 or ids0[rows[0]] < 0:
                    raise ValueError('infeasible assignment at column %d' % j)
                ids1[j] = ids0[rows[0]]
        if self.stored is None:
            self.last_id = max(self.last_id, nxt - 1)
        else:
            self.last_id = nxt - 1
        if not same or (ids1 >= 0).any():
            self.stored, self.stored_ids = f1, ids1.copy()
        return ids0, ids1, int(same)


def tracks_of(assignments, counts, frame_idx=None):
    """Per-frame IDs of a gapless sequence from its pairs' assignments [(det, link, new), ...] (pair t-1 joins frames
    t-1 and t): a list of int64 [n_t]; the last emission of a frame stands (a frame whose pair kept nothing is emitted
    again by the next pair)."""
    tr = Tracker()
    tracks = [np.full(n, -1, np.int64) for n in counts]
    for p, (det, link, new) in enumerate(assignments):
        f0, f1 = (p, p + 1) if frame_idx is None else frame_idx[p]
        ids0, ids1, start = tr.pair(det, link, new, counts[p], counts[p + 1], f0, f1)
        if not start:
            tracks[p] = ids0
        tracks[p + 1] = ids1
    return tracks


def load_fixture(path):
    """One tests/golden/track_ids_*.npz (tools/gen_golden_tracks.py) -> per pair a dict: N, M, f0, f1, the assignment
    (det, link [N, M], new, end) and the reference's result: emitted (the kept IDs of the emitted frames: two arrays,
    or one when frame_start = 1), frame_start, last_id.  Also the raw file."""
    z = np.load(path)
    pairs, bo, eo = [], 0, 0
    for p in range(len(z['N'])):
        N, M = int(z['N'][p]), int(z['M'][p])
        L = N + M
        blk = z['blocks'][bo:bo + 3 * L + N * M].astype(np.float32)
        bo += 3 * L + N * M
        emitted = []
        for n in z['emit_len'][p]:
            if n >= 0:
                emitted.append(z['emit_ids'][eo:eo + n])
                eo += n
        pairs.append({'N': N, 'M': M, 'f0': int(z['frame_idx'][p, 0]), 'f1': int(z['frame_idx'][p, 1]), 'block': blk,
                      'det': blk[:L], 'new': blk[L:2 * L], 'end': blk[2 * L:3 * L], 'link': blk[3 * L:].reshape(N, M),
                      'emitted': emitted, 'frame_start': int(z['frame_start'][p]), 'last_id': int(z['last_id'][p])})
    assert bo == len(z['blocks']) and eo == len(z['emit_ids'])
    return pairs, z


def check_pair(pair, ids0, ids1, frame_start, last_id):
    """a pair's per-detection IDs against what the reference emitted for it (exact)"""
    ids0, ids1 = np.asarray(ids0), np.asarray(ids1)
    N, M = pair['N'], pair['M']
    assert ids0.shape == (N,) and ids1.shape == (M,)
    assert np.array_equal(ids0 >= 0, pair['det'][:N] == 1) and np.array_equal(ids1 >= 0, pair['det'][N:] == 1)
    assert frame_start == pair['frame_start'] and last_id == pair['last_id'], (frame_start, last_id, pair['last_id'])
    got = [ids1[ids1 >= 0]] if frame_start else [ids0[ids0 >= 0], ids1[ids1 >= 0]]
    assert len(got) == len(pair['emitted'])
    for g, w in zip(got, pair['emitted']):
        assert np.array_equal(g, w), (g, w)
