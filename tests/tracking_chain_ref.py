"""The tracker's ID bookkeeping on WINDOWS of 2 .. 8 frames (reference tracking_model.py assign_det_id + align_id, which
are written for len(det_split) frames) restated by detection index in plain numpy - the host oracle of the window tests.
Serial loops on purpose: nothing here is shared with mmmot_amd.tracks or csrc/track_ids.hip, and
tests/golden/track_chain_ids_*.npz (made by the reference itself, tools/gen_golden_track_chains.py) arbitrate."""
import numpy as np


class ChainTracker:
    def __init__(self):
        self.last_id = 0
        self.stored = None       # frame index of the stored frame
        self.stored_ids = None   # its per-detection IDs, -1 where the detection was not kept

    def window(self, det, links, new, split, frame_idx):
        """One window's assignment (det [L], links [n_t x n_{t+1} ...], new [L], 0 / 1) -> (ids: T arrays, frame_start,
        stored); -1 marks a rejected detection.  Raises on an assignment no solver returns.  ``stored`` = 0 is the
        reference's quirk: the first frame was the stored one and frame 1 keeps nothing, so the state keeps its frame
        (only last_id moves) and the window's frames never reach the tracks."""
        split = [int(n) for n in split]
        T = len(split)
        assert 2 <= T <= 8 and len(frame_idx) == T and len(links) == T - 1
        det, new = np.asarray(det).reshape(-1), np.asarray(new).reshape(-1)
        st = np.concatenate([[0], np.cumsum(split)])
        same = self.stored is not None and self.stored == int(frame_idx[0])
        nxt = 0 if self.stored is None else self.last_id + 1
        ids = [np.full(split[0], -1, np.int64)]
        for i in range(split[0]):
            if det[i] != 1:
                continue
            if same and self.stored_ids[i] >= 0:
                ids[0][i] = self.stored_ids[i]
            else:
                ids[0][i] = nxt
                nxt += 1
        for t in range(1, T):
            link = np.asarray(links[t - 1]).reshape(split[t - 1], split[t])
            cur = np.full(split[t], -1, np.int64)
            for j in range(split[t]):
                g = st[t] + j
                if det[g] != 1:
                    continue
                if new[g] == 1:
                    cur[j] = nxt
                    nxt += 1
                else:
                    rows = np.flatnonzero(link[:, j] == 1)
                    if len(rows) != 1 or ids[-1][rows[0]] < 0:
                        raise ValueError('infeasible assignment at frame %d, column %d' % (t, j))
                    cur[j] = ids[-1][rows[0]]
            ids.append(cur)
        if self.stored is None:
            self.last_id = max(self.last_id, nxt - 1)
        else:
            self.last_id = nxt - 1
        stored = (not same) or bool((ids[1] >= 0).any())
        if stored:
            self.stored, self.stored_ids = int(frame_idx[-1]), ids[-1].copy()
        return ids, int(same), int(stored)


def tracks_of_windows(assignments, windows, counts):
    """Per-frame IDs of a sequence from its windows' assignments [(det, links, new), ...]; ``windows``: per window the
    positions of its frames in the sequence (they serve as frame indices), ``counts``: detections per frame.  A list of
    int64 [n_t]: frames ``frame_start ..`` of every STORED window, the last emission of a frame stands."""
    tr = ChainTracker()
    tracks = [np.full(n, -1, np.int64) for n in counts]
    for (det, links, new), fr in zip(assignments, windows):
        ids, start, stored = tr.window(det, links, new, [counts[f] for f in fr], fr)
        if stored:
            for f, i in list(zip(fr, ids))[start:]:
                tracks[f] = i
    return tracks


def load_fixture(path):
    """One tests/golden/track_chain_ids_*.npz -> per window a dict: T, split, frames, the assignment (block; det, new,
    end, links [n_t, n_{t+1}]) and the reference's result: emitted (the kept IDs of frames frame_start .. T-1),
    frame_start, last_id.  Also the raw file."""
    z = np.load(path)
    wins, bo, eo = [], 0, 0
    for w in range(len(z['chains'])):
        T = int(z['chains'][w, 0])
        split = [int(n) for n in z['chains'][w, 3:3 + T]]
        L = sum(split)
        K = sum(a * b for a, b in zip(split[:-1], split[1:]))
        blk = z['blocks'][bo:bo + 3 * L + K].astype(np.float32)
        bo += 3 * L + K
        links, o = [], 3 * L
        for a, b in zip(split[:-1], split[1:]):
            links.append(blk[o:o + a * b].reshape(a, b))
            o += a * b
        emitted = []
        for n in z['emit_len'][w, :T]:
            if n >= 0:
                emitted.append(z['emit_ids'][eo:eo + n])
                eo += n
        wins.append({'T': T, 'split': split, 'frames': [int(f) for f in z['frame_idx'][w, :T]], 'block': blk,
                     'det': blk[:L], 'new': blk[L:2 * L], 'end': blk[2 * L:3 * L], 'links': links, 'emitted': emitted,
                     'frame_start': int(z['frame_start'][w]), 'last_id': int(z['last_id'][w])})
    assert bo == len(z['blocks']) and eo == len(z['emit_ids'])
    return wins, z


def check_window(win, ids, frame_start, last_id):
    """a window's per-detection IDs against what the reference emitted for it (exact)"""
    split = win['split']
    st = np.concatenate([[0], np.cumsum(split)])
    assert len(ids) == win['T']
    for t, i in enumerate(ids):
        i = np.asarray(i)
        assert i.shape == (split[t],)
        assert np.array_equal(i >= 0, win['det'][st[t]:st[t + 1]] == 1), t
    assert frame_start == win['frame_start'] and last_id == win['last_id'], (frame_start, last_id, win['last_id'])
    got = [np.asarray(i)[np.asarray(i) >= 0] for i in ids[frame_start:]]
    assert len(got) == len(win['emitted'])
    for g, w in zip(got, win['emitted']):
        assert np.array_equal(g, w), (g, w)


def final_tracks(z):
    """the reference's final ``frames_id`` of a fixture: {frame index: kept IDs}, the last entry of a frame stands"""
    ref, o = {}, 0
    for f, n in zip(z['frames_id_frame'], z['frames_id_len']):
        ref[int(f)] = z['frames_id'][o:o + n]
        o += n
    return ref


def check_final(z, tracks):
    """``tracks``: {frame index: per-detection IDs} merged from the stored windows, against the final ``frames_id``"""
    ref = final_tracks(z)
    assert ref, 'the fixture holds no frames'
    for f, want in ref.items():
        got = np.asarray(tracks[f])
        assert np.array_equal(got[got >= 0], want), (f, got, want)
    for f, got in tracks.items():  # a frame the reference never stored holds no ID
        if f not in ref:
            assert not (np.asarray(got) >= 0).any(), f
