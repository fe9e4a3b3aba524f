"""Track IDs on the device: the last step of the reference's ``TrackingModule.predict`` (tracking_model.py:77-81,
``assign_det_id`` then ``align_id``), which turns each pair's 0/1 assignment into IDs that stay stable over a sequence.

IDs are a chain over the pairs of a sequence (pair t needs the IDs pair t-1 gave frame t), so the step is one small
launch (csrc/track_ids.hip, one workgroup walking B pairs in order) queued behind the solve, with the sequence's state
(last ID, the stored frame and its per-detection IDs) in a device block that the launch updates in place:

    state = TrackState('cuda')
    ids_per_frame, frame_start = track_ids(state, assign_det, assign_link, assign_new, assign_end, det_split,
                                           (frame_a, frame_b))        # instead of assign_det_id + align_id

IDs are per DETECTION: ``ids[j] = -1`` where ``assign_det[j] != 1`` (the detection is in no track); the reference's
``frames_id`` entry of a frame, which lists kept detections only, is ``ids[ids >= 0]``.  ``frame_start = 1`` when the
pair's first frame was the stored one: only the second frame is emitted, as ``align_id`` returns it.

Two deliberate differences from the reference.  It recognises "the same detection of frame t in both pairs" by exact
equality of ``bbox`` (and ``location``), because its dataset prepares each frame twice; here a frame is prepared once and
identity is the detection index - the same whenever the boxes within a frame are distinct.  And where the reference
raises or stops in a debugger on an assignment no solver returns (a kept, non-new second-frame detection without
exactly one link from a kept row), the kernel writes -1, sets the state's error flag, and ``TrackingError`` is raised
when the result reaches the host.

Windows of 2 .. 8 frames (what ``association.associate_chain`` solves; the same kernel body on the chain table) go the
same way on the same state: ``track_chain_ids`` is the drop-in, ``queue_chain_ids`` / ``split_chain_ids`` / ``assign_chain_ids`` the
batched form, ``merge_chain_tracks`` the per-frame list, ``window_starts`` the schedule of a sequence's windows.  One
behaviour of the reference is kept: a window whose frame 0 continues the stored frame and whose frame 1 keeps nothing
is not stored (``stored`` = 0) - only ``last_id`` moves, and its frames are not part of the tracks.  The pair forms are
the two-frame readings of the window forms: ``split_ids`` of ``split_chain_ids``, ``merge_tracks`` of
``merge_chain_tracks`` (a pair has no ``stored`` word and is always written).

Many sequences: ``TrackStates(S)`` is a table of S states, ``queue_ids_multi`` / ``queue_chain_ids_multi`` number the
pairs / windows of several sequences in ONE launch (one workgroup per sequence, ``mmmot_track_ids_multi``), each group
named by ``stream_of``, and ``split_ids_multi`` reads the buffer back per group and names the sequence in its error.
"""
import numpy as np
import torch

from . import torch_ops
from .association import chain_block_size, chain_of, chains_table, pairs_table, split_of
from .torch_ops import TRACK_STATE_HEAD, TRACK_STATE_INTS

EINFEASIBLE, ECONTRACT = 1, 2
KITTI_NAMES = ('Car', 'Van', 'Truck', 'Pedestrian', 'Person', 'Cyclist', 'Tram', 'Misc')


class TrackingError(RuntimeError):
    pass


class TrackState:
    """The ID state of ONE sequence on the device: int32 [last_id, stored frame or -1, error flags, detections of the
    stored frame | its per-detection IDs x 512] (include/mmmot_hip.h, mmmot_track_ids)."""

    def __init__(self, device='cuda'):
        init = torch.full((TRACK_STATE_INTS,), -1, dtype=torch.int32)
        init[0] = init[2] = init[3] = 0
        self._init = init.to(device)
        self.buf = self._init.clone()

    def reset(self):
        """start a new sequence (the reference's ``clear_mem``); queued on the current stream"""
        self.buf.copy_(self._init)

    def snapshot(self):
        return self.buf.clone()

    def restore(self, snap):
        self.buf.copy_(snap)

    def read(self):
        """host view (waits for the stream): last_id, the stored frame (None: none) and its IDs, the error flags"""
        h = self.buf.cpu().numpy()
        n = int(h[3])
        return {'last_id': int(h[0]), 'frame': None if h[1] < 0 else int(h[1]), 'flags': int(h[2]),
                'ids': h[TRACK_STATE_HEAD:TRACK_STATE_HEAD + n].astype(np.int64)}


def check_flags(flags):
    if flags & EINFEASIBLE:
        raise TrackingError('track_ids: a kept second-frame detection with new != 1 has not exactly one link from a kept '
                            'detection of the first frame - not a solver output (tests/association_ref.feasible)')
    if flags & ECONTRACT:
        raise TrackingError('track_ids: the stored frame and the first frame of the next pair share a frame index but '
                            'not a detection count, or a pair lies outside the launch limits')


def frame_table(frame_idx, B):
    t = torch.as_tensor(np.asarray(frame_idx, dtype=np.int64).reshape(-1, 2), dtype=torch.int32)
    if t.shape[0] != B:
        raise ValueError('track_ids: %d frame index pairs for %d pairs' % (t.shape[0], B))
    return t


def queue_ids(state, blocks, splits, frame_idx, max_nm=0):
    """Queue the ID launch for B consecutive pairs of the state's sequence; nothing waits.  ``blocks``: the flat device
    output of mmmot::associate for ``splits``.  Returns the device int32 buffer [per pair: ids N | ids M | frame_start |
    last_id] with the state's error flags appended as the last element."""
    pairs, _ = pairs_table(splits)
    ids = torch.ops.mmmot.track_ids(blocks, pairs, frame_table(frame_idx, len(splits)), state.buf, int(max_nm))
    return torch.cat([ids, state.buf[2:3]])


def split_ids(flat, splits):
    """host int32 buffer of ``queue_ids`` -> per pair (ids0 [N], ids1 [M], frame_start, last_id), int64 arrays; raises
    ``TrackingError`` on the error flags"""
    return [(i[0], i[1], start, last) for i, start, last in split_chain_ids(flat, splits, tail=2)]


def assign_ids(state, blocks, splits, frame_idx, max_nm=0):
    """IDs of B consecutive pairs in one launch and one copy: per pair (ids0, ids1, frame_start, last_id)."""
    splits = [(int(N), int(M)) for N, M in splits]
    return split_ids(queue_ids(state, blocks, splits, frame_idx, max_nm).cpu().numpy(), splits)


def track_ids(state, assign_det, assign_link, assign_new, assign_end, det_split, frame_idx):
    """Drop-in for the reference's ``assign_det_id`` + ``align_id`` on one pair: takes what ``ortools_solve`` /
    ``association.associate`` returns (CPU or device tensors) and the frame indices of the pair's two frames.  Returns
    (ids_per_frame, frame_start): per EMITTED frame a CPU int64 tensor with one ID per detection (-1: rejected) - both
    frames, or the second only when frame_start = 1."""
    N, M = split_of(det_split)
    L = N + M
    link = assign_link[0]
    if assign_det.numel() != L or assign_new.numel() != L or assign_end.numel() != L or link.numel() != N * M:
        raise ValueError('track_ids: assignment does not match det_split [%d, %d]' % (N, M))
    block = torch.cat([t.detach().reshape(-1).to(torch.float32) for t in (assign_det, assign_new, assign_end, link)])
    ids0, ids1, start, _ = assign_ids(state, block.to(state.buf.device), [(N, M)], [frame_idx])[0]
    frames = [torch.from_numpy(ids1)] if start else [torch.from_numpy(ids0), torch.from_numpy(ids1)]
    return frames, start


def merge_tracks(tracks, t, ids0, ids1, frame_start, on_tracks=None):
    """pair (t-1, t) into the per-frame list: the last emission of a frame stands (a frame whose pair kept nothing is
    emitted again by the next pair, as the reference does).  A pair is always written: the two-frame, ``stored`` = 1
    call of ``merge_chain_tracks``"""
    merge_chain_tracks(tracks, (t - 1, t), (ids0, ids1), frame_start, 1, on_tracks)


# ---- windows of 2 .. 8 frames (a pair's IDs are read as the two-frame case, with two trailing words) -----------------
def window_starts(n_frames, window):
    """The window schedule as a pure function: [(first frame, frame count)] of the windows of a sequence of
    ``n_frames`` frames.  Windows of ``window`` frames start at 0, window - 1, 2 (window - 1), .. (neighbours share a
    frame); the last one is shorter (at least 2 frames) when the sequence does not divide."""
    n_frames, window = int(n_frames), int(window)
    if not 2 <= window <= torch_ops.CHAIN_MAX_T:
        raise ValueError('window must lie in 2 .. %d, got %d' % (torch_ops.CHAIN_MAX_T, window))
    return [(s, min(window, n_frames - s)) for s in range(0, n_frames - 1, window - 1)]


def chain_frame_table(frame_idx, splits):
    """CPU int32 [B, 8]: per window its T frame indices, padded with 0"""
    if len(frame_idx) != len(splits):
        raise ValueError('track_chain_ids: %d frame index rows for %d windows' % (len(frame_idx), len(splits)))
    t = np.zeros((len(splits), torch_ops.CHAIN_MAX_T), np.int32)
    for r, (f, s) in enumerate(zip(frame_idx, splits)):
        f = np.asarray(f, dtype=np.int64).reshape(-1)
        if len(f) != len(s):
            raise ValueError('track_chain_ids: window %d has %d frame indices for %d frames' % (r, len(f), len(s)))
        t[r, :len(f)] = f
    return torch.from_numpy(t)


def queue_chain_ids(state, blocks, splits, frame_idx, max_n=0):
    """Queue the ID launch for B consecutive windows of the state's sequence; nothing waits.  ``blocks``: the flat
    device output of mmmot::associate_chains for ``splits`` (per window [n_0 .. n_{T-1}]); ``frame_idx``: per window its
    T frame indices.  Returns the device int32 buffer [per window: ids L | frame_start | last_id | stored] with the
    state's error flags appended as the last element."""
    chains, _ = chains_table(splits)
    ids = torch.ops.mmmot.track_chain_ids(blocks, chains, chain_frame_table(frame_idx, splits), state.buf, int(max_n))
    return torch.cat([ids, state.buf[2:3]])


def split_chain_ids(flat, splits, tail=3):
    """host int32 buffer of ``queue_chain_ids`` -> per window (ids_per_frame: T int64 arrays, frame_start, last_id,
    stored); raises ``TrackingError`` on the error flags.  ``tail`` = 2: the buffer of ``queue_ids``, without ``stored``"""
    flat = np.asarray(flat)
    check_flags(int(flat[-1]))
    res, o = [], 0
    for split in splits:
        ids = []
        for n in split:
            ids.append(flat[o:o + n].astype(np.int64))
            o += n
        res.append((ids, *(int(w) for w in flat[o:o + tail])))
        o += tail
    return res


def assign_chain_ids(state, blocks, splits, frame_idx, max_n=0):
    """IDs of B consecutive windows in one launch and one copy: per window (ids_per_frame, frame_start, last_id,
    stored)."""
    splits = [[int(n) for n in s] for s in splits]
    return split_chain_ids(queue_chain_ids(state, blocks, splits, frame_idx, max_n).cpu().numpy(), splits)


def track_chain_ids(state, assign_det, assign_links, assign_new, assign_end, det_split, frame_idx):
    """Drop-in for the reference's ``assign_det_id`` + ``align_id`` on one window of ``len(det_split)`` = 2 .. 8 frames:
    takes what ``ortools_solve`` / ``association.associate_chain`` returns (CPU or device tensors) and the window's T
    frame indices.  Returns (ids_per_frame, frame_start): per EMITTED frame a CPU int64 tensor with one ID per detection
    (-1: rejected) - all T frames, or frames 1 .. T-1 when frame_start = 1.  As in the reference, a window with
    frame_start = 1 whose frame 1 keeps nothing does not enter the sequence's tracks (``assign_chain_ids`` reports it as
    ``stored`` = 0; ``merge_chain_tracks`` honours it)."""
    split = chain_of(det_split)
    L = sum(split)
    if assign_det.numel() != L or assign_new.numel() != L or assign_end.numel() != L or \
            len(assign_links) != len(split) - 1 or \
            any(l.numel() != a * b for l, a, b in zip(assign_links, split[:-1], split[1:])):
        raise ValueError('track_chain_ids: assignment does not match det_split %s' % (split,))
    block = torch.cat([t.detach().reshape(-1).to(torch.float32)
                       for t in (assign_det, assign_new, assign_end, *assign_links)])
    ids, start, _, _ = assign_chain_ids(state, block.to(state.buf.device), [split], [frame_idx])[0]
    return [torch.from_numpy(i) for i in ids[start:]], start


# ---- many sequences in one launch (mmmot_track_ids_multi / mmmot_track_chain_ids_multi) -----------------------------
class TrackStates:
    """The ID states of S sequences as ONE device table int32 [S, TRACK_STATE_INTS]; ``states[s]`` is the view of row s,
    usable wherever a ``TrackState.buf`` is (the single-state ops included)."""

    def __init__(self, S, device='cuda'):
        if int(S) < 1:
            raise ValueError('TrackStates: S >= 1 sequences, got %s' % (S,))
        init = torch.full((int(S), TRACK_STATE_INTS), -1, dtype=torch.int32)
        init[:, 0] = init[:, 2] = init[:, 3] = 0
        self._init = init.to(device)
        self.buf = self._init.clone()

    def __len__(self):
        return int(self.buf.shape[0])

    def __getitem__(self, s):
        return self.buf[int(s)]

    def _rows(self, streams):
        return torch.as_tensor(sorted(int(s) for s in streams), dtype=torch.long, device=self.buf.device)

    def reset(self, streams=None):
        """start new sequences: all of them, or the listed ones; queued on the current stream"""
        if streams is None:
            self.buf.copy_(self._init)
        elif len(streams):
            r = self._rows(streams)
            self.buf[r] = self._init[r]

    def snapshot(self):
        return self.buf.clone()

    def restore(self, snap, streams=None):
        """the whole table from ``snapshot()``, or the listed sequences' rows of it"""
        if streams is None:
            self.buf.copy_(snap)
        elif len(streams):
            r = self._rows(streams)
            self.buf[r] = snap[r]

    def read(self, s):
        """host view of sequence s (waits for the stream), as ``TrackState.read``"""
        h = self.buf[int(s)].cpu().numpy()
        n = int(h[3])
        return {'last_id': int(h[0]), 'frame': None if h[1] < 0 else int(h[1]), 'flags': int(h[2]),
                'ids': h[TRACK_STATE_HEAD:TRACK_STATE_HEAD + n].astype(np.int64)}


def stream_major(stream_of, S):
    """The host tables of a multi-state launch: (order, seq_start).  ``order``: int64 [B], the groups' indices sorted by
    stream, groups of one stream in the order given (stable); ``seq_start``: int32 [S + 1] with the groups of stream s
    at [seq_start[s], seq_start[s+1]) of that order - an empty range for a stream without groups."""
    so = np.asarray(stream_of, dtype=np.int64).reshape(-1)
    if so.size and (so.min() < 0 or so.max() >= int(S)):
        raise ValueError('stream_of names a stream outside [0, %d)' % int(S))
    order = np.argsort(so, kind='stable')
    seq_start = np.zeros(int(S) + 1, np.int32)
    np.cumsum(np.bincount(so, minlength=int(S)), out=seq_start[1:])
    return order, seq_start


def _reorder_blocks(blocks, sizes, order):
    """the solver blocks (``sizes`` fp32 each, one after the other) in the order ``order``: one gather on the device"""
    if np.array_equal(order, np.arange(len(order))):
        return blocks
    off = np.cumsum(sizes) - sizes
    idx = np.concatenate([np.arange(off[g], off[g] + sizes[g]) for g in order] + [np.zeros(0, np.int64)])
    return blocks[torch.from_numpy(idx.astype(np.int64)).to(blocks.device, non_blocking=True)]


def _queue_multi(op, table_of, frames_of, states, blocks, splits, frame_idx, stream_of, max_n):
    if len(stream_of) != len(splits):
        raise ValueError('%s: %d stream names for %d groups' % (op, len(stream_of), len(splits)))
    order, seq_start = stream_major(stream_of, len(states))
    splits = [splits[g] for g in order]
    sizes = np.asarray([chain_block_size(s) for s in splits], dtype=np.int64)
    inv = np.argsort(order)  # the blocks lie in the order given: block g goes to place inv[g]
    blocks = _reorder_blocks(blocks, sizes[inv], order)
    ids = getattr(torch.ops.mmmot, op)(blocks, table_of(splits)[0], frames_of([frame_idx[g] for g in order], splits),
                                       torch.from_numpy(seq_start), states.buf, int(max_n))
    return torch.cat([ids, states.buf[:, 2]])


def queue_ids_multi(states, blocks, splits, frame_idx, stream_of, max_nm=0):
    """Queue ONE ID launch for the pairs of several sequences; nothing waits.  ``states``: a TrackStates; ``blocks``,
    ``splits``, ``frame_idx`` as ``queue_ids`` takes them, in any order of the groups; ``stream_of[g]`` names the
    sequence of group g, whose groups must follow each other in the order of that sequence.  The groups are reordered
    to stream-major on the host (``stream_major``; the blocks follow in one device gather when the order changes).
    Returns the device int32 buffer [per pair in STREAM-MAJOR order: ids N | ids M | frame_start | last_id] with the
    error flags of all S sequences appended; ``split_ids_multi`` reads it back in the order given."""
    splits = [(int(N), int(M)) for N, M in splits]
    return _queue_multi('track_ids_multi', pairs_table, lambda f, s: frame_table(f, len(s)), states, blocks, splits,
                        frame_idx, stream_of, max_nm)


def queue_chain_ids_multi(states, blocks, splits, frame_idx, stream_of, max_n=0):
    """``queue_ids_multi`` for WINDOWS of 2 .. 8 frames (per window ids L | frame_start | last_id | stored)"""
    splits = [[int(n) for n in s] for s in splits]
    return _queue_multi('track_chain_ids_multi', chains_table, chain_frame_table, states, blocks, splits, frame_idx,
                        stream_of, max_n)


def split_ids_multi(flat, splits, stream_of, tail=2):
    """host int32 buffer of ``queue_ids_multi`` (``tail`` = 3: of ``queue_chain_ids_multi``) -> per group, in the order
    of ``splits`` / ``stream_of``, what ``split_ids`` (``split_chain_ids``) gives; raises ``TrackingError`` naming the
    sequence whose error flags are set"""
    flat = np.asarray(flat)
    splits = [[int(n) for n in s] for s in splits]
    n_ids = sum(sum(s) + tail for s in splits)
    S = flat.size - n_ids
    order, _ = stream_major(stream_of, S)
    for s in range(S):
        try:
            check_flags(int(flat[n_ids + s]))
        except TrackingError as e:
            raise TrackingError('stream %d: %s' % (s, e)) from None
    body = np.concatenate([flat[:n_ids], np.zeros(1, flat.dtype)])  # the flag word split_chain_ids checks: clean here
    major = split_chain_ids(body, [splits[g] for g in order], tail=tail)
    res = [None] * len(splits)
    for g, r in zip(order, major):
        res[g] = (r[0][0], r[0][1], r[1], r[2]) if tail == 2 else r
    return res


def merge_chain_tracks(tracks, frames, ids, frame_start, stored, on_tracks=None):
    """one window into the per-frame list: ``frames`` = the window's positions in ``tracks``, ``ids`` its per-frame IDs.
    Frames ``frame_start ..`` are written, and only when ``stored``; the last emission of a frame stands."""
    if not stored:
        return
    for t, i in list(zip(frames, ids))[int(frame_start):]:
        tracks[t] = i
        if on_tracks is not None:
            on_tracks(t, i)


def write_kitti_tracks(path, frames, ids, frame_idx=None, scores=None):
    """The reference's result file (utils/data_util.py:80-128 write_kitti_result + kitti_result_line) on the host:
    ``frames``: per frame the detection dict the pipeline holds (FrameFeed.dets: bbox [n, 4], dimensions [n, 3] lhw,
    location [n, 3], rotation_y [n]; optional name (KITTI class index or string), truncated, occluded, alpha, else the
    format's "unknown" values); ``ids``: per frame the per-detection IDs (pipe.tracks).  Kept detections only,
    dimensions lhw -> hwl, score 0.9, values at fp32 as the reference's tensors; ``frame_idx``: the frames' numbers
    (default 0, 1, ..); ``scores``: per frame the per-detection scores, written in place of the constant 0.9."""
    f4 = lambda v: '{:.4f}'.format(float(np.float32(v)))
    lines = []
    for t, (d, fid) in enumerate(zip(frames, ids)):
        frame = t if frame_idx is None else int(frame_idx[t])
        fid = np.asarray(fid)
        for j in np.flatnonzero(fid >= 0):
            name = d['name'][j] if 'name' in d else 0
            name = name if isinstance(name, str) else KITTI_NAMES[int(name)]
            dims = np.asarray(d['dimensions'][j])[[1, 2, 0]]
            row = [str(frame), str(int(fid[j])), name,
                   f4(d['truncated'][j]) if 'truncated' in d else '-1',
                   str(int(d['occluded'][j])) if 'occluded' in d else '-1',
                   f4(d['alpha'][j]) if 'alpha' in d else '-10']
            row += [f4(v) for v in np.asarray(d['bbox'][j]).reshape(-1)] + [f4(v) for v in dims]
            row += [f4(v) for v in np.asarray(d['location'][j]).reshape(-1)] + [f4(d['rotation_y'][j]),
                                                                                f4(0.9 if scores is None else scores[t][j])]
            lines.append(' '.join(row))
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


# ---- gap filling: a box for every listed frame a track skipped (csrc/fill_tracks.hip) -----------
FILL_KEYS = ('frames', 'ids', 'frame_idx', 'scores', 'poses', 'calib')
FILL_STATUS = ((torch_ops.FILL_EDUP, 'a track ID occurs twice in one frame'),
               (torch_ops.FILL_ECAPACITY, 'more rows than the capacity of the call'),
               (torch_ops.FILL_ECONTRACT, 'frame numbers that do not increase, or a broken frame / sequence table'))


class FilledTracks:
    """What ``fill_gaps`` returns for one sequence: ``frames[t]`` a copy of the frame's detection dict with the new rows
    appended, ``ids[t]`` / ``scores[t]`` (None when no scores were given) extended likewise, ``filled[t]`` the bool mask
    of the new rows, ``src[t]`` int64 [new rows, 4] = (frame, detection, frame, detection) of the two observations a row
    was blended from (positions in this sequence's lists), ``info`` = {'rows', 'links_filled', 'links_too_long'}."""

    def __init__(self, frames, ids, scores, filled, src, info):
        self.frames, self.ids, self.scores, self.filled, self.src, self.info = frames, ids, scores, filled, src, info


def fill_weights():
    """wtab[n][k] = k / n in fp64, n = 1 .. MMMOT_FILL_MAX + 1 (row 0 stays 0): the kernel and a host restatement read
    the same bits"""
    w = np.zeros((torch_ops.FILL_WT, torch_ops.FILL_WT), np.float64)
    k = np.arange(torch_ops.FILL_WT, dtype=np.float64)
    for n in range(1, torch_ops.FILL_WT):
        w[n] = k / np.float64(n)
    return w


def box_rows(d, m, scores=None):
    """fp32 [m, 12] rows of a frame's detection dict, the ``det`` layout of mmmot_fill_tracks and mmmot_gate_links: 2D
    box x1 y1 x2 y2, dimensions lhw -> h w l, location x y z (camera frame), rotation_y, score (0.9 without ``scores``,
    the constant ``write_kitti_tracks`` writes)"""
    row = np.empty((m, 12), np.float32)
    row[:, 0:4] = np.asarray(d['bbox'], dtype=np.float64).reshape(m, 4)
    row[:, 4:7] = np.asarray(d['dimensions'], dtype=np.float64).reshape(m, 3)[:, [1, 2, 0]]
    row[:, 7:10] = np.asarray(d['location'], dtype=np.float64).reshape(m, 3)
    row[:, 10] = np.asarray(d['rotation_y'], dtype=np.float64).reshape(m)
    row[:, 11] = 0.9 if scores is None else np.asarray(scores, dtype=np.float64).reshape(m)
    return row


def _fill_sequence(seq):
    if isinstance(seq, dict):
        unknown = set(seq) - set(FILL_KEYS)
        if unknown:
            raise ValueError('fill_gaps: unknown sequence entries %s' % sorted(unknown))
        return tuple(seq.get(k) for k in FILL_KEYS)
    seq = tuple(seq)
    if not 2 <= len(seq) <= len(FILL_KEYS):
        raise ValueError('fill_gaps: a sequence is a dict or a tuple of %s' % (FILL_KEYS,))
    return seq + (None,) * (len(FILL_KEYS) - len(seq))


def sequence_tables(seqs, what):
    """The tables of mmmot_fill_tracks / mmmot_smooth_tracks from normalised sequences (``_fill_sequence``): ({det fp32
    [L, 12], ids, frame_start, frame_no, seq_start}, per sequence its int64 frame numbers, per sequence whether it
    carries poses).  ``what`` names the caller in the errors."""
    if not seqs:
        raise ValueError('%s: no sequence' % what)
    det, ids, counts, frame_no, seq_start, moving = [], [], [], [], [0], []
    for s, (frames, fids, frame_idx, scores, poses, calib) in enumerate(seqs):
        n = len(frames)
        if len(fids) != n or (frame_idx is not None and len(frame_idx) != n) or (scores is not None and len(scores) != n):
            raise ValueError('%s: sequence %d has %d frames but ids / frame_idx / scores of another length' % (what, s, n))
        if poses is not None and (len(poses) != n or any(p is None for p in poses)):
            raise ValueError('%s: sequence %d: poses are given for all frames or none' % (what, s))
        if poses is not None and calib is None:
            raise ValueError('%s: sequence %d: poses need calib (R0_rect, Tr_velo_to_cam, Tr_imu_to_velo)' % (what, s))
        moving.append(poses is not None and n > 0)
        no = np.arange(n, dtype=np.int64) if frame_idx is None else np.asarray(frame_idx, dtype=np.int64).reshape(-1)
        if np.abs(no).max(initial=0) >= 2 ** 31:
            raise ValueError('%s: sequence %d: frame numbers must fit 32 bits' % (what, s))
        for t, (d, fid) in enumerate(zip(frames, fids)):
            fid = np.asarray(fid, dtype=np.int64).reshape(-1)
            det.append(box_rows(d, len(fid), None if scores is None else scores[t]))
            ids.append(fid)
            counts.append(len(fid))
        frame_no.append(no)
        seq_start.append(seq_start[-1] + n)
    tab = {'det': np.concatenate(det + [np.zeros((0, 12), np.float32)]),
           'ids': np.concatenate(ids + [np.zeros(0, np.int64)]).astype(np.int32),
           'frame_start': np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32),
           'frame_no': np.concatenate(frame_no + [np.zeros(0, np.int64)]).astype(np.int32),
           'seq_start': np.asarray(seq_start, np.int32)}
    return tab, frame_no, moving


def pack_fill(sequences, max_fill=7, capacity=None):
    """The host side of ``fill_gaps_batch`` before the launches: per sequence (frames, ids, frame_idx, scores, poses,
    calib) as ``fill_gaps`` takes them (a tuple, or a dict with those keys) -> the tables of mmmot_fill_tracks.  Returns a
    dict: ``packed`` (the int32 block of torch_ops.fill_layout), ``sizes``, the tables by name (``det`` fp32 [L, 12],
    ``ids``, ``frame_start``, ``frame_no``, ``seq_start``, ``xf`` fp64 [F, max_fill + 1, 33] or None when no sequence
    moves, ``wtab``) and ``sequences`` (the normalised inputs, for ``unpack_fill``).  ``capacity``: the rows the output
    holds; by default the exact count, walked on the host from the IDs.  A sequence with poses gets the records
    ``ego.box_motion`` of every pair of listed frames a filled link can join; in a call where only some sequences move
    the others get identity records, which give the standing-camera result."""
    from . import ego
    max_fill = int(max_fill)
    if not 1 <= max_fill <= torch_ops.FILL_MAX:
        raise ValueError('fill_gaps: max_fill must lie in 1 .. %d, got %d' % (torch_ops.FILL_MAX, max_fill))
    seqs = [_fill_sequence(s) for s in sequences]
    tab, frame_no, moving = sequence_tables(seqs, 'fill_gaps')
    tab.update(wtab=fill_weights(), xf=None)
    seq_start, F, S, rows = tab['seq_start'].tolist(), len(tab['frame_no']), len(seqs), 0
    for (frames, fids, _, _, _, _), no in zip(seqs, frame_no):
        last = {}
        for t, fid in enumerate(fids):
            fid = np.asarray(fid, dtype=np.int64).reshape(-1)
            for i in fid[fid >= 0]:
                a = last.get(int(i))
                if a is not None and 2 <= no[t] - no[a] <= max_fill + 1:
                    rows += t - a - 1
                last[int(i)] = t
    if any(moving):
        xf = np.zeros((F, max_fill + 1, torch_ops.FILL_REC), np.float64)
        xf[:, :, 0:16] = xf[:, :, 16:32] = np.eye(4).reshape(-1)
        for s, (frames, _, _, _, poses, calib) in enumerate(seqs):
            if not moving[s]:
                continue
            no, f0 = frame_no[s], seq_start[s]
            for p in range(len(frames)):
                for q in range(p + 1, min(p + max_fill + 2, len(frames))):
                    if no[q] - no[p] > max_fill + 1:  # no filled link reaches that far: the record is never read
                        break
                    C, Ci, dyaw = ego.box_motion(poses[p], poses[q], calib)
                    rec = xf[f0 + p, q - p - 1]
                    rec[0:16], rec[16:32], rec[32] = C.reshape(-1), Ci.reshape(-1), dyaw
        tab['xf'] = xf
    L = len(tab['ids'])
    capacity = rows if capacity is None else int(capacity)
    sizes = [L, F, S, max_fill, capacity, int(tab['xf'] is not None)]
    inp, _, n_in, _ = torch_ops.fill_layout(sizes)
    packed = np.zeros(n_in, np.int32)
    for name, (o, n) in inp.items():
        if n:
            packed[o:o + n] = np.ascontiguousarray(tab[name]).reshape(-1).view(np.int32)
    return dict(tab, packed=packed, sizes=sizes, sequences=seqs)


def _extend(values, new, like_list):
    if isinstance(values, (list, tuple)) and like_list:
        return list(values) + list(new)
    values = np.asarray(values)
    return np.concatenate([values, np.asarray(new, dtype=values.dtype).reshape((len(new),) + values.shape[1:])])


def unpack_fill(p, block):
    """The host side of ``fill_gaps_batch`` behind the launches: ``p`` from ``pack_fill``, ``block`` the host int32 block
    of mmmot::fill_tracks (torch_ops.fill_layout()[1]) -> one ``FilledTracks`` per sequence; raises ``TrackingError``
    naming the sequence on a status word.  The inputs are not modified: the frame dicts are copied, the extended
    arrays are new."""
    o = torch_ops.sections(np.asarray(block), torch_ops.fill_layout(p['sizes'])[1])
    rows = o['out'].view(np.float32).reshape(-1, 12).astype(np.float64)
    out_id, out_src = o['out_id'].astype(np.int64), o['out_src'].reshape(-1, 2).astype(np.int64)
    fill_start, info = o['fill_start'].astype(np.int64), o['info'].reshape(-1, 4)
    for s, st in enumerate(info[:, 0]):
        for bit, text in FILL_STATUS:
            if st & bit:
                raise TrackingError('fill_gaps: sequence %d: %s' % (s, text))
    frame_start, seq_start = p['frame_start'].astype(np.int64), p['seq_start']
    frame_of = np.searchsorted(frame_start, out_src, side='right') - 1  # empty frames share their start: the last one holds it
    res = []
    for s, (frames, fids, _, scores, _, _) in enumerate(p['sequences']):
        f0 = int(seq_start[s])
        nf, ni, ns, nm, nsrc = [], [], [], [], []
        for t, (d, fid) in enumerate(zip(frames, fids)):
            a, b = int(fill_start[f0 + t]), int(fill_start[f0 + t + 1])
            r, m = rows[a:b], len(np.asarray(fid).reshape(-1))
            src = np.stack([frame_of[a:b, 0] - f0, out_src[a:b, 0] - frame_start[frame_of[a:b, 0]],
                            frame_of[a:b, 1] - f0, out_src[a:b, 1] - frame_start[frame_of[a:b, 1]]], 1)
            d = dict(d)
            d['bbox'] = _extend(np.asarray(d['bbox']).reshape(m, 4), r[:, 0:4], False)
            d['dimensions'] = _extend(np.asarray(d['dimensions']).reshape(m, 3), r[:, [6, 4, 5]], False)
            d['location'] = _extend(np.asarray(d['location']).reshape(m, 3), r[:, 7:10], False)
            d['rotation_y'] = _extend(np.asarray(d['rotation_y']).reshape(m), r[:, 10], False)
            for key, unknown in (('truncated', -1), ('occluded', -1), ('alpha', -10)):
                if key in d:
                    d[key] = _extend(d[key], [unknown] * (b - a), True)
            if 'name' in d:
                d['name'] = _extend(d['name'], [frames[ta]['name'][ja] for ta, ja in src[:, 0:2]], True)
            nf.append(d)
            ni.append(np.concatenate([np.asarray(fid, dtype=np.int64).reshape(-1), out_id[a:b]]))
            if scores is not None:
                ns.append(_extend(np.asarray(scores[t]).reshape(m), r[:, 11], False))
            nm.append(np.arange(m + b - a) >= m)
            nsrc.append(src)
        res.append(FilledTracks(nf, ni, ns if scores is not None else None, nm, nsrc,
                                {'rows': int(info[s, 1]), 'links_filled': int(info[s, 2]),
                                 'links_too_long': int(info[s, 3])}))
    return res


def fill_gaps_batch(sequences, max_fill=7, device='cuda'):
    """``fill_gaps`` for many sequences - all 21 KITTI validation sequences, say - in ONE upload, ONE set of launches
    (mmmot_fill_tracks: five, whatever the sequences hold) and ONE copy back.  ``sequences``: per sequence the tuple
    (frames, ids[, frame_idx, scores, poses, calib]) or a dict with those keys.  Returns one ``FilledTracks`` per
    sequence, bit for bit what ``fill_gaps`` returns for it alone."""
    p = pack_fill(sequences, max_fill)
    host = torch.empty(len(p['packed']), dtype=torch.int32, pin_memory=True)
    host.numpy()[:] = p['packed']
    block = torch.ops.mmmot.fill_tracks(host.to(device, non_blocking=True), p['sizes'])
    return unpack_fill(p, block.cpu().numpy())


def fill_gaps(frames, ids, frame_idx=None, scores=None, poses=None, calib=None, max_fill=7, device='cuda'):
    """The last step of an offline tracker: a box for every listed frame a track skipped.  ``frames`` / ``ids`` /
    ``frame_idx`` / ``scores`` are what ``write_kitti_tracks`` takes (``ids`` with holes, as
    ``SequencePipeline.run_global(max_gap=G)`` leaves them).  Two observations of one ID with no observation between
    them, n = 2 .. ``max_fill`` + 1 frame numbers apart, are joined by one interpolated box per listed frame between
    them: the 2D box, the dimensions and the score blended linearly with w = (frames since the earlier one) / n, the yaw
    along the shorter arc, the location blended in the earlier frame's coordinates and moved into the hole frame's
    (DESIGN section 12a).  ``poses``: per frame (pos, rad) as ``FrameFeed(pose=)`` takes them, for all frames or none
    (a standing camera); with poses ``calib`` is the frame-info dict holding ``calib/R0_rect``, ``calib/Tr_velo_to_cam``
    and ``calib/Tr_imu_to_velo``.  Returns a ``FilledTracks``; ``write_kitti_tracks(path, ft.frames, ft.ids, frame_idx,
    ft.scores)`` and ``evaluate.labels_from_tracks(ft.frames, ft.ids, ..)`` take it as it is.  The inputs are not
    modified.  Raises ``TrackingError`` when an ID occurs twice in a frame or the frame numbers do not increase."""
    return fill_gaps_batch([(frames, ids, frame_idx, scores, poses, calib)], max_fill, device)[0]


# ---- smoothing: a Kalman filter forwards, an RTS pass backwards along every track (csrc/smooth_tracks.hip; 12b) ------
SMOOTH_KEYS = ('frames', 'ids', 'frame_idx', 'observed', 'poses', 'calib', 'scores')
SMOOTH_STATUS = tuple((bit, text) for bit, text in FILL_STATUS if bit != torch_ops.FILL_ECAPACITY)


class TrackSmoother:
    """The parameters of ``smooth_tracks``, per frame number: for the location (metres), the yaw
    (radians) and the dimensions h w l (metres) a process noise ``q`` (white acceleration; a random walk for the
    dimensions), a measurement variance ``r`` and - location and yaw - the variance ``v0`` of the velocity a track
    starts with.  A group with ``r = 0`` is left as it is.  ``q_dim = 0`` makes the size constant over a track: the mean
    of its observations.  ``yaw_flip``: a yaw step beyond pi/2 between two observations is read as the detector's front
    / back confusion and pi is added.  The defaults suit KITTI at 10 Hz (a detector noise of 0.2 m and 0.1 rad, objects
    that change their per-frame velocity by about 0.1 m); none of them was tuned on real data."""

    NAMES = ('q_loc', 'r_loc', 'v0_loc', 'q_yaw', 'r_yaw', 'v0_yaw', 'q_dim', 'r_dim')

    def __init__(self, q_loc=0.01, r_loc=0.04, v0_loc=1.0, q_yaw=0.001, r_yaw=0.01, v0_yaw=0.04, q_dim=0.0, r_dim=0.01,
                 yaw_flip=False):
        values = (q_loc, r_loc, v0_loc, q_yaw, r_yaw, v0_yaw, q_dim, r_dim)
        for name, v in zip(self.NAMES, values):
            v = float(v)
            if not (0.0 <= v < float('inf')):
                raise ValueError('TrackSmoother: %s must be finite and >= 0, got %r' % (name, v))
            setattr(self, name, v)
        for grp in ('loc', 'yaw'):
            if getattr(self, 'r_' + grp) > 0 and not getattr(self, 'v0_' + grp) > 0:
                raise ValueError('TrackSmoother: v0_%s must be > 0 where r_%s > 0' % (grp, grp))
        self.yaw_flip = bool(yaw_flip)

    def params(self):
        return tuple(getattr(self, n) for n in self.NAMES)

    def __repr__(self):
        return 'TrackSmoother(%s, yaw_flip=%r)' % (', '.join('%s=%r' % (n, getattr(self, n)) for n in self.NAMES),
                                                   self.yaw_flip)


class SmoothedTracks:
    """What ``smooth_tracks`` returns for one sequence: ``frames[t]`` a copy of the frame's detection dict with
    ``dimensions`` (lhw), ``location`` and ``rotation_y`` replaced, ``ids[t]`` / ``scores[t]`` (None when no scores were
    given) copies of what came, ``velocity[t]`` float64 [n, 4] = vx, vy, vz in the frame's camera axes and the yaw rate, per
    frame number (0 for rows that were copied), ``info`` = {'tracks', 'rows_changed', 'rows_copied'}."""

    def __init__(self, frames, ids, scores, velocity, info):
        self.frames, self.ids, self.scores, self.velocity, self.info = frames, ids, scores, velocity, info


def _smooth_sequence(seq):
    if isinstance(seq, dict):
        unknown = set(seq) - set(SMOOTH_KEYS)
        if unknown:
            raise ValueError('smooth_tracks: unknown sequence entries %s' % sorted(unknown))
        return tuple(seq.get(k) for k in SMOOTH_KEYS)
    seq = tuple(seq)
    if not 2 <= len(seq) <= len(SMOOTH_KEYS):
        raise ValueError('smooth_tracks: a sequence is a dict or a tuple of %s' % (SMOOTH_KEYS,))
    return seq + (None,) * (len(SMOOTH_KEYS) - len(seq))


def pack_smooth(sequences, smoother=None):
    """The host side of ``smooth_tracks_batch`` before the launches: per sequence (frames, ids, frame_idx, observed,
    poses, calib, scores) as ``smooth_tracks`` takes them (a tuple, or a dict with those keys) -> the tables of
    mmmot_smooth_tracks.  Returns a dict: ``packed`` (the int32 block of torch_ops.smooth_layout), ``sizes``, the tables
    by name (``det``, ``ids``, ``frame_start``, ``frame_no``, ``seq_start`` as for ``pack_fill``; ``observed`` int32 [L]
    or None when no sequence has a mask; ``xf0`` fp64 [F, 33] or None when no sequence moves: per listed frame
    ``ego.box_motion`` from the first frame of its sequence), ``smoother`` and ``sequences``.  In a call where only some
    sequences move or carry a mask the others get identity records / an all-ones mask, which give the same bits."""
    from . import ego
    smoother = TrackSmoother() if smoother is None else smoother
    if not isinstance(smoother, TrackSmoother):
        raise ValueError('smooth_tracks: smoother must be a tracks.TrackSmoother, got %r' % (smoother,))
    seqs = [_smooth_sequence(s) for s in sequences]
    tab, _, moving = sequence_tables([(f, i, n, sc, p, c) for f, i, n, _, p, c, sc in seqs], 'smooth_tracks')
    L, F, S = len(tab['ids']), len(tab['frame_no']), len(seqs)
    tab.update(observed=None, xf0=None)
    if any(q[3] is not None for q in seqs):
        obs = np.ones(L, np.int32)
        for s, (frames, fids, _, mask, _, _, _) in enumerate(seqs):
            if mask is None:
                continue
            if len(mask) != len(frames):
                raise ValueError('smooth_tracks: sequence %d has %d frames but a mask of another length' % (s, len(frames)))
            for t, m in enumerate(mask):
                a, b = (int(v) for v in tab['frame_start'][tab['seq_start'][s] + t:][:2])
                m = np.asarray(m).reshape(-1)
                if len(m) != b - a:
                    raise ValueError('smooth_tracks: sequence %d, frame %d: the mask has %d entries for %d detections'
                                     % (s, t, len(m), b - a))
                obs[a:b] = m != 0
        tab['observed'] = obs
    if any(moving):
        xf0 = np.zeros((F, torch_ops.FILL_REC), np.float64)
        xf0[:, 0:16] = xf0[:, 16:32] = np.eye(4).reshape(-1)
        for s, (frames, _, _, _, poses, calib, _) in enumerate(seqs):
            if not moving[s]:
                continue
            f0 = int(tab['seq_start'][s])
            for p in range(1, len(frames)):  # frame 0 of a sequence keeps the identity
                C, Ci, dyaw = ego.box_motion(poses[0], poses[p], calib)
                xf0[f0 + p, 0:16], xf0[f0 + p, 16:32], xf0[f0 + p, 32] = C.reshape(-1), Ci.reshape(-1), dyaw
        tab['xf0'] = xf0
    sizes = [L, F, S, int(tab['xf0'] is not None), int(tab['observed'] is not None), int(smoother.yaw_flip)]
    sizes += torch_ops.smooth_param_bits(smoother.params())
    inp, _, n_in, _ = torch_ops.smooth_layout(sizes)
    packed = np.zeros(n_in, np.int32)
    for name, (o, n) in inp.items():
        if n:
            packed[o:o + n] = np.ascontiguousarray(tab[name]).reshape(-1).view(np.int32)
    return dict(tab, packed=packed, sizes=sizes, sequences=seqs, smoother=smoother)


def unpack_smooth(p, block):
    """The host side of ``smooth_tracks_batch`` behind the launches: ``p`` from ``pack_smooth``, ``block`` the host int32
    block of mmmot::smooth_tracks -> one ``SmoothedTracks`` per sequence; raises ``TrackingError`` naming the sequence
    on a status word.  The inputs are not modified: the frame dicts are copied, the replaced arrays are new."""
    o = torch_ops.sections(np.asarray(block), torch_ops.smooth_layout(p['sizes'])[1])
    rows = o['out'].view(np.float32).reshape(-1, 12).astype(np.float64)
    vel, info = o['vel'].view(np.float32).reshape(-1, 4).astype(np.float64), o['info'].reshape(-1, 4)
    for s, st in enumerate(info[:, 0]):
        for bit, text in SMOOTH_STATUS:
            if st & bit:
                raise TrackingError('smooth_tracks: sequence %d: %s' % (s, text))
    frame_start, seq_start = p['frame_start'].astype(np.int64), p['seq_start']
    res = []
    for s, (frames, fids, _, _, _, _, scores) in enumerate(p['sequences']):
        f0 = int(seq_start[s])
        nf, ni, ns, nv = [], [], [], []
        for t, (d, fid) in enumerate(zip(frames, fids)):
            a, b = int(frame_start[f0 + t]), int(frame_start[f0 + t + 1])
            r, d = rows[a:b], dict(d)
            d['dimensions'], d['location'], d['rotation_y'] = r[:, [6, 4, 5]], r[:, 7:10].copy(), r[:, 10].copy()
            nf.append(d)
            ni.append(np.asarray(fid, dtype=np.int64).reshape(-1).copy())
            if scores is not None:
                ns.append(np.array(scores[t]).reshape(-1))
            nv.append(vel[a:b].copy())
        res.append(SmoothedTracks(nf, ni, ns if scores is not None else None, nv,
                                  {'tracks': int(info[s, 1]), 'rows_changed': int(info[s, 2]),
                                   'rows_copied': int(info[s, 3])}))
    return res


def smooth_tracks_batch(sequences, smoother=None, device='cuda'):
    """``smooth_tracks`` for many sequences in ONE upload, ONE set of launches (mmmot_smooth_tracks: five, whatever the
    sequences hold) and ONE copy back.  ``sequences``: per sequence the tuple (frames, ids[, frame_idx, observed, poses,
    calib, scores]) or a dict with those keys.  Returns one ``SmoothedTracks`` per sequence, bit for bit what ``smooth_tracks``
    returns for it alone."""
    p = pack_smooth(sequences, smoother)
    host = torch.empty(len(p['packed']), dtype=torch.int32, pin_memory=True)
    host.numpy()[:] = p['packed']
    block = torch.ops.mmmot.smooth_tracks(host.to(device, non_blocking=True), p['sizes'])
    return unpack_smooth(p, block.cpu().numpy())


def smooth_tracks(frames, ids, frame_idx=None, observed=None, poses=None, calib=None, smoother=None, device='cuda',
                  scores=None):
    """A trajectory per track in place of the detector's boxes one by one: a fixed-interval smoother (a Kalman filter
    forwards, a Rauch-Tung-Striebel pass backwards) over every track of the sequence.  ``frames`` /
    ``ids`` / ``frame_idx`` are what ``write_kitti_tracks`` takes.  The location and the yaw follow a constant-velocity
    model (the yaw unwrapped along the track), h w l a random walk; rows whose ``observed[t][j]`` is false carry no
    measurement - ``observed=[~m for m in filled.filled]`` for a ``FilledTracks``, whose straight-line rows are then
    replaced by the smoother's.  Rows behind a track's last observation are extrapolated, rows in front of its first one,
    rejected rows (ID -1) and tracks of one row are returned as they are.  ``poses`` / ``calib`` as for ``fill_gaps``: with
    a moving camera the filter runs in the first frame's coordinates.  ``smoother``: a ``TrackSmoother`` (default: its
    defaults); ``scores``: per frame the per-detection scores, carried through (``FilledTracks.scores``).  Returns a ``SmoothedTracks``; ``write_kitti_tracks(path, st.frames, st.ids, frame_idx, st.scores)`` and
    ``evaluate.labels_from_tracks(st.frames, st.ids, .., box3d=True)`` take it as it is.  The 2D box and the score are
    not changed.  Raises ``TrackingError`` when an ID occurs twice in a frame or the frame numbers do not increase."""
    return smooth_tracks_batch([(frames, ids, frame_idx, observed, poses, calib, scores)], smoother, device)[0]


# ---- stitching: the tail of a track joined to the head of a later one (csrc/stitch_tracks.hip) ---
STITCH_KEYS = ('frames', 'ids', 'frame_idx', 'velocity', 'poses', 'calib')
STITCH_STATUS = SMOOTH_STATUS + ((torch_ops.STITCH_ETOOMANY, 'more than %d tracks' % torch_ops.STITCH_MAXK),)


class TrackStitcher:
    """The parameters of ``stitch_tracks`` and its two fp64 tables.  The tail of a track and the
    head of a later one, ``min_dt <= dt <= max_dt`` frame numbers apart, are a candidate when the constant-velocity
    prediction of one lies within ``drift * dt + slack`` metres of the other - forwards from the tail, backwards from
    the head, both where both tracks have a velocity (``min_rows`` rows or more and a ``velocity`` given).  Two tracks
    without a velocity are compared as they stand, within ``max_speed * dt + slack``.  ``drift`` and ``max_speed`` are
    in metres per frame number, ``slack`` in metres; ``mode`` 'ground' measures in the camera's x / z plane, '3d' with
    y; ``max_size_ratio`` > 0 also bounds the factor between the two boxes' h, w and l; ``gap_penalty`` lowers the
    score of a candidate by that much per frame number beyond the first.  The defaults are stated choices for KITTI at
    10 Hz (0.5 m per frame of velocity error, 40 m/s, the motion gate's 2 m of slack, three seconds of occlusion); none
    of them was tuned on real data."""

    def __init__(self, max_dt=30, min_dt=1, drift=0.5, max_speed=4.0, slack=2.0, min_rows=3, mode='ground',
                 max_size_ratio=0.0, gap_penalty=0.0):
        fin = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not (whole(min_dt) and whole(max_dt) and 1 <= int(min_dt) <= int(max_dt) <= torch_ops.STITCH_MAX_DT):
            raise ValueError('TrackStitcher: min_dt and max_dt must be integers with 1 <= min_dt <= max_dt <= %d, got %r, '
                             '%r' % (torch_ops.STITCH_MAX_DT, min_dt, max_dt))
        if not (fin(drift) and fin(max_speed) and fin(slack) and min(drift, max_speed, slack) >= 0
                and drift + slack > 0 and max_speed + slack > 0):
            raise ValueError('TrackStitcher: drift, max_speed and slack must be finite and >= 0 with every radius > 0, '
                             'got %r, %r, %r' % (drift, max_speed, slack))
        if not (whole(min_rows) and int(min_rows) >= 1):
            raise ValueError('TrackStitcher: min_rows must be an integer >= 1, got %r' % (min_rows,))
        if mode not in torch_ops.STITCH_MODES:
            raise ValueError('TrackStitcher: mode must be one of %s, got %r' % (sorted(torch_ops.STITCH_MODES), mode))
        if not (fin(max_size_ratio) and (max_size_ratio == 0 or max_size_ratio >= 1)):
            raise ValueError('TrackStitcher: max_size_ratio must be 0 (off) or a finite factor >= 1, got %r'
                             % (max_size_ratio,))
        if not (fin(gap_penalty) and gap_penalty >= 0):
            raise ValueError('TrackStitcher: gap_penalty must be finite and >= 0, got %r' % (gap_penalty,))
        self.max_dt, self.min_dt, self.min_rows, self.mode = int(max_dt), int(min_dt), int(min_rows), mode
        self.drift, self.max_speed, self.slack = float(drift), float(max_speed), float(slack)
        self.max_size_ratio, self.gap_penalty = float(max_size_ratio), float(gap_penalty)
        dt = np.arange(self.max_dt + 1, dtype=np.float64)
        r = np.stack([np.float64(self.drift) * dt + np.float64(self.slack),
                      np.float64(self.max_speed) * dt + np.float64(self.slack)])
        self.r2 = r * r
        self.inv_r2 = np.full_like(self.r2, np.nan)  # entry 0 is never read: dt >= 1
        self.inv_r2[:, 1:] = np.float64(1.0) / self.r2[:, 1:]
        self.r2[:, 0] = np.nan

    def __repr__(self):
        return 'TrackStitcher(%s)' % ', '.join('%s=%r' % (n, getattr(self, n)) for n in (
            'max_dt', 'min_dt', 'drift', 'max_speed', 'slack', 'min_rows', 'mode', 'max_size_ratio', 'gap_penalty'))


class StitchedTracks:
    """What ``stitch_tracks`` returns for one sequence: ``ids[t]`` int64, the frame's IDs with every stitched track
    under the ID of the first track of its chain; ``pairs`` int64 [stitches, 4] = (frame, detection, frame, detection)
    of the tail row and the head row of every stitch (positions in the sequence's lists); ``links`` float32 [K, K] the
    scores, tails on rows and heads on columns, tracks in the order of their first rows (NaN: no candidate);
    ``objective`` the sum of the kept scores (NaN without tracks); ``info`` = {'tracks', 'stitches', 'rows_changed'}.
    ``filled`` / ``smoothed``: set by ``SequencePipeline.run_global(stitch=)`` - the second ``fill_gaps`` /
    ``smooth_tracks`` over the relabelled sequence - else None."""

    def __init__(self, ids, pairs, links, objective, info):
        self.ids, self.pairs, self.links, self.objective, self.info = ids, pairs, links, objective, info
        self.filled = self.smoothed = None


def _stitch_sequence(seq):
    if isinstance(seq, dict):
        unknown = set(seq) - set(STITCH_KEYS)
        if unknown:
            raise ValueError('stitch_tracks: unknown sequence entries %s' % sorted(unknown))
        return tuple(seq.get(k) for k in STITCH_KEYS)
    seq = tuple(seq)
    if not 2 <= len(seq) <= len(STITCH_KEYS):
        raise ValueError('stitch_tracks: a sequence is a dict or a tuple of %s' % (STITCH_KEYS,))
    return seq + (None,) * (len(STITCH_KEYS) - len(seq))


def pack_stitch(sequences, stitcher=None):
    """The host side of ``stitch_tracks_batch`` before the launches: per sequence (frames, ids, frame_idx, velocity,
    poses, calib) as ``stitch_tracks`` takes them (a tuple, or a dict with those keys) -> the tables of
    mmmot_stitch_tracks.  Returns a dict: ``packed`` (the int32 block of torch_ops.stitch_layout), ``sizes``, the tables
    by name (``det``, ``ids``, ``frame_start``, ``frame_no``, ``seq_start`` as for ``pack_fill``; ``vel`` fp32 [L, 4] or
    None; ``xf0`` as for ``pack_smooth``; ``k_start`` and ``pairs``, the tracks per sequence counted here from the IDs;
    ``r2`` / ``inv_r2``), ``stitcher`` and ``sequences``.  The velocities are given for every sequence of a call or for
    none: a missing one would not be a zero velocity."""
    from . import ego
    stitcher = TrackStitcher() if stitcher is None else stitcher
    if not isinstance(stitcher, TrackStitcher):
        raise ValueError('stitch_tracks: stitcher must be a tracks.TrackStitcher, got %r' % (stitcher,))
    seqs = [_stitch_sequence(s) for s in sequences]
    tab, _, moving = sequence_tables([(f, i, n, None, p, c) for f, i, n, _, p, c in seqs], 'stitch_tracks')
    L, F, S = len(tab['ids']), len(tab['frame_no']), len(seqs)
    tab.update(vel=None, xf0=None, r2=stitcher.r2, inv_r2=stitcher.inv_r2)
    with_vel = [q[3] is not None for q in seqs]
    if any(with_vel):
        if not all(with_vel):
            raise ValueError('stitch_tracks: velocities are given for every sequence of a call or for none')
        vel = np.zeros((L, 4), np.float32)
        for s, (frames, _, _, velocity, _, _) in enumerate(seqs):
            if len(velocity) != len(frames):
                raise ValueError('stitch_tracks: sequence %d has %d frames but velocities of another length'
                                 % (s, len(frames)))
            for t, v in enumerate(velocity):
                a, b = (int(x) for x in tab['frame_start'][tab['seq_start'][s] + t:][:2])
                v = np.asarray(v, dtype=np.float64).reshape(b - a, -1) if b > a else np.zeros((0, 3))
                if v.shape[1] < 3:
                    raise ValueError('stitch_tracks: sequence %d, frame %d: a velocity is vx, vy, vz[, yaw rate] per '
                                     'detection' % (s, t))
                vel[a:b, 0:3] = v[:, 0:3]
        tab['vel'] = vel
    if any(moving):
        xf0 = np.zeros((F, torch_ops.FILL_REC), np.float64)
        xf0[:, 0:16] = xf0[:, 16:32] = np.eye(4).reshape(-1)
        for s, (frames, _, _, _, poses, calib) in enumerate(seqs):
            if not moving[s]:
                continue
            f0 = int(tab['seq_start'][s])
            for p in range(1, len(frames)):  # frame 0 of a sequence keeps the identity
                C, Ci, dyaw = ego.box_motion(poses[0], poses[p], calib)
                xf0[f0 + p, 0:16], xf0[f0 + p, 16:32], xf0[f0 + p, 32] = C.reshape(-1), Ci.reshape(-1), dyaw
        tab['xf0'] = xf0
    K = []
    for s in range(S):
        a, b = (int(tab['frame_start'][f]) for f in tab['seq_start'][s:s + 2])
        kept = tab['ids'][a:b]
        K.append(len(np.unique(kept[kept >= 0])))
    K = np.asarray(K, np.int64)
    k_start = np.concatenate([[0], np.cumsum(K)])
    link_off = np.concatenate([[0], np.cumsum(K * K)])
    if 6 * k_start[-1] + link_off[-1] >= 2 ** 31:
        raise ValueError('stitch_tracks: the link blocks of the call exceed 32-bit offsets')
    tab['k_start'] = k_start.astype(np.int32)
    tab['pairs'] = np.stack([K, K, 2 * k_start[:-1], link_off[:-1]], 1).astype(np.int32)
    sizes = [L, F, S, int(k_start[-1]), int(link_off[-1]), int(K.max()), int(tab['xf0'] is not None),
             int(tab['vel'] is not None), stitcher.min_dt, stitcher.max_dt, stitcher.min_rows,
             torch_ops.STITCH_MODES[stitcher.mode]]
    sizes += torch_ops.stitch_param_bits(stitcher.max_size_ratio, stitcher.gap_penalty)
    inp, _, n_in, _ = torch_ops.stitch_layout(sizes)
    packed = np.zeros(n_in, np.int32)
    for name, (o, n) in inp.items():
        if n:
            packed[o:o + n] = np.ascontiguousarray(tab[name]).reshape(-1).view(np.int32)
    return dict(tab, packed=packed, sizes=sizes, sequences=seqs, stitcher=stitcher)


def unpack_stitch(p, block):
    """The host side of ``stitch_tracks_batch`` behind the launches: ``p`` from ``pack_stitch``, ``block`` the host int32
    block of mmmot::stitch_tracks -> one ``StitchedTracks`` per sequence; raises ``TrackingError`` naming the sequence
    on a status word.  The inputs are not modified."""
    o = torch_ops.sections(np.asarray(block), torch_ops.stitch_layout(p['sizes'])[1])
    out_ids, nxt, info = o['out_ids'].astype(np.int64), o['next'].astype(np.int64), o['info'].reshape(-1, 4)
    links, objective = o['links'].view(np.float32), o['objective']
    for s, st in enumerate(info[:, 0]):
        for bit, text in STITCH_STATUS:
            if st & bit:
                raise TrackingError('stitch_tracks: sequence %d: %s' % (s, text))
    frame_start, seq_start = p['frame_start'].astype(np.int64), p['seq_start']
    res = []
    for s, (frames, _, _, _, _, _) in enumerate(p['sequences']):
        f0, K, lo = int(seq_start[s]), int(p['pairs'][s, 0]), int(p['pairs'][s, 3])
        a, b = int(frame_start[f0]), int(frame_start[int(seq_start[s + 1])])
        ids = [out_ids[int(frame_start[f0 + t]):int(frame_start[f0 + t + 1])].copy() for t in range(len(frames))]
        tails = a + np.flatnonzero(nxt[a:b] >= 0)
        rows = np.stack([tails, nxt[tails]], 1).reshape(-1, 2)
        frame_of = np.searchsorted(frame_start, rows, side='right') - 1  # empty frames share their start
        pairs = np.stack([frame_of[:, 0] - f0, rows[:, 0] - frame_start[frame_of[:, 0]],
                          frame_of[:, 1] - f0, rows[:, 1] - frame_start[frame_of[:, 1]]], 1).astype(np.int64)
        res.append(StitchedTracks(ids, pairs, links[lo:lo + K * K].reshape(K, K).copy(), float(objective[s]),
                                  {'tracks': int(info[s, 1]), 'stitches': int(info[s, 2]),
                                   'rows_changed': int(info[s, 3])}))
    return res


def stitch_tracks_batch(sequences, stitcher=None, device='cuda'):
    """``stitch_tracks`` for many sequences in ONE upload, ONE set of launches (mmmot_stitch_tracks: seven and the pair
    solver's, whatever the sequences hold) and ONE copy back.  ``sequences``: per sequence the tuple (frames, ids[,
    frame_idx, velocity, poses, calib]) or a dict with those keys.  Returns one ``StitchedTracks`` per sequence, bit for
    bit what ``stitch_tracks`` returns for it alone."""
    p = pack_stitch(sequences, stitcher)
    host = torch.empty(len(p['packed']), dtype=torch.int32, pin_memory=True)
    host.numpy()[:] = p['packed']
    block = torch.ops.mmmot.stitch_tracks(host.to(device, non_blocking=True), p['sizes'])
    return unpack_stitch(p, block.cpu().numpy())


def stitch_tracks(frames, ids, frame_idx=None, velocity=None, poses=None, calib=None, stitcher=None, device='cuda'):
    """The second level of an offline tracker: tracks that an occlusion longer than the solve's gap limit broke are
    rejoined.  Every track of the sequence is one node; the tail of a track is matched to the head
    of a later one, one to one and with the largest total score, when the constant-velocity prediction of one reaches
    the other (``TrackStitcher``), and the later track takes the earlier one's ID.  ``frames`` / ``ids`` / ``frame_idx``
    are what ``write_kitti_tracks`` takes; ``velocity``: ``SmoothedTracks.velocity`` (per frame [n, >= 3]: vx, vy, vz per
    frame number in the frame's camera axes), or None: tracks are then compared as they stand; ``poses`` / ``calib`` as for
    ``fill_gaps``: with a moving camera the comparison runs in the first frame's coordinates.  No appearance is
    compared.  Returns a ``StitchedTracks``, whose ``ids`` go to ``write_kitti_tracks``, ``labels_from_tracks``,
    ``fill_gaps`` and ``smooth_tracks`` as they are.  The inputs are not modified.  Raises ``TrackingError`` when an ID
    occurs twice in a frame, the frame numbers do not increase or the sequence holds more than 512 tracks."""
    return stitch_tracks_batch([(frames, ids, frame_idx, velocity, poses, calib)], stitcher, device)[0]
