#!/usr/bin/env python
"""Makes tests/golden/track_chain_ids_*.npz with the REFERENCE's own ID bookkeeping on windows of 2 .. 8 frames.

    python tools/gen_golden_track_chains.py --reference /path/to/mmMOT

Built like tools/gen_golden_tracks.py, whose stand-ins and synthetic detections it uses: the reference's
``TrackingModule`` is imported from its checkout (nothing of it is copied).  A sequence is a list of segments of
consecutive frames; each segment is cut into windows of T frames that start at its frames 0, T-1, 2 (T-1), .. (the last
one shorter when the segment does not divide).  Per window, scores come from tests/association_chain_ref.random_chain
(alternating 'eval' and 'masked'), the assignment from ``milp_route`` (``lp_route``, which asserts an integral vertex,
above 100 detections a frame), checked by ``feasible``; then ``assign_det_id`` + ``align_id`` run on the window.
Stored per sequence, as data only: the chain table rows (T, score offset, link offset, n_0 .. n_7), the frame indices
[W, 8], the windows' assignment blocks [det L | new L | end L | link_0 | ..] (uint8), what the reference returned after
every window - the kept IDs of the emitted frames, ``frame_start`` and ``last_id`` - and the final ``frames_id`` list
with its frame indices.  Each set is asserted to hold the cases it is named for.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
from association_chain_ref import feasible, lp_route, milp_route, random_chain  # noqa: E402
from gen_golden_tracks import GOLDEN, REJECT, as_ref, import_reference, make_dets  # noqa: E402

MAX_T = 8


def windows_of(idx, T):
    """the windows of one segment: lists of frame indices"""
    return [idx[s:s + T] for s in range(0, len(idx) - 1, T - 1)]


def run_sequence(TrackingModule, rng, segments, counts, T, reject=()):
    """segments: lists of frame indices; counts: {frame index: detections}; reject: {(window, frame of the window)}
    whose detections are all rejected.  Returns the fixture dict and per window a summary for the asserts."""
    dets = {f: make_dets(rng, n, f) for f, n in counts.items()}
    tm = TrackingModule(types.SimpleNamespace(test_mode=0), None, None, det_type='3D')
    tm.clear_mem()
    t32 = lambda x: torch.from_numpy(np.asarray(x, np.float32))
    rows, fidx, blocks, emit_len, emit_ids, starts, last_ids, info = [], [], [], [], [], [], [], []
    so = lo = 0
    wins = [w for seg in segments for w in windows_of(seg, T)]
    for w, fr in enumerate(wins):
        split = [counts[f] for f in fr]
        st = np.concatenate([[0], np.cumsum(split)])
        det, new, end, links = random_chain(rng, split, 1.0, 'eval' if w % 2 == 0 else 'masked')
        for ww, t in reject:
            if ww == w:
                det[st[t]:st[t + 1]] = REJECT
        route = lp_route if max(split) > 100 else milp_route
        (a_det, a_links, a_new, a_end), _ = route(det, new, end, links, split)
        assert feasible((a_det, a_links, a_new, a_end), split)
        ids, out = tm.assign_det_id(t32(a_det), [t32(l).view(1, *l.shape) for l in a_links], t32(a_new), t32(a_end),
                                    [torch.tensor([n]) for n in split], [as_ref(dets[f]) for f in fr])
        r_ids, _, start = tm.align_id(ids, out)
        assert len(r_ids) == len(fr) - start
        lens = [-1] * MAX_T
        for k, e in enumerate(r_ids):
            e = np.asarray(e, dtype=np.int64).reshape(-1)
            lens[k + start] = len(e)
            emit_ids.append(e)
        K = sum(a * b for a, b in zip(split[:-1], split[1:]))
        rows.append([len(fr), so, lo] + split + [0] * (MAX_T - len(fr)))
        so, lo = so + sum(split), lo + K
        fidx.append(list(fr) + [0] * (MAX_T - len(fr)))
        blocks.append(np.concatenate([a_det, a_new, a_end] + [l.reshape(-1) for l in a_links]).astype(np.uint8))
        emit_len.append(lens)
        starts.append(int(start))
        last_ids.append(int(tm.last_id))
        kept = [a_det[st[t]:st[t + 1]] == 1 for t in range(len(fr))]
        info.append({'T': len(fr), 'split': split, 'start': int(start), 'kept': [int(k.sum()) for k in kept],
                     'linked_last': int(((a_det[st[-2]:] == 1) & (a_new[st[-2]:] == 0)).sum()),
                     'kept_past_256': sum(int(k[256:].sum()) for k in kept)})
    fx = {'chains': np.asarray(rows, np.int32), 'frame_idx': np.asarray(fidx, np.int32),
          'blocks': np.concatenate(blocks), 'emit_len': np.asarray(emit_len, np.int32),
          'emit_ids': np.concatenate(emit_ids + [np.zeros(0, np.int64)]).astype(np.int64),
          'frame_start': np.asarray(starts, np.int32), 'last_id': np.asarray(last_ids, np.int64),
          'frames_id_len': np.asarray([len(x) for x in tm.frames_id], np.int32),
          'frames_id': np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in tm.frames_id] + [np.zeros(0, np.int64)]),
          'frames_id_frame': np.asarray([int(d['frame_idx'][0]) for d in tm.frames_det], np.int32)}
    return fx, info


def quirk(i):
    """the window's first frame was the stored one and its frame 1 keeps nothing: nothing of it is stored"""
    return i['start'] == 1 and i['kept'][1] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('MMMOT_REFERENCE'), required='MMMOT_REFERENCE' not in os.environ)
    args = ap.parse_args()
    TrackingModule, _ = import_reference(args.reference)
    os.makedirs(GOLDEN, exist_ok=True)
    seqs = {}

    # KITTI shape: 40 frames of 10-12 detections in windows of 3, a gap after frame 24, frame 1 of window 5 rejected
    rng = np.random.default_rng(11)
    segs = [list(range(25)), list(range(30, 45))]
    counts = {f: int(rng.integers(10, 13)) for s in segs for f in s}
    fx, info = seqs['kitti3'] = run_sequence(TrackingModule, rng, segs, counts, 3, reject={(5, 1)})
    assert len(info) == 19 and info[12]['start'] == 0, 'kitti3: the window behind the gap starts anew'
    assert quirk(info[5]) and info[5]['kept'][2] > 0 and info[6]['start'] == 0, 'kitti3: quirk window'

    # windows of 8 over 22 frames of 2-6 detections (22 = 1 + 3 * 7: three full windows)
    rng = np.random.default_rng(3)
    counts = {f: int(rng.integers(2, 6)) for f in range(22)}
    fx, info = seqs['t8'] = run_sequence(TrackingModule, rng, [list(range(22))], counts, 8)
    assert [i['T'] for i in info] == [8, 8, 8] and all(i['linked_last'] > 0 for i in info), 't8: linked last frames'

    # roles, windows of 5 over 18 frames (the last window is short: 2 frames): frame 0 of the first window rejected,
    # frame 1 of window 1 (quirk) and frame T-1 of window 2 rejected; frame 16 is empty: the last frame of window 3 and
    # frame 0 of window 4; frame 14 is empty: a middle frame of window 3
    rng = np.random.default_rng(5)
    counts = {f: int(rng.integers(3, 7)) for f in range(18)}
    counts[14] = counts[16] = 0
    fx, info = seqs['roles5'] = run_sequence(TrackingModule, rng, [list(range(18))], counts, 5,
                                              reject={(0, 0), (1, 1), (2, 4)})
    assert [i['T'] for i in info] == [5, 5, 5, 5, 2], 'roles5: a short last window'
    assert info[0]['kept'][0] == 0 and info[2]['kept'][4] == 0
    assert quirk(info[1]) and sum(info[1]['kept'][2:]) > 0 and info[2]['start'] == 0, 'roles5: quirk window'
    assert info[3]['split'][2] == 0 and info[3]['split'][4] == 0 and info[4]['split'][0] == 0, 'roles5: empty frames'

    # roles, windows of 3 over 15 frames: frame 1 of window 2 (quirk), frame 0 of window 1 (kept by window 0, rejected
    # now) and frame T-1 of window 5 rejected; frame 8 is empty: the last frame of window 3 and frame 0 of window 4; frame 13: the middle of window 6
    rng = np.random.default_rng(4)
    counts = {f: int(rng.integers(3, 7)) for f in range(15)}
    counts[8] = counts[13] = 0
    fx, info = seqs['roles3'] = run_sequence(TrackingModule, rng, [list(range(15))], counts, 3,
                                              reject={(2, 1), (1, 0), (5, 2)})
    assert quirk(info[2]) and info[2]['kept'][2] > 0 and info[3]['start'] == 0, 'roles3: quirk window'
    assert info[3]['split'][2] == 0 and info[4]['split'][0] == 0 and info[6]['split'][1] == 0, 'roles3: empty frames'
    assert info[5]['kept'][2] == 0

    # the wave boundaries of both launch forms: windows of 4 over counts cycling through 1, 63, 64, 65, 129, 128
    rng = np.random.default_rng(6)
    cyc = (1, 63, 64, 65, 129, 128)
    counts = {f: cyc[f % 6] for f in range(14)}
    fx, info = seqs['waves'] = run_sequence(TrackingModule, rng, [list(range(14))], counts, 4)
    assert [i['T'] for i in info] == [4, 4, 4, 4, 2]

    # the four-wave kernel's second pass over a frame
    rng = np.random.default_rng(7)
    counts = dict(enumerate((300, 257, 300, 131, 260)))
    fx, info = seqs['n300'] = run_sequence(TrackingModule, rng, [list(range(5))], counts, 3)
    assert all(i['kept_past_256'] > 0 for i in info), 'n300: kept detections beyond the first pass of 256 threads'

    for name, (fx, info) in seqs.items():
        assert sum(i['start'] for i in info) > 0, '%s: no window continues the stored frame' % name
        path = os.path.join(GOLDEN, 'track_chain_ids_%s.npz' % name)
        np.savez_compressed(path, **fx)
        print('%-7s windows %3d  continued %3d  quirk %2d  last_id %4d  %7d bytes' % (
            name, len(info), sum(i['start'] for i in info), sum(quirk(i) for i in info), int(fx['last_id'][-1]),
            os.path.getsize(path)))


if __name__ == '__main__':
    main()
