"""Inputs shared by tests/test_gate_cpu.py and tests/test_gate_gpu.py: small tables for mmmot_gate_links, the detection
dicts ``association.pack_gate`` takes, and the crafted scene in which two similar objects swap their IDs across a hole
unless the motion gate removes the links no object could have travelled."""
import numpy as np

from mmmot_amd import ego, synth

import fill_cases
import gate_ref


def tables(rng, counts, frame_no=None):
    """det [L, 12] fp32 with the centres drawn so close that a radius of a few metres passes some links and gates
    others (x in +-8 m, y in -2 .. 3 m, z in 5 .. 25 m), frame_start, frame_no (default 0, 1, ..)"""
    det = fill_cases.random_dets(rng, int(sum(counts)))
    n = len(det)
    det[:, 7], det[:, 9] = rng.uniform(-8, 8, n), rng.uniform(5, 25, n)
    return dict(det=det, frame_start=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                frame_no=np.arange(len(counts), dtype=np.int32) if frame_no is None else np.asarray(frame_no, np.int32))


def holey_numbers(rng, n):
    """strictly increasing frame numbers with steps of 1 .. 3"""
    return np.cumsum(rng.integers(1, 4, n)).astype(np.int32)


def gap_blocks(counts, G, first=0, off=0):
    """the block table of one sequence in the gap-by-gap layout of ``gap_sequences_table``, its frames numbered from
    ``first`` and its links laid out from ``off``; returns (rows, the offset behind them)"""
    rows = []
    for g in range(1, G + 1):
        for t in range(len(counts) - g):
            rows.append((first + t, first + t + g, off, 0))
            off += counts[t] * counts[t + g]
    return rows, off


def random_links(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def frame_dicts(t):
    """the detection dicts of the frames of ``tables``: fp64 copies of the fp32 rows, which ``pack_gate`` rounds back"""
    out = []
    for a, b in zip(t['frame_start'][:-1], t['frame_start'][1:]):
        d = t['det'][a:b].astype(np.float64)
        out.append({'bbox': d[:, 0:4], 'dimensions': d[:, [6, 4, 5]], 'location': d[:, 7:10], 'rotation_y': d[:, 10]})
    return out


def records(poses, pairs, n_frames, rec_gaps):
    """xf [F, rec_gaps, REC] with the ``ego.box_motion`` record of every listed pair, identity elsewhere"""
    xf = identity_records(n_frames, rec_gaps)
    for a, b in pairs:
        C, Ci, dyaw = ego.box_motion(poses[a], poses[b], fill_cases.CALIB)
        xf[a, b - a - 1, 0:16], xf[a, b - a - 1, 16:32], xf[a, b - a - 1, 32] = C.reshape(-1), Ci.reshape(-1), dyaw
    return xf


def identity_records(n_frames, rec_gaps):
    xf = np.zeros((n_frames, rec_gaps, gate_ref.REC), np.float64)
    xf[:, :, 0:16] = xf[:, :, 16:32] = np.eye(4).reshape(-1)
    return xf


def drive(n_frames, seed):
    return synth.ego_poses(n_frames, seed)


# ---- the swap scene: the persistent objects of fill_cases over 8 frames; objects 0 and 1 are missed in frames 3 and 4 ---
SWAP_FRAMES, SWAP_HOLE, SWAP_GAP = 8, (3, 4), 3


def swap_scene():
    """(frames, objects per frame, split, (det, links nested by gap, new, end) fp32).  Every object links to its own
    later box with 5.5 and to every other box with -5, except that objects 0 and 1 - two similar cars 5.9 m apart - link
    to EACH OTHER'S box behind the hole with 6.0, the same score both ways: appearance alone prefers the swap."""
    frames, objs = [], []
    for t in range(SWAP_FRAMES):
        here = [o for o in range(fill_cases.N_OBJ) if not (o in (0, 1) and t in SWAP_HOLE)]
        rows = [fill_cases.scene_row(o, t) for o in here]
        frames.append({k: np.asarray([r[k] for r in rows], np.float64) for k in ('bbox', 'dimensions', 'location', 'rotation_y')})
        objs.append(here)
    split = [len(o) for o in objs]
    L = sum(split)
    det, new, end = np.full(L, 5.0, np.float32), np.full(L, -0.5, np.float32), np.full(L, -0.5, np.float32)
    new[:split[0]] = 0.0
    end[L - split[-1]:] = 0.0
    links = []
    for g in range(1, SWAP_GAP + 1):
        row = []
        for t in range(SWAP_FRAMES - g):
            blk = np.full((split[t], split[t + g]), -5.0, np.float32)
            for j, a in enumerate(objs[t]):
                for k, b in enumerate(objs[t + g]):
                    if a == b:
                        blk[j, k] = 5.5
                    elif {a, b} == {0, 1} and t < SWAP_HOLE[0] and t + g > SWAP_HOLE[1]:
                        blk[j, k] = 6.0
            row.append(blk)
        links.append(row)
    return frames, objs, split, (det, links, new, end)
