#!/usr/bin/env python
"""Makes tests/golden/track_ids_*.npz and tests/golden/tracks_kitti_0001.txt with the REFERENCE's own ID bookkeeping.

    python tools/gen_golden_tracks.py --reference /path/to/mmMOT

The reference's ``TrackingModule`` is imported from its checkout (nothing of it is copied); the modules its imports
pull in and this step never calls (``solvers``, ``pyproj``, ``cv2``, ``numba.njit``) are replaced by stand-ins.  Per
seeded sequence and per pair, scores come from tests/association_ref.random_instance, the assignment from ``lsa_route``
(a genuine solver output), and ``assign_det_id`` + ``align_id`` run on synthetic ``dets`` dicts with distinct boxes.
Stored per sequence, as data only: N, M and the frame indices of every pair, the pairs' assignment blocks
[det L | new L | end L | link N*M] (uint8), and what the reference returned after every pair: the IDs of the emitted
frames (kept detections only), ``frame_start`` and ``last_id``; also the final ``frames_id`` list.  The KITTI-shaped
sequence also keeps its ``dets`` and the text ``write_kitti_result`` wrote for it.
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from association_ref import feasible, lsa_route, random_instance  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REJECT = -100.0  # a det score that rejects the detection whatever its other scores


def import_reference(path):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def njit(*a, **k):
        return a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f)
    stub('solvers', ortools_solve=None)
    stub('pyproj')
    stub('cv2')
    stub('numba', njit=njit, jit=njit)
    sys.path.insert(0, path)
    from tracking_model import TrackingModule
    from utils.data_util import write_kitti_result
    return TrackingModule, write_kitti_result


def make_dets(rng, n, frame):
    """one frame's detections as the reference's dataset hands them over ([1, n, ...] tensors), boxes distinct"""
    x0 = np.sort(rng.choice(1100, n, replace=False)).astype(np.float32) + rng.random(n).astype(np.float32)
    y0 = (150 + 100 * rng.random(n)).astype(np.float32)
    bbox = np.stack([x0, y0, x0 + 30 + 60 * rng.random(n), y0 + 30 + 60 * rng.random(n)], 1).astype(np.float32)
    d = {'name': rng.integers(0, 6, n).astype(np.int64),
         'truncated': np.round(rng.random(n), 2).astype(np.float32),
         'occluded': rng.integers(0, 3, n).astype(np.int64),
         'alpha': (rng.random(n) * 6 - 3).astype(np.float32),
         'bbox': bbox,
         'dimensions': (1 + 3 * rng.random((n, 3))).astype(np.float32),
         'location': (rng.standard_normal((n, 3)) * 20).astype(np.float32),
         'rotation_y': (rng.random(n) * 6 - 3).astype(np.float32),
         'frame_idx': np.int64(frame)}
    return d


def as_ref(d):
    r = {k: torch.from_numpy(np.asarray(v)).unsqueeze(0) for k, v in d.items() if k != 'frame_idx'}
    r['frame_idx'] = torch.tensor([int(d['frame_idx'])])
    return r


def run_sequence(TrackingModule, rng, frames, pairs, reject0=(), reject1=(), scale=1.0):
    """frames: {frame index: detection count}; pairs: [(f0, f1)]; reject0 / reject1: indices of the pairs whose first /
    second frame keeps nothing.  Returns the fixture dict, the per-frame dets and the tracker."""
    dets = {f: make_dets(rng, n, f) for f, n in frames.items()}
    tm = TrackingModule(types.SimpleNamespace(test_mode=0), None, None, det_type='3D')
    tm.clear_mem()
    out = {'N': [], 'M': [], 'frame_idx': [], 'blocks': [], 'emit_len': [], 'emit_ids': [], 'frame_start': [], 'last_id': []}
    for p, (f0, f1) in enumerate(pairs):
        N, M = frames[f0], frames[f1]
        det, new, end, link = random_instance(rng, N, M, scale, 'eval' if p % 2 == 0 else 'masked')
        if p in reject0:
            det[:N] = REJECT
        if p in reject1:
            det[N:] = REJECT
        (a_det, a_link, a_new, a_end), _ = lsa_route(det, new, end, link, N, M)
        assert feasible((a_det, a_link, a_new, a_end), N, M)
        ids, _, start = tm.assign_then_align(a_det, a_link, a_new, a_end, N, M, [as_ref(dets[f0]), as_ref(dets[f1])])
        lens = [-1, -1]
        for k, e in enumerate(ids):
            e = np.asarray(e, dtype=np.int64).reshape(-1)
            lens[k + (2 - len(ids))] = len(e)
            out['emit_ids'].append(e)
        out['N'].append(N)
        out['M'].append(M)
        out['frame_idx'].append((f0, f1))
        out['blocks'].append(np.concatenate([a_det, a_new, a_end, a_link.reshape(-1)]).astype(np.uint8))
        out['emit_len'].append(lens)
        out['frame_start'].append(start)
        out['last_id'].append(int(tm.last_id))
    fx = {'N': np.asarray(out['N'], np.int32), 'M': np.asarray(out['M'], np.int32),
          'frame_idx': np.asarray(out['frame_idx'], np.int32).reshape(-1, 2),
          'blocks': np.concatenate(out['blocks']), 'emit_len': np.asarray(out['emit_len'], np.int32).reshape(-1, 2),
          'emit_ids': np.concatenate(out['emit_ids']).astype(np.int64),
          'frame_start': np.asarray(out['frame_start'], np.int32), 'last_id': np.asarray(out['last_id'], np.int64),
          'frames_id_len': np.asarray([len(x) for x in tm.frames_id], np.int32),
          'frames_id': np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in tm.frames_id] + [np.zeros(0, np.int64)]),
          'frames_id_frame': np.asarray([int(d['frame_idx'][0]) for d in tm.frames_det], np.int32)}
    return fx, dets, tm


def chain(idx):
    return [(a, b) for a, b in zip(idx[:-1], idx[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('MMMOT_REFERENCE'), required='MMMOT_REFERENCE' not in os.environ)
    args = ap.parse_args()
    TrackingModule, write_kitti_result = import_reference(args.reference)

    def assign_then_align(self, a_det, a_link, a_new, a_end, N, M, dets):
        t = lambda x: torch.from_numpy(np.asarray(x, np.float32))
        ids, out = self.assign_det_id(t(a_det), [t(a_link).view(1, N, M)], t(a_new), t(a_end),
                                      [torch.tensor([N]), torch.tensor([M])], dets)
        return self.align_id(ids, out)
    TrackingModule.assign_then_align = assign_then_align

    os.makedirs(GOLDEN, exist_ok=True)
    seqs = {}
    # KITTI shape: 40 frames of 10-12 detections, a gap after frame 24 (case b), the second frame of pair 17 keeps nothing
    rng = np.random.default_rng(1)
    idx = list(range(25)) + list(range(30, 45))
    frames = {f: int(rng.integers(10, 13)) for f in idx}
    pairs = chain(idx[:25]) + chain(idx[25:])
    seqs['kitti'] = run_sequence(TrackingModule, rng, frames, pairs, reject1={17})
    # a sequence start whose first frame keeps nothing; later both a quirk pair and an EMPTY frame (no detections)
    rng = np.random.default_rng(2)
    idx = list(range(10))
    frames = {f: int(rng.integers(5, 10)) for f in idx}
    frames[6] = 0
    seqs['start'] = run_sequence(TrackingModule, rng, frames, chain(idx), reject0={0}, reject1={3})
    rng = np.random.default_rng(3)
    seqs['n64'] = run_sequence(TrackingModule, rng, {f: 64 for f in range(6)}, chain(list(range(6))))
    rng = np.random.default_rng(4)
    seqs['n12x100'] = run_sequence(TrackingModule, rng, {f: (12, 100)[f % 2] for f in range(6)}, chain(list(range(6))),
                                   reject1={2})
    rng = np.random.default_rng(5)
    seqs['n300'] = run_sequence(TrackingModule, rng, {0: 300, 1: 260, 2: 300, 3: 131}, chain(list(range(4))))

    for name, (fx, dets, tm) in seqs.items():
        if name == 'kitti':
            for f, d in dets.items():
                for k, v in d.items():
                    if k != 'frame_idx':
                        fx['dets_%d_%s' % (f, k)] = v
            with tempfile.TemporaryDirectory() as tmp:
                write_kitti_result(tmp, '0001', 'golden', tm.frames_id, tm.frames_det, part='val')
                text = open(os.path.join(tmp, 'golden', 'val', '0001.txt')).read()
            with open(os.path.join(GOLDEN, 'tracks_kitti_0001.txt'), 'w') as f:
                f.write(text)
        path = os.path.join(GOLDEN, 'track_ids_%s.npz' % name)
        np.savez_compressed(path, **fx)
        print('%-8s pairs %3d  case c %3d  last_id %4d  %7d bytes' % (name, len(fx['N']), int(fx['frame_start'].sum()),
                                                                     int(fx['last_id'][-1]), os.path.getsize(path)))


if __name__ == '__main__':
    main()
