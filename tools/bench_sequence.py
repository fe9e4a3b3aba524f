"""Frames/s of the three orders of a tracked sequence in one process (mmmot_amd/pipeline.py): per-pair (every frame
through the trunk twice, what bench.py's extra.pipeline times), online with cached appearance rows (reuse_appearance=True:
one trunk over the new frame's crops per pair) and offline (run_offline: the trunk over K frames per launch sequence, the
pairs B at a time on the rows).  Workload = bench.py's pipeline leg: 100 synthetic KITTI-shaped frames
(mmmot_amd.synth.make_frame(7000 + t, 120000, n_det), 10-12 detections), 224-pixel 8-bit crops, Fusion A, overlapped
stage A.  Each repeat runs every mode once, in turn; the wall clock of a run ends in a synchronise; one untimed run of
every mode first.  The scores of the three modes must be bitwise equal.  Writes <out>/bench_sequence.json.
--associate adds the device association to every pair (SequencePipeline(associate=True)), --track the track IDs as well
(track=True; implies --associate): the tracks of the three modes must then be equal too.  --ego gives every frame a pose
of a synthetic drive (mmmot_amd.synth.ego_poses), so each frame's points are aligned to the previous frame on the device
(DESIGN section 14); without it the camera stands still and nothing is aligned.
--window T [T ..] measures the windowed path instead (SequencePipeline(window=T), DESIGN section 12, always with
association and track IDs): frames/s of ``run`` and ``run_offline`` for the pair path (window 2) and for every T given,
each repeat running all of them in turn; the two orders of a window must give bitwise equal scores and equal tracks.
Writes <out>/bench_sequence_windows.json.
--streams S [S ..] measures the lockstep order (LockstepPipeline, DESIGN section 12 "Many sequences"): aggregate frames/s
over S sequences of the workload's shape (different seeds) stepped together, beside SequencePipeline(reuse_appearance=True,
associate=True, track=True) on one of them in the same run; sequence 0 of every lockstep run must equal that run bit for
bit.  Writes <out>/bench_sequence_streams.json.
--global-gap G [G ..] measures the whole-sequence order with skip links (run_global(max_gap=G), DESIGN section 11 "skip
links"): wall time of ``run_global`` per gap on the workload, every gap once per repeat, with the number of trajectories
each gap leaves; and the solver alone on a planted instance (T = 400 frames, 8 hidden tracks whose detections are missed
with probability 0.1): mmmot_associate_sequences beside mmmot_associate_sequences_gap at G = 1 and at the gaps given, in
one process, interleaved, HIP-event time of the operator call, median of --solver-calls calls.  Writes
<out>/bench_sequence_gaps.json.
--fill measures the gap filling alone (tracks.fill_gaps_batch; no model is built): 21 sequences of
--fill-frames frames in all (default 8000), 10 - 12 tracks a frame whose detections are missed with probability 0.1,
max_fill = 7, a standing camera (--ego: a synthetic drive per sequence).  HIP-event time of the operator call for all
sequences at once and for 21 calls, one per sequence, interleaved, median of --solver-calls after one untimed round; the
wall time of ``fill_gaps_batch`` (packing, upload, launches, copy, unpacking) and of the NumPy restatement
tests/fill_ref.py on the same tables, whose rows must equal the device's bit for bit.  Writes
<out>/bench_sequence_fill.json.
--smooth measures the track smoothing alone (tracks.smooth_tracks_batch; no model is built) on the
--fill scene after its gaps were filled on the device, the filled rows as unobserved ones, TrackSmoother() defaults:
HIP-event time of the operator call on resident blocks for all sequences at once and for 21 calls, interleaved, median
of --solver-calls after one untimed round; the wall time of ``smooth_tracks_batch`` and of the NumPy restatement
tests/smooth_ref.py on the same tables, whose block must equal the device's bit for bit.  Writes
<out>/bench_sequence_smooth.json.
--stitch measures the tracklet stitching alone (tracks.stitch_tracks_batch; no model is built) on the
--smooth scene with every track cut into tracklets by holes of 9 .. 20 frames, filled and smoothed first so that the rows
carry velocities: the operator on resident blocks as for --smooth, the wall time of ``stitch_tracks_batch`` and of the
NumPy restatement tests/stitch_ref.py on the same tables, whose block must equal the device's bit for bit (the fp64
objectives to 1e-9 relative).  Writes <out>/bench_sequence_stitch.json.
--gate G measures the motion gate (run_global(max_gap=G, gate=MotionGate(--gate-speed, --gate-slack)), DESIGN section 11
"motion gate") beside the same call with gate=None on the same feeds, interleaved: wall time of ``run_global``, the gap
pairs forwarded and left out, the links gated; and the gate's two launches alone on the sequence's own tables (the
count-only one and the one that gates the flat link scores in place), HIP-event time of the operator call, median of
--solver-calls calls, with the wall time of the copy that brings the kept counts back.  The synthetic frames hold
unrelated random boxes, so far more pairs are left out than in a real sequence.  Writes <out>/bench_sequence_gate.json.

    python tools/bench_sequence.py --out <dir> [--repeats 3] [--trunk f16x3] [-K 16] [-B 8] [--associate | --track] [--ego]
    python tools/bench_sequence.py --out <dir> --window 3 5 [--repeats 3] [-K 16] [-B 8] [-W 4] [--ego]
    python tools/bench_sequence.py --out <dir> --streams 1 2 4 8 16 [--frames 40] [--repeats 3]
    python tools/bench_sequence.py --out <dir> --global-gap 1 2 3 4 [--frames 100] [--repeats 3] [--solver-calls 20]
    python tools/bench_sequence.py --out <dir> --fill [--fill-frames 8000] [--ego] [--solver-calls 20]
    python tools/bench_sequence.py --out <dir> --smooth [--fill-frames 8000] [--ego] [--solver-calls 20]
    python tools/bench_sequence.py --out <dir> --stitch [--fill-frames 8000] [--ego] [--solver-calls 20]
    python tools/bench_sequence.py --out <dir> --gate 3 [--gate-speed 4.0] [--gate-slack 2.0] [--frames 100] [--ego]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmmot_amd import TrackingNet  # noqa: E402
from mmmot_amd.pipeline import SequencePipeline  # noqa: E402
from mmmot_amd.weights import init_module  # noqa: E402
from seq_workload import KW, detections, sequence_feeds  # noqa: E402


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and all(torch.equal(p, q) for p, q in zip(x[1], y[1]))
                                    and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]) for x, y in zip(a, b))


def flat(res):
    return [t for sc, a in res for t in (sc[0], sc[2], sc[3], *sc[1], a[0], a[2], a[3], *a[1])]


def bench_windows(args, model, dev):
    """frames/s of the windowed path beside the pair path, both orders, in one process"""
    n = args.frames
    ndet, feeds = detections(n), sequence_feeds(n, ego=0 if args.ego else None)
    K, B, W = args.frames_per_encode, args.pairs_per_forward, args.windows_per_forward
    modes = {}
    for T in [2] + sorted(set(args.window) - {2}):
        modes['window%d_run' % T] = (T, lambda p: p.run(feeds))
        modes['window%d_offline' % T] = (T, lambda p: p.run_offline(feeds, frames_per_encode=K, pairs_per_forward=B,
                                                                   windows_per_forward=W))
    make = lambda T: SequencePipeline(model, 224, associate=True, track=True, window=T)
    first, fps, stats, last_id = {}, {k: [] for k in modes}, {}, {}
    for name, (T, run) in modes.items():  # untimed: workspace growth, plan caches, first-forward range checks
        pipe = make(T)
        res = run(pipe)
        ref = first.setdefault(T, (flat(res), pipe.tracks))
        if len(ref[0]) != len(flat(res)) or not all(torch.equal(x, y) for x, y in zip(ref[0], flat(res))):
            raise SystemExit('%s: scores or assignments differ between the orders' % name)
        if not all(np.array_equal(x, y) for x, y in zip(ref[1], pipe.tracks)):
            raise SystemExit('%s: tracks differ between the orders' % name)
        last_id[T] = int(max(int(x.max()) for x in pipe.tracks if len(x)))
    for _ in range(args.repeats):
        for name, (T, run) in modes.items():
            pipe = make(T)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(pipe)
            torch.cuda.synchronize()
            fps[name].append((n - 1) / (time.perf_counter() - t0))
            stats[name] = dict(pipe.stats)
    med = {k: float(np.median(v)) for k, v in fps.items()}
    rec = {
        'frames_per_s': {k: round(v, 1) for k, v in med.items()},
        'frames_per_s_runs': {k: [round(x, 1) for x in v] for k, v in fps.items()},
        'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in fps.items()},
        'orders_bitwise_equal': True, 'ego': bool(args.ego), 'last_track_id': last_id, 'stats': stats,
        'trunk': model.engine().trunk, 'range_events': len(model.engine().range_events),
        'frames': n, 'repeats': args.repeats, 'frames_per_encode': K, 'pairs_per_forward': B, 'windows_per_forward': W,
        'device': torch.cuda.get_device_name(dev),
        'workload': '%d synthetic KITTI-shaped frames (make_frame(7000 + t, 120000, n_det)), %d-%d detections (mean %.1f), '
                    '224x224 8-bit crops, Fusion A, overlapped stage A, association and track IDs on; frames/s = '
                    '(frames - 1) per wall second, median of the repeats' % (n, ndet.min(), ndet.max(), ndet.mean()),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_windows.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def bench_streams(args, model, dev):
    """aggregate frames/s of LockstepPipeline over S copies of the workload (different seeds) beside the single-sequence
    online order on one of them, association and track IDs on, all in one process"""
    from mmmot_amd.pipeline import LockstepPipeline
    n, counts = args.frames, sorted(set(args.streams))
    if counts[0] < 1:
        raise SystemExit('--streams takes counts >= 1')
    streams = [sequence_feeds(n, seed=s) for s in range(counts[-1])]
    kw = dict(associate=True, track=True)
    modes = {'single': lambda: SequencePipeline(model, 224, reuse_appearance=True, **kw).run(streams[0])}
    for S in counts:
        modes['lockstep%d' % S] = lambda S=S: LockstepPipeline(model, 224, **kw).run(streams[:S])
    frames = dict({'lockstep%d' % S: S * (n - 1) for S in counts}, single=n - 1)
    want = flat(modes['single']())   # untimed, and the check: sequence 0 of every lockstep run equals the single run
    for name in list(modes)[1:]:
        got = flat(modes[name]()[0])
        if len(got) != len(want) or not all(torch.equal(x, y) for x, y in zip(got, want)):
            raise SystemExit('%s: sequence 0 differs from the single-sequence run' % name)
    fps = {k: [] for k in modes}
    for _ in range(args.repeats):
        for name, run in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            fps[name].append(frames[name] / (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in fps.items()}
    rec = {
        'frames_per_s': {k: round(v, 1) for k, v in med.items()},
        'frames_per_s_runs': {k: [round(x, 1) for x in v] for k, v in fps.items()},
        'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in fps.items()},
        'vs_single': {k: round(med[k] / med['single'], 3) for k in modes},
        'sequence0_bitwise_equal': True, 'trunk': model.engine().trunk, 'range_events': len(model.engine().range_events),
        'frames': n, 'repeats': args.repeats, 'streams': counts, 'device': torch.cuda.get_device_name(dev),
        'workload': 'S sequences of %d synthetic KITTI-shaped frames each (make_frame(7000 + 100000 s + t, 120000, n_det), '
                    '10-12 detections), 224x224 8-bit crops, Fusion A, overlapped stage A, association and track IDs on; '
                    'single = SequencePipeline(reuse_appearance=True) on sequence 0; frames/s = S (frames - 1) pairs per wall '
                    'second, median of the repeats' % n,
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_streams.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def planted_gaps(T, tracks, p_miss, G, seed=0):
    """(split, flat device scores [det | new | end | links gap by gap]) of ``tracks`` hidden tracks over T frames, each
    detection missed with probability p_miss (never in the first or the last frame): det in [5, 6], the links of one
    track in [5, 6], all others in [-6, -5], new / end in [-1, 0] with the eval zeros"""
    rng = np.random.default_rng(seed)
    frames = [[h for h in rng.permutation(tracks) if t in (0, T - 1) or rng.random() >= p_miss] for t in range(T)]
    split = [len(f) for f in frames]
    L = sum(split)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)
    det, new, end = u(5, 6, L), u(-1, 0, L), u(-1, 0, L)
    new[:split[0]] = 0
    end[L - split[-1]:] = 0
    links = []
    for g in range(1, G + 1):
        for t in range(T - g):
            same_track = np.equal.outer(np.asarray(frames[t]), np.asarray(frames[t + g]))
            links.append(np.where(same_track, u(5, 6, *same_track.shape), u(-6, -5, *same_track.shape)).reshape(-1))
    return split, torch.from_numpy(np.concatenate([det, new, end] + links)).cuda()


def bench_gaps(args, model, dev):
    """wall time of run_global per gap, and the solver alone: the old entry beside the new one, interleaved"""
    from mmmot_amd.association import gap_sequences_table, sequences_table
    n, gaps = args.frames, sorted(set(args.global_gap))
    if gaps[0] < 1 or gaps[-1] > 8:
        raise SystemExit('--global-gap takes gaps in 1 .. 8')
    feeds = sequence_feeds(n, ego=0 if args.ego else None)
    K, B = args.frames_per_encode, args.pairs_per_forward
    run = lambda G: SequencePipeline(model, 224).run_global(feeds, frames_per_encode=K, pairs_per_forward=B, max_gap=G)
    tracks = {G: run(G).n_tracks for G in gaps}  # untimed
    wall = {G: [] for G in gaps}
    for _ in range(args.repeats):
        for G in gaps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(G)
            torch.cuda.synchronize()
            wall[G].append(1e3 * (time.perf_counter() - t0))
    # the solver alone
    T, Gmax = 400, gaps[-1]
    split, flat = planted_gaps(T, 8, 0.1, Gmax)
    L, K1 = sum(split), sum(a * b for a, b in zip(split[:-1], split[1:]))
    parts = flat[0:L], flat[L:2 * L], flat[2 * L:3 * L], flat[3 * L:]
    old_tab = sequences_table([split])[:2]
    calls = {'sequences': lambda: torch.ops.mmmot.associate_sequences(*parts[:3], parts[3][:K1], *old_tab)}
    for G in sorted(set([1] + gaps)):
        tab = gap_sequences_table([split], G)[:2]
        calls['gap%d' % G] = lambda G=G, tab=tab: torch.ops.mmmot.associate_sequences_gap(*parts, *tab, G)
    ms, found = {k: [] for k in calls}, {}
    for i in range(args.solver_calls + 1):  # the first round untimed
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms[name].append(e0.elapsed_time(e1))
            found[name] = [int(x) for x in out[3][0].cpu()]
    if found['sequences'] != found['gap1']:
        raise SystemExit('the two entries differ at one gap: %s, %s' % (found['sequences'], found['gap1']))
    rec = {
        'run_global_ms': {str(G): round(float(np.median(v)), 2) for G, v in wall.items()},
        'run_global_ms_runs': {str(G): [round(x, 2) for x in v] for G, v in wall.items()},
        'run_global_trajectories': {str(G): t for G, t in tracks.items()},
        'solver_ms': {k: round(float(np.median(v)), 3) for k, v in ms.items()},
        'solver_ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        'solver_info': {k: dict(zip(('status', 'trajectories', 'augmentations', 'passes'), v)) for k, v in found.items()},
        'solver_instance': 'T = %d frames, 8 hidden tracks, p_miss = 0.1: L = %d detections, n_t = %d .. %d (mean %.1f)'
                           % (T, L, min(split), max(split), L / T),
        'solver_calls': args.solver_calls, 'frames': n, 'repeats': args.repeats, 'frames_per_encode': K,
        'pairs_per_forward': B, 'ego': bool(args.ego), 'trunk': model.engine().trunk,
        'device': torch.cuda.get_device_name(dev),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_gaps.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def bench_gate(args, model, dev):
    """run_global(max_gap=G) with and without a MotionGate, interleaved, and the gate's two launches alone"""
    from mmmot_amd.association import MotionGate, gap_pairs, pack_gate
    n, G = args.frames, args.gate
    if not 2 <= G <= 8 or n <= G:
        raise SystemExit('--gate takes a gap in 2 .. 8 and needs more frames than that')
    feeds = sequence_feeds(n, ego=0 if args.ego else None)
    K, B = args.frames_per_encode, args.pairs_per_forward
    gate = MotionGate(max_speed=args.gate_speed, slack=args.gate_slack)
    modes = {'plain': None, 'gated': gate}

    def run(g):
        pipe = SequencePipeline(model, 224)
        res = pipe.run_global(feeds, frames_per_encode=K, pairs_per_forward=B, max_gap=G, gate=g)
        return pipe, res

    stats, tracks = {}, {}
    for name, g in modes.items():  # untimed
        pipe, res = run(g)
        stats[name], tracks[name] = dict(pipe.stats), res.n_tracks
    wall = {k: [] for k in modes}
    for _ in range(args.repeats):
        for name, g in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(g)
            torch.cuda.synchronize()
            wall[name].append(1e3 * (time.perf_counter() - t0))
    # the two launches alone, on the tables of this sequence
    kept_feeds = [f for f in feeds if len(f.dets['bbox'])]
    p = pack_gate([f.dets for f in kept_feeds], None, [f.pose for f in kept_feeds] if args.ego else None,
                  feeds[0].info if args.ego else None, gap_pairs(len(kept_feeds), G))
    packed, sizes = gate.block(p)
    packed = torch.from_numpy(packed).cuda()
    link = torch.randn(p['n_link'], device='cuda')
    calls = {'count_only': lambda: torch.ops.mmmot.gate_links(packed, None, sizes, gate.max_size_ratio, gate.weight),
             'gate_in_place': lambda: torch.ops.mmmot.gate_links(packed, link, sizes, gate.max_size_ratio, gate.weight)}
    ms, copy_ms, kept = {k: [] for k in calls}, [], None
    for i in range(args.solver_calls + 1):  # the first round untimed
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = out.cpu()
            if i:
                ms[name].append(e0.elapsed_time(e1))
                copy_ms.append(1e3 * (time.perf_counter() - t0))
    rec = {
        'run_global_ms': {k: round(float(np.median(v)), 2) for k, v in wall.items()},
        'run_global_ms_runs': {k: [round(x, 2) for x in v] for k, v in wall.items()},
        'stats': stats, 'trajectories': tracks,
        'gap_pairs_forwarded': {k: v.get('gap_pairs', 0) for k, v in stats.items()},
        'gate_launch_ms': {k: round(float(np.median(v)), 4) for k, v in ms.items()},
        'gate_launch_ms_min_max': {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        'kept_copy_wall_ms': round(float(np.median(copy_ms)), 4),
        'blocks': int(sizes[2]), 'links': int(p['n_link']), 'links_kept': int(kept.sum()),
        'gate': {'max_speed': gate.max_speed, 'slack': gate.slack, 'max_dt': gate.max_dt, 'mode': gate.mode},
        'max_gap': G, 'calls': args.solver_calls, 'frames': n, 'repeats': args.repeats, 'frames_per_encode': K,
        'pairs_per_forward': B, 'ego': bool(args.ego), 'trunk': model.engine().trunk,
        'device': torch.cuda.get_device_name(dev),
        'note': 'the synthetic frames hold unrelated random boxes: the share of gap pairs left out is far larger than '
                'in a sequence whose objects persist',
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_gate.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def fill_workload(n_seq, n_frames, p_miss, ego, seed=0):
    """per sequence (frames, ids, None, None, poses, calib): 10 - 12 hidden tracks with linear boxes, every detection
    missed with probability p_miss"""
    from mmmot_amd import synth
    rng = np.random.default_rng(seed)
    calib = {'calib/R0_rect': synth.KITTI_R0, 'calib/Tr_velo_to_cam': synth.KITTI_TR,
             'calib/Tr_imu_to_velo': synth.KITTI_IMU2VELO}
    seqs = []
    for s in range(n_seq):
        T = n_frames // n_seq + (s < n_frames % n_seq)
        n = int(rng.integers(10, 13))
        x0, v = rng.uniform(-30, 30, (n, 3)), rng.uniform(-0.2, 0.2, (n, 3))
        frames, ids = [], []
        for t in range(T):
            seen = np.flatnonzero(rng.random(n) >= p_miss)
            loc = x0[seen] + v[seen] * t
            bbox = np.concatenate([loc[:, :2] * 10 + 500, loc[:, :2] * 10 + 580], 1)
            frames.append({'bbox': bbox, 'dimensions': np.tile([4.0, 1.5, 1.8], (len(seen), 1)), 'location': loc,
                           'rotation_y': 0.01 * t + 0.3 * seen})
            ids.append(seen.astype(np.int64))
        seqs.append((frames, ids, None, None, synth.ego_poses(T, s) if ego else None, calib if ego else None))
    return seqs


def bench_fill(args):
    """the operator for all sequences at once beside one call per sequence, and the host routes around them"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import fill_ref
    from mmmot_amd import tracks
    max_fill, n_seq = 7, 21
    seqs = fill_workload(n_seq, args.fill_frames, 0.1, args.ego)
    up = lambda p: (torch.from_numpy(p['packed']).cuda(), p['sizes'])
    t0 = time.perf_counter()
    p = tracks.pack_fill(seqs, max_fill)
    pack_ms = 1e3 * (time.perf_counter() - t0)
    batch, singles = up(p), [up(tracks.pack_fill([s], max_fill)) for s in seqs]
    calls = {'batch': lambda: [torch.ops.mmmot.fill_tracks(*batch)],
             'singles': lambda: [torch.ops.mmmot.fill_tracks(*b) for b in singles]}
    ms, out = {k: [] for k in calls}, {}
    for i in range(args.solver_calls + 1):  # the first round untimed
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = call()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms[name].append(e0.elapsed_time(e1))
    wall = []
    for _ in range(4):  # the first untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        filled = tracks.fill_gaps_batch(seqs, max_fill)
        wall.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    ref = fill_ref.fill(p['det'], p['ids'], p['frame_start'], p['frame_no'], p['seq_start'], p['xf'], p['wtab'], max_fill,
                        p['sizes'][4])
    ref_ms = 1e3 * (time.perf_counter() - t0)
    got = out['batch'][0].cpu().numpy()
    if not np.array_equal(got, fill_ref.block_of(ref, p['sizes'])):
        raise SystemExit('the device rows differ from the restatement')
    rows = [int(b.cpu().numpy()[-4 + 1]) for b in out['singles']]
    if rows != [f.info['rows'] for f in filled] or sum(rows) != len(ref['out']):
        raise SystemExit('the single calls and the batch count different rows')
    L, F = p['sizes'][0], p['sizes'][1]
    rec = {
        'op_ms': {k: round(float(np.median(v)), 3) for k, v in ms.items()},
        'op_ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        'fill_gaps_batch_wall_ms': round(float(np.median(wall[1:])), 1), 'pack_fill_wall_ms': round(pack_ms, 1),
        'numpy_restatement_wall_ms': round(ref_ms, 1),
        'instance': '%d sequences, %d frames, %d detections, p_miss = 0.1, max_fill = %d: %d rows from %d links, %d links '
                    'too long' % (n_seq, F, L, max_fill, len(ref['out']), int(ref['info'][:, 2].sum()),
                                  int(ref['info'][:, 3].sum())),
        'calls': args.solver_calls, 'ego': bool(args.ego), 'device': torch.cuda.get_device_name(0),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_fill.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def bench_smooth(args):
    """the smoothing operator for all sequences at once beside one call per sequence, and the host routes around them"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import smooth_ref
    from mmmot_amd import tracks
    n_seq = 21
    filled = tracks.fill_gaps_batch(fill_workload(n_seq, args.fill_frames, 0.1, args.ego), 7)
    base = fill_workload(n_seq, args.fill_frames, 0.1, args.ego)
    seqs = [(f.frames, f.ids, None, [~m for m in f.filled], b[4], b[5]) for f, b in zip(filled, base)]
    up = lambda p: (torch.from_numpy(p['packed']).cuda(), p['sizes'])
    t0 = time.perf_counter()
    p = tracks.pack_smooth(seqs)
    pack_ms = 1e3 * (time.perf_counter() - t0)
    batch, singles = up(p), [up(tracks.pack_smooth([s])) for s in seqs]
    calls = {'batch': lambda: [torch.ops.mmmot.smooth_tracks(*batch)],
             'singles': lambda: [torch.ops.mmmot.smooth_tracks(*b) for b in singles]}
    ms, out = {k: [] for k in calls}, {}
    for i in range(args.solver_calls + 1):  # the first round untimed
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = call()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms[name].append(e0.elapsed_time(e1))
    wall = []
    for _ in range(4):  # the first untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smoothed = tracks.smooth_tracks_batch(seqs)
        wall.append(1e3 * (time.perf_counter() - t0))
    print('device done, the restatement runs', flush=True)
    t0 = time.perf_counter()
    prm = dict(zip(smooth_ref.PARAMS, p['smoother'].params()), yaw_flip=p['smoother'].yaw_flip)
    ref = smooth_ref.smooth(p['det'], p['ids'], p['frame_start'], p['frame_no'], p['seq_start'], p['observed'], p['xf0'],
                            **prm)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    if not np.array_equal(out['batch'][0].cpu().numpy(), smooth_ref.block_of(ref, p['sizes'])):
        raise SystemExit('the device block differs from the restatement')
    info = [b.cpu().numpy()[-4:].tolist() for b in out['singles']]
    if info != ref['info'].tolist() or [list(s.info.values()) for s in smoothed] != [r[1:] for r in info]:
        raise SystemExit('the single calls and the batch report different counters')
    L, F = p['sizes'][0], p['sizes'][1]
    rec = {
        'op_ms': {k: round(float(np.median(v)), 3) for k, v in ms.items()},
        'op_ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        'smooth_tracks_batch_wall_ms': round(float(np.median(wall[1:])), 1), 'pack_smooth_wall_ms': round(pack_ms, 1),
        'numpy_restatement_wall_ms': round(ref_ms, 1),
        'instance': '%d sequences, %d frames, %d rows (%d of them filled, unobserved): %d tracks smoothed, %d rows '
                    'changed, %d copied; longest track %d rows'
                    % (n_seq, F, L, int((p['observed'] == 0).sum()), int(ref['info'][:, 1].sum()),
                       int(ref['info'][:, 2].sum()), int(ref['info'][:, 3].sum()), max(len(s[0]) for s in seqs)),
        'calls': args.solver_calls, 'ego': bool(args.ego), 'device': torch.cuda.get_device_name(0),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_smooth.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def cut_tracks(seqs, seed=1):
    """the sequences of ``fill_workload`` with every track cut into tracklets: about every 60 frames an object is hidden
    for 9 .. 20 frames - longer than the 8 frames the sequence flow bridges - and comes back under a fresh ID"""
    rng = np.random.default_rng(seed)
    out = []
    for frames, ids, no, scores, poses, calib in seqs:
        T, n = len(frames), 1 + max(int(i.max(initial=-1)) for i in ids)
        hidden, label, fresh = np.zeros((T, n), bool), np.zeros((T, n), np.int64), n
        for o in range(n):
            t, cur = int(rng.integers(20, 60)), o
            label[:, o] = o
            while t < T:
                h = int(rng.integers(9, 21))
                hidden[t:t + h, o] = True
                cur, fresh = fresh, fresh + 1
                label[t + h:, o] = cur
                t += h + int(rng.integers(40, 80))
        nf, ni = [], []
        for t, (d, fid) in enumerate(zip(frames, ids)):
            keep = ~hidden[t, fid]
            nf.append({k: np.asarray(v)[keep] for k, v in d.items()})
            ni.append(label[t, fid[keep]])
        out.append((nf, ni, no, scores, poses, calib))
    return out


def bench_stitch(args):
    """the stitching operator for all sequences at once beside one call per sequence, and the host routes around them"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import stitch_ref
    from mmmot_amd import tracks
    n_seq = 21
    base = cut_tracks(fill_workload(n_seq, args.fill_frames, 0.1, args.ego))
    filled = tracks.fill_gaps_batch(base, 7)
    smoothed = tracks.smooth_tracks_batch([(f.frames, f.ids, None, [~m for m in f.filled], b[4], b[5])
                                           for f, b in zip(filled, base)])
    seqs = [(s.frames, s.ids, None, s.velocity, b[4], b[5]) for s, b in zip(smoothed, base)]
    up = lambda p: (torch.from_numpy(p['packed']).cuda(), p['sizes'])
    t0 = time.perf_counter()
    p = tracks.pack_stitch(seqs)
    pack_ms = 1e3 * (time.perf_counter() - t0)
    batch, singles = up(p), [up(tracks.pack_stitch([s])) for s in seqs]
    calls = {'batch': lambda: [torch.ops.mmmot.stitch_tracks(*batch)],
             'singles': lambda: [torch.ops.mmmot.stitch_tracks(*b) for b in singles]}
    ms, out = {k: [] for k in calls}, {}
    for i in range(args.solver_calls + 1):  # the first round untimed
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = call()
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms[name].append(e0.elapsed_time(e1))
    wall = []
    for _ in range(4):  # the first untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stitched = tracks.stitch_tracks_batch(seqs)
        wall.append(1e3 * (time.perf_counter() - t0))
    print('device done, the restatement runs', flush=True)
    k = p['stitcher']
    t0 = time.perf_counter()
    ref = stitch_ref.stitch(p['det'], p['ids'], p['frame_start'], p['frame_no'], p['seq_start'], p['vel'], p['xf0'],
                            p['k_start'], p['pairs'], p['r2'], p['inv_r2'], k.min_dt, k.max_dt, k.min_rows,
                            stitch_ref.MODES[k.mode], k.max_size_ratio, k.gap_penalty, max_k=p['sizes'][5],
                            n_link=p['sizes'][4])
    ref_ms = 1e3 * (time.perf_counter() - t0)
    got, want = out['batch'][0].cpu().numpy(), stitch_ref.block_of(ref, p['sizes'])
    S = p['sizes'][2]
    if not np.array_equal(got[2 * S:], want[2 * S:]):  # behind the fp64 objectives, which are compared by value
        raise SystemExit('the device block differs from the restatement')
    obj = np.abs(got[:2 * S].view(np.float64) - ref['objective'])
    if not (obj <= 1e-9 * np.abs(ref['objective'])).all():
        raise SystemExit('the objectives differ from the restatement by %g' % obj.max())
    info = [b.cpu().numpy()[-4:].tolist() for b in out['singles']]
    if info != ref['info'].tolist() or [list(s.info.values()) for s in stitched] != [r[1:] for r in info]:
        raise SystemExit('the single calls and the batch report different counters')
    L, F = p['sizes'][0], p['sizes'][1]
    K = np.diff(p['k_start'])
    rec = {
        'op_ms': {k: round(float(np.median(v)), 3) for k, v in ms.items()},
        'op_ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        'stitch_tracks_batch_wall_ms': round(float(np.median(wall[1:])), 1), 'pack_stitch_wall_ms': round(pack_ms, 1),
        'numpy_restatement_wall_ms': round(ref_ms, 1), 'objective_difference': float(obj.max()),
        'instance': '%d sequences, %d frames, %d rows: %d tracklets (%d .. %d a sequence), %d links with a score, %d '
                    'stitches, %d rows relabelled'
                    % (n_seq, F, L, int(K.sum()), int(K.min()), int(K.max()), int(np.isfinite(ref['links']).sum()),
                       int(ref['info'][:, 2].sum()), int(ref['info'][:, 3].sum())),
        'calls': args.solver_calls, 'ego': bool(args.ego), 'device': torch.cuda.get_device_name(0),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence_stitch.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--trunk', default='f16x3')
    ap.add_argument('-K', '--frames-per-encode', type=int, default=16)
    ap.add_argument('-B', '--pairs-per-forward', type=int, default=8)
    ap.add_argument('--associate', action='store_true')
    ap.add_argument('--track', action='store_true')
    ap.add_argument('--ego', action='store_true', help='a moving camera: align every frame to the one before it')
    ap.add_argument('--window', type=int, nargs='+', default=None,
                    help='measure the windowed path for these window lengths (3 .. 8) beside the pair path')
    ap.add_argument('-W', '--windows-per-forward', type=int, default=4)
    ap.add_argument('--streams', type=int, nargs='+', default=None,
                    help='measure LockstepPipeline over these numbers of sequences (e.g. 1 2 4 8 16) beside one sequence alone')
    ap.add_argument('--global-gap', type=int, nargs='+', default=None,
                    help='time run_global(max_gap=G) for these gaps (1 .. 8) and the sequence solvers alone')
    ap.add_argument('--solver-calls', type=int, default=20)
    ap.add_argument('--fill', action='store_true', help='time the gap filling alone: all sequences at once, one call each, NumPy')
    ap.add_argument('--fill-frames', type=int, default=8000)
    ap.add_argument('--smooth', action='store_true',
                    help='time the track smoothing alone on the filled --fill scene: all sequences at once, one call each, NumPy')
    ap.add_argument('--stitch', action='store_true',
                    help='time the tracklet stitching alone on the --smooth scene with its tracks cut by holes longer than '
                         '8 frames: all sequences at once, one call each, NumPy')
    ap.add_argument('--gate', type=int, default=None,
                    help='time run_global(max_gap=G) with and without a MotionGate, and the gate launches alone')
    ap.add_argument('--gate-speed', type=float, default=4.0, help='MotionGate(max_speed=), metres per frame')
    ap.add_argument('--gate-slack', type=float, default=2.0, help='MotionGate(slack=), metres')
    args = ap.parse_args()
    if args.fill:
        return bench_fill(args)
    if args.smooth:
        return bench_smooth(args)
    if args.stitch:
        return bench_stitch(args)
    assoc = args.associate or args.track
    kw = dict(associate=assoc, track=True) if args.track else dict(associate=assoc)
    if args.repeats < 3 or args.frames < 2:
        raise SystemExit('--repeats must be >= 3 and --frames >= 2')
    dev = torch.device('cuda', 0)
    model = TrackingNet(**KW)
    init_module(model, seed=0)
    model.eval().to(dev)
    model.set_trunk(args.trunk)
    if args.window:
        return bench_windows(args, model, dev)
    if args.streams:
        return bench_streams(args, model, dev)
    if args.global_gap:
        return bench_gaps(args, model, dev)
    if args.gate:
        return bench_gate(args, model, dev)
    n = args.frames
    ndet, feeds = detections(n), sequence_feeds(n, ego=0 if args.ego else None)
    K, B = args.frames_per_encode, args.pairs_per_forward
    modes = {
        'per_pair': lambda p: p.run(feeds),
        'online': lambda p: p.run(feeds),
        'offline': lambda p: p.run_offline(feeds, frames_per_encode=K, pairs_per_forward=B),
    }
    make = {'per_pair': lambda: SequencePipeline(model, 224, **kw), 'offline': lambda: SequencePipeline(model, 224, **kw),
            'online': lambda: SequencePipeline(model, 224, reuse_appearance=True, **kw)}
    scores = (lambda res: [r[0] for r in res]) if assoc else (lambda res: res)
    results, stats, fps, tracks = {}, {}, {k: [] for k in modes}, {}
    for name, run in modes.items():  # untimed: workspace growth, plan caches, first-forward range checks
        pipe = make[name]()
        results[name] = scores(run(pipe))
        tracks[name] = pipe.tracks
    if args.track and not all(len(tracks[k]) == n and all(np.array_equal(x, y) for x, y in zip(tracks[k], tracks['per_pair']))
                              for k in modes):
        raise SystemExit('the tracks of the three orders differ')
    for _ in range(args.repeats):
        for name, run in modes.items():
            pipe = make[name]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run(pipe)
            torch.cuda.synchronize()
            fps[name].append((n - 1) / (time.perf_counter() - t0))
            stats[name] = dict(pipe.stats)
            if not same(scores(res), results['per_pair']):
                raise SystemExit('%s: scores differ from the per-pair order' % name)
    med = {k: float(np.median(v)) for k, v in fps.items()}
    rec = {
        'frames_per_s': {k: round(v, 1) for k, v in med.items()},
        'frames_per_s_runs': {k: [round(x, 1) for x in v] for k, v in fps.items()},
        'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in fps.items()},
        'speedup_vs_per_pair': {k: round(med[k] / med['per_pair'], 3) for k in modes},
        'bitwise_equal': True,
        'associate': assoc, 'track': bool(args.track), 'ego': bool(args.ego),
        'last_track_id': int(max(int(x.max()) for x in tracks['per_pair'] if len(x))) if args.track else None,
        'stats': stats,
        'trunk': model.engine().trunk,
        'range_events': len(model.engine().range_events),
        'frames': n, 'repeats': args.repeats, 'frames_per_encode': K, 'pairs_per_forward': B,
        'device': torch.cuda.get_device_name(dev),
        'workload': '%d synthetic KITTI-shaped frames (make_frame(7000 + t, 120000, n_det)), %d-%d detections (mean %.1f), '
                    '224x224 8-bit crops, Fusion A, overlapped stage A; frames/s = (frames - 1) pairs per wall second, '
                    'median of the repeats' % (n, ndet.min(), ndet.max(), ndet.mean()),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_sequence.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
