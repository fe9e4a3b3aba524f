"""Wall time of the evaluation calls of mmmot_amd/evaluate.py on a synthetic input shaped like the KITTI validation
split: 11 sequences, about 3 000 frames, 5 to 12 boxes a frame on either side (tests/hota_cases.random_sequence: drifting
ground-truth boxes, jittered tracker boxes with an ID change half way, strays, DontCare areas).

--hota times ``hota_sequences`` (packing on the host, one upload, the launches of mmmot_hota, one read-back, the ratios)
beside the NumPy + scipy restatement tests/hota_ref.py on the same tables, and the packed tables alone through
``run_hota`` (upload, launches, read-back).  Every timed run ends in a synchronise; one untimed run first; each repeat
runs all of them in turn.  Whether the two records agree in their integer fields is reported.  Writes <out>/bench_hota.json.

--mot3d times ``evaluate_3d_sequences`` (3D IoU, 40 levels: packing, one upload, the launches of mmmot_mot3d, one
read-back, the ratios) and its single operating point (levels = 0) on 3D scenes of the same shape
(tests/mot3d_cases.random_sequence), beside the NumPy restatement tests/mot3d_ref.py, which is run once.  Whether the
two agree in the thresholds and the per-level counters is reported.  Writes <out>/bench_mot3d.json.

--clear-mot times ``evaluate_sequences`` (packing, one upload, the launches of mmmot_clear_mot, one read-back, the ratios)
on the workload of --hota.  Writes <out>/bench_clear_mot.json.

    python tools/bench_evaluate.py --hota --out <dir> [--repeats 3]
    python tools/bench_evaluate.py --clear-mot --out <dir> [--repeats 3]
    python tools/bench_evaluate.py --mot3d --out <dir> [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hota_cases  # noqa: E402
import hota_ref  # noqa: E402
from mmmot_amd import evaluate as E  # noqa: E402

FRAMES = [297, 800, 145, 373, 233, 106, 154, 294, 209, 270, 139]  # 3 020 frames in 11 sequences


def workload():
    rng = np.random.default_rng(2024)
    gts, trs = [], []
    for s, n in enumerate(FRAMES):
        counts = [tuple(int(v) for v in rng.integers(5, 13, 2)) for _ in range(n)]
        g, t = hota_cases.random_sequence(np.random.default_rng(9000 + s), counts, n_gid=40, n_stray=12)
        gts.append(g)
        trs.append(t)
    return gts, trs


def bench_hota(args):
    gts, trs = workload()
    p = E.pack_hota(gts, trs)
    params = [25., 0., 2., 1.]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    modes = {'hota_sequences': lambda: E.hota_sequences(gts, trs), 'run_hota': lambda: E.run_hota(p, params),
             'numpy_restatement': lambda: hota_ref.hota(gts, trs)}
    h, want = modes['hota_sequences'](), modes['numpy_restatement']()  # untimed
    modes['run_hota']()
    equal = all(np.array_equal(getattr(h, k), want[k]) for k in ('TP', 'FN', 'FP', 'IDTP', 'IDFN', 'IDFP'))
    times = {k: [] for k in modes}
    for _ in range(args.repeats):
        for k, fn in modes.items():
            times[k].append(timed(fn)[0])
    res = {'sequences': len(FRAMES), 'frames': int(sum(FRAMES)), 'gt_boxes': p['sizes'][0], 'tracker_boxes': p['sizes'][1],
           'id_pairs': p['sizes'][5], 'repeats': args.repeats, 'HOTA': h.HOTA, 'IDF1': h.IDF1, 'integer_fields_equal': equal,
           'seconds': {k: {'min': min(v), 'median': float(np.median(v)), 'max': max(v)} for k, v in times.items()}}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_hota.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def bench_clear_mot(args):
    gts, trs = workload()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    m = E.evaluate_sequences(gts, trs)  # untimed
    times = [timed(lambda: E.evaluate_sequences(gts, trs))[0] for _ in range(args.repeats)]
    res = {'sequences': len(FRAMES), 'frames': int(sum(FRAMES)), 'repeats': args.repeats, 'MOTA': float(m.MOTA),
           'tp': int(m.tp), 'fp': int(m.fp), 'fn': int(m.fn), 'id_switches': int(m.id_switches),
           'seconds': {'evaluate_sequences': {'min': min(times), 'median': float(np.median(times)), 'max': max(times)}}}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_clear_mot.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def bench_mot3d(args):
    import mot3d_cases
    import mot3d_ref
    rng = np.random.default_rng(2024)
    gts, trs = [], []
    for s, n in enumerate(FRAMES):
        counts = [tuple(int(v) for v in rng.integers(5, 13, 2)) for _ in range(n)]
        g, t = mot3d_cases.random_sequence(np.random.default_rng(9000 + s), counts, n_gid=40)
        gts.append(g)
        trs.append(t)
    p = E.pack_3d(gts, trs)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    modes = {'evaluate_3d_sequences': lambda: E.evaluate_3d_sequences(gts, trs),
             'evaluate_3d_sequences_levels0': lambda: E.evaluate_3d_sequences(gts, trs, levels=0)}
    m = modes['evaluate_3d_sequences']()  # untimed
    modes['evaluate_3d_sequences_levels0']()
    times = {k: [] for k in modes}
    for _ in range(args.repeats):
        for k, fn in modes.items():
            times[k].append(timed(fn)[0])
    t_ref, want = timed(lambda: mot3d_ref.sweep(E.concat(gts), E.concat(trs), '3d'))
    keys = ('tp', 'itp', 'fn', 'ifn', 'fp', 'n_itr', 'id_switches', 'fragments')
    equal = bool(np.array_equal(m.thr, want['thr'])) and all(
        m.counters[k][:8].tolist() == [want['levels'][k][q] for q in keys] for k in range(40) if want['reachable'][k])
    res = {'sequences': len(FRAMES), 'frames': int(sum(FRAMES)), 'gt_boxes': p['sizes'][0], 'tracker_boxes': p['sizes'][1],
           'cells': p['cells'], 'levels': 40, 'reachable': int(m.reachable.sum()), 'repeats': args.repeats, 'AMOTA': m.AMOTA,
           'sAMOTA': m.sAMOTA, 'AMOTP': m.AMOTP, 'thresholds_and_counters_equal': equal,
           'seconds': dict({k: {'min': min(v), 'median': float(np.median(v)), 'max': max(v)} for k, v in times.items()},
                           numpy_restatement={'once': t_ref})}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_mot3d.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--hota', action='store_true', help='time hota_sequences beside the NumPy restatement')
    ap.add_argument('--clear-mot', action='store_true', help='time evaluate_sequences')
    ap.add_argument('--mot3d', action='store_true', help='time evaluate_3d_sequences beside the NumPy restatement')
    ap.add_argument('--out', required=True)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not (args.hota or args.clear_mot or args.mot3d):
        ap.error('nothing to measure: give --hota, --clear-mot or --mot3d')
    if args.hota:
        bench_hota(args)
    if args.clear_mot:
        bench_clear_mot(args)
    if args.mot3d:
        bench_mot3d(args)
