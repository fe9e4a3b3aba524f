"""A/B of a tracked sequence between a PARENT tree and this tree, both sides in the SAME mode (--mode plain: scores only;
associate: SequencePipeline(associate=True); track: associate=True, track=True), on one device in one job, in alternating
child processes (as tools/ab_forward.py alternates its builds): per-pair order, online (reuse_appearance=True) and
run_offline.  Workload = tools/seq_workload.py's (synthetic KITTI-shaped frames, 10-12 detections, 224-pixel 8-bit crops,
Fusion A, overlapped stage A), 40 frames.  Each child builds the workload, runs every order once untimed and once timed
(wall clock between synchronises); the medians and spreads over the children of a side are reported per mode and order,
and whether this tree's median lies inside the parent side's min - max.  With the track mode also the HIP-event time of
the ID launch alone for B = 1 / 8 / 64 pairs of 12 x 12.  Writes <out>/ab_sequence.json.

    python tools/ab_sequence.py --parent <checkout of the parent commit, library built> --out profiles/seq
                                [--mode plain associate track] [--repeats 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {'plain': {}, 'associate': {'associate': True}, 'track': {'associate': True, 'track': True}}
ORDERS = ('per_pair', 'online', 'offline')


def child(root, mode, frames):
    sys.path.insert(0, root)   # the package of ``root``; the workload module (beside this file) imports it lazily
    import torch
    from mmmot_amd import TrackingNet
    from mmmot_amd.pipeline import SequencePipeline
    from mmmot_amd.weights import init_module
    from seq_workload import KW, sequence_feeds
    import mmmot_amd
    assert os.path.realpath(os.path.dirname(mmmot_amd.__file__)).startswith(os.path.realpath(root))
    model = TrackingNet(**KW)
    init_module(model, seed=0)
    model.eval().to('cuda')
    model.set_trunk('f16x3')
    feeds = sequence_feeds(frames)
    runs = {'per_pair': (lambda p: p.run(feeds), {}), 'online': (lambda p: p.run(feeds), {'reuse_appearance': True}),
            'offline': (lambda p: p.run_offline(feeds), {})}
    out = {}
    for name in ORDERS:
        run, kw = runs[name]
        run(SequencePipeline(model, 224, **kw, **MODES[mode]))
        pipe = SequencePipeline(model, 224, **kw, **MODES[mode])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(pipe)
        torch.cuda.synchronize()
        out[name] = (frames - 1) / (time.perf_counter() - t0)
    print('AB_SEQUENCE ' + json.dumps(out))


def launch_times():
    """HIP-event microseconds of the ID launch alone (median of 200), B consecutive 12 x 12 pairs of one sequence"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from mmmot_amd.tracks import TrackState, queue_ids
    rng = np.random.default_rng(0)
    n, res = 12, {}
    for B in (1, 8, 64):
        blocks = []
        for _ in range(B):  # a feasible assignment: k links, the other detections kept at random
            k = int(rng.integers(4, 10))
            rows, cols = rng.permutation(n)[:k], rng.permutation(n)[:k]
            link = np.zeros((n, n), np.float32)
            link[rows, cols] = 1
            x0, x1 = (rng.random(n) < 0.7).astype(np.float32), (rng.random(n) < 0.7).astype(np.float32)
            m0, m1 = link.sum(1) > 0, link.sum(0) > 0
            det = np.concatenate([np.where(m0, 1, x0), np.where(m1, 1, x1)])
            new = np.concatenate([np.where(m0, 1, x0), np.where(m1, 0, x1)])
            end = np.concatenate([np.where(m0, 0, x0), np.where(m1, 1, x1)])
            blocks.append(np.concatenate([det, new, end, link.reshape(-1)]).astype(np.float32))
        blocks = torch.from_numpy(np.concatenate(blocks)).cuda()
        state, splits, fidx = TrackState('cuda'), [(n, n)] * B, [(t, t + 1) for t in range(B)]
        ts = []
        for i in range(220):
            state.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            queue_ids(state, blocks, splits, fidx)   # the table upload, the launch and the flag's gather
            e1.record()
            torch.cuda.synchronize()
            if i >= 20:
                ts.append(e0.elapsed_time(e1) * 1e3)
        assert state.read()['flags'] == 0
        res['B%d' % B] = {'median_us': round(float(np.median(ts)), 1), 'min_us': round(min(ts), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent')
    ap.add_argument('--out')
    ap.add_argument('--mode', nargs='+', choices=list(MODES), default=list(MODES))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--child', nargs=2, metavar=('ROOT', 'MODE'))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.frames)
    if not args.parent or not args.out or args.repeats < 5:
        raise SystemExit('--parent, --out and --repeats >= 5 are needed')
    import numpy as np
    sides = {'parent': os.path.abspath(args.parent), 'tree': ROOT}
    runs = {m: {side: {o: [] for o in ORDERS} for side in sides} for m in args.mode}
    for r in range(args.repeats):
        for mode in args.mode:
            for side, root in sides.items():
                env = dict(os.environ, PYTHONPATH=root)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', root, mode, '--frames',
                                    str(args.frames)], cwd=root, env=env, stdout=subprocess.PIPE, timeout=300)
                if p.returncode != 0:
                    raise SystemExit('child %s failed with status %d' % (side, p.returncode))  # nothing more is started
                line = [l for l in p.stdout.decode().splitlines() if l.startswith('AB_SEQUENCE ')][-1]
                for k, v in json.loads(line[len('AB_SEQUENCE '):]).items():
                    runs[mode][side][k].append(v)
                print(r, mode, side, line, flush=True)
    rec = {'frames': args.frames, 'repeats': args.repeats, 'unit': 'frames/s, (frames - 1) pairs per wall second'}
    for mode in args.mode:
        rec[mode] = {side: {o: {'median': round(float(np.median(v)), 1), 'min': round(min(v), 1), 'max': round(max(v), 1),
                                'spread': round((max(v) - min(v)) / float(np.median(v)), 4), 'runs': [round(x, 1) for x in v]}
                            for o, v in runs[mode][side].items()} for side in sides}
        par, tree = rec[mode]['parent'], rec[mode]['tree']
        rec[mode]['tree_over_parent'] = {o: round(tree[o]['median'] / par[o]['median'], 4) for o in ORDERS}
        rec[mode]['tree_median_inside_parent_range'] = {o: par[o]['min'] <= tree[o]['median'] <= par[o]['max']
                                                        for o in ORDERS}
    if 'track' in args.mode:
        rec['id_launch'] = launch_times()
    import torch
    rec['device'] = torch.cuda.get_device_name(0)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'ab_sequence.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
