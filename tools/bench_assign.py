"""Cost of the device frame-pair association (csrc/assign.hip) beside its host stand-ins and inside a tracked sequence.

* device: HIP-event time per launch (median of --iters after warm-up) of mmmot_associate_pairs for B in {1, 16, 64} x
  N = M in {12, 64, 128} plus one uneven shape, for every kernel variant (0 = the automatic choice);
* host: the same instances (one pair) through scipy.optimize.milp on the literal two-frame program (tests/association_ref,
  what ortools' CBC would be handed; ortools itself is not installed) and through linear_sum_assignment on the reduction;
* pipeline: frames/s of SequencePipeline.run with associate=True against False on tools/bench_sequence.py's workload
  (synthetic KITTI-shaped frames, 10-12 detections, 224-pixel 8-bit crops, Fusion A), alternating, median of --repeats.

Writes <out>/bench_assign.json and prints it.

    python tools/bench_assign.py --out <dir> [--iters 50] [--frames 40] [--repeats 3]

``--chain`` measures the chain association (csrc/assign_chain.hip) instead, with the same HIP-event timing per launch:
mmmot_associate_chains for B in {1, 16, 64} x three frames of 12 / 64 / 128 detections for either kernel variant; the
chain kernel at T = 2 against mmmot_associate_pairs on the identical instances (12 x 12, 64 x 64, 128 x 128); and the
host stand-ins for CBC, scipy's linprog and milp on the literal program (tests/association_chain_ref).  Writes
<out>/bench_assign_chain.json.

    python tools/bench_assign.py --chain --out <dir> [--iters 200]

``--sequence`` measures the whole-sequence association (csrc/assign_sequence.hip): HIP-event time per launch (median
of --iters) of mmmot_associate_sequences at B = 1 and B = 21 on two shapes of T = 1000 frames - "planted": n_t uniform in
5 .. 15, hidden tracks that die with probability 1 / 40 per frame, kind eval (det ~ N(1, 1), new / end ~ N(-1, 1) with the
eval zeros, planted links ~ N(2, 1), all others ~ N(-2, 1)); "random": n_t in 0 .. 4, standard normal scores, kind eval,
the long case of tests/test_association_sequence_gpu.py - with the augmentations and passes of sequence 0.  Beside them,
on the same box: the host's linprog on the literal program (tests/association_chain_ref.lp_route) with and without the
construction of the program, and mmmot_associate_pairs over the sequence's T - 1 pairs in one launch (empty frames left
out).  Writes <out>/bench_assign_sequence.json.

    python tools/bench_assign.py --sequence --out <dir> [--iters 50] [--shapes planted,random] [--batches 1,21]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmmot_amd import _lib  # noqa: E402
from mmmot_amd.association import pairs_table  # noqa: E402
from mmmot_amd.ops import HipOps  # noqa: E402
from mmmot_amd.torch_ops import associate_layout  # noqa: E402


def instances(B, N, M, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        L = N + M
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        det, new, end, link = f(L), f(L), f(L), f(N, M)
        new[:N] = 0
        end[N:] = 0
        out.append((N, M, (det, new, end, link)))
    return out


def device_ms(ops, insts, variant, iters):
    splits = [(N, M) for N, M, _ in insts]
    pairs, _ = pairs_table(splits)
    cat = lambda k: torch.from_numpy(np.concatenate([x[2][k].reshape(-1) for x in insts])).cuda()
    det, new, end, link = cat(0), cat(1), cat(2), cat(3)
    total, off, max_nm = associate_layout(pairs, det.numel(), link.numel())
    B = len(insts)
    table = torch.cat([pairs.reshape(-1), off.to(torch.int32)]).cuda()
    out = torch.empty(total, dtype=torch.float32, device='cuda')
    obj = torch.empty(B, dtype=torch.float64, device='cuda')
    assert _lib.load().mmmot_set_assign_variant(variant) == 0
    try:
        run = lambda: ops.associate_pairs(det, new, end, link, table[:4 * B], B, max_nm, out, table[4 * B:], obj)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
    finally:
        _lib.load().mmmot_set_assign_variant(0)
    return statistics.median(ts)


def chain_instances(B, split, seed):
    """B chains of the 'eval' kind (new = 0 in the first frame, end = 0 in the last), standard normal scores"""
    from association_chain_ref import random_chain
    rng = np.random.default_rng(seed)
    return [(list(split), random_chain(rng, split, 1.0, 'eval')) for _ in range(B)]


def chain_device_ms(ops, insts, variant, iters):
    from mmmot_amd.association import chains_table
    from mmmot_amd.torch_ops import chain_layout
    chains, _ = chains_table([s for s, _ in insts])
    cat = lambda k: torch.from_numpy(np.concatenate([sc[k].reshape(-1) for _, sc in insts])).cuda()
    det, new, end = cat(0), cat(1), cat(2)
    link = torch.from_numpy(np.concatenate([l.reshape(-1) for _, sc in insts for l in sc[3]])).cuda()
    total, off, max_n, max_L = chain_layout(chains, det.numel(), link.numel())
    B = len(insts)
    table = torch.cat([chains.reshape(-1), off.to(torch.int32)]).cuda()
    out = torch.empty(total, dtype=torch.float32, device='cuda')
    obj = torch.empty(B, dtype=torch.float64, device='cuda')
    assert _lib.load().mmmot_set_chain_variant(variant) == 0
    try:
        run = lambda: ops.associate_chains(det, new, end, link, table[:11 * B], B, max_n, max_L, out, table[11 * B:], obj)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
    finally:
        _lib.load().mmmot_set_chain_variant(0)
    return statistics.median(ts)


def chain_main(args):
    from association_chain_ref import lp_route, milp_route
    ops = HipOps()
    res = {'instances': "random_chain(.., scale 1, 'eval')", 'iters': args.iters, 'chain_ms_per_launch': [],
           'two_frames_ms_per_launch': [], 'host_ms_per_chain': []}
    for n in (12, 64, 128):
        split = [n, n, n]
        for B in (1, 16, 64):
            insts = chain_instances(B, split, seed=n * 1000 + B)
            row = {'split': split, 'B': B}
            for v in (0, 1, 2):
                row['variant%d' % v] = round(chain_device_ms(ops, insts, v, args.iters), 4)
            row['auto_us_per_chain'] = round(row['variant0'] * 1e3 / B, 2)
            res['chain_ms_per_launch'].append(row)
            print(json.dumps(row), flush=True)
        _, (det, new, end, links) = chain_instances(1, split, seed=n)[0]
        h = {'split': split}
        for name, fn in (('linprog_ms', lp_route), ('milp_ms', milp_route)):
            ts = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                fn(det, new, end, links, split)
                ts.append((time.perf_counter() - t0) * 1e3)
            h[name] = round(statistics.median(ts), 3)
        res['host_ms_per_chain'].append(h)
        print(json.dumps(h), flush=True)
    for n in (12, 64, 128):  # T = 2: the chain kernel and the pair kernel on the identical instances
        for B in (1, 16, 64):
            insts = chain_instances(B, [n, n], seed=n * 77 + B)
            pair_insts = [(n, n, (sc[0], sc[1], sc[2], sc[3][0])) for _, sc in insts]
            row = {'N': n, 'M': n, 'B': B, 'pairs_auto': round(device_ms(ops, pair_insts, 0, args.iters), 4)}
            for v in (0, 1, 2):
                row['chain_variant%d' % v] = round(chain_device_ms(ops, insts, v, args.iters), 4)
            row['chain_over_pairs'] = round(row['chain_variant0'] / row['pairs_auto'], 2)
            res['two_frames_ms_per_launch'].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_assign_chain.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def planted_sequence(rng, T=1000, lo=5, hi=15, mean_len=40):
    """the "planted" shape of --sequence: (split, (det, new, end, links))"""
    live, nxt, frames = [], 0, []
    for t in range(T):
        live = [h for h in live if rng.random() > 1.0 / mean_len]
        target = int(rng.integers(lo, hi + 1))
        live = [live[i] for i in sorted(rng.permutation(len(live))[:target])]
        while len(live) < target:
            live.append(nxt)
            nxt += 1
        frames.append([live[i] for i in rng.permutation(len(live))])
    split = [len(f) for f in frames]
    L = sum(split)
    g = lambda mu, *s: (mu + rng.standard_normal(s)).astype(np.float32)
    det, new, end = g(1, L), g(-1, L), g(-1, L)
    new[:split[0]] = 0
    end[L - split[-1]:] = 0
    links = []
    for t in range(T - 1):
        l = g(-2, split[t], split[t + 1])
        pos = {h: k for k, h in enumerate(frames[t + 1])}
        for j, h in enumerate(frames[t]):
            if h in pos:
                l[j, pos[h]] = g(2)
        links.append(l)
    return split, (det, new, end, links)


def random_sequence(rng, T=1000, hi=5):
    from association_chain_ref import random_chain
    split = [int(n) for n in rng.integers(0, hi, T)]
    return split, random_chain(rng, split, 1.0, 'eval')


def sequence_device_ms(ops, insts, iters):
    """(median ms per launch, info of sequence 0)"""
    from mmmot_amd.association import sequences_table
    from mmmot_amd.torch_ops import SEQ_ROW, sequence_layout
    seqs, nts, _, _ = sequences_table([s for s, _ in insts])
    cat = lambda k: torch.from_numpy(np.concatenate([sc[k].reshape(-1) for _, sc in insts])).cuda()
    det, new, end = cat(0), cat(1), cat(2)
    link = torch.from_numpy(np.concatenate([l.reshape(-1) for _, sc in insts for l in sc[3]])).cuda()
    total, off, woff, units, max_n, max_L, max_T = sequence_layout(seqs, nts, det.numel(), link.numel())
    B = len(insts)
    rows = torch.cat([seqs, off.to(torch.int32)[:, None], woff.to(torch.int32)[:, None]], 1)
    table = torch.cat([rows.reshape(-1), nts]).cuda()
    out = torch.empty(total, dtype=torch.float32, device='cuda')
    ids = torch.empty(det.numel(), dtype=torch.int32, device='cuda')
    obj = torch.empty(B, dtype=torch.float64, device='cuda')
    info = torch.empty((B, 4), dtype=torch.int32, device='cuda')
    ws = torch.empty(units, dtype=torch.float64, device='cuda')
    run = lambda: ops.associate_sequences(det, new, end, link, table[:SEQ_ROW * B], table[SEQ_ROW * B:], B, max_T, max_n,
                                          max_L, out, ids, obj, info, ws)
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), [int(x) for x in info[0].cpu()], float(obj[0].cpu())


def sequence_main(args):
    from association_chain_ref import _program, lp_route
    ops = HipOps()
    res = {'iters': args.iters, 'rows': []}
    makers = {'planted': planted_sequence, 'random': random_sequence}
    for name in args.shapes.split(','):
        first = makers[name](np.random.default_rng(1000))
        split, sc = first
        row = {'shape': name, 'T': len(split), 'L': sum(split)}
        for B in [int(b) for b in args.batches.split(',')]:
            insts = [first] + [makers[name](np.random.default_rng(1000 + b)) for b in range(1, B)]
            ms, info, obj = sequence_device_ms(ops, insts, args.iters)
            row['B%d_ms_per_launch' % B] = round(ms, 3)
            row['status'], row['tracks'], row['augmentations'], row['passes'] = info
            print(json.dumps(row), flush=True)
        t0 = time.perf_counter()
        _program(sc[0], sc[1], sc[2], sc[3], split)
        t1 = time.perf_counter()
        _, wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split)
        t2 = time.perf_counter()
        row['host_program_ms'], row['host_lp_route_ms'] = round((t1 - t0) * 1e3, 1), round((t2 - t1) * 1e3, 1)
        row['host_solve_only_ms'] = round((t2 - t1 - (t1 - t0)) * 1e3, 1)
        row['objective_matches_host'] = bool(abs(obj - wobj) <= 1e-9 * max(1.0, abs(wobj)))
        st = np.concatenate([[0], np.cumsum(split)])
        pair_insts = [(split[t], split[t + 1], (sc[0][st[t]:st[t + 2]], sc[1][st[t]:st[t + 2]], sc[2][st[t]:st[t + 2]],
                                                  sc[3][t])) for t in range(len(split) - 1) if split[t] and split[t + 1]]
        row['pairs'] = len(pair_insts)
        row['pair_solver_ms_per_launch'] = round(device_ms(ops, pair_insts, 0, max(args.iters, 50)), 4)
        res['rows'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_assign_sequence.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def host_ms(fn, inst, reps):
    N, M, (det, new, end, link) = inst
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(det, new, end, link, N, M)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def pipeline_fps(frames, repeats):
    from mmmot_amd import TrackingNet
    from mmmot_amd.pipeline import time_sequence
    from mmmot_amd.weights import init_module
    from seq_workload import KW, sequence_feeds
    model = TrackingNet(**KW)
    init_module(model, seed=0)
    model.eval().cuda()
    feeds = sequence_feeds(frames)
    fps = {False: [], True: []}
    for assoc in (False, True):  # untimed warm run of both
        time_sequence(model, feeds[:6], 224, associate=assoc)
    for _ in range(repeats):
        for assoc in (False, True):
            fps[assoc].append(time_sequence(model, feeds, 224, associate=assoc)[0])
    return {'frames': frames, 'repeats': repeats, 'fps_associate_false': round(statistics.median(fps[False]), 2),
            'fps_associate_true': round(statistics.median(fps[True]), 2),
            'all_false': [round(x, 2) for x in fps[False]], 'all_true': [round(x, 2) for x in fps[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--chain', action='store_true', help='measure the chain association instead')
    ap.add_argument('--sequence', action='store_true', help='measure the whole-sequence association instead')
    ap.add_argument('--shapes', default='planted,random', help='--sequence: which of its shapes')
    ap.add_argument('--batches', default='1,21', help='--sequence: sequences per launch')
    args = ap.parse_args()
    if args.chain:
        return chain_main(args)
    if args.sequence:
        return sequence_main(args)
    from association_ref import lsa_route, milp_route
    ops = HipOps()
    res = {'device_ms_per_launch': [], 'host_ms_per_pair': []}
    shapes = [(12, 12), (64, 64), (128, 128), (12, 100)]
    for N, M in shapes:
        for B in (1, 16, 64):
            insts = instances(B, N, M, seed=N * 1000 + M + B)
            row = {'N': N, 'M': M, 'B': B}
            for v in (0, 1, 2, 3, 4):
                if v >= 3 and max(N, M) > 128:
                    continue
                row['variant%d' % v] = round(device_ms(ops, insts, v, args.iters), 4)
            row['auto_us_per_pair'] = round(row['variant0'] * 1e3 / B, 2)
            res['device_ms_per_launch'].append(row)
            print(json.dumps(row), flush=True)
        inst = instances(1, N, M, seed=N)[0]
        h = {'N': N, 'M': M, 'lsa_ms': round(host_ms(lsa_route, inst, args.host_reps), 3)}
        if N * M <= 64 * 64:  # the literal program at 128 x 128 takes HiGHS too long to be worth the wait
            h['milp_ms'] = round(host_ms(milp_route, inst, args.host_reps), 3)
        res['host_ms_per_pair'].append(h)
        print(json.dumps(h), flush=True)
    if not args.no_pipeline:
        res['pipeline'] = pipeline_fps(args.frames, args.repeats)
        print(json.dumps(res['pipeline']), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_assign.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
