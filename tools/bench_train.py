#!/usr/bin/env python
"""Time one training step of the WHOLE network (reference tracking_model.py:50-66: training-mode forward -> TrackingLoss ->
backward -> SGD step) at the shape of BASELINE.json configs[0] (one KITTI-like frame pair: N=10, M=12, 224x224 crops,
ragged ~300 pts/det) and at a cfg2-like sample (N=M=32, 64x64 crops, 512 pts/det).  GPU box only.

    python tools/bench_train.py
    python tools/bench_train.py --labels    # the label step alone on the same samples
    python tools/bench_train.py --optim     # the optimizer step alone at the full model's 216 tensors
    python tools/bench_train.py --dropout   # the step with use_dropout on against off, and the two dropout launches
    python tools/bench_train.py --feed      # the training feed: step alone, TrainingPipeline.run serial / overlapped
    python tools/bench_train.py --end-max   # the two launches of the end_mode='max' backward beside pair_expand_bwd

``--feed`` builds 8 two-frame samples of cfg1's shape from ``synth.make_sequence`` (poses, jittered boxes, 224 x 224
crops, random-resized-crop + flip) and times (a) ``TrainingPipeline.step`` alone on one prepared sample (30 steps behind
5, a device synchronise inside the timed window, three runs), (b) ``run`` over 16 samples with ``overlap=False`` and (c)
with ``overlap=True`` (wall clock per step, the two taking turns, three runs), ``prepare`` alone, and the augment launch
alone (events around 50 back-to-back launches at the sample's L and at 32 copies of it) as GB/s of the 15 bytes a pixel it
must move.  The step is the whole network under the one-launch Adam; the default mode's step (SGD on ``make_pair``
inputs) is the yardstick for (a).

``--labels`` times mmmot_amd.labels.generate_gt alone instead of the step, class / id tensors and targets on the device
as in the reference's ``step``.  The reference's own host loop is not timed here: the repository holds no copy of it.

``--optim`` times one optimizer step under ``true_wd`` at the 216 trainable tensors of the network, every one with a
gradient: (a) the path before optim.Adam - optim.OptimWrapper over torch.optim.Adam, which takes the wrapper's loop of
one ``mul_`` per parameter and then torch's step - and (b) mmmot_amd.build_optim's wrapper over optim.Adam, one launch.  Wall time with a
device synchronise inside the timed window, 200 calls behind 20 warm-up calls, three runs of each.  The kernel alone is
timed with events around 50 back-to-back launches on a prepared table, and launch by launch behind a pass over another
1 GB (the back-to-back launches find part of their data in the last-level cache), against the 28 bytes an element it
must move.

``--dropout`` times the cfg1 training step (image branch frozen and whole network) with ``use_dropout=True`` against
the same step with it off - 30 steps behind 5 warm-up steps each, the two models taking turns, three rounds - and the
two dropout launches (csrc/dropout.hip) beside the launches they extend, on [P][512] rows: at cfg1's P and at 64 times
that (past the last-level cache), events around 50 back-to-back launches, three runs.

``--end-max`` times the backward of the new / end pool in both end modes on the pair rows of one sample (three modality
rows): ``pair_expand_bwd`` (end_mode 'avg') against ``segment_argmax`` + ``pair_expand_max_bwd`` (end_mode 'max'), with
``segment_mean(take_max)`` - the forward's pool, which reads the same rows as the arg-max pass - beside them; at cfg1's
N = 10, M = 12 and at N = M = 32 and 128, events around 50 back-to-back launches, three runs.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from mmmot_amd import TrackingLoss, TrackingNet  # noqa: E402
from mmmot_amd.synth import make_pair  # noqa: E402
from mmmot_amd.weights import init_module  # noqa: E402


SHAPES = {'cfg1 N=10 M=12 224x224': (10, 12, 224, 300, True), 'cfg2-like N=M=32 64x64': (32, 32, 64, 512, False)}


def time_labels(dev):
    """median wall time of the label step alone, a device synchronise inside the timed window"""
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import labels_ref
    from mmmot_amd import labels
    for name, (N, M, _, _, _) in list(SHAPES.items()) + [('N=M=64', (64, 64, 0, 0, False))]:
        rng = np.random.default_rng(N)
        # two thirds of the detections positive, most ids continued in the second frame
        cls = [rng.choice([1, 1, 0], n).astype(np.int64) for n in (N, M)]
        ids = [rng.permutation(N + 4)[:N].astype(np.int64), rng.permutation(N + 4)[:M].astype(np.int64)]
        t = lambda v: torch.from_numpy(v).view(1, -1, 1).to(dev)
        det_cls, det_id = [t(c) for c in cls], [t(i) for i in ids]
        score, ds = torch.zeros(N + M, device=dev), [torch.tensor([N]), torch.tensor([M])]
        times = []
        for it in range(520):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = labels.generate_gt(score, det_cls, det_id, ds)
            torch.cuda.synchronize()
            if it >= 20:  # the first calls warm up
                times.append(time.perf_counter() - t0)
        want = labels_ref.block_of(labels_ref.generate_gt(cls, ids, [N, M]))
        got = torch.cat([out[0], out[2], out[3], out[1][0].reshape(-1)]).cpu().numpy()
        assert (got == want).all(), name
        times.sort()
        print('%-24s labels.generate_gt median %.3f ms, min %.3f ms, 90th percentile %.3f ms over %d calls' % (
            name, times[len(times) // 2] * 1e3, times[0] * 1e3, times[(9 * len(times)) // 10] * 1e3, len(times)))


def time_optim(dev):
    import functools
    from mmmot_amd import optim, torch_ops
    from mmmot_amd.ops import HipOps
    cfg = dict(lr_scheduler=dict(optim='Adam', base_lr=3e-4), weight_decay=0.01, fixed_wd=True)

    def fresh():
        model = TrackingNet(**dict(bench.BASE_KW, score_fusion_arch='C', affinity_op='minus_abs', softmax_mode='dual_add'))
        init_module(model, seed=0)
        model.to(dev)
        g = torch.Generator(device=dev).manual_seed(3)
        for p in model.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-3
        return model

    def timed(step):
        times = []
        for it in range(220):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            if it >= 20:
                times.append(time.perf_counter() - t0)
        times.sort()
        return times[len(times) // 2] * 1e3, times[0] * 1e3, times[(9 * len(times)) // 10] * 1e3

    model = fresh()
    w = optim.build_optim(model, cfg)
    groups = [g['params'] for g in w.opt.param_groups]
    n_t, n_el = sum(len(g) for g in groups), sum(p.numel() for g in groups for p in g)
    print('optimizer step, true_wd: %d tensors in groups of %s, %d elements, %.1f MB to move at 28 B an element' % (
        n_t, [len(g) for g in groups], n_el, n_el * 28 / 1e6))
    res = {'a': [], 'b': []}
    for run in range(3):
        model_a = fresh()
        wa = optim.OptimWrapper.create(functools.partial(torch.optim.Adam, betas=(0.9, 0.99)), 3e-4,
                                       optim.get_layer_groups(model_a), wd=0.01, true_wd=True, bn_wd=True)
        assert [len(g['params']) for g in wa.opt.param_groups] == [len(g) for g in groups]
        res['a'].append(timed(wa.step))
        del model_a, wa
        model_b = fresh()
        wb = optim.build_optim(model_b, cfg)
        res['b'].append(timed(wb.step))
        del model_b, wb
        for k, what in (('a', '(a) mul_ loop + torch.optim.Adam'), ('b', '(b) optim.Adam, one launch      ')):
            print('run %d  %s  median %.3f ms, min %.3f ms, 90th percentile %.3f ms over 200 calls' % ((run + 1, what) + res[k][-1]))
    med = lambda k: sorted(r[0] for r in res[k])[1]
    print('median of the three runs: (a) %.3f ms, (b) %.3f ms, (a) / (b) = %.2f' % (med('a'), med('b'), med('a') / med('b')))

    # the kernel alone: the tables of one step, recorded from the optimizer, launched back to back
    class Recorder:
        name, dtype = 'recorder', torch.float32

        def adam_step(self, *a):
            self.args = a
    rec = Recorder()
    wr = optim.build_optim(model, cfg, ops=rec)
    wr.step()
    chunks, ptrs, scal, b1, b2, eps = rec.args
    table, chunks = torch_ops.adam_pack(ptrs, scal, dev), chunks.to(dev)
    ops = HipOps()
    launch = lambda: ops.adam_step_table(table, int(ptrs.shape[0]), chunks, int(chunks.shape[0]), b1, b2, eps)
    for _ in range(5):
        launch()
    rates = []
    for run in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            launch()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 50
        rates.append(n_el * 28 / (ms * 1e-3) / 1e12)
        print('kernel run %d: %.4f ms a launch over 50 back-to-back launches of %d workgroups, %.2f TB/s, %.0f %% of the 6.29 TB/s '
              'copy rate' % (run + 1, ms, int(chunks.shape[0]), rates[-1], 100 * rates[-1] / 6.29))
    # back-to-back launches find part of their 340 MB in the last-level cache; behind a pass over another 1 GB they do not
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    cold = []
    for _ in range(12):
        flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        cold.append(e0.elapsed_time(e1))
    cold = sorted(cold[2:])
    ms = cold[len(cold) // 2]
    print('kernel behind a 1 GB cache flush, one launch between two events: median %.4f ms (min %.4f, max %.4f) over 10, '
          '%.2f TB/s, %.0f %% of the 6.29 TB/s copy rate' % (ms, cold[0], cold[-1], n_el * 28 / (ms * 1e-3) / 1e12,
                                                           100 * n_el * 28 / (ms * 1e-3) / 1e12 / 6.29))


def time_dropout(dev):
    import numpy as np
    from mmmot_amd.ops import HipOps
    from mmmot_amd.plan import Segments
    N, M, S, pts, ragged = SHAPES['cfg1 N=10 M=12 224x224']
    dets, info, ds = make_pair(N, M, S, pts, seed=4000, ragged=ragged)
    dets, info = dets.to(dev), {k: v.to(dev) for k, v in info.items()}
    g = torch.Generator().manual_seed(1)
    L = N + M
    gt_det = (torch.rand(L, generator=g) > 0.3).float().to(dev)
    gt_new, gt_end = (torch.rand(L, generator=g) > 0.6).float().to(dev), (torch.rand(L, generator=g) > 0.6).float().to(dev)
    gt_link = [(torch.rand(1, N, M, generator=g) > 0.9).float().to(dev)]
    crit = TrackingLoss(detloss_type='bce', linkloss_type='l2', det_ratio=1.5, trans_ratio=0.001)
    models = {}
    for flag in (False, True):
        m = TrackingNet(**dict(bench.BASE_KW, score_fusion_arch='C', affinity_op='multiply', softmax_mode='none',
                               use_dropout=flag))
        init_module(m, seed=0)
        models[flag] = (m.to(dev).train(), torch.optim.SGD(m.parameters(), lr=1e-4))

    def steps(flag, n):
        model, opt = models[flag]
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det, links, new, end, trans = model(dets, info, ds)
            loss = crit(ds, gt_det, gt_link, gt_new, gt_end, det, links, new, end, trans)
            opt.zero_grad()
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)
    for frozen in (True, False):
        for flag in (False, True):
            models[flag][0].freeze_appearance = frozen
            steps(flag, 5)
        for rnd in range(3):
            for flag in (False, True):
                ts = steps(flag, 30)
                print('cfg1 %-19s round %d  use_dropout=%-5s step median %.2f ms, min %.2f ms, 90th percentile %.2f ms over 30' % (
                    'image branch frozen' if frozen else 'whole network', rnd + 1, flag, ts[15] * 1e3, ts[0] * 1e3, ts[27] * 1e3))
    # ---- the launches: [P][512] rows, cfg1's detections (and 64 copies of them: 440 MB, past the last-level cache) ----
    ops = HipOps()
    cnt1 = np.diff(info['points_split'].reshape(-1).cpu().numpy().astype(np.int64))
    for copies in (1, 64):
        cnt = np.tile(cnt1, copies)
        P, Lt, C = int(cnt.sum()), len(cnt), 512
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        segs = Segments(start, cnt, np.ones(Lt), np.zeros(Lt), dev)
        X = torch.randn(P, C, device=dev)
        sc, sh = torch.rand(1, C, device=dev) + 0.5, torch.randn(1, C, device=dev) * 0.1
        out, dS, dX = torch.empty(Lt, C, device=dev), torch.randn(Lt, C, device=dev), torch.empty(P, C, device=dev)
        row_det = torch.from_numpy(np.repeat(np.arange(Lt), cnt).astype(np.int32)).to(dev)
        inv = torch.from_numpy((1.0 / cnt).astype(np.float32)).to(dev)
        launches = [
            ('segment_mean(relu)', lambda: ops.segment_mean(X, C, segs, out, sc=sc, sh=sh, relu=True)),
            ('segment_mean_dropout', lambda: ops.segment_mean_dropout(X, C, segs, out, sc, sh, 12345, 0x80000000, 2.0)),
            ('rows_gather_scale', lambda: ops.rows_gather_scale(dS, row_det, inv, dX, C)),
            ('rows_gather_scale_dropout', lambda: ops.rows_gather_scale_dropout(dS, row_det, inv, dX, C, 12345, 0x80000000, 2.0)),
        ]
        print('[P][512] rows: P = %d in %d segments, %.1f MB' % (P, Lt, P * C * 4 / 1e6))
        for name, fn in launches:
            for _ in range(5):
                fn()
            ms = []
            for run in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(50):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / 50)
            med = sorted(ms)[1]
            print('  %-26s %.4f / %.4f / %.4f ms a launch (three runs of 50), median %.2f TB/s of the tensor' % (
                name, ms[0], ms[1], ms[2], P * C * 4 / (med * 1e-3) / 1e12))


def time_end_max(dev):
    from mmmot_amd.backward import _aux
    from mmmot_amd.ops import HipOps
    from mmmot_amd.plan import BatchPlan
    ops, C = HipOps(), 512
    for N, M in ((10, 12), (32, 32), (128, 128)):
        plan = BatchPlan([([N, M], None)], 32, dev, use_points=False)
        PT, VT, aux = plan.pair_tiles, plan.v_tiles, _aux(plan)
        ya = torch.randn(PT.R, 1024, device=dev)           # the stacked layer's output: the pool reads its first half
        sc, sh = torch.rand(PT.G, C, device=dev) + 0.5, torch.randn(PT.G, C, device=dev) * 0.1
        V, dV = torch.empty(VT.R, C, device=dev), torch.randn(VT.R, C, device=dev)
        idx, dA = torch.empty(VT.R, C, dtype=torch.int32, device=dev), torch.empty(PT.R, C, device=dev)
        common = (PT, PT.g_row0, plan.pg_N, plan.pg_M, aux.vrow0)
        launches = [
            ('segment_mean(take_max)', lambda: ops.segment_mean(ya[:, :C], C, plan.v_segs, V, sc=sc, sh=sh, relu=True, take_max=True)),
            ('pair_expand_bwd', lambda: ops.pair_expand_bwd(dV, dA, C, *common)),
            ('segment_argmax', lambda: ops.segment_argmax(ya[:, :C], C, plan.v_segs, idx, sc=sc, sh=sh, relu=True)),
            ('pair_expand_max_bwd', lambda: ops.pair_expand_max_bwd(dV, idx, dA, C, *common)),
        ]
        print('N = %d, M = %d: %d pair rows x 512 (%.2f MB), %d new / end vectors' % (N, M, PT.R, PT.R * C * 4 / 1e6, VT.R))
        for name, fn in launches:
            for _ in range(5):
                fn()
            ms = []
            for run in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(50):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / 50)
            print('  %-24s %.4f / %.4f / %.4f ms a launch (three runs of 50)' % (name, ms[0], ms[1], ms[2]))


def time_feed(dev):
    import numpy as np
    from mmmot_amd import augment, build_optim
    from mmmot_amd.crops import crop_resize_u8
    from mmmot_amd.ops import HipOps
    from mmmot_amd.pipeline import FrameFeed
    from mmmot_amd.synth import make_sequence
    from mmmot_amd.train_pipeline import TrainingPipeline, TrainSample
    S, NS = 224, 8
    frames = make_sequence(NS + 1, 4000, ego=1)  # cfg1's shape: 10-12 detections, 120k-point sweeps, 375 x 1242 frames
    rng = np.random.default_rng(1)

    def sample(fr):
        feeds = [FrameFeed(img, sweep, info, dets, pose=(info['pos'], info['rad'])) for img, sweep, info, dets in fr]
        gts = [{'bbox': f[3]['bbox'], 'id': np.arange(len(f[3]['bbox'])), 'name': np.zeros(len(f[3]['bbox']), np.int64)}
               for f in fr]
        return TrainSample(feeds, gts, [f[3]['bbox'] + rng.uniform(-3, 3, f[3]['bbox'].shape) for f in fr])
    samples = [sample(frames[k:k + 2]) for k in range(NS)]
    cfg = dict(lr_scheduler=dict(optim='Adam', base_lr=3e-4), weight_decay=0.01, fixed_wd=True)
    crit = TrackingLoss(detloss_type='bce', linkloss_type='l2', det_ratio=1.5, trans_ratio=0.001)

    def pipe(overlap):
        model = TrackingNet(**dict(bench.BASE_KW, score_fusion_arch='C', affinity_op='multiply', softmax_mode='none'))
        init_module(model, seed=0)
        model.to(dev).train()
        return TrainingPipeline(model, crit, build_optim(model, cfg), size=S, augment=augment.RandomResizedCropFlip(S),
                                seed=0, overlap=overlap)
    pipes = {False: pipe(False), True: pipe(True)}
    L = sum(len(f.dets['bbox']) for f in samples[0].feeds)
    print('training feed, cfg1 shape: %d samples of 2 frames, %d crops of %d x %d in the first' % (NS, L, S, S))
    # (a) the step alone on one prepared sample
    for run in range(3):
        p = pipes[False]
        prepared = p.prepare(samples[0])
        ts = []
        for it in range(35):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = p.step(prepared)
            torch.cuda.synchronize()
            if it >= 5:
                ts.append(time.perf_counter() - t0)
        ts.sort()
        print('(a) run %d  step alone on a prepared sample: median %.2f ms, min %.2f ms, 90th percentile %.2f ms over 30; '
              'loss %.4f' % (run + 1, ts[15] * 1e3, ts[0] * 1e3, ts[27] * 1e3, loss.item()))
    # (b) / (c): run() over the samples, serial and overlapped, taking turns
    for p in pipes.values():
        p.run(samples)
    for run in range(3):
        for overlap in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = pipes[overlap].run(samples + samples)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert bool(torch.isfinite(losses).all())
            print('(%s) run %d  run(overlap=%-5s): %.2f ms a step over %d steps (prepare + step, wall clock)' % (
                'c' if overlap else 'b', run + 1, overlap, dt / (2 * NS) * 1e3, 2 * NS))
    # prepare alone, serial: what (b) adds to (a)
    ts = []
    for it in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipes[False].prepare(samples[it % NS])
        torch.cuda.synchronize()
        if it >= 2:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    print('prepare alone (serial, synchronised): median %.2f ms, min %.2f ms over 10' % (ts[5] * 1e3, ts[0] * 1e3))
    # the augment launch alone: at the sample's L and at 32 copies of it (past the last-level cache)
    ops = HipOps()
    ms_ = torch.tensor([0.485, 0.456, 0.406, 0.229, 0.224, 0.225], device=dev)
    u8 = torch.cat([crop_resize_u8(f.img.to(dev), b, S) for f, b in zip(samples[0].feeds, samples[0].boxes)])
    for copies in (1, 32):
        x = u8.repeat(copies, 1, 1, 1)
        Lc = int(x.shape[0])
        table = torch.from_numpy(augment.RandomResizedCropFlip(S).draw(Lc, torch.Generator().manual_seed(2))).to(dev)
        out = torch.empty(Lc, 3, S, S, device=dev)
        nbytes = Lc * S * S * (3 + 12)
        for _ in range(5):
            ops.crop_augment(x, table, ms_, out, None, Lc, S)
        rates = []
        for run in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(50):
                ops.crop_augment(x, table, ms_, out, None, Lc, S)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 50
            rates.append(nbytes / (ms * 1e-3) / 1e9)
            print('augment launch, L = %d: run %d  %.4f ms a launch over 50 back-to-back launches, %.0f GB/s of the %.1f MB it '
                  'must move, %.1f %% of the 6.29 TB/s copy rate' % (Lc, run + 1, ms, rates[-1], nbytes / 1e6,
                                                                    100 * rates[-1] / 6290))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--feed', action='store_true', help='time the training feed: the step alone, TrainingPipeline.run '
                    'serial and overlapped, and the augment launch alone')
    ap.add_argument('--dropout', action='store_true', help='time the training step with use_dropout on against off, and '
                    'the two dropout launches beside the launches they extend')
    ap.add_argument('--optim', action='store_true', help='time the optimizer step alone: torch.optim.Adam under the '
                    'wrapper against optim.Adam')
    ap.add_argument('--labels', action='store_true', help='time the label step (labels.generate_gt) alone')
    ap.add_argument('--end-max', action='store_true', help="time the two launches of the end_mode='max' backward beside "
                    'pair_expand_bwd')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    if args.feed:
        return time_feed(dev)
    if args.end_max:
        return time_end_max(dev)
    if args.labels:
        return time_labels(dev)
    if args.dropout:
        return time_dropout(dev)
    if args.optim:
        return time_optim(dev)
    for name, (N, M, S, pts, ragged) in SHAPES.items():
        model = TrackingNet(**dict(bench.BASE_KW, score_fusion_arch='C', affinity_op='multiply', softmax_mode='none'))
        init_module(model, seed=0)
        model.to(dev).train()
        crit = TrackingLoss(detloss_type='bce', linkloss_type='l2', det_ratio=1.5, trans_ratio=0.001)
        opt = torch.optim.SGD(model.parameters(), lr=1e-4)
        dets, info, ds = make_pair(N, M, S, pts, seed=4000, ragged=ragged)
        dets, info = dets.to(dev), {k: v.to(dev) for k, v in info.items()}
        g = torch.Generator().manual_seed(1)
        L = N + M
        gt_det = (torch.rand(L, generator=g) > 0.3).float().to(dev)
        gt_new, gt_end = (torch.rand(L, generator=g) > 0.6).float().to(dev), (torch.rand(L, generator=g) > 0.6).float().to(dev)
        gt_link = [(torch.rand(1, N, M, generator=g) > 0.9).float().to(dev)]
        for frozen in (False, True):
            model.freeze_appearance = frozen
            ts, tf, losses = [], [], []
            for it in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                det, links, new, end, trans = model(dets, info, ds)
                loss = crit(ds, gt_det, gt_link, gt_new, gt_end, det, links, new, end, trans)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                opt.zero_grad()
                loss.backward()
                opt.step()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                losses.append(loss.item())
                if it:
                    ts.append(t2 - t0)
                    tf.append(t1 - t0)
            ts.sort(); tf.sort()
            print('%-24s %-22s step %.1f ms (forward + loss %.1f ms), loss %.4f -> %.4f, peak memory %.2f GB' % (
                name, 'image branch frozen' if frozen else 'whole network', ts[len(ts) // 2] * 1e3, tf[len(tf) // 2] * 1e3,
                losses[0], losses[-1], torch.cuda.max_memory_allocated() / 2 ** 30))


if __name__ == '__main__':
    main()
