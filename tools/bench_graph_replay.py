"""Latency of one hipGraph replay (``TrackingNet.capture`` -> ``GraphedForward.__call__``) at the shape of bench.py's
latency leg - cfg1: fusion A, N = 10, M = 12, 224-pixel crops, ragged ~300 points a detection, B = 1, f16x3 - and the
host cost of the staleness check every replay makes.  50 untimed replays first; then blocks of 200 replays, each replay
followed by a synchronise, wall time per replay, the median of each block.

    python tools/bench_graph_replay.py [--blocks 5] [--package <dir that holds another mmmot_amd>]

--package times another copy of the package (the parent commit's, for a before / after in one call: run the two in turn).
"""
import argparse
import json
import os
import statistics
import sys
import time
import timeit

ap = argparse.ArgumentParser()
ap.add_argument('--blocks', type=int, default=5)
ap.add_argument('--package', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package))

import torch  # noqa: E402
import mmmot_amd  # noqa: E402
from mmmot_amd import TrackingNet  # noqa: E402
from mmmot_amd.synth import CONFIGS, make_pair  # noqa: E402
from mmmot_amd.weights import init_module  # noqa: E402

assert os.path.abspath(mmmot_amd.__file__).startswith(os.path.abspath(args.package)), mmmot_amd.__file__
cfg = CONFIGS['cfg1']
model = TrackingNet(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True,
                    appear_fpn=False, point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2',
                    end_mode='avg', test_mode=2, neg_threshold=0.2, dropblock=0, use_dropout=False,
                    score_fusion_arch=cfg['fusion'], affinity_op=cfg['affinity_op'], softmax_mode=cfg['softmax_mode'])
init_module(model, 0)
model.eval().cuda()
dets, info, ds = make_pair(cfg['N'], cfg['M'], cfg['S'], cfg['pts'], seed=1, ragged=cfg['ragged'])
plan = model.make_plan([([cfg['N'], cfg['M']], info['points_split'].reshape(-1).long().numpy())], cfg['S'])
crops, points = dets.cuda(), info['points'].reshape(-1, 3).contiguous().cuda()
g = model.capture(plan, crops, points)
for _ in range(50):
    g(crops, points)
torch.cuda.synchronize()
medians = []
for _ in range(args.blocks):
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        g(crops, points)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    medians.append(round(statistics.median(ts) * 1e3, 4))
stale_us = min(timeit.repeat(g.stale, number=2000, repeat=5)) / 2000 * 1e6
print(json.dumps(dict(package=os.path.abspath(args.package), trunk=model.engine().trunk, replay_ms_median_of_200=medians,
                      stale_check_us=round(stale_us, 2))), flush=True)
