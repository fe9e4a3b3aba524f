"""Appearance rows computed once per frame and reused across the pairs of a sequence, on the device.  Every comparison is
bitwise (torch.equal) against the path that runs the trunk on the crops: TrackingNet.encode_appearance against the
appearance half of `cat` of a plain forward, shape (a) (forward_batch on rows) against forward_batch on crops, shape (b)
(forward_appearance) against model(dets, det_info, dets_split), the online / offline sequence orders against the per-pair
SequencePipeline.run - also across a weight change or a trunk change mid-sequence.  The range-guard case (trained-like
'wild' statistics of tests/test_robust_gpu.py) stays within TOL of the oracle and encodes the rejected rows again.
CPU twin: tests/test_appearance_reuse_cpu.py."""
import warnings

import numpy as np
import pytest
import torch

from common import (TOL, CallLog, assert_same_scores, build_model, case_inputs, check_over_poison, get_case, normalise_u8,
                    scores, u8_crops)
from mmmot_amd import TrackingNet
from mmmot_amd.modules import AppearanceRows
from mmmot_amd.synth import make_pair
from mmmot_amd.weights import generate_state_dict_trained, init_module
from test_appearance_reuse_cpu import _value_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_MODELS = {}


def model(name, trunk='f16x3'):
    c, base = get_case(name)
    m = _MODELS.get(name)
    if m is None:
        m = _MODELS[name] = build_model(c, base, device=DEV)
    m.set_trunk(trunk)
    return m, c


def dev_inputs(c):
    dets, info, ds = case_inputs(c)
    return dets.to(DEV), {k: v.to(DEV) for k, v in info.items()}, ds


def pair_plan(m, c, info, ds, rows=(0, 1, 2)):
    return m.make_plan([([int(d) for d in ds], info['points_split'].reshape(-1).long().cpu().numpy())], c['S'], rows=rows)


def same_tuple(got, want, what):
    assert_same_scores(scores(got), scores(want), what)


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('trunk', ['f16x3', 'f32', 'f16q8'])
def test_encode_appearance_equals_the_forwards_appearance_half(trunk, u8):
    m, c = model('s2_C_multiply_none', trunk)   # 64-pixel crops: f16q8 runs its fp8 arithmetic
    dets, info, ds = dev_inputs(c)
    if u8:
        dets = u8_crops(dets.cpu()).to(DEV)
    N = int(ds[0])
    plan = pair_plan(m, c, info, ds)
    with torch.no_grad():
        want = m.engine().forward(plan, dets, info['points'].reshape(-1, 3))['cat'][:, :512].clone()
        whole, first, second = m.encode_appearance(dets), m.encode_appearance(dets[:N]), m.encode_appearance(dets[N:])
    assert m.engine().trunk == trunk
    assert torch.equal(whole.rows, want) and torch.equal(first.rows, want[:N]) and torch.equal(second.rows, want[N:])
    assert m.appearance_is_current(first)


def _batch(m, specs, S, seed):
    """B samples of ragged counts -> (plan, crops, points, per-frame crops)"""
    ins = [make_pair(N, M, S, 20, seed=seed + i, ragged=True) for i, (N, M) in enumerate(specs)]
    samples = [([N, M], x[1]['points_split'].reshape(-1).long().numpy()) for (N, M), x in zip(specs, ins)]
    plan = m.make_plan(samples, S)
    frames = []
    for (N, M), x in zip(specs, ins):
        frames += [x[0][:N].to(DEV), x[0][N:].to(DEV)]
    return plan, torch.cat([x[0] for x in ins]).to(DEV), torch.cat([x[1]['points'].reshape(-1, 3) for x in ins]).to(DEV), frames


SHAPE_A = ['s2_A_multiply_none', 's2_B_minus_abs_dual_add', 's2_C_minus_single', 's2_C_minus_abs_dual_add',
           's2_A_minus_abs_dual_add', 's2_C_minus_dual_max', 's6_endmax_A']


@pytest.mark.parametrize('name', SHAPE_A)
def test_shape_a_equals_forward_batch_on_crops(name):
    m, c = model(name)
    for specs in ([(c['N'], c['M'])], [(5, 7), (1, 3), (9, 2), (4, 4)]):
        plan, crops, pts, frames = _batch(m, specs, c['S'], 300)
        with torch.no_grad():
            want = m.forward_batch(plan, crops, pts)
            want = [scores(w) for w in want]
            rows = torch.cat([m.encode_appearance(f).rows for f in frames])
            got = m.forward_batch(plan, None, pts, appearance=rows)
        assert len(got) == len(specs)
        for b, (g, w) in enumerate(zip(got, want)):
            assert_same_scores(scores(g), w, '%s B=%d sample %d' % (name, len(specs), b))


def test_shape_a_image_only_rows():
    m, c = model('s2_C_multiply_none')
    dets, info, ds = dev_inputs(c)
    N = int(ds[0])
    plan = pair_plan(m, c, info, ds, rows=(0,))
    with torch.no_grad():
        want = scores(m.forward_batch(plan, dets, None)[0])
        rows = torch.cat([m.encode_appearance(dets[:N]).rows, m.encode_appearance(dets[N:]).rows])
        m.engine().ops = log = CallLog(m.engine().ops)
        got = scores(m.forward_batch(plan, None, None, appearance=rows)[0])
        m.engine().ops = log.ops
    assert_same_scores(got, want, 'rows=(0,)')
    assert not any('conv' in k or 'pointnet' in k or k == 'skippool_head' for k in log.calls), log.calls


@pytest.mark.parametrize('name', ['s2_C_minus_abs_dual_add', 's1_A_multiply_none', 's1_C_minus_abs_dual_add',
                                  's6_endmax_C', 's8_S100_A'])
def test_shape_b_equals_the_pair_forward(name):
    m, c = model(name)
    dets, info, ds = dev_inputs(c)
    N = int(ds[0])
    with torch.no_grad():
        want = m(dets, info, ds)
        prev = m.encode_appearance(dets[:N])
        got, nxt = m.forward_appearance(prev, dets[N:], info, ds, return_rows=True)
        second = m.encode_appearance(dets[N:])
    same_tuple(got, want, name)
    assert isinstance(nxt, AppearanceRows) and torch.equal(nxt.rows, second.rows) and m.appearance_is_current(nxt)


@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('trunk', ['f16x3', 'f32', 'f16q8'])
def test_shape_b_every_trunk_and_crop_type(trunk, u8):
    m, c = model('s2_C_multiply_none', trunk)
    dets, info, ds = dev_inputs(c)
    if u8:
        dets = u8_crops(dets.cpu()).to(DEV)
    N = int(ds[0])
    with torch.no_grad():
        want = m(dets, info, ds)
        got = m.forward_appearance(m.encode_appearance(dets[:N]), dets[N:], info, ds)
    same_tuple(got, want, '%s %s' % (trunk, 'u8' if u8 else 'fp32'))
    assert m.engine().trunk == trunk


def test_shape_b_keeps_pointnet_beside_the_smaller_trunk():
    """the image-first launch of forward(): the LiDAR branch goes to the engine's side stream, for shape (b) too"""
    m, c = model('s2_C_multiply_none')
    dets, info, ds = dev_inputs(c)
    N = int(ds[0])
    eng = m.engine()
    with torch.no_grad():
        prev = m.encode_appearance(dets[:N])
        seen = []
        orig = eng.pointnet

        def pointnet(plan, points, cat):
            seen.append(torch.cuda.current_stream(points.device) != torch.cuda.default_stream(points.device))
            return orig(plan, points, cat)
        eng.pointnet = pointnet
        try:
            got = m.forward_appearance(prev, dets[N:], info, ds)
        finally:
            del eng.pointnet
        want = m(dets, info, ds)
    same_tuple(got, want, 'pointnet beside the trunk')
    assert seen == [True]


@pytest.mark.parametrize('mode', ['a', 'b'])
def test_supplied_rows_over_a_poisoned_workspace(mode):
    m, c = model('s2_C_minus_abs_dual_add')
    dets, info, ds = dev_inputs(c)
    N = int(ds[0])
    plan = pair_plan(m, c, info, ds)
    with torch.no_grad():
        prev = m.encode_appearance(dets[:N])
        rows = torch.cat([prev.rows, m.encode_appearance(dets[N:]).rows])
        want = scores(m(dets, info, ds))
    pts = info['points'].reshape(-1, 3).contiguous()
    call = ((lambda: m.forward_batch(plan, None, pts, appearance=rows)[0]) if mode == 'a' else
            (lambda: m.forward_appearance(prev, dets[N:], info, ds)))
    got = check_over_poison(m, call, 'shape (%s)' % mode)
    assert_same_scores(got, want, 'shape (%s) vs the pair forward' % mode)


def test_every_value_error_comes_before_any_launch():
    m, c = model('s2_C_multiply_none')
    dets, info, ds = dev_inputs(c)
    with torch.no_grad():
        m(dets, info, ds)
    eng = m.engine()
    eng.ops = log = CallLog(eng.ops)
    try:
        for what, call in _value_errors(m, c, dets, info, ds):
            with pytest.raises(ValueError):
                with torch.no_grad():
                    call()
            assert log.calls == [], (what, log.calls)
    finally:
        eng.ops = log.ops


# ---- sequences ---------------------------------------------------------------------------------------------------------
KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True, appear_fpn=False,
          point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg', test_mode=2,
          neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='C', affinity_op='multiply',
          softmax_mode='none')
S = 64
_FEEDS = []


def feeds():
    if not _FEEDS:
        from mmmot_amd.pipeline import FrameFeed
        from mmmot_amd.synth import make_frame
        _FEEDS.extend(FrameFeed(*make_frame(90 + t, 20000, 4 + t % 3)) for t in range(7))
    return _FEEDS


def seq_model(seed=0, **kw):
    m = TrackingNet(**dict(KW, **kw))
    init_module(m, seed=seed)
    return m.eval().to(DEV)


def same_sequences(a, b, what):
    assert len(a) == len(b), what
    for t, (x, y) in enumerate(zip(a, b)):
        assert_same_scores((x[0], x[1], x[2], x[3]), (y[0], y[1], y[2], y[3]), '%s, pair %d' % (what, t + 1))


@pytest.mark.parametrize('overlap', [True, False], ids=['overlap', 'serial'])
def test_online_and_offline_equal_the_per_pair_order(overlap):
    from mmmot_amd.pipeline import SequencePipeline
    fs = feeds()
    m = seq_model()
    per = SequencePipeline(m, S, overlap=overlap)
    want = per.run(fs)
    on = SequencePipeline(m, S, overlap=overlap, reuse_appearance=True)
    got_on = on.run(fs)
    off = SequencePipeline(m, S, overlap=overlap)
    got_off = off.run_offline(fs, frames_per_encode=3, pairs_per_forward=2)   # 3 does not divide 7 frames
    same_sequences(got_on, want, 'online')
    same_sequences(got_off, want, 'offline')
    assert per.stats['encoded_frames'] == 2 * (len(fs) - 1)
    assert on.stats['encoded_frames'] == off.stats['encoded_frames'] == len(fs)
    assert on.stats['pairs'] == off.stats['pairs'] == len(fs) - 1 and on.stats['recomputed_pairs'] == 0


@pytest.mark.parametrize('change', ['load_state_dict', 'set_trunk'])
def test_a_change_mid_sequence_is_followed(change):
    from mmmot_amd.pipeline import SequencePipeline
    fs = feeds()
    other = {k: v.to(DEV) for k, v in seq_model(seed=1).state_dict().items()}

    def at(m):
        def on_scores(t, sc):
            if t == 3:
                m.load_state_dict(other) if change == 'load_state_dict' else m.set_trunk('f32')
        return on_scores
    m = seq_model()
    want = SequencePipeline(m, S).run(fs, on_scores=at(m))
    m = seq_model()
    pipe = SequencePipeline(m, S, reuse_appearance=True)
    got = pipe.run(fs, on_scores=at(m))
    same_sequences(got, want, change)
    assert pipe.stats['encoded_frames'] == len(fs) + 1   # frame 3's rows encoded again under the new weights / trunk
    if change == 'set_trunk':
        assert m.engine().trunk == 'f32'


def wild_f16q8_model():
    """trained-like 'wild' statistics (tests/test_robust_gpu.py) in f16q8: activations leave the e4m3 / fp16 range.  A first
    forward with the guard off, so that the guard's checks that follow are the asynchronous ones of a running sequence."""
    from test_robust_cpu import KW as RKW
    m = TrackingNet(**RKW)
    sd = generate_state_dict_trained(m.state_dict(), 0, 'wild')
    m.load_state_dict(sd)
    m.eval().to(DEV)
    m.set_trunk('f16q8')
    eng = m.engine()
    eng.guard.enabled = False
    dets, info, ds = make_pair(2, 2, S, 5, seed=11)
    with torch.no_grad():
        m(dets.to(DEV), {k: v.to(DEV) for k, v in info.items()}, ds)
    eng.guard.enabled = True
    return m, sd


def assert_pairs_near_oracle(m, sd, fs, got):
    from mmmot_amd.pipeline import SequencePipeline
    from oracle import restatement as R
    from test_robust_cpu import CFG
    prep = SequencePipeline(m, S, overlap=False)
    frames = [prep._prepare(f) for f in fs]
    tm = m.test_mode
    for t in range(1, len(fs)):
        a, b = frames[t - 1], frames[t]
        crops = normalise_u8(torch.cat([a['crops'], b['crops']]))
        split = np.concatenate([a['split'], a['split'][-1] + b['split'][1:]])
        with torch.no_grad():
            o = R.tracking_forward(sd, CFG, crops, torch.cat([a['points'], b['points']]).cpu().unsqueeze(0),
                                   torch.tensor(split, dtype=torch.float32).unsqueeze(0), [a['n'], b['n']])
        det, links, new, end = got[t - 1]
        err = max((det - o[0][tm]).abs().max().item(), (links[0] - o[1][0][tm:tm + 1]).abs().max().item(),
                  (new - o[2][tm]).abs().max().item(), (end - o[3][tm]).abs().max().item())
        assert err < TOL, (t, err, m.engine().range_events)


def test_range_guard_drops_the_rows_it_rejects():
    """the online pipeline: the rows the guard rejects are encoded again, in the lowered arithmetic, with their pair"""
    from mmmot_amd.pipeline import SequencePipeline
    fs = feeds()[:4]
    m, sd = wild_f16q8_model()
    pipe = SequencePipeline(m, S, reuse_appearance=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = pipe.run(fs)
    eng = m.engine()
    assert eng.range_events and eng.trunk != 'f16q8', eng.range_events
    # rejected rows are encoded again: before their pair when the verdict is in by then, else with the pair recomputed
    assert pipe.stats['encoded_frames'] > len(fs), pipe.stats
    assert_pairs_near_oracle(m, sd, fs, got)


def test_direct_cached_pair_loop_never_uses_rejected_rows():
    """the reference-side loop of INTEGRATION.md on forward_appearance itself (no pipeline): rows are checked with
    appearance_is_current, which takes the guard's verdict on the forward that made them; rejected rows are never scored,
    and a pair whose own new rows the guard rejects after its scores were read is computed again"""
    from mmmot_amd.pipeline import SequencePipeline
    from mmmot_amd.tracker_glue import scores_for_solver
    fs = feeds()[:4]
    m, sd = wild_f16q8_model()
    prep = SequencePipeline(m, S, overlap=False)
    frames = [prep._prepare(f) for f in fs]
    got, rows, encodes, repeats = [], None, 0, 0
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter('ignore')
        for t in range(1, len(frames)):
            a, b = frames[t - 1], frames[t]
            ds = [torch.tensor([a['n']]), torch.tensor([b['n']])]
            for attempt in range(3):
                while rows is None or not m.appearance_is_current(rows):
                    rows = m.encode_appearance(a['crops'])
                    encodes += 1
                out, nxt = m.forward_appearance(rows, b['crops'], SequencePipeline._pair_info(a, b), ds,
                                                return_rows=True)
                sc = scores_for_solver(*out[:4], m.test_mode)
                if m.appearance_is_current(nxt) and m.appearance_is_current(rows):
                    break
                repeats += 1
            got.append(sc)
            rows = nxt
    eng = m.engine()
    assert eng.range_events and eng.trunk != 'f16q8', eng.range_events
    assert encodes + repeats > 1, (encodes, repeats)   # some rows were rejected and encoded again
    assert_pairs_near_oracle(m, sd, fs, got)
