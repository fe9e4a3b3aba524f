"""The hipGraph replay of a forward (TrackingNet.capture -> GraphedForward): the path bench.py times and the README
recommends for fixed-shape serving.  It runs code no eager forward runs - launches recorded once with the host values of
capture time, input clones, result views into the workspace arena, a range guard that only counts - so it is compared
here with the eager forward of the SAME plan on inputs the graph was NOT captured with:

  A  replay == forward_batch bit for bit on fresh inputs, per fusion / affinity / softmax / end mode / point layout /
     frame count / trunk arithmetic, and the captured set against the imported reference's golden;
  B  other call shapes: B = 3, uint8 crops, single-modality plans, the two-stream fork, in-place inputs;
  C  the arena: poisoned, re-allocated by a larger eager forward, shared with a second graph;
  D  the range guard: check_range() raises once a replay leaves the fp16 range, and only then;
  E  staleness: every way the packed weights fall behind the parameters makes __call__ raise;
  F  inputs of another shape or type are refused before anything is copied.

An input set of a plan keeps the plan's point split and draws new crop pixels and new point coordinates from another
seed; set 0 is the golden fixture's.  CPU twin of the host rules: tests/test_graph_cpu.py."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import (POISON, TOL, assert_same_scores, build_model, case_inputs, compare_outputs, edit_below_half_max,
                    get_case, golden, normalise_u8, packed_scalars, poison_workspace, scores, u8_crops)
from mmmot_amd import TrackingNet
from mmmot_amd.pack import VGG_STAGES
from mmmot_amd.synth import make_pair
from mmmot_amd.weights import calibrate_bn, generate_state_dict_trained
from oracle import restatement as R
from test_robust_cpu import CFG, KW, linf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

_MODELS = {}


def model(name, trunk='f16x3', private=False):
    """the case's model on the device (built once per case; private=True: a copy of its own, for tests that edit
    parameters), on a FRESH engine with the given trunk"""
    c, base = get_case(name)
    m = None if private else _MODELS.get(name)
    if m is None:
        m = build_model(c, base, device=DEV)
        if not private:
            _MODELS[name] = m
    m.set_trunk(trunk)
    m.engine()
    return m, c


def fresh_inputs(split, kin, L, S, seed):
    """new crops [L,3,S,S] and new point coordinates [P,kin] for the point split `split` (int64 [L+1])"""
    crops = make_pair(L, 0, S, 1, seed)[0]
    g = np.random.Generator(np.random.Philox(key=[0x6e3a, int(seed)]))
    cnt = np.diff(split)
    centres = g.uniform([5.0, -20.0, -2.0], [60.0, 20.0, 0.5], (L, 3))
    pts = g.standard_normal((int(split[-1]), 3)) * [1.6, 0.7, 0.6] + np.repeat(centres, cnt, axis=0)
    if kin == 4:
        pts = np.concatenate([pts, g.uniform(0.0, 1.0, (pts.shape[0], 1))], axis=1)
    return crops, torch.from_numpy(pts.astype(np.float32))


def case_sets(m, c, n=3, rows=(0, 1, 2)):
    """-> (plan of the golden case, n input sets [(crops, points)] on the device; set 0 = the golden's inputs)"""
    dets, info, ds = case_inputs(c)
    fc = [int(d) for d in ds]
    kin = int(info['points'].shape[-1])
    split = info['points_split'].reshape(-1).long().numpy()
    plan = m.make_plan([(fc, split)], c['S'], rows=rows)
    sets = [(dets, info['points'].reshape(-1, kin))]
    sets += [fresh_inputs(split, kin, sum(fc), c['S'], 100 * c['seed'] + k) for k in range(1, n)]
    return plan, [(a.contiguous().to(DEV), b.contiguous().to(DEV)) for a, b in sets]


def eager(m, plan, crops, points):
    with torch.no_grad():
        return [scores(r) for r in m.forward_batch(plan, crops, points)]


def differ(a, b):
    return any(not torch.equal(x, y) for x, y in zip([a[0], a[2], a[3]] + a[1], [b[0], b[2], b[3]] + b[1]))


def eager_all(m, plan, sets):
    """the eager scores of every set (computed once, before anything is captured); the sets must not give the same
    scores, or a replay that ignores its inputs would pass"""
    want = [eager(m, plan, c, p) for c, p in sets]
    for k in range(1, len(sets)):
        assert all(differ(a, b) for a, b in zip(want[k], want[0])), 'input set %d gives the scores of set 0' % k
    return want


def replay(g, crops, points):
    """one replay -> host copies of the result views (taken before anything else runs on the engine)"""
    return [scores(r) for r in g(crops, points)]


def check_replays(g, sets, want, what, order=(1, 2, 0, 1)):
    got = {}
    for k in order:
        r = replay(g, *sets[k])
        assert len(r) == len(want[k])
        for b, (x, y) in enumerate(zip(r, want[k])):
            assert_same_scores(x, y, '%s: replay of input set %d, sample %d, vs the eager forward' % (what, k, b))
        if k in got:
            for b, (x, y) in enumerate(zip(r, got[k])):
                assert_same_scores(x, y, '%s: second replay of input set %d, sample %d' % (what, k, b))
        got[k] = r
    return got


# ---- A. replay equals eager on inputs the graph was not captured with -------------------------------------------------
A_CASES = [(n, 'f16x3') for n in ('s2_A_multiply_none', 's2_B_minus_abs_dual_add', 's2_C_minus_single', 's2_C_minus_dual',
                                  's2_C_minus_dual_max', 's6_endmax_C', 's7_refl_B', 's5_3frames_B', 's1_C_multiply_none')]
A_CASES += [('s2_B_minus_abs_dual_add', 'f32'), ('s5_3frames_B', 'f32'), ('s2_C_multiply_none', 'f16q8')]


@pytest.mark.parametrize('name,trunk', A_CASES, ids=['%s-%s' % nt for nt in A_CASES])
def test_replay_equals_eager_on_fresh_inputs(name, trunk):
    m, c = model(name, trunk)
    eng = m.engine()
    if trunk == 'f16q8':
        assert c['S'] == 64 and eng.q8_in_force(64)
    plan, sets = case_sets(m, c)
    want = eager_all(m, plan, sets)
    g = m.capture(plan, *sets[0])
    got = check_replays(g, sets, want, '%s %s' % (name, trunk))
    # the golden's own inputs through the graph, against the imported reference
    det, links, new, end = got[0][0]
    compare_outputs((det, links, new, end, None), golden(name), TOL)
    assert g.check_range() == (0, 0, 0) or trunk == 'f16q8'  # (e4m3 saturation below the guard's limit is not an event)
    assert eng.trunk == trunk and not eng.range_events and not g.stale()


# ---- B. other call shapes --------------------------------------------------------------------------------------------
def test_replay_of_a_batch_of_three_samples():
    m, c = model('s2_C_multiply_none')
    S, counts = 32, [(5, 7), (1, 1), (9, 2)]
    ins = [make_pair(n, k, S, 20, seed=5100 + i, ragged=True) for i, (n, k) in enumerate(counts)]
    splits = [x[1]['points_split'].reshape(-1).long().numpy() for x in ins]
    plan = m.make_plan([(list(fc), sp) for fc, sp in zip(counts, splits)], S)
    sets = [(torch.cat([x[0] for x in ins]), torch.cat([x[1]['points'].reshape(-1, 3) for x in ins]))]
    for k in (1, 2):
        fr = [fresh_inputs(sp, 3, sum(fc), S, 5200 + 10 * k + i) for i, (fc, sp) in enumerate(zip(counts, splits))]
        sets.append((torch.cat([x[0] for x in fr]), torch.cat([x[1] for x in fr])))
    sets = [(a.to(DEV), b.to(DEV)) for a, b in sets]
    want = eager_all(m, plan, sets)
    assert len(want[0]) == 3 and [tuple(w[1][0].shape[1:]) for w in want[0]] == counts
    check_replays(m.capture(plan, *sets[0]), sets, want, 'B = 3')


@pytest.mark.parametrize('trunk', ['f16x3', 'f16q8'])
def test_replay_of_uint8_crops(trunk):
    """the bytes go through the graph's own uint8 buffer into the fused first launch: equal to the eager uint8 forward,
    and to the replay of a graph captured on the host-normalised fp32 crops (the project's uint8 property)"""
    m, c = model('s2_C_multiply_none', trunk)
    plan, sets = case_sets(m, c)
    u8 = [(u8_crops(a.cpu()).to(DEV), p) for a, p in sets]
    f32 = [(normalise_u8(a).to(DEV), p) for a, p in u8]
    want = eager_all(m, plan, u8)
    g8 = m.capture(plan, *u8[0])
    assert g8.crops.dtype == torch.uint8 and tuple(g8.crops.shape) == (12, 64, 64, 3)
    got8 = check_replays(g8, u8, want, 'uint8 crops, %s' % trunk)
    g32 = m.capture(plan, *f32[0])
    got32 = check_replays(g32, f32, want, 'normalised crops of the same bytes, %s' % trunk)
    for k in got8:
        assert_same_scores(got8[k][0], got32[k][0], 'uint8 graph vs fp32 graph, set %d, %s' % (k, trunk))
    assert m.engine().trunk == trunk and m.engine().q8_in_force(64) == (trunk == 'f16q8')


@pytest.mark.parametrize('rows', [(0,), (1,)])
def test_replay_of_a_single_modality_plan(rows):
    m, c = model('s2_C_multiply_none')
    plan, sets = case_sets(m, c, rows=rows)
    sets = [(a, None) if rows == (0,) else (None, p) for a, p in sets]
    want = eager_all(m, plan, sets)
    assert tuple(want[0][0][0].shape) == (1, 12)
    g = m.capture(plan, *sets[0])
    assert (g.crops is None) == (rows == (1,)) and (g.points is None) == (rows == (0,))
    check_replays(g, sets, want, 'rows %r' % (rows,))


def test_replay_of_the_two_stream_fork():
    m, c = model('s2_C_multiply_none')
    plan, sets = case_sets(m, c)
    want = eager_all(m, plan, sets)     # one stream
    m.engine().two_streams = True
    check_replays(m.capture(plan, *sets[0]), sets, want, 'two_streams')


def test_replay_of_inputs_written_in_place():
    m, c = model('s2_C_multiply_none')
    plan, sets = case_sets(m, c)
    want = eager_all(m, plan, sets)
    g = m.capture(plan, *sets[0])
    g.crops.copy_(sets[1][0])
    g.points.copy_(sets[1][1])
    assert_same_scores([scores(r) for r in g()][0], want[1][0], 'g() after writing set 1 into its buffers')
    g.crops.copy_(sets[2][0])
    g.points.copy_(sets[2][1])
    assert_same_scores(replay(g, g.crops, g.points)[0], want[2][0], 'g(g.crops, g.points): no copy')
    assert_same_scores(replay(g, None, sets[1][1])[0], eager(m, plan, sets[2][0], sets[1][1])[0],
                       'crops=None keeps the crop buffer')


# ---- C. the arena ----------------------------------------------------------------------------------------------------
def test_replay_over_a_poisoned_and_a_reallocated_arena():
    m, c = model('s2_C_multiply_none')
    eng = m.engine()
    plan, sets = case_sets(m, c, n=2)
    want = eager_all(m, plan, sets)
    g = m.capture(plan, *sets[0])
    kept = replay(g, *sets[1])
    assert_same_scores(kept[0], want[1][0], 'replay of set 1')
    for byte in POISON:
        poison_workspace(eng, byte)
        assert_same_scores(replay(g, *sets[1])[0], kept[0], 'replay over a workspace filled with 0x%02X' % byte)
    sizes = {k: t.numel() for k, t in eng.ws.items()}
    big = make_pair(20, 20, 64, 40, seed=5300, ragged=True)
    with torch.no_grad():
        m(big[0].to(DEV), {k: v.to(DEV) for k, v in big[1].items()}, big[2])
    assert any(eng.ws[k].numel() > n for k, n in sizes.items()), 'the larger forward re-allocated nothing'
    assert_same_scores(replay(g, *sets[1])[0], kept[0], 'replay after a larger eager forward re-allocated the arena')
    small = make_pair(2, 3, 32, 10, seed=5301, ragged=True)
    with torch.no_grad():
        m(small[0].to(DEV), {k: v.to(DEV) for k, v in small[1].items()}, small[2])
    assert_same_scores(replay(g, *sets[1])[0], kept[0], 'replay after a smaller eager forward')
    assert m.engine() is eng and not g.stale()


def test_two_graphs_of_one_model_do_not_disturb_each_other():
    m, c = model('s2_C_multiply_none')
    plan1, sets1 = case_sets(m, c, n=2)
    c2, _ = get_case('s6_endmax_C')     # another plan (9 x 6 detections of 32 pixels) on the same model
    plan2, sets2 = case_sets(m, c2, n=2)
    want1, want2 = eager_all(m, plan1, sets1), eager_all(m, plan2, sets2)
    g1 = m.capture(plan1, *sets1[0])
    g2 = m.capture(plan2, *sets2[0])
    for k in (1, 0, 1):
        assert_same_scores(replay(g1, *sets1[k])[0], want1[k][0], 'first graph, set %d' % k)
        assert_same_scores(replay(g2, *sets2[k])[0], want2[k][0], 'second graph, set %d' % k)
    assert_same_scores(replay(g1, None, None)[0], want1[1][0], 'first graph again, inputs kept')


# ---- D. the range guard of a captured forward ------------------------------------------------------------------------
RANGE_FACTOR = 4096.0


def trunk_activation_max(sd, crops):
    """largest activation any trunk layer stores (fp32 on the host, the layers of oracle.restatement.vgg_stage)"""
    x, worst, ends = crops, 0.0, []
    for s, stage in enumerate(VGG_STAGES):
        p = 'appearance.layers.%d.' % s
        for idx, cin, cout, pool in stage:
            b = p + '%d.' % (idx + 1)
            x = F.conv2d(x, sd[p + '%d.weight' % idx], sd[p + '%d.bias' % idx], padding=1)
            x = F.relu(F.batch_norm(x, sd[b + 'running_mean'], sd[b + 'running_var'], sd[b + 'weight'], sd[b + 'bias'],
                                    False, 0.0, R.EPS))
            worst = max(worst, float(x.max()))
            if pool:
                x = F.max_pool2d(x, 2, 2)
        ends.append(x)
    return worst, ends


def calibrated_model(sd):
    m = TrackingNet(**KW)
    m.load_state_dict(sd)
    m.eval().to(DEV)
    m.set_trunk('f16x3')
    return m


def test_check_range_raises_once_a_replay_leaves_the_fp16_range():
    """Weights: the 'calibrated' profile of tests/test_robust_gpu.py (seed 0), BatchNorm statistics calibrated at input
    scale 1; 6 x 5 detections of 64 pixels.  The fp32 restatement of the trunk stores at most 20.6 on these crops and
    2.147e5 on the crops times RANGE_FACTOR = 4096 (the largest activation is linear in the factor to three digits:
    52.4 per unit, so 2 x 65000 needs a factor of 2481; 4096 is the next power of two, an exact scaling): 3.3 times the
    65000 the fp16 `hi` half clamps at.  A replay cannot lower the arithmetic by itself - check_range() is all there is."""
    m0 = TrackingNet(**KW)
    sd = generate_state_dict_trained(m0.state_dict(), 0, 'calibrated')
    calibrate_bn(sd, make_pair(8, 8, 64, 4, seed=4100)[0])
    dets, info, ds = make_pair(6, 5, 64, 40, seed=4000, ragged=True)
    hot = dets * RANGE_FACTOR
    with torch.no_grad():
        keep = {}
        R.appearance(dets, sd, keep)
        amax, ends = trunk_activation_max(sd, dets)
        assert all(torch.equal(e, keep['vgg_stage%d' % s]) for s, e in enumerate(ends)), 'not the oracle\'s trunk'
        hot_max = trunk_activation_max(sd, hot)[0]
    print('largest trunk activation: %.4g in range, %.4g at factor %g' % (amax, hot_max, RANGE_FACTOR))
    assert amax < 65000 / 100 and hot_max > 2 * 65000
    dinfo = {k: v.to(DEV) for k, v in info.items()}
    points = dinfo['points'].reshape(-1, 3).contiguous()
    crops, hot_d = dets.to(DEV), hot.to(DEV)
    # the precondition on code that is tested elsewhere: the eager guard of a fresh model sees these inputs clamp
    fresh = calibrated_model(sd)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref_hot = R.tracking_forward(sd, CFG, hot, info['points'], info['points_split'], [6, 5])
        out = fresh(hot_d, dinfo, ds)
    ev = fresh.engine().range_events
    assert ev and any(e['fp16_clamped'] > 0 for e in ev) and fresh.engine().trunk == 'f32', ev
    assert linf((out[0].cpu(), [l.cpu() for l in out[1]], out[2].cpu(), out[3].cpu()), ref_hot) < TOL

    m = calibrated_model(sd)
    eng = m.engine()
    plan = m.make_plan([([6, 5], info['points_split'].reshape(-1).long().numpy())], 64)
    want = eager(m, plan, crops, points)
    g = m.capture(plan, crops, points)
    for _ in range(2):
        assert_same_scores(replay(g, crops, points)[0], want[0], 'in-range replay')
    assert g.check_range() == (0, 0, 0)
    assert eng.trunk == 'f16x3' and not eng.range_events
    g(hot_d, points)
    with pytest.raises(RuntimeError, match='left the fp16 range'):
        g.check_range()
    assert eng.trunk == 'f16x3', 'a replay cannot change the captured arithmetic'
    # the counters were reset by the read: an in-range replay passes again
    assert_same_scores(replay(g, crops, points)[0], want[0], 'in-range replay after the out-of-range one')
    assert g.check_range() == (0, 0, 0)
    m.set_trunk('f32')
    with pytest.raises(RuntimeError, match='stale'):
        g(crops, points)
    g32 = m.capture(plan, crops, points)
    det, links, new, end = replay(g32, hot_d, points)[0]
    err = linf((det, links, new, end), ref_hot)
    print('f32 graph on the out-of-range inputs vs the oracle: %.2e' % err)
    assert err < TOL
    assert g32.check_range() == (0, 0, 0) and m.engine().trunk == 'f32'


# ---- E. staleness ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['invalidate', 'set_trunk', 'load_state_dict', 'to'])
def test_a_repack_makes_the_replay_raise(how):
    m, c = model('s2_C_multiply_none')
    plan, sets = case_sets(m, c, n=2)
    want = eager_all(m, plan, sets)
    g = m.capture(plan, *sets[0])
    assert_same_scores(replay(g, *sets[1])[0], want[1][0], 'before %s' % how)
    if how == 'invalidate':
        m.invalidate()
    elif how == 'set_trunk':
        m.set_trunk('f16x3')
    elif how == 'load_state_dict':
        m.load_state_dict(m.state_dict())
    else:
        m.to(DEV)
    for _ in range(2):  # before and after the engine is rebuilt
        with pytest.raises(RuntimeError, match='stale'):
            g(*sets[1])
        m.engine()
    assert_same_scores(replay(m.capture(plan, *sets[0]), *sets[1])[0], want[1][0], 're-captured after %s' % how)


def test_a_head_edit_makes_the_replay_raise_until_refresh_head():
    m, c = model('s2_C_multiply_none', private=True)
    plan, sets = case_sets(m, c, n=2)
    g = m.capture(plan, *sets[0])
    before = replay(g, *sets[1])[0]
    scalars = packed_scalars(m.engine().P)
    assert len(scalars) >= 4  # the three output biases and the fp16-split scales
    edit_below_half_max(m.w_link.conv1[3].weight, 1.01)
    bn = m.w_det[1]
    edit_below_half_max(m.w_det[0].weight, 0.99, gain=bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps))
    assert not m.head_is_current() and m._pack_version == g._pack_version
    with pytest.raises(RuntimeError, match=r'stale.*refresh_head\(\).*capture again'):
        g(*sets[1])
    eng = m.engine()
    assert m.refresh_head() is eng
    assert packed_scalars(eng.P) == scalars, 'the edit was meant to keep every by-value scalar of the packed head'
    assert not g.stale()
    after = replay(g, *sets[1])[0]
    assert_same_scores(after, eager(m, plan, *sets[1])[0], 'replay after refresh_head() vs the eager forward')
    assert m.engine() is eng
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1][0], before[1][0])


def test_an_encoder_edit_makes_the_replay_raise_until_recapture():
    m, c = model('s2_C_multiply_none', private=True)
    plan, sets = case_sets(m, c, n=2)
    g = m.capture(plan, *sets[0])
    before = replay(g, *sets[1])[0]
    with torch.no_grad():
        m.point_net.conv2.weight.mul_(1.01)
    with pytest.raises(RuntimeError, match='stale'):
        g(*sets[1])
    m.refresh_head()    # re-packs the heads only
    with pytest.raises(RuntimeError, match='stale'):
        g(*sets[1])
    g2 = m.capture(plan, *sets[0])
    assert not g2.stale() and g.stale()
    after = replay(g2, *sets[1])[0]
    assert_same_scores(after, eager(m, plan, *sets[1])[0], 're-captured after an encoder edit vs the eager forward')
    assert not g2.stale() and not torch.equal(after[1][0], before[1][0])


def test_a_training_forward_makes_the_replay_raise():
    m, c = model('s2_C_multiply_none', private=True)
    plan, sets = case_sets(m, c, n=2)
    g = m.capture(plan, *sets[0])
    replay(g, *sets[1])
    dets, info, ds = case_inputs(c)
    m.train()
    m.freeze_appearance = True
    m(dets.to(DEV), {k: v.to(DEV) for k, v in info.items()}, ds)
    m.eval()
    assert m._trained_since_pack or not m._packed_is_current()
    with pytest.raises(RuntimeError, match='stale'):
        g(*sets[1])
    want = eager(m, plan, *sets[1])[0]  # re-packs
    with pytest.raises(RuntimeError, match='stale'):
        g(*sets[1])
    assert_same_scores(replay(m.capture(plan, *sets[0]), *sets[1])[0], want, 're-captured after a training forward')


# ---- F. inputs refused before any copy -------------------------------------------------------------------------------
def test_inputs_of_another_shape_or_type_are_refused_before_any_copy():
    m, c = model('s2_C_multiply_none')
    plan, sets = case_sets(m, c, n=2)
    want = eager_all(m, plan, sets)
    u8 = [u8_crops(a.cpu()).to(DEV) for a, _ in sets]
    g = m.capture(plan, *sets[0])
    g8 = m.capture(plan, u8[0], sets[0][1])
    want8 = eager(m, plan, u8[0], sets[0][1])[0]
    (c1, p1), S = sets[1], c['S']
    bad = [(g, c1[:1], p1, 'crops'), (g, c1[0], p1, 'crops'), (g, u8[1], p1, 'crops'),
           (g, c1.to(torch.uint8), p1, 'crops'), (g8, c1, p1, 'crops'), (g8, u8[1].float(), p1, 'crops'),
           (g, c1, torch.cat([p1, p1[:, :1]], 1).contiguous(), 'points'), (g, None, p1[:1], 'points'),
           (g, c1.half(), None, 'crops'), (g, None, p1.double(), 'points')]
    for gr, crops, points, which in bad:
        buf = (gr.crops.clone(), gr.points.clone())
        with pytest.raises(ValueError, match='%s of a captured forward' % which):
            gr(crops, points)
        assert torch.equal(gr.crops, buf[0]) and torch.equal(gr.points, buf[1]), 'a refused call changed the buffers'
    # nothing was copied and nothing replayed: both graphs still hold, and return, their captured set
    assert_same_scores(replay(g, None, None)[0], want[0][0], 'fp32 graph after the refusals')
    assert_same_scores(replay(g8, None, None)[0], want8, 'uint8 graph after the refusals')
    # crops=None is no error: it keeps the crop buffer
    assert_same_scores(replay(g, None, p1)[0], eager(m, plan, sets[0][0], p1)[0], 'crops=None, new points')
    with pytest.raises(ValueError, match='captured without points'):
        m.capture(m.make_plan([([5, 7], None)], S, rows=(0,)), sets[0][0], None)(None, p1)
