"""Appearance rows computed once per frame (TrackingNet.encode_appearance) in place of crops, on the torch emulation of the
C-ABI: the engine's bookkeeping of shape (a) (every row given) and shape (b) (the first frame's rows + the second frame's
crops), the Meta kernels of the new operators, the validity stamp and every host check before a launch.  GPU twin with
the bitwise comparisons: tests/test_appearance_reuse_gpu.py."""
import pytest
import torch

from common import CallLog, assert_same_scores, build_model, case_inputs, get_case, scores, u8_crops
from fake_ops import TorchOps
from mmmot_amd import torch_ops
from mmmot_amd.modules import AppearanceRows, StaleAppearanceError
from mmmot_amd.plan import BatchPlan, CropPlan


def model(name='s6_endmax_C', trunk='f16x3'):
    c, base = get_case(name)
    m = build_model(c, base, ops=TorchOps())
    m.set_trunk(trunk)
    return m, c


def pair_plan(m, c, info, ds, rows=(0, 1, 2)):
    fc = [int(d) for d in ds]
    ps = info['points_split'].reshape(-1).long().cpu().numpy()
    return m.make_plan([(fc, ps)], c['S'], rows=rows)


def full_cat(m, plan, dets, info):
    with torch.no_grad():
        return m.engine().forward(plan, dets, info['points'].reshape(-1, 3))['cat'][:, :512].clone()


def test_shape_a_rows_supplied_equal_rows_computed():
    m, c = model()
    dets, info, ds = case_inputs(c)
    plan = pair_plan(m, c, info, ds)
    pts = info['points'].reshape(-1, 3)
    rows = full_cat(m, plan, dets, info)
    with torch.no_grad():
        want = scores(m.forward_batch(plan, dets, pts)[0])
        log = CallLog(m.engine().ops)
        m.engine().ops = log
        got = scores(m.forward_batch(plan, None, pts, appearance=rows)[0])
        m.engine().ops = log.ops
    assert_same_scores(got, want, 'shape (a)')
    assert not any(k.startswith('conv') or k == 'skippool_head' for k in log.calls), log.calls
    assert 'pointnet_layer1' in log.calls


def test_shape_b_leading_rows_and_trailing_crops():
    m, c = model()
    dets, info, ds = case_inputs(c)
    N = int(ds[0])
    plan = pair_plan(m, c, info, ds)
    pts = info['points'].reshape(-1, 3)
    rows = full_cat(m, plan, dets, info)
    with torch.no_grad():
        out = m.engine().forward(plan, dets[N:].contiguous(), pts, appearance=rows[:N].clone())
        cat = out['cat'][:, :512]
        assert torch.equal(cat[:N], rows[:N])            # the supplied rows, copied in
        assert torch.allclose(cat[N:], rows[N:], atol=1e-5, rtol=0)   # the trunk on the M crops alone
        enc = m.encode_appearance(dets[N:])
        assert isinstance(enc, AppearanceRows) and enc.rows.shape == (len(dets) - N, 512)
        assert torch.equal(enc.rows, cat[N:])           # same crops, same tables: same rows
        res, nxt = m.forward_appearance(m.encode_appearance(dets[:N]), dets[N:], info, ds, return_rows=True)
        ref = m(dets, info, ds)
    assert torch.equal(nxt.rows, enc.rows) and m.appearance_is_current(nxt)
    for a, b in zip(scores(res), scores(ref)):
        for x, y in zip(a, b) if isinstance(a, list) else [(a, b)]:
            assert torch.allclose(x, y, atol=1e-5, rtol=0)


def test_encode_appearance_owns_its_rows_and_takes_uint8_crops():
    m, c = model()
    dets, info, ds = case_inputs(c)
    with torch.no_grad():
        a = m.encode_appearance(dets)
        ws = [t for k, t in m.engine().ws.items() if isinstance(k, str)]
        assert not any(a.rows.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for t in ws)
        u8 = u8_crops(dets)
        b = m.encode_appearance(u8)
        plan = pair_plan(m, c, info, ds)
        ref = m.engine().forward(plan, u8, info['points'].reshape(-1, 3))['cat'][:, :512]
    assert torch.equal(b.rows, ref)
    assert [len(r) for r in a.split([int(ds[0]), int(ds[1])])] == [int(ds[0]), int(ds[1])]


def test_stamp_follows_weights_trunk_mode_and_range_events():
    m, c = model()
    dets, _, _ = case_inputs(c)
    with torch.no_grad():
        r = m.encode_appearance(dets)
    eng = m.engine()
    pv, serial, trunk, fwd, nev = r.stamp
    assert (pv, serial, trunk, nev) == (m._pack_version, eng.serial, 'f16x3', len(eng.range_events))
    assert fwd == eng.guard.n_forward - 1
    assert m.appearance_is_current(r)
    m.train()
    assert not m.appearance_is_current(r)
    m.eval()
    assert m.appearance_is_current(r)
    # an out-of-range event recorded after the rows (late detection covers the forward that made them)
    eng.range_events.append(dict(forward=fwd + 1, affected_forwards=(fwd, fwd), recomputed=False))
    assert not m.appearance_is_current(r)
    eng.range_events.pop()
    assert m.appearance_is_current(r)
    eng.trunk = 'f32'                   # the guard lowered the arithmetic
    assert not m.appearance_is_current(r)
    eng.trunk = 'f16x3'
    with torch.no_grad():
        next(m.parameters()).add_(0.0)  # an in-place edit: the engine re-packs at its next eval entry
    assert not m.appearance_is_current(r)
    for change in (lambda: m.set_trunk('f32'), lambda: m.load_state_dict(m.state_dict()), m.invalidate,
                   lambda: m.set_ops(TorchOps()), lambda: m.to('cpu')):
        with torch.no_grad():
            r = m.encode_appearance(dets)
        assert m.appearance_is_current(r)
        change()
        assert not m.appearance_is_current(r)


def test_stale_rows_are_refused_before_any_launch():
    m, c = model()
    dets, info, ds = case_inputs(c)
    N = int(ds[0])
    with torch.no_grad():
        r = m.encode_appearance(dets[:N])
    m.set_trunk('f32')
    m.engine().ops = log = CallLog(m.engine().ops)
    with pytest.raises(StaleAppearanceError):
        m.forward_appearance(r, dets[N:], info, ds)
    assert log.calls == []


def test_settle_range_records_a_late_event_and_stales_the_rows():
    m, c = model(trunk='f16x3')
    dets, _, _ = case_inputs(c)
    with torch.no_grad():
        m.encode_appearance(dets)          # first forward: synchronous check
        r = m.encode_appearance(dets)      # second: asynchronous read-back queued
    eng = m.engine()
    eng.guard.block[1] += 3                # fp16-clamped elements counted by that trunk (what the epilogues count) ...
    eng.guard.host[1] += 3                 # ... and the completed read-back queued behind it
    with pytest.warns(RuntimeWarning, match='detected late'):
        assert not m.appearance_is_current(r)   # takes the guard's verdict on the forward that made the rows
    ev = eng.range_events[-1]
    assert ev['now'] == 'f32' and not ev['recomputed'] and ev['affected_forwards'][1] == r.stamp[3]


def test_rows_the_guard_rejects_are_refused_before_they_are_used():
    """the direct cached-pair call: the read-back of the forward that made the rows has completed (the caller read its
    results) but no later forward inspected it yet - forward_appearance takes the verdict first and refuses the rows"""
    m, c = model(trunk='f16x3')
    dets, info, ds = case_inputs(c)
    N = int(ds[0])
    with torch.no_grad():
        m.encode_appearance(dets[N:])          # first forward: synchronous check
        r = m.encode_appearance(dets[:N])      # forward 1: asynchronous read-back queued ...
    eng = m.engine()
    eng.guard.block[1] += 3                    # ... and its trunk left the fp16 range
    eng.guard.host[1] += 3
    eng.ops = log = CallLog(eng.ops)
    with pytest.warns(RuntimeWarning, match='detected late'), pytest.raises(StaleAppearanceError):
        m.forward_appearance(r, dets[N:], info, ds)
    assert log.calls == [] and eng.trunk == 'f32'
    assert eng.out_of_range_window == (r.stamp[3], r.stamp[3])
    with torch.no_grad():                      # encoded again in the lowered arithmetic: usable
        r = m.encode_appearance(dets[:N])
        out, nxt = m.forward_appearance(r, dets[N:], info, ds, return_rows=True)
    assert m.appearance_is_current(r) and m.appearance_is_current(nxt) and r.stamp[2] == 'f32'


def _value_errors(m, c, dets, info, ds):
    """(what, call) for every host check of supplied rows; inputs on the model's device"""
    N = int(ds[0])
    plan = pair_plan(m, c, info, ds)
    eng = m.engine()
    dev = dets.device
    pts = info['points'].reshape(-1, 3).contiguous()
    rows = torch.zeros(plan.Lt, 512, device=dev)
    lidar_only = pair_plan(m, c, info, ds, rows=(1,))
    p2 = BatchPlan([([N, int(ds[1])], info['points_split'].reshape(-1).long().cpu().numpy())] * 2, c['S'], dev)
    pts2 = torch.cat([pts, pts])
    return [
        ('wrong width', lambda: eng.forward(plan, None, pts, appearance=torch.zeros(plan.Lt, 256, device=dev))),
        ('wrong count', lambda: eng.forward(plan, None, pts, appearance=rows[1:].clone())),
        ('wrong dtype', lambda: eng.forward(plan, None, pts, appearance=rows.double())),
        ('not contiguous', lambda: eng.forward(plan, None, pts, appearance=torch.zeros(512, plan.Lt, device=dev).t())),
        ('wrong device', lambda: eng.forward(plan, None, pts, appearance=rows.to('meta'))),
        ('not a tensor', lambda: eng.forward(plan, None, pts, appearance=rows.tolist())),
        ('rows and crops for every frame', lambda: eng.forward(plan, dets, pts, appearance=rows)),
        ('rows for the second frame too', lambda: eng.forward(plan, dets[N:].contiguous(), pts,
                                                              appearance=rows[:N + 1].clone())),
        ('crops for both frames', lambda: eng.forward(plan, dets, pts, appearance=rows[:N].clone())),
        ('crops of the wrong side', lambda: eng.forward(plan, torch.zeros(plan.Lt - N, 3, 34, 34, device=dev), pts,
                                                        appearance=rows[:N].clone())),
        ('rows beside crops on a B = 2 plan', lambda: eng.forward(p2, dets[N:].contiguous(), pts2,
                                                                  appearance=rows[:N].clone())),
        ('rows on a LiDAR-only plan', lambda: eng.forward(lidar_only, None, pts, appearance=rows)),
        ('image_first', lambda: eng.image_first(plan, dets, appearance=rows[:N].clone())),
        ('module', lambda: m.forward_batch(plan, None, pts, appearance='rows')),
    ]


def test_every_value_error_comes_before_any_launch():
    m, c = model()
    dets, info, ds = case_inputs(c)
    with torch.no_grad():
        m(dets, info, ds)
    eng = m.engine()
    eng.ops = log = CallLog(eng.ops)
    for what, call in _value_errors(m, c, dets, info, ds):
        with pytest.raises(ValueError):
            with torch.no_grad():
                call()
        assert log.calls == [], (what, log.calls)
        assert eng._head_start is None, what


def test_meta_kernels_give_the_output_shapes():
    m, c = model('s2_C_multiply_none')
    dets, info, ds = case_inputs(c)
    N, M = int(ds[0]), int(ds[1])
    plan = pair_plan(m, c, info, ds)
    eh, ph = torch_ops.engine_handle(m.engine()), torch_ops.plan_handle(plan)
    meta = lambda *s: torch.empty(*s, device='meta')
    det, link, new, end = torch.ops.mmmot.forward_batch_appearance(meta(N + M, 512), meta(plan.P, 3), eh, ph)
    assert det.shape == new.shape == end.shape == (3, N + M) and link.shape == (3 * N * M,) and det.is_meta
    det, link, new, end, rows = torch.ops.mmmot.forward_pair_appearance(meta(N, 512), meta(M, 3, 64, 64),
                                                                        meta(plan.P, 3), eh, ph)
    assert det.shape == (3, N + M) and link.shape == (3 * N * M,) and rows.shape == (M, 512)
    cp = CropPlan(7, 64, 'cpu')
    rows = torch.ops.mmmot.encode_appearance(meta(7, 3, 64, 64), eh, torch_ops.plan_handle(cp))
    assert rows.shape == (7, 512) and rows.is_meta
    with pytest.raises(NotImplementedError):  # no CPU kernel: no fallback
        torch.ops.mmmot.forward_batch_appearance(torch.zeros(N + M, 512), info['points'].reshape(-1, 3), eh, ph)


def test_crop_plan_matches_the_pair_plan_tables():
    plan = BatchPlan([([3, 5], None)], 64, 'cpu', rows=(0,), use_points=False)
    cp = plan.tail_crops()
    assert cp is plan.tail_crops() and cp.Lt == 5 and cp.S == 64
    for hw in (256, 64, 16, 4):
        a, b = cp.crop_segments(hw), CropPlan(5, 64, 'cpu').crop_segments(hw)
        assert len(a.levels) == len(b.levels) and a.levels[0].n == b.levels[0].n
        assert (a.levels[0].h_count == b.levels[0].h_count).all() and (a.levels[0].h_start == b.levels[0].h_start).all()
    with pytest.raises(ValueError):
        BatchPlan([([3, 5, 2], None)], 64, 'cpu', rows=(0,), use_points=False).tail_crops()


def test_default_paths_are_unchanged_by_the_new_keyword():
    m, c = model('s1_C_minus_abs_dual_add')
    dets, info, ds = case_inputs(c)
    plan = pair_plan(m, c, info, ds)
    with torch.no_grad():
        a = scores(m.forward_batch(plan, dets, info['points'].reshape(-1, 3))[0])
        b = scores(m(dets, info, ds))
    assert_same_scores(a, b, 'forward_batch vs forward')
    # the rows of N = 1 frames: shape (b) with one leading and one trailing detection
    with torch.no_grad():
        out = m.forward_appearance(m.encode_appearance(dets[:1]), dets[1:], info, ds)
    for x, y in zip(scores(out), b):
        for u, v in zip(x, y) if isinstance(x, list) else [(x, y)]:
            assert torch.allclose(u, v, atol=1e-5, rtol=0)
