"""TrackingNet's bookkeeping, on the CPU over tests/fake_ops.TorchOps: the one snapshot of the tensors the engine was packed
from, the one head layout shared by the host packing and the device refresh, and the plan caches."""
import pytest
import torch

from common import build_model, case_inputs, get_case, scores, assert_same_scores
from fake_ops import TorchOps
from mmmot_amd.pack import pack_weights

HEAD_KEYS = ('fusion', 'w_link')


def _edit(module, seed):
    """in-place edit of every parameter of `module` (what optimizer.step() does), each by its own amounts"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(1.0 + 0.01 * torch.randn(p.shape, generator=g)).add_(1e-3 * torch.randn(p.shape, generator=g))


def _ptrs(eng):
    return {(s, k): v.data_ptr() for s in HEAD_KEYS for k, v in eng.P[s].items() if torch.is_tensor(v)}


@pytest.mark.parametrize('fusion', ['A', 'B', 'C'])
def test_device_refresh_equals_host_packing(fusion):
    """refresh_head_device() (live fp32 parameters, on their device) and pack_weights (fp64 on the host) lay the head out
    the same way: pure data movement, so every fp32 entry agrees bit for bit, and the refresh keeps the addresses."""
    c, base = get_case('s2_%s_multiply_none' % fusion)
    m = build_model(c, base, ops=TorchOps())
    eng = m.engine()
    ptrs = _ptrs(eng)
    _edit(m.fusion_module, 1)
    _edit(m.w_link, 2)
    assert m.refresh_head_device() is eng
    want = pack_weights(m.state_dict(), fusion, 'cpu')
    n = 0
    for s in HEAD_KEYS:
        for k, v in want[s].items():
            if not torch.is_tensor(v) or k.endswith('_h16'):
                continue
            assert torch.equal(eng.P[s][k], v), (s, k)
            n += 1
    assert n == {'A': 4, 'B': 8, 'C': 8}[fusion] + 24, n # every fp32 tensor entry of the two sections was compared
    for k in ('b9', 'nb6'):
        assert eng.P['w_link'][k] == want['w_link'][k], k
    assert _ptrs(eng) == ptrs


def test_snapshot_truth_table():
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    ins = case_inputs(c)
    eng = m.engine()
    assert m.head_is_current() and m._packed_is_current()
    # a head parameter: the head and the pack are stale
    with torch.no_grad():
        m.w_link.conv1[3].weight.mul_(1.001)
    assert not m.head_is_current() and not m._packed_is_current()
    # refresh_head(): the head is current again, the encoders' snapshot is untouched
    with torch.no_grad():
        m.point_net.conv2.weight.mul_(1.001)
    assert m.refresh_head() is eng and m.head_is_current()
    assert not m._packed_is_current(), 'refresh_head() took the edited encoder for packed'
    with torch.no_grad():
        m(*ins)
    assert m.engine() is not eng, 'the eval forward did not re-pack after an encoder edit'
    # an encoder parameter alone: the head is current, the pack is stale, the next eval forward re-packs
    eng = m.engine()
    with torch.no_grad():
        m.point_net.conv2.weight.mul_(1.001)
    assert m.head_is_current() and not m._packed_is_current()
    with torch.no_grad():
        m(*ins)
    assert m.engine() is not eng and m._packed_is_current()
    # refresh_head_device(): the head is current, captured graphs are stale, the next eval forward re-packs
    eng, v = m.engine(), m._pack_version
    _edit(m.w_link, 3)
    assert not m.head_is_current()
    assert m.refresh_head_device() is eng and m.head_is_current() and m._pack_version > v
    with torch.no_grad():
        got = scores(m(*ins))
    assert m.engine() is not eng, 'the eval forward ran on the stale fp16-split copies'
    m.invalidate()
    with torch.no_grad():
        assert_same_scores(got, scores(m(*ins)), 'forward after refresh_head_device vs a freshly invalidated model')


def test_plan_cache_keeps_the_most_recently_used():
    from mmmot_amd.plan import PlanCache
    built = []
    build = lambda k: lambda: (built.append(k), 'plan %s' % k)[1]
    cache = PlanCache(3)
    for k in 'abc':
        assert cache.get(k, build(k)) == 'plan %s' % k
    assert built == ['a', 'b', 'c'] and len(cache) == 3
    assert cache.get('a', build('a')) == 'plan a' and built == ['a', 'b', 'c']  # a hit does not build
    cache.get('d', build('d'))                                                   # 'b' is the least recently used now
    assert len(cache) == 3 and built == ['a', 'b', 'c', 'd']
    for k in 'acd':
        cache.get(k, build(k))
    assert built == ['a', 'b', 'c', 'd']                                         # all three were kept ...
    cache.get('b', build('b'))
    assert built == ['a', 'b', 'c', 'd', 'b'] and len(cache) == 3                # ... and 'b' was the one evicted
    cache.clear()
    assert len(cache) == 0
    assert PlanCache('0').capacity == 1 and PlanCache('8').capacity == 8         # MMMOT_TRAIN_PLAN_CACHE: at least 1


def test_model_plan_caches(monkeypatch):
    import mmmot_amd.modules as modules
    monkeypatch.delenv('MMMOT_TRAIN_PLAN_CACHE', raising=False)
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    m.freeze_appearance = True
    dets, info, ds = ins = case_inputs(c)
    built = []

    class CountedPlan(modules.BatchPlan):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(modules, 'BatchPlan', CountedPlan)
    assert (m._plans.capacity, m._img_plans.capacity, m._crop_plans.capacity, m._train_plans.capacity) == (64, 256, 256, 8)
    m.engine()  # (packing starts from an empty _plans)
    with torch.no_grad():
        m(*ins)
        m(*ins)
        assert len(built) == 1 and len(m._plans) == 1  # the second forward hit
        m._plans.clear()
        m(*ins)
        assert len(built) == 2 and len(m._plans) == 1  # cleared: the next forward builds its plan again
        m.encode_appearance(dets)
        m._image_plan([int(d) for d in ds], c['S'], 'cpu')
    m.train()
    m(*ins)
    m.eval()
    caches = (m._plans, m._img_plans, m._crop_plans, m._train_plans)
    assert [len(x) for x in caches] == [1, 1, 1, 1]
    m.invalidate()
    assert [len(x) for x in caches] == [0, 0, 0, 0]
    assert caches == (m._plans, m._img_plans, m._crop_plans, m._train_plans)  # emptied, not replaced
