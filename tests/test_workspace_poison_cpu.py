"""CPU twin of tests/test_workspace_poison_gpu.py on the torch emulation of the C-ABI: the engine's launch schedule reads
only workspace entries that the same forward wrote (views, padding and re-used buffers included) - a forward over a
workspace filled with 0xFF / 0x7B bytes returns the scores of the forward before it bit for bit."""
import pytest
import torch

from common import (POISON, assert_same_scores, build_model, case_inputs, check_over_poison, get_case,
                    poison_workspace, scores, u8_crops)
from fake_ops import TorchOps
from mmmot_amd.synth import make_pair


def model(name, trunk, **knobs):
    c, base = get_case(name)
    m = build_model(c, base, ops=TorchOps())
    m.set_trunk(trunk)
    eng = m.engine()
    for k, v in knobs.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    return m, c


CASES = [
    ('s1_C_minus_abs_dual_add', 'f16x3', {}),
    ('s6_endmax_A', 'f32', {}),
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0}),
    ('s5_3frames_B', 'f16x3', {}),
    ('s6_endmax_C', 'f16x3', {'pn_gram': False}),
    ('s6_endmax_C', 'f16x3', {'pn_fused': False}),
    ('s6_endmax_C', 'f16x3', {'fuse_conv1': False, 'sp_fused': False}),
]


@pytest.mark.parametrize('name,trunk,knobs', CASES,
                         ids=['%s-%s%s' % (n, t, ''.join('-%s=%s' % kv for kv in k.items())) for n, t, k in CASES])
def test_forward_over_a_poisoned_workspace(name, trunk, knobs):
    m, c = model(name, trunk, **knobs)
    dets, info, ds = case_inputs(c)
    check_over_poison(m, lambda: m(dets, info, ds), '%s %s %r' % (name, trunk, knobs))


def test_rows_and_uint8_crops_over_a_poisoned_workspace():
    m, c = model('s6_endmax_C', 'f16x3')
    dets, info, ds = case_inputs(c)
    for rows in ((0,), (1,)):
        check_over_poison(m, lambda: m.forward_rows(dets, info, ds, rows=rows), 'rows %r' % (rows,))
    u8 = u8_crops(dets)
    check_over_poison(m, lambda: m(u8, info, ds), 'uint8 crops')


def test_poison_reaches_every_scratch_entry_and_no_constant():
    m, c = model('s6_endmax_C', 'f32')
    dets, info, ds = case_inputs(c)
    with torch.no_grad():
        m(u8_crops(dets), info, ds)
    eng = m.engine()
    consts = {k: v.clone() for k, v in eng.ws.items() if not isinstance(k, str)}
    assert consts, 'the uint8 path keeps its mean / std constant in the workspace'
    poison_workspace(eng, 0xFF)
    for k, v in eng.ws.items():
        if isinstance(k, str):
            assert bool((v.view(torch.uint8) == 0xFF).all()), k
        else:
            assert torch.equal(v, consts[k]), k


def test_small_batch_after_a_large_one_over_poison():
    name = 's6_endmax_A'
    m, c = model(name, 'f16x3')
    small = case_inputs(c)
    with torch.no_grad():
        want = scores(m(*small))
    m, _ = model(name, 'f16x3')
    dets, info, ds = make_pair(9, 8, 48, 30, seed=77, ragged=True)
    with torch.no_grad():
        m(dets, info, ds)
        for byte in POISON:
            poison_workspace(m.engine(), byte)
            assert_same_scores(scores(m(*small)), want, 'small batch after a large one, 0x%02X' % byte)
