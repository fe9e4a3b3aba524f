"""A forward reads only what it wrote.  Engine.buf / buf64 hand out torch.empty slices of a reused arena: memory that
usually holds finite, often identical values, so a kernel that reads outside its own writes (padding rows of a tile, a
view's tail beyond [:n], K-padding channels times zero weights, the lower 32 x 32 blocks of the K = 128 Gram partials)
still returns stable scores.  Here every scratch entry of the workspace is filled byte-wise between two forwards - 0xFF
(NaN in every float format of the path) and 0x7B (finite but huge: 1.3e36 as f32, 61280 as f16, 352 as e4m3) - and the
second forward must return the first one's scores bit for bit.  A large batch followed by a small one over poison must
equal a fresh engine's small batch (reads past a view).  No workspace buffer feeds an address computation: every entry is
float-typed data; the integer tables live in the plan objects.  CPU twin: tests/test_workspace_poison_cpu.py."""
import pytest
import torch

from common import (POISON, assert_same_scores, build_model, case_inputs, check_over_poison, get_case,
                    poison_workspace, scores, u8_crops)
from mmmot_amd.synth import make_pair

pytestmark = pytest.mark.gpu

_MODELS = {}


def model(name, trunk, **knobs):
    """the case's model on the device (built once per case), on a FRESH engine with the given trunk and engine knobs"""
    c, base = get_case(name)
    m = _MODELS.get(name)
    if m is None:
        m = _MODELS[name] = build_model(c, base, device='cuda')
    m.set_trunk(trunk)  # a new engine: new workspace, knobs back at their defaults
    eng = m.engine()
    for k, v in knobs.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    return m, c


def dev_inputs(c):
    dets, info, ds = case_inputs(c)
    return dets.cuda(), {k: v.cuda() for k, v in info.items()}, ds


CASES = [  # (golden case: fusion / affinity / softmax / counts, trunk, engine knobs)
    ('s2_A_multiply_none', 'f32', {}),
    ('s2_A_multiply_none', 'f16x3', {}),
    ('s2_A_multiply_none', 'f16q8', {}),
    ('s2_B_multiply_none', 'f32', {}),
    ('s2_B_multiply_none', 'f16x3', {}),
    ('s2_B_multiply_none', 'f16q8', {}),
    ('s2_C_multiply_none', 'f32', {}),
    ('s2_C_multiply_none', 'f16x3', {}),
    ('s2_C_multiply_none', 'f16q8', {}),
    ('s2_A_minus_abs_dual_add', 'f16x3', {}),
    ('s2_C_minus_dual_max', 'f16q8', {}),
    ('s2_C_minus_single', 'f16x3', {}),
    ('s1_C_minus_abs_dual_add', 'f16x3', {}),          # N = M = 1
    ('s1_A_multiply_none', 'f32', {}),
    ('s6_endmax_A', 'f16x3', {}),                      # 4 x 11, end_mode max
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0}),      # 9 x 6, hq8 trunk at 32-pixel crops
    ('s5_3frames_B', 'f16x3', {}),                     # three frames
    ('s7_refl_C', 'f16x3', {}),                        # four point channels
    ('s8_S100_A', 'f16x3', {}),                        # odd maps on the way down
    ('s8_S40_C', 'f16q8', {'q8_min_crop': 0}),
    ('s4_cfg4like_C', 'f16x3', {}),                    # 32 x 32
    ('s2_C_minus_abs_dual_add', 'f16x3', {'pn_gram': False}),
    ('s2_C_minus_abs_dual_add', 'f16x3', {'pn_fused': False}),
    ('s2_C_minus_abs_dual_add', 'f16x3', {'fuse_conv1': False}),
    ('s2_C_minus_abs_dual_add', 'f16q8', {'fuse_conv1': False}),
    ('s2_C_minus_abs_dual_add', 'f16x3', {'pn_mlp64': False, 'sp_fused': False}),
    ('s2_C_minus_abs_dual_add', 'f16x3', {'two_streams': True}),
]


@pytest.mark.parametrize('name,trunk,knobs', CASES,
                         ids=['%s-%s%s' % (n, t, ''.join('-%s=%s' % kv for kv in k.items())) for n, t, k in CASES])
def test_forward_over_a_poisoned_workspace(name, trunk, knobs):
    m, c = model(name, trunk, **knobs)
    dets, info, ds = dev_inputs(c)
    check_over_poison(m, lambda: m(dets, info, ds), '%s %s %r' % (name, trunk, knobs))
    assert m.engine().trunk == trunk


@pytest.mark.parametrize('rows', [(0,), (1,)])
def test_single_modality_rows_over_a_poisoned_workspace(rows):
    """cfg5: image-only / LiDAR-only rows (the other branch's buffers are never written in these forwards)"""
    m, c = model('s2_C_multiply_none', 'f16x3')
    dets, info, ds = dev_inputs(c)
    check_over_poison(m, lambda: m.forward_rows(dets, info, ds, rows=rows), 'rows %r' % (rows,))


@pytest.mark.parametrize('trunk', ['f32', 'f16x3', 'f16q8'])
def test_uint8_crops_over_a_poisoned_workspace(trunk):
    """f32: mmmot_u8_normalize into the workspace; f16x3 / f16q8: the fused first launch reads the bytes"""
    m, c = model('s2_C_multiply_none', trunk)
    dets, info, ds = dev_inputs(c)
    u8 = u8_crops(dets.cpu()).cuda()
    check_over_poison(m, lambda: m(u8, info, ds), 'uint8 crops, %s' % trunk)


def test_cfg3_over_a_poisoned_workspace():
    """full cfg3 size (64 x 64 detections of 128 pixels, 2048 points each): the K = 128 Gram route over many super-tiles"""
    m, c = model('f_cfg3_C', 'f16x3')
    dets, info, ds = dev_inputs(c)
    check_over_poison(m, lambda: m(dets, info, ds), 'f_cfg3_C')


@pytest.mark.parametrize('trunk', ['f32', 'f16x3', 'f16q8'])
def test_small_batch_after_a_large_one_over_poison(trunk):
    """every workspace entry is larger than the small batch needs: reads past a view's [:n] meet the poison"""
    name = 's2_C_minus_abs_dual_add'
    m, c = model(name, trunk)
    small = dev_inputs(c)
    with torch.no_grad():
        want = scores(m(*small))          # a fresh engine
    m, _ = model(name, trunk)              # another fresh engine: large batch first
    dets, info, ds = make_pair(40, 36, 96, 300, seed=77, ragged=True)
    with torch.no_grad():
        m(dets.cuda(), {k: v.cuda() for k, v in info.items()}, ds)
        for byte in POISON:
            poison_workspace(m.engine(), byte)
            assert_same_scores(scores(m(*small)), want, 'small batch after a large one, %s, 0x%02X' % (trunk, byte))
