"""Host checks of the 8-bit crop input (Engine._check_crops, mmmot_amd.engine.check_crop_layout, train.forward_train) on
the torch emulation of the C-ABI: a wrong layout, side or stride is refused with a ValueError before any operator is
called, and the training-mode forward refuses uint8 crops as its first step.  The device twins are in
tests/test_u8_crops_gpu.py."""
import pytest
import torch

from common import CallLog, assert_same_scores, build_model, case_inputs, get_case, normalise_u8, scores, u8_crops
from fake_ops import TorchOps


def _model(name='s6_endmax_A'):
    c, base = get_case(name)
    m = build_model(c, base, ops=TorchOps())
    dets, info, ds = case_inputs(c)
    return m, c, dets, info, ds


def test_u8_input_helpers_keep_channels_apart():
    m, c, dets, info, ds = _model()
    u8 = u8_crops(dets)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (dets.shape[0], c['S'], c['S'], 3) and u8.is_contiguous()
    assert int(u8.min()) == 0 and int(u8.max()) == 255
    for ch, lo in enumerate((0, 96, 192)):
        v = u8[..., ch].long()
        assert int(v.min()) >= lo and int(v.max()) <= lo + 63
    x = normalise_u8(u8)
    assert x.dtype == torch.float32 and tuple(x.shape) == tuple(dets.shape)
    # the three channels land in disjoint normalised ranges
    hi = [float(x[:, ch].max()) for ch in range(3)]
    lo = [float(x[:, ch].min()) for ch in range(3)]
    assert hi[0] < lo[1] and hi[1] < lo[2]


def test_bad_uint8_crops_are_refused_before_any_operator():
    m, c, dets, info, ds = _model()
    S = c['S']
    u8 = u8_crops(dets)
    eng = m.engine()
    log = CallLog(eng.ops)
    eng.ops = log
    with torch.no_grad():
        with pytest.raises(ValueError, match=r'uint8 crops must be \[L,S,S,3\]'):
            m(u8.permute(0, 3, 1, 2).contiguous(), info, ds)  # NCHW bytes
        for bad in (41, 30):  # odd side; a side that leaves nothing after five poolings
            with pytest.raises(ValueError, match='crop side'):
                m(torch.zeros(dets.shape[0], bad, bad, 3, dtype=torch.uint8), info, ds)
        with pytest.raises(ValueError, match=r'uint8 crops must be \[L,S,S,3\]'):
            m(torch.zeros(dets.shape[0], S, S + 2, 3, dtype=torch.uint8), info, ds)  # H != W
        # the batched entry takes the crops as they are: a strided uint8 view is refused (the reference-shaped call
        # makes it contiguous first, below)
        fc = [int(d) for d in ds]
        plan = m.make_plan([(fc, info['points_split'].reshape(-1).long().numpy())], S)
        strided = torch.cat([u8, u8], dim=2)[:, :, :S]
        assert tuple(strided.shape) == tuple(u8.shape) and not strided.is_contiguous()
        with pytest.raises(ValueError, match='crops must be a contiguous'):
            m.forward_batch(plan, strided, info['points'].reshape(-1, 3).contiguous())
        with pytest.raises(ValueError, match='crops must be a contiguous'):
            m.forward_batch(plan, u8.permute(0, 3, 1, 2).contiguous(), info['points'].reshape(-1, 3).contiguous())
    assert log.calls == [], 'operators were called before the crops were refused: %r' % log.calls
    with torch.no_grad():
        want = scores(m(u8, info, ds))
        assert log.calls, 'the call log records nothing'
        assert_same_scores(scores(m(strided, info, ds)), want, 'strided uint8 crops, reference-shaped call')


def test_training_forward_refuses_uint8_crops_first():
    m, c, dets, info, ds = _model()
    u8 = u8_crops(dets)
    eng = m.engine()
    log = CallLog(eng.ops)
    eng.ops = log
    m.train()
    with pytest.raises(ValueError, match='uint8'):
        m(u8, info, ds)
    assert log.calls == [] and len(m._train_plans) == 0, 'work was queued before the check'
    m.eval()


@pytest.mark.parametrize('trunk,fuse', [('f32', True), ('f16x3', True), ('f16x3', False), ('f16q8', True)])
def test_uint8_crops_on_every_entry_point(trunk, fuse):
    """the emulation's schedule: uint8 crops == their host normalisation on the reference-shaped call, the batched entry
    (B = 2, unequal counts) and the image-only rows"""
    m, c, dets, info, ds = _model('s6_endmax_A')
    m.set_trunk(trunk)
    eng = m.engine()
    eng.fuse_conv1 = fuse
    eng.q8_min_crop = 0
    S = c['S']
    u8 = u8_crops(dets)
    x = normalise_u8(u8)
    with torch.no_grad():
        assert_same_scores(scores(m(u8, info, ds)), scores(m(x, info, ds)), 'reference-shaped call')
        assert_same_scores(scores(m.forward_rows(u8, info, ds, rows=(0,))), scores(m.forward_rows(x, info, ds, rows=(0,))),
                           'image-only rows')
        from mmmot_amd.synth import make_pair
        d2, i2, s2 = make_pair(2, 3, S, 6, seed=4321, ragged=True)
        fc = [[int(d) for d in ds], [int(d) for d in s2]]
        ps = [info['points_split'].reshape(-1).long().numpy(), i2['points_split'].reshape(-1).long().numpy()]
        plan = m.make_plan(list(zip(fc, ps)), S)
        pts = torch.cat([info['points'].reshape(-1, 3), i2['points'].reshape(-1, 3)]).contiguous()
        u8b = torch.cat([u8, u8_crops(d2)])
        a = m.forward_batch(plan, u8b, pts)
        b = m.forward_batch(plan, normalise_u8(u8b), pts)
        for k in range(2):
            assert_same_scores(scores(a[k]), scores(b[k]), 'batched entry, sample %d' % k)
