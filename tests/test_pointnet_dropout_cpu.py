"""Dropout of the LiDAR encoder, host side: the NumPy restatement of the device mask
(tests/dropout_ref.py) against Random123's known answers and its own statistics, the oracle's PointNet with a dropout
factor against fixtures made by running the IMPORTED reference's PointNet_v1(use_dropout=True)
(tools/gen_golden_pointnet_dropout.py), ``pointnet_autograd`` on the float64 emulation of the C-ABI against that
restatement, and what the ``use_dropout`` flag does to the module.  tests/test_pointnet_dropout_gpu.py runs the kernels."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dropout_ref as D
from common import GOLD, case_kwargs, get_case
from fake_ops import TorchOps
from mmmot_amd import PointNet_v1, TrackingNet, build_model
from mmmot_amd.synth import make_pair
from mmmot_amd.train import dropout_constants, pointnet_autograd
from mmmot_amd.weights import init_module
from oracle import restatement as R

FIXTURES = ('xyz', 'refl')


class DropOps(TorchOps):
    """TorchOps plus the three dropout operators of csrc/dropout.hip in executable-specification form, the mask from
    the NumPy restatement"""

    @staticmethod
    def _keep(seed, threshold, R_, C, like):
        return torch.from_numpy(D.mask(seed, threshold, R_, C)).to(like.dtype)

    def segment_mean_dropout(self, X, C, segs, out, sc, sh, seed, threshold, scale, use_group=True):
        keep = self._keep(seed, threshold, X.shape[0], C, X)
        for s in range(segs.n):
            st, cnt = int(segs.h_start[s]), int(segs.h_count[s])
            g = int(segs.h_group[s]) if use_group else 0
            rows = torch.relu(X[st:st + cnt, :C] * sc[g, :C] + sh[g, :C]) * keep[st:st + cnt] * scale
            out[s, :C] = rows.mean(0)

    def rows_gather_scale_dropout(self, S, rowidx, scale, X, C, seed, threshold, dscale):
        self.rows_gather_scale(S, rowidx, scale, X, C)
        X[:, :C] = X[:, :C] * self._keep(seed, threshold, X.shape[0], C, X) * dscale

    def dropout_mask(self, seed, threshold, out):
        out.copy_(torch.from_numpy(D.mask(seed, threshold, out.shape[0], out.shape[1]).astype(np.uint8)))


# ---- the generator ----------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]


@pytest.mark.parametrize('counter,key,want', KAT)
def test_philox_known_answers(counter, key, want):
    got = D.philox4x32_10(counter, key)
    assert ' '.join('%08x' % int(w) for w in got) == want


def test_mask_is_a_function_of_seed_row_and_channel():
    """element (r, c) = word c & 3 of the call with counter (r, c >> 2, 0, 0) and the seed's halves as the key"""
    seed = 0x0123456789ABCDEF
    w = D.words(seed, 9, 16)
    for r, c in ((0, 0), (7, 13), (8, 6)):
        one = D.philox4x32_10((r, c >> 2, 0, 0), (seed & 0xffffffff, seed >> 32))
        assert int(w[r, c]) == int(one[c & 3])
    assert (D.words(seed, 4, 16, row0=5) == w[5:9]).all()  # no dependence on how the rows are cut
    assert (D.words(seed, 9, 8) == w[:, :8]).all()


def test_mask_statistics():
    m = D.mask(20191027, 0x80000000, 300, 512)
    print('keep fraction %.5f, channels %.3f-%.3f, rows %.3f-%.3f' % (m.mean(), m.mean(0).min(), m.mean(0).max(),
                                                                      m.mean(1).min(), m.mean(1).max()))
    assert abs(m.mean() - 0.5) <= 0.0051          # 4 sigma of 153 600 fair draws
    assert np.abs(m.mean(0) - 0.5).max() <= 0.115  # 300 per channel
    assert np.abs(m.mean(1) - 0.5).max() <= 0.088  # 512 per row
    agree = (D.mask(1, 0x80000000, 300, 512) == D.mask(2, 0x80000000, 300, 512)).mean()
    assert abs(agree - 0.5) <= 0.0051, agree
    assert D.mask(20191027, 0, 300, 512).all()
    assert D.mask(20191027, 0xFFFFFFFF, 300, 512).mean() < 1e-4
    assert D.threshold_of(0.5) == 0x80000000 and D.threshold_of(0.0) == 0 and D.threshold_of(1.0) == 0xFFFFFFFF
    assert dropout_constants(0.5) == (0x80000000, 2.0) and dropout_constants(0.0) == (0, 1.0)
    assert dropout_constants(0.75) == (0xC0000000, 4.0)
    for p in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            dropout_constants(p)


# ---- the oracle's PointNet with a dropout factor -------------------------------------------------------------------
def pointnet_with_drop(points, split, sd, drop=None):
    """oracle.restatement.pointnet, restated, with ``drop`` [1][512][P] (mask * 1 / (1 - p)) between the bn1 ReLU and the
    last per-detection average (reference modules/point_net.py:28-39)"""
    _gn = R._gn
    q = 'point_net.feat.'
    t1 = R.stn_transform(sd, q + 'stn1.', points.shape[1])
    x = torch.bmm(points.transpose(2, 1), t1).transpose(2, 1)
    x = F.relu(_gn(F.conv1d(x, sd[q + 'conv1.weight'], sd[q + 'conv1.bias']), sd, q + 'bn1', 64))
    t2 = R.stn_transform(sd, q + 'stn2.', 64)
    x = torch.bmm(x.transpose(2, 1), t2).transpose(2, 1)
    skip = x
    for i, g in ((2, 64), (3, 64), (4, 128), (5, 1024)):
        x = F.relu(_gn(F.conv1d(x, sd[q + 'conv%d.weight' % i], sd[q + 'conv%d.bias' % i]), sd, q + 'bn%d' % i, g))
    avg = R._segment_avg(x, split)
    counts = (split[1:] - split[:-1]).long()
    rep = torch.repeat_interleave(avg, counts, dim=-1)
    x = torch.cat([skip, rep], dim=1)
    x = F.relu(_gn(F.conv1d(x, sd['point_net.conv1.weight'], sd['point_net.conv1.bias']), sd, 'point_net.bn1', 512))
    if drop is not None:
        x = x * drop
    x = R._segment_avg(x, split)
    x = F.relu(_gn(F.conv1d(x, sd['point_net.conv2.weight'], sd['point_net.conv2.bias']), sd, 'point_net.bn2', 16))
    return x[0].t(), [t1, t2]


_cache = {}


def fixture(name):
    """(npz, case, points [1][P][kin] float64, split, float64 leaves keyed like the oracle's state dict, drop factor,
    (restated out, {key: gradient})) of one reference fixture; computed once"""
    if name not in _cache:
        g = np.load(os.path.join(GOLD, 'pointnet_dropout_%s.npz' % name))
        c = dict(ast.literal_eval(str(g['case'])))
        _, info, _ = make_pair(c['N'], c['M'], c['S'], c['pts'], c['seed'], c['ragged'], reflectivity=bool(c['refl']))
        split = info['points_split'].reshape(-1).long()
        pn = PointNet_v1(3 + c['refl'], use_dropout=True)
        init_module(pn, 0)
        train = {k for k, p in pn.named_parameters() if p.requires_grad}
        sd = {'point_net.' + k: (v.detach().double().clone().requires_grad_(k in train) if v.dtype.is_floating_point
                                 else v.clone()) for k, v in pn.state_dict().items()}
        keep = D.mask(int(g['mask_seed']), 0x80000000, int(split[-1]), 512)
        drop = torch.from_numpy(keep.T.astype(np.float64) * 2.0).unsqueeze(0)
        pts = info['points'].double()
        out, trans = pointnet_with_drop(pts.transpose(-1, -2), split, sd, drop)
        loss_weights(out, trans).backward()
        grads = {k: v.grad for k, v in sd.items() if v.dtype.is_floating_point and v.grad is not None}
        _cache[name] = (g, c, pts, split, sd, drop, (out.detach(), grads))
    return _cache[name]


def loss_weights(out, trans):
    """the fixed loss of tests/test_train_gpu.py::test_pointnet_backward_on_the_device"""
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(out)
    wt = torch.randn(64, 64, generator=torch.Generator().manual_seed(4)).to(out)
    return (out * w).sum() + (trans[1][0] * wt).sum()


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_without_a_factor_is_the_oracle(name):
    g, c, pts, split, sd, drop, _ = fixture(name)
    with torch.no_grad():
        a, ta = pointnet_with_drop(pts.transpose(-1, -2), split, sd, None)
        b, tb = R.pointnet(pts.transpose(-1, -2), split, sd)
    assert a.dtype == torch.float64 and torch.equal(a, b) and torch.equal(ta[0], tb[0]) and torch.equal(ta[1], tb[1])


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_with_the_mask_matches_the_reference_fixture(name):
    """the IMPORTED reference, its nn.Dropout replaced by the same factor: where the factor acts and everything the
    gradient passes through, to 1e-12 (float64 on both sides)"""
    g, c, pts, split, sd, drop, (out, grads) = fixture(name)
    assert 1 in g['counts'] and abs(float(g['keep_fraction']) - 0.5) < 0.02
    assert np.abs(out.numpy() - g['out']).max() < 1e-12
    keys = [str(k) for k in g['grad_keys']]
    seen = 0
    for k, (s1, s2, amax) in zip(keys, g['grad_norms']):
        if k not in grads:  # the STN trunks behind the one-value-per-group GroupNorm: rounding residue in the reference
            assert amax < 1e-12, (k, amax)
            continue
        seen += 1
        got = grads[k].numpy()
        tol = 1e-12 * max(1.0, amax)
        assert abs(got.sum() - s1) < tol * got.size and abs(np.abs(got).max() - amax) < tol, k
        assert abs((got ** 2).sum() - s2) < 1e-12 * max(1.0, s2), k
        if 'g:' + k in g.files:
            assert np.abs(got - g['g:' + k]).max() < tol, k
    assert seen >= 28 and set(grads) <= set(keys)
    # the factor matters: without it the output is another one
    with torch.no_grad():
        plain, _ = R.pointnet(pts.transpose(-1, -2), split, sd)
    assert (plain - out).abs().max().item() > 1e-3


# ---- pointnet_autograd on the float64 emulation --------------------------------------------------------------------
def dropout_model(c, ops, use_dropout=True, **kw):
    cs, base = get_case('s2_C_multiply_none')
    m = TrackingNet(**dict(case_kwargs(cs, base), without_reflectivity=not c['refl'], use_dropout=use_dropout, **kw))
    init_module(m, 0)
    m.set_ops(ops)
    return m


@pytest.mark.parametrize('name', FIXTURES)
def test_pointnet_autograd_on_the_float64_emulation_matches_the_restatement(name):
    g, c, pts, split, sd, drop, (ref_out, ref_grads) = fixture(name)
    m = dropout_model(c, DropOps(torch.float64))
    m.point_net.load_state_dict({k[len('point_net.'):]: v.detach() for k, v in sd.items()})  # the fixture's weights
    m = m.double()
    m.train()
    plan = m.make_plan([([c['N'], c['M']], split.numpy())], c['S'])
    out, trans = pointnet_autograd(m, plan, pts[0].contiguous(), dropout_seed=int(g['mask_seed']))
    assert out.dtype == torch.float64
    loss_weights(out, trans).backward()
    assert (out.detach() - ref_out).abs().max().item() < 1e-9 * ref_out.abs().max().item()
    seen = 0
    for k, p in m.named_parameters():
        if k not in ref_grads:
            assert p.grad is None, k
            continue
        seen += 1
        ref = ref_grads[k]
        err = (p.grad - ref).abs().max().item()
        assert err < 1e-9 * max(ref.abs().max().item(), 1e-300) or err < 1e-9 * 1e-3, (k, err, ref.abs().max().item())
    assert seen >= 28
    # eval mode: no dropout - the plain oracle
    m.eval()
    with torch.no_grad():
        out_eval, _ = pointnet_autograd(m, plan, pts[0].contiguous(), dropout_seed=1)
        plain, _ = R.pointnet(pts.transpose(-1, -2), split, sd)
    assert (out_eval - plain).abs().max().item() < 1e-9 * plain.abs().max().item()


# ---- the module ------------------------------------------------------------------------------------------------------
RRC = dict(use_dropout=True, dropblock=5, affinity_op='minus_abs', softmax_mode='dual_add', score_fusion_arch='C')


def test_module_keeps_the_reference_dropout():
    on, off = PointNet_v1(3, use_dropout=True), PointNet_v1(3, use_dropout=False)
    assert isinstance(on.dropout, nn.Dropout) and on.dropout.p == 0.5 and off.dropout is None
    assert list(on.state_dict()) == list(off.state_dict())
    common = dict(model=dict(point_arch='v1', point_len=512, appear_arch='vgg', appear_len=512, appear_skippool=True,
                             appear_fpn=False, end_arch='v2', end_mode='avg', affinity_op=RRC['affinity_op'],
                             softmax_mode=RRC['softmax_mode'], score_arch='branch_cls', neg_threshold=0,
                             score_fusion_arch=RRC['score_fusion_arch'], test_mode=2),
                  sample_max_len=2, without_reflectivity=True, use_dropout=RRC['use_dropout'], dropblock=RRC['dropblock'])
    m = build_model(dict(common=common))
    assert isinstance(m.point_net.dropout, nn.Dropout) and m.point_net.dropout.p == 0.5
    _, c, pts, split, *_ = fixture('xyz')
    m = dropout_model(c, DropOps())
    m.point_net.dropout.p = 1.0  # no finite scale: refused, not guessed at
    m.train()
    plan = m.make_plan([([c['N'], c['M']], split.numpy())], c['S'])
    with pytest.raises(ValueError):
        pointnet_autograd(m, plan, pts[0].float().contiguous())


def _train_forward(m, c, seed):
    dets, info, ds = make_pair(c['N'], c['M'], 32, c['pts'], c['seed'], c['ragged'], reflectivity=bool(c['refl']))
    m.freeze_appearance = True
    m.train()
    torch.manual_seed(seed)
    before = torch.get_rng_state()
    out = m(dets, info, ds)
    return out, before, torch.get_rng_state()


def test_no_draw_from_the_global_generator_without_dropout():
    """use_dropout=False consumes exactly the generator state it consumed before dropout existed (here: none - frozen
    image branch, no DropBlock); pinned against a model whose ``dropout`` is None by assignment.  use_dropout=True
    makes one draw per training forward and the same torch.manual_seed gives the same scores."""
    _, c, *_ = fixture('xyz')
    flag = dropout_model(c, DropOps())
    off = dropout_model(c, DropOps(), use_dropout=False)
    none = dropout_model(c, DropOps())
    none.point_net.dropout = None
    o_off, b0, a0 = _train_forward(off, c, 5)
    o_none, b1, a1 = _train_forward(none, c, 5)
    assert torch.equal(b0, a0) and torch.equal(b1, a1) and torch.equal(b0, b1)
    assert torch.equal(o_off[0], o_none[0]) and torch.equal(o_off[1][0], o_none[1][0])
    o_on, b2, a2 = _train_forward(flag, c, 5)
    assert torch.equal(b2, b0) and not torch.equal(a2, b2)
    torch.manual_seed(5)
    torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)
    assert torch.equal(torch.get_rng_state(), a2)  # exactly one 63-bit draw
    o_on2, _, _ = _train_forward(flag, c, 5)
    o_on3, _, _ = _train_forward(flag, c, 6)
    assert torch.equal(o_on[0], o_on2[0]) and not torch.equal(o_on[0], o_on3[0]) and not torch.equal(o_on[0], o_off[0])
    # eval mode: the flag changes nothing (fresh models: the training forwards above moved w_det's running statistics)
    flag, off = dropout_model(c, DropOps()).eval(), dropout_model(c, DropOps(), use_dropout=False).eval()
    dets, info, ds = make_pair(c['N'], c['M'], 32, c['pts'], c['seed'], c['ragged'])
    with torch.no_grad():
        a, b = flag(dets, info, ds), off(dets, info, ds)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
