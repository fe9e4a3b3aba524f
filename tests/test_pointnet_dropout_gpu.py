"""Dropout of the LiDAR encoder on the device (csrc/dropout.hip): the three entry points against
the NumPy restatement of the mask (tests/dropout_ref.py) and against the kernels they extend, ``pointnet_autograd`` with
dropout against the float64 oracle with the same mask, and the training-mode forward end to end."""
import numpy as np
import pytest
import torch

import dropout_ref as D
from common import case_inputs, case_kwargs, get_case
from mmmot_amd import TrackingNet
from mmmot_amd.plan import Segments
from mmmot_amd.synth import make_pair
from mmmot_amd.train import pointnet_autograd
from mmmot_amd.weights import init_module
from oracle import restatement as R
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)
from test_pointnet_dropout_cpu import loss_weights, pointnet_with_drop
from test_train_cpu import oracle_sd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HALF = 0x80000000
SEEDS = (0x0123456789ABCDEF, 0)

_masks = {}


def ref_mask(seed, threshold, R_, C):
    """the NumPy mask as a bool tensor; computed once per argument set"""
    key = (seed, threshold, R_, C)
    if key not in _masks:
        _masks[key] = torch.from_numpy(D.mask(seed, threshold, R_, C))
    return _masks[key]


def einval(fn, *a, **kw):
    with pytest.raises(RuntimeError, match='MMMOT_EINVAL'):
        fn(*a, **kw)


@pytest.mark.parametrize('R_,C', [(1, 4), (300, 512), (257, 64)])
def test_dropout_mask_matches_the_restatement_bit_for_bit(hip, R_, C):
    for seed in SEEDS:
        for thr in (0, HALF, 0xC0000000, 0xFFFFFFFF):
            out = torch.full((R_, C), 7, dtype=torch.uint8, device=DEV)
            hip.dropout_mask(seed, thr, out)
            assert torch.equal(out.cpu(), ref_mask(seed, thr, R_, C).to(torch.uint8)), (hex(seed), hex(thr))


@pytest.mark.parametrize('R_,C', [(300, 512), (16500, 512), (300, 4)])
def test_rows_gather_scale_dropout_is_the_plain_kernel_times_the_mask(hip, R_, C):
    """R = 16 500 at C = 512: 2.1 M lane items, past the 8 192-block grid cap - the grid-stride loop runs"""
    seed = SEEDS[0]
    S = rnd(37, C, seed=1).cuda()
    idx = torch.randint(0, 37, (R_,), generator=torch.Generator().manual_seed(2)).int().cuda()
    scale = (rnd(37, seed=3).abs() + 0.1).cuda()
    plain = torch.empty(R_, C, device=DEV)
    hip.rows_gather_scale(S, idx, scale, plain, C)
    want = plain.cpu() * ref_mask(seed, HALF, R_, C).float() * 2.0
    runs = []
    for _ in range(2):
        buf = torch.full((R_ + 2, C + 8), float('nan'), device=DEV)
        hip.rows_gather_scale_dropout(S, idx, scale, buf[1:R_ + 1, 4:4 + C], C, seed, HALF, 2.0)
        got = buf.cpu()
        assert torch.isnan(got[0]).all() and torch.isnan(got[-1]).all()
        assert torch.isnan(got[:, :4]).all() and torch.isnan(got[:, 4 + C:]).all()
        runs.append(got[1:R_ + 1, 4:4 + C].clone())
    assert torch.equal(runs[0], want), int((runs[0] != want).sum())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    frac = (runs[0] == 0).float().mean().item()
    assert abs(frac - 0.5) < 0.1


COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 257, 1000]


POOL_COUNTS = [1, 3, 4, 5, 13, 16, 17, 65]  # around the 4-wave split and the 16-row stride (tests/test_segpool_gpu.py)


def ragged(C, dev, counts=COUNTS):
    """segments of `counts` rows, alternating between two groups with their own sc / sh"""
    cnt = np.asarray(counts)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    grp = np.arange(len(cnt)) % 2
    X = rnd(int(cnt.sum()), C, seed=11)
    sc, sh = rnd(2, C, seed=12) * 0.5 + 1.0, rnd(2, C, seed=13) * 0.3
    return X, sc, sh, Segments(start, cnt, np.ones(len(cnt)), grp, dev), grp


@pytest.mark.parametrize('C,counts', [pytest.param(512, COUNTS, id='512'), pytest.param(8, COUNTS, id='8'),
                                      pytest.param(4, POOL_COUNTS, id='4-short'), pytest.param(260, POOL_COUNTS, id='260-short')])
def test_segment_mean_dropout_keeping_everything_is_segment_mean(hip, C, counts):
    X, sc, sh, sg, _ = ragged(C, DEV, counts)
    Xg, scg, shg = X.cuda(), sc.cuda(), sh.cuda()
    want = torch.empty(sg.n, C, device=DEV)
    hip.segment_mean(Xg, C, sg, want, sc=scg, sh=shg, relu=True)
    got = torch.full((sg.n, C), float('nan'), device=DEV)
    hip.segment_mean_dropout(Xg, C, sg, got, scg, shg, SEEDS[0], 0, 1.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('C', [512, 8])
def test_segment_mean_dropout_masked(hip, C):
    """threshold 0x80000000, scale 2 against a float64 evaluation with the NumPy mask.  The bound is measured: the same
    sums in torch fp32 on the host are the yardstick, the device may be 4 x as far from float64 (relative to the
    largest output) - the optimizer tests' convention."""
    seed = SEEDS[0]
    X, sc, sh, sg, grp = ragged(C, DEV)
    keep = ref_mask(seed, HALF, X.shape[0], C)

    def evaluate(dtype):
        out = torch.empty(sg.n, C, dtype=dtype)
        k, x = keep.to(dtype), X.to(dtype)
        for s in range(sg.n):
            st, n, g = int(sg.h_start[s]), int(sg.h_count[s]), int(grp[s])
            rows = torch.relu(x[st:st + n] * sc[g].to(dtype) + sh[g].to(dtype)) * k[st:st + n] * 2.0
            out[s] = rows.sum(0) / n
        return out
    ref, host32 = evaluate(torch.float64), evaluate(torch.float32)
    runs = []
    for _ in range(2):
        buf = torch.full((sg.n + 2, C + 8), float('nan'), device=DEV)
        hip.segment_mean_dropout(X.cuda(), C, sg, buf[1:sg.n + 1, 4:4 + C], sc.cuda(), sh.cuda(), seed, HALF, 2.0)
        got = buf.cpu()
        assert torch.isnan(got[0]).all() and torch.isnan(got[-1]).all()
        assert torch.isnan(got[:, :4]).all() and torch.isnan(got[:, 4 + C:]).all()
        runs.append(got[1:sg.n + 1, 4:4 + C].clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    top = ref.abs().max().item()
    dev_err = (runs[0].double() - ref).abs().max().item() / top
    host_err = (host32.double() - ref).abs().max().item() / top
    print('segment_mean_dropout C=%d: device error %.3e, host fp32 error %.3e (relative to the largest output)' % (
        C, dev_err, host_err))
    assert torch.isfinite(runs[0]).all() and dev_err <= 4.0 * host_err
    # a single-row segment: exactly the mask times 2 times the normalised row
    one = torch.relu(torch.addcmul(sh[0], X[0], sc[0]))
    assert ((runs[0][0] == 0) | keep[0]).all() and (runs[0][0][~keep[0]] == 0).all()
    close(runs[0][0], one * keep[0].float() * 2.0, 1e-6, 'single-row segment')


def test_launchers_reject_bad_arguments(hip):
    C = 8
    X, sc, sh, sg, _ = ragged(C, DEV)
    Xg, scg, shg = X.cuda(), sc.cuda(), sh.cuda()
    out = torch.zeros(sg.n, C, device=DEV)
    wide = torch.zeros(X.shape[0], C + 2, device=DEV)
    einval(hip.segment_mean_dropout, Xg, 6, sg, out, scg, shg, 1, HALF, 2.0)                 # C % 4
    einval(hip.segment_mean_dropout, wide[:, :C], C, sg, out, scg, shg, 1, HALF, 2.0)        # ldx % 4
    einval(hip.segment_mean_dropout, Xg, C, sg, torch.zeros(sg.n, C + 4, device=DEV)[:, 1:C + 1], scg, shg, 1, HALF, 2.0)
    einval(hip.segment_mean_dropout, Xg, C, sg, out, None, None, 1, HALF, 2.0)               # no normalisation table
    S = torch.ones(3, C, device=DEV)
    idx = torch.zeros(5, dtype=torch.int32, device=DEV)
    Xo = torch.zeros(5, C, device=DEV)
    einval(hip.rows_gather_scale_dropout, S, idx, None, Xo, 6, 1, HALF, 2.0)
    einval(hip.rows_gather_scale_dropout, S, idx, None, torch.zeros(5, C + 4, device=DEV)[:, 1:C + 1], C, 1, HALF, 2.0)
    einval(hip.rows_gather_scale_dropout, torch.ones(3, C + 2, device=DEV)[:, :C], idx, None, Xo, C, 1, HALF, 2.0)
    einval(hip.dropout_mask, 1, HALF, torch.zeros(5, 6, dtype=torch.uint8, device=DEV))
    m = torch.zeros(4, 16, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert hip.lib.mmmot_dropout_mask(1, HALF, 2 ** 32, 16, m.data_ptr(), stream) == -1       # a row index needs 32 bits
    assert hip.lib.mmmot_dropout_mask(1, HALF, 4, 16, None, stream) == -1
    assert hip.lib.mmmot_dropout_mask(1, HALF, 4, 16, m.data_ptr() + 4, stream) == -1         # alignment
    assert hip.lib.mmmot_rows_gather_scale_dropout(S.data_ptr(), C, idx.data_ptr(), None, Xo.data_ptr(), C, 2 ** 32, C, 1,
                                                   HALF, 2.0, stream) == -1
    torch.cuda.synchronize()
    assert (out == 0).all() and (Xo == 0).all() and (m == 0).all()  # nothing was launched


def test_backward_regenerates_the_forward_mask(hip):
    """the zero pattern of rows_gather_scale_dropout over an all-ones S is dropout_mask for the same seed"""
    R_, C = 777, 512
    for seed in SEEDS:
        S = torch.ones(1, C, device=DEV)
        idx = torch.zeros(R_, dtype=torch.int32, device=DEV)
        X = torch.full((R_, C), float('nan'), device=DEV)
        hip.rows_gather_scale_dropout(S, idx, None, X, C, seed, HALF, 2.0)
        m = torch.zeros(R_, C, dtype=torch.uint8, device=DEV)
        hip.dropout_mask(seed, HALF, m)
        assert torch.equal(X, m.float() * 2.0)


def dropout_net(c, base, use_dropout=True, device=DEV, **kw):
    m = TrackingNet(**dict(case_kwargs(c, base), use_dropout=use_dropout, **kw))
    init_module(m, 0)
    return m.to(device)


def test_pointnet_autograd_with_dropout_on_the_device():
    """the mask is an exact factor of 0 or 2: the bounds of test_train_gpu.py::test_pointnet_backward_on_the_device"""
    c, base = get_case('s2_C_multiply_none')
    m = dropout_net(c, base)
    m.train()
    dets, info, ds = case_inputs(c)
    ps = info['points_split'].reshape(-1).long()
    points = info['points'].reshape(-1, 3).contiguous().to(DEV)
    plan = m.make_plan([([int(x) for x in ds], ps.numpy())], c['S'])
    seed = 0xFEDCBA9876543210
    out, trans = pointnet_autograd(m, plan, points, dropout_seed=seed)
    assert m.engine().ops.name == 'hip'
    loss_weights(out, trans).backward()
    sd = oracle_sd(m)
    sd = {k: (v.detach().cpu().double().requires_grad_(v.requires_grad) if v.dtype.is_floating_point else v.cpu())
          for k, v in sd.items()}
    drop = ref_mask(seed, HALF, int(ps[-1]), 512).t().double().unsqueeze(0) * 2.0
    ref_out, ref_trans = pointnet_with_drop(info['points'].double().transpose(-1, -2), ps, sd, drop)
    loss_weights(ref_out, ref_trans).backward()
    err = (out.detach().cpu().double() - ref_out.detach()).abs().max().item()
    with torch.no_grad():
        plain, _ = R.pointnet(info['points'].double().transpose(-1, -2), ps, sd)
    assert (plain - ref_out).abs().max().item() > 1e-2  # dropout is on
    assert err < 2e-4, err
    gmax = max(v.grad.abs().max().item() for k, v in sd.items() if k.startswith('point_net.') and v.grad is not None)
    worst, seen = 0.0, 0
    for k, p in m.named_parameters():
        ref = sd[k].grad if k.startswith('point_net.') else None
        if ref is None:
            assert p.grad is None, k
            continue
        seen += 1
        e = (p.grad.cpu().double() - ref).abs().max().item()
        assert e < 3e-4 * ref.abs().max().item() + 3e-6 * (1.0 + gmax), (k, e, ref.abs().max().item())
        if ref.abs().max().item() > 1e-6 * gmax:  # not the tensors whose reference gradient is rounding residue
            worst = max(worst, e / ref.abs().max().item())
    assert seen >= 28
    print('pointnet backward with dropout: output error %.1e, worst relative gradient error %.1e over %d tensors' % (
        err, worst, seen))


def train_forward(m, inputs, seed):
    dets, info, ds = inputs
    m.train()
    m.zero_grad()
    torch.manual_seed(seed)
    det, links, new, end, trans = m(dets.to(DEV), {k: v.to(DEV) for k, v in info.items()}, ds)
    (det.sum() + (links[0] ** 2).sum() + new.sum() - end.sum()).backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    return det.detach().clone(), links[0].detach().clone(), grads


def test_forward_train_with_dropout_end_to_end():
    c, base = get_case('s2_C_multiply_none')
    inputs = make_pair(3, 2, 32, 30, 77, ragged=True)
    m = dropout_net(c, base)
    m.freeze_appearance = True
    a = train_forward(m, inputs, 123)
    b = train_forward(m, inputs, 123)
    d = train_forward(m, inputs, 124)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2]) and any(k.startswith('point_net.') for k in a[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert not torch.equal(a[0], d[0])
    # eval mode: the flag changes nothing
    on, off = dropout_net(c, base).eval(), dropout_net(c, base, use_dropout=False).eval()
    dets, info, ds = inputs
    with torch.no_grad():
        so = on(dets.to(DEV), {k: v.to(DEV) for k, v in info.items()}, ds)
        sf = off(dets.to(DEV), {k: v.to(DEV) for k, v in info.items()}, ds)
    assert torch.equal(so[0], sf[0]) and torch.equal(so[1][0], sf[1][0]) and torch.equal(so[2], sf[2]) and \
        torch.equal(so[3], sf[3])


def test_dropblock_keeps_its_draws_with_dropout(monkeypatch):
    """dropblock = 5 and dropout together (the reference's rrc config): the seed of the dropout mask is drawn AFTER the
    image branch, so the stage-2 and stage-3 DropBlock masks - and with them the image features - are those of the same
    model without dropout under the same torch.manual_seed"""
    import mmmot_amd.train as T
    c, base = get_case('s2_C_multiply_none')
    inputs = make_pair(3, 2, 64, 30, 78, ragged=True)
    seed, gamma = 47, 0.1 / 25
    torch.manual_seed(seed)  # at this seed DropBlock drops a block in both stages (5 crops: 4 x 4 and 2 x 2 maps)
    assert (torch.rand(5, 4, 4) < gamma).any() and (torch.rand(5, 2, 2) < gamma).any()
    seen = []
    orig = T.appearance_autograd

    def spy(model, plan, dets):
        img = orig(model, plan, dets)
        seen.append(img.detach().clone())
        return img
    monkeypatch.setattr(T, 'appearance_autograd', spy)
    dets = {}
    for name, kw in (('both', dict(use_dropout=True, dropblock=5)), ('dropblock', dict(use_dropout=False, dropblock=5)),
                     ('dropout', dict(use_dropout=True, dropblock=0))):
        dets[name] = train_forward(dropout_net(c, base, **kw), inputs, seed)[0]
    img_both, img_block, img_drop = seen
    assert torch.equal(img_both, img_block)
    assert not torch.equal(img_both, img_drop)       # DropBlock did drop something
    assert not torch.equal(dets['both'], dets['dropblock'])  # and so did dropout
