"""Host logic of the training backward of the pairwise block (mmmot_amd/backward.py) on the torch emulation of the
C-ABI: the launch schedule, the tape, the table building and the gradient algebra must reproduce torch.autograd
through the ORACLE's affinity / new_end / softmax (the CPU restatement of reference modules/gcn.py:68-82,
new_end.py:62-82, tracking_net.py:106-126).  The GPU suite (tests/test_backward_gpu.py) runs the same comparison
through the HIP kernels."""
import pytest
import torch

from common import build_model, get_case
from fake_ops import TorchOps
from mmmot_amd.backward import affinity_autograd, affinity_backward, affinity_forward_train
from mmmot_amd.synth import make_pair
from oracle import restatement as R


def oracle_block(sd, F3, counts, op, sm):
    """link / new / end of the oracle for a list of frame counts, from F3 [nR, 512, L] (reference layout)"""
    links, news, ends = [], [], []
    start = 0
    for i in range(len(counts) - 1):
        mid, stop = start + counts[i], start + counts[i] + counts[i + 1]
        logit, new, end = R.affinity(F3[:, :, start:mid], F3[:, :, mid:stop], sd, op)
        links.append(R.softmax_mode(logit, sm).squeeze(1))
        news.append(new)
        ends.append(end)
        start = mid
    return links, news, ends


def reference_grads(model, samples, F, op, sm, w_link, w_new, w_end):
    """autograd through the oracle in float64; F [nR, Lt, 512] (ours) <-> [nR, 512, L] per sample (reference)"""
    sd = {k: v.detach().double().clone().requires_grad_(k.startswith('w_link.')) for k, v in model.state_dict().items()}
    Fd = F.detach().double().clone().requires_grad_(True)
    loss = 0.0
    off, lo = 0, 0
    for counts in samples:
        L = sum(counts)
        F3 = Fd[:, off:off + L].permute(0, 2, 1)
        links, news, ends = oracle_block(sd, F3, counts, op, sm)
        d0 = off
        for p, (lk, nw, en) in enumerate(zip(links, news, ends)):
            N, M = counts[p], counts[p + 1]
            n = lk.numel()
            loss = loss + (lk.reshape(-1) * w_link[lo:lo + n].double()).sum()
            lo += n
            loss = loss + (nw * w_new[:, d0 + N:d0 + N + M].double()).sum() + (en * w_end[:, d0:d0 + N].double()).sum()
            d0 += N
        off += L
    loss.backward()
    return Fd.grad, {k: v.grad for k, v in sd.items() if k.startswith('w_link.')}


@pytest.mark.parametrize('op,sm,samples', [
    ('multiply', 'none', [[3, 4]]),
    ('minus_abs', 'dual_add', [[5, 2], [1, 6]]),
    ('minus', 'dual', [[2, 3, 2]]),
    ('multiply', 'dual_max', [[4, 4]]),
    ('minus_abs', 'single', [[1, 1], [3, 5]]),
])
def test_backward_matches_autograd_through_the_oracle(op, sm, samples):
    from mmmot_amd.plan import BatchPlan
    c, base = get_case('s2_C_multiply_none')
    c = dict(c, aff=op, sm=sm)
    if any(len(s) > 2 for s in samples):
        c['counts'] = samples[0]
    m = build_model(c, base, ops=TorchOps())
    m.set_trunk('f32')  # exact-fp32 GEMMs in the emulated forward: the comparison is about the gradient algebra
    eng = m.engine()
    plan = BatchPlan([(s, None) for s in samples], 32, 'cpu', use_points=False)
    g = torch.Generator().manual_seed(3)
    F = torch.randn(3, plan.Lt, 512, generator=g) * 0.7
    R_ = plan.pair_tiles.R
    w_link, w_new, w_end = torch.randn(R_, generator=g), torch.randn(3, plan.Lt, generator=g), torch.randn(3, plan.Lt, generator=g)
    link, new, end, tape = affinity_forward_train(eng, plan, F)
    dF, grads = affinity_backward(eng, plan, F, tape, w_link, w_new, w_end)
    dF_ref, g_ref = reference_grads(m, samples, F, op, sm, w_link, w_new, w_end)
    scale = dF_ref.abs().max().item()
    assert (dF.double() - dF_ref).abs().max().item() < 2e-4 * scale, 'dF'
    assert set(grads) == set(g_ref)
    gmax = max(v.abs().max().item() for v in g_ref.values())
    for k, ref in g_ref.items():
        got = grads[k].double().reshape(ref.shape)
        # relative to the parameter's own largest gradient, plus fp32 rounding noise of the whole backward (the bias of
        # a conv that feeds a per-channel GroupNorm has an exactly zero gradient: only noise is left to compare)
        tol = 2e-4 * ref.abs().max().item() + 2e-6 * (1.0 + gmax)
        assert (got - ref).abs().max().item() < tol, (k, (got - ref).abs().max().item(), ref.abs().max().item())


def test_autograd_function_fills_grads():
    from mmmot_amd.plan import BatchPlan
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    m.set_trunk('f32')
    plan = BatchPlan([([3, 2], None)], 32, 'cpu', use_points=False)
    F = (torch.randn(3, 5, 512, generator=torch.Generator().manual_seed(1)) * 0.7).requires_grad_(True)
    link, new, end = affinity_autograd(m, plan, F)
    (link.sum() + 2 * new.sum() - end.sum()).backward()
    assert F.grad is not None and F.grad.shape == F.shape and torch.isfinite(F.grad).all()
    for k, p in m.named_parameters():
        if k.startswith('w_link.'):
            assert p.grad is not None and p.grad.shape == p.shape, k
        else:
            assert p.grad is None, k


# ---- second slice: fusion module + training-mode w_det + pairwise block = the whole head -------------------------------
def head_reference(model, counts, cat, fusion, op, sm, w):
    """autograd through the oracle's fusion / affinity and a float64 training-mode w_det (BatchNorm1d on batch statistics,
    no sigmoid: reference tracking_net.py:149-151 with self.training)"""
    import torch.nn.functional as Fn
    heads = ('fusion_module.', 'w_det.', 'w_link.')
    sd = {k: v.detach().double().clone().requires_grad_(k.startswith(heads) and v.dtype.is_floating_point and
                                                        'running' not in k and 'num_batches' not in k)
          for k, v in model.state_dict().items()}
    c = cat.detach().double().clone().requires_grad_(True)
    F3 = R.fusion(c.t().unsqueeze(0), sd, fusion)                    # 3 x 512 x L
    x = F3
    for i, bn in ((0, 1), (3, 4)):
        x = Fn.conv1d(x, sd['w_det.%d.weight' % i], sd['w_det.%d.bias' % i])
        x = Fn.relu(Fn.batch_norm(x, None, None, sd['w_det.%d.weight' % bn], sd['w_det.%d.bias' % bn], True, 0.0, 1e-5))
    det = Fn.conv1d(x, sd['w_det.6.weight'], sd['w_det.6.bias']).squeeze(1)
    links, news, ends = oracle_block(sd, F3, counts, op, sm)
    N, M = counts
    loss = (det * w['det'].double()).sum() + (links[0].reshape(-1) * w['link'].double()).sum() + \
        (news[0] * w['new'][:, N:].double()).sum() + (ends[0] * w['end'][:, :N].double()).sum()
    loss.backward()
    return c.grad, {k: v.grad for k, v in sd.items() if v.requires_grad}, det.detach()


@pytest.mark.parametrize('fusion,op,sm', [('A', 'multiply', 'none'), ('B', 'minus_abs', 'dual_add'), ('C', 'multiply', 'none'),
                                          ('C', 'minus_abs', 'dual_add')])
def test_head_backward_matches_autograd(fusion, op, sm):
    from mmmot_amd.backward import head_backward, head_forward_train
    from mmmot_amd.plan import BatchPlan
    c, base = get_case('s2_C_multiply_none')
    c = dict(c, fusion=fusion, aff=op, sm=sm)
    m = build_model(c, base, ops=TorchOps())
    m.set_trunk('f32')
    eng = m.engine()
    counts = [4, 5]
    plan = BatchPlan([(counts, None)], 32, 'cpu', use_points=False)
    g = torch.Generator().manual_seed(5)
    cat = torch.randn(plan.Lt, 1024, generator=g) * 0.8
    w = dict(det=torch.randn(3, plan.Lt, generator=g), link=torch.randn(plan.pair_tiles.R, generator=g),
             new=torch.randn(3, plan.Lt, generator=g), end=torch.randn(3, plan.Lt, generator=g))
    det, link, new, end, tape = head_forward_train(eng, m, plan, cat)
    dcat, grads = head_backward(eng, m, plan, cat, tape, w['det'], w['link'], w['new'], w['end'])
    dcat_ref, g_ref, det_ref = head_reference(m, counts, cat, fusion, op, sm, w)
    assert (det.double() - det_ref).abs().max().item() < 2e-4  # training-mode scores: raw, batch-statistics BatchNorm
    assert (dcat.double() - dcat_ref).abs().max().item() < 3e-4 * dcat_ref.abs().max().item(), 'dcat'
    assert set(grads) == set(g_ref), sorted(set(grads) ^ set(g_ref))
    gmax = max(v.abs().max().item() for v in g_ref.values())
    for k, ref in g_ref.items():
        got = grads[k].double().reshape(ref.shape)
        tol = 3e-4 * ref.abs().max().item() + 3e-6 * (1.0 + gmax)
        assert (got - ref).abs().max().item() < tol, (k, (got - ref).abs().max().item(), ref.abs().max().item())


def test_head_autograd_updates_batchnorm_buffers_like_torch():
    from mmmot_amd.backward import head_autograd
    from mmmot_amd.plan import BatchPlan
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    m.set_trunk('f32')
    plan = BatchPlan([([3, 4], None)], 32, 'cpu', use_points=False)
    cat = (torch.randn(plan.Lt, 1024, generator=torch.Generator().manual_seed(2)) * 0.8).requires_grad_(True)
    rm0, rv0 = m.w_det[1].running_mean.clone(), m.w_det[1].running_var.clone()
    det, link, new, end = head_autograd(m, plan, cat)
    (det.sum() + link.sum() + new.sum() - end.sum()).backward()
    assert cat.grad is not None and torch.isfinite(cat.grad).all()
    for k, p in m.named_parameters():
        assert (p.grad is not None) == (k.split('.')[0] in ('fusion_module', 'w_det', 'w_link')), k
    # running statistics: the momentum update of torch's training-mode BatchNorm1d on the same conv output
    import torch.nn.functional as Fn
    F3 = R.fusion(cat.detach().t().unsqueeze(0), {k: v.detach() for k, v in m.state_dict().items()}, 'C')
    x = Fn.conv1d(F3, m.w_det[0].weight.detach(), m.w_det[0].bias.detach())
    rm, rv = rm0.clone(), rv0.clone()
    Fn.batch_norm(x, rm, rv, None, None, True, 0.1, 1e-5)
    assert torch.allclose(m.w_det[1].running_mean, rm, atol=1e-5) and torch.allclose(m.w_det[1].running_var, rv, atol=1e-5)


def test_refresh_head_repacks_only_the_head():
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    eng = m.engine()
    vgg_before, pn_before = eng.P['vgg'], eng.P['pointnet']
    wa_before = eng.P['w_link']['wa'].clone()
    with torch.no_grad():
        m.w_link.conv1[0].weight.mul_(1.5)
    assert m.refresh_head() is eng and eng.P['vgg'] is vgg_before and eng.P['pointnet'] is pn_before
    wa = eng.P['w_link']['wa']
    assert torch.allclose(wa[512:], wa_before[512:] * 1.5) and torch.equal(wa[:512], wa_before[:512])
    assert 'wa_h16' in eng.P['w_link']  # the fp16-split copies are rebuilt too


def test_two_level_segment_sums_equal_the_direct_sums():
    """long strided sums (the per-tile partials of a full-resolution trunk layer: thousands of rows per segment) are
    summed in two levels - chunks, then chunk sums; short ones keep their single table"""
    import numpy as np
    from mmmot_amd.tape import SEGSUM_CHUNK, chunked_segments, colsum, segsum
    c, base = get_case('s2_C_multiply_none')
    eng = build_model(c, base, ops=TorchOps(torch.float64)).engine()
    g = torch.Generator().manual_seed(5)
    T, C = 5 * SEGSUM_CHUNK + 37, 8
    X = torch.randn(2 * T + 6, C, generator=g, dtype=torch.float64).float()
    segs = chunked_segments(np.array([0, 1, 2 * T]), np.array([T, T, 3]), 2, 'cpu')
    assert len(segs.levels) == 2 and segs.levels[0].n == 2 * 6 + 1 and segs.levels[1].n == 3
    out = torch.zeros(3, C)
    segsum(eng, X, C, segs, out)
    want = torch.stack([X[0:2 * T:2].double().sum(0), X[1:2 * T:2].double().sum(0), X[2 * T:2 * T + 6:2].double().sum(0)])
    assert (out.double() - want).abs().max().item() < 1e-4
    short = chunked_segments(np.array([0, 1]), np.array([40, 40]), 2, 'cpu')
    assert len(short.levels) == 1
    tall = torch.randn(9000, C, generator=g)
    assert (colsum(eng, tall).double() - tall.double().sum(0)).abs().max().item() < 1e-3
    # 9000 x 8 is viewed as 1125 rows of 64 (three halvings, 1125 is odd), summed as 9 chunks of 128 rows, then the 9 chunk
    # sums, then the eight row classes are folded
    assert [lv.n for lv in eng._colsum_segs[(1125, 'cpu')].levels] == [9, 1]
    assert (9000, 'cpu') not in eng._colsum_segs
    odd = torch.randn(1001, 12, generator=g)                      # odd row count: no folding, 8 chunks, then one segment
    assert (colsum(eng, odd).double() - odd.double().sum(0)).abs().max().item() < 1e-3
    assert [lv.n for lv in eng._colsum_segs[(1001, 'cpu')].levels] == [8, 1]
    wide = torch.randn(4096, 520, generator=g)[:, :512]           # a column slice (not contiguous): summed as it lies
    assert (colsum(eng, wide).double() - wide.double().sum(0)).abs().max().item() < 2e-3
    small = torch.randn(7, 16, generator=g)
    assert (colsum(eng, small).double() - small.double().sum(0)).abs().max().item() < 1e-5


# ---- the head's training forward is the engine's forward, recorded (Engine.recording) ---------------------------------
def tape_tensors(obj):
    """every tensor reachable from a tape: through dicts, lists, tuples and tape.Layer records"""
    from mmmot_amd.tape import Layer
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from tape_tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from tape_tensors(v)
    elif isinstance(obj, Layer):
        yield from tape_tensors(vars(obj))


def check_tape_owns_its_storage(m, device):
    """head_forward_train -> an eval forward of OTHER inputs through the same engine (it overwrites the whole workspace
    arena) -> head_backward: the gradients are those of the backward with no forward in between, bit for bit, and nothing
    on the tape lives in the arena"""
    from mmmot_amd.backward import head_backward, head_forward_train
    c, _ = get_case('s2_C_multiply_none')
    eng = m.engine()
    ins = make_pair(c['N'], c['M'], c['S'], c['pts'], seed=c['seed'] + 1, ragged=True)
    plan = m.make_plan([([c['N'], c['M']], ins[1]['points_split'].reshape(-1).long().numpy())], c['S'])
    g = torch.Generator().manual_seed(8)
    cat = (torch.randn(plan.Lt, 1024, generator=g) * 0.8).to(device)
    w = [torch.randn(3, plan.Lt, generator=g).to(device), torch.randn(plan.pair_tiles.R, generator=g).to(device),
         torch.randn(3, plan.Lt, generator=g).to(device), torch.randn(3, plan.Lt, generator=g).to(device)]
    det, link, new, end, tape = head_forward_train(eng, m, plan, cat)
    dcat0, grads0 = head_backward(eng, m, plan, cat, tape, *w)
    with torch.no_grad():
        m.forward_batch(plan, ins[0].to(device), ins[1]['points'].reshape(-1, 3).contiguous().to(device))
    dcat1, grads1 = head_backward(eng, m, plan, cat, tape, *w)
    assert torch.equal(dcat0, dcat1), 'dcat'
    assert set(grads0) == set(grads1)
    for k in grads0:
        assert torch.equal(grads0[k], grads1[k]), k
    arena = {t.untyped_storage().data_ptr() for t in tape_tensors(list(eng.ws.values()))}
    assert len(arena) > 10  # the eval forward filled it
    on_tape = list(tape_tensors(tape))
    assert len(on_tape) > 50
    for t in on_tape:
        assert t.untyped_storage().data_ptr() not in arena


def test_a_tape_owns_its_storage():
    c, base = get_case('s2_C_multiply_none')
    check_tape_owns_its_storage(build_model(c, base, ops=TorchOps()), 'cpu')


HEAD_CASES = [('A', 'multiply', 'none'), ('B', 'minus_abs', 'dual_add'), ('C', 'multiply', 'none'),
              ('C', 'minus_abs', 'dual_add')]  # those of test_head_backward_matches_autograd


def check_recorded_forward_is_the_eval_forward(m, counts, device):
    """fusion_forward_train / affinity_forward_train against Engine.fuse / Engine.affinity on the same inputs, both on
    the fp32 weights: F, link, new and end bit for bit"""
    from mmmot_amd.backward import fusion_forward_train
    from mmmot_amd.plan import BatchPlan
    eng = m.engine()
    plan = BatchPlan([(counts, None)], 32, device, use_points=False)
    assert plan.pair_uniform32 == (counts[1] % 32 == 0)
    cat = (torch.randn(plan.Lt, 1024, generator=torch.Generator().manual_seed(6)) * 0.8).to(device)
    with eng.fp32_mlp():
        F, _ = fusion_forward_train(eng, plan, cat)
        link, new, end, _ = affinity_forward_train(eng, plan, F)
        F_eval = eng.buf('F', 3, plan.Lt, 512)
        eng.fuse(plan, cat, F_eval)
        link_eval, new_eval, end_eval = eng.affinity(plan, F_eval)
    assert torch.equal(F, F_eval), 'F'
    assert torch.equal(link, link_eval) and torch.equal(new, new_eval) and torch.equal(end, end_eval)


@pytest.mark.parametrize('counts', [[32, 32], [5, 3]])
@pytest.mark.parametrize('fusion,op,sm', HEAD_CASES)
def test_recorded_forward_is_the_eval_forward(fusion, op, sm, counts):
    c, base = get_case('s2_C_multiply_none')
    m = build_model(dict(c, fusion=fusion, aff=op, sm=sm), base, ops=TorchOps())
    check_recorded_forward_is_the_eval_forward(m, counts, 'cpu')


def test_weight_grad_share_rule():
    """weight_grad splits the row reduction into one share per 8 tiles, at most 16; shares=1 is one launch with nsplit 1"""
    import types
    from mmmot_amd.plan import RowTiles
    from mmmot_amd.tape import weight_grad

    class Stub:
        def __init__(self):
            self.calls = []

        def gemm_tn(self, dY, tiles, N, K, dW, db, nsplit=1, **kw):
            self.calls.append(nsplit)
            dW.zero_(), db.zero_()

        def segment_mean(self, X, C, segs, out, **kw):
            out.zero_()

    eng = types.SimpleNamespace(ops=Stub())
    for T, want in ((7, 1), (8, 1), (200, 16)):
        tiles = RowTiles([T * 128], 'cpu')
        assert tiles.T == T
        dY, X = torch.zeros(tiles.R, 64), torch.zeros(tiles.R, 64)
        dW, db = weight_grad(eng, dY, tiles, 64, 64, X=X)
        assert eng.ops.calls == [want] and dW.shape == (64, 64) and db.shape == (64,)
        dW, db = weight_grad(eng, dY, tiles, 64, 64, shares=1, X=X)
        assert eng.ops.calls == [want, 1] and dW.shape == (64, 64) and db.shape == (64,)
        eng.ops.calls.clear()


# ---- the executable specification of the backward kernels (tests/fake_ops.py) against torch.autograd, float64 -----------
# tests/test_backward_kernels_gpu.py compares the HIP kernels with these functions at their edge forms; here the edge
# forms of the specification itself are pinned (float64 against float64: 1e-10 of the tensor's maximum).
def _same64(got, ref, what):
    scale = max(ref.abs().max().item(), 1e-30)
    assert (got.double() - ref.double()).abs().max().item() <= 1e-10 * scale, what


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('C,NG', [(8, 8), (8, 1), (12, 3)])
def test_gn_backward_spec_matches_autograd_on_column_slices(C, NG, relu):
    """gn_bwd_partial -> per-group sums -> gn_bwd_finalize -> gn_bwd_apply on the views Layer.columns() hands out
    (Y[:, c0:], gamma[c0:], sc1[:, c0:]), with and without the ReLU mask, one channel per norm group and one norm group"""
    from mmmot_amd.plan import RowTiles
    emu, eps, c0 = TorchOps(torch.float64), 1e-5, 4
    tiles = RowTiles([5, 130, 1], 'cpu')
    R, G, CG = tiles.R, tiles.G, C // NG
    g = torch.Generator().manual_seed(21)
    r64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Yw, dAw, gw, bw = r64(R, c0 + C), r64(R, c0 + C), r64(c0 + C) + 1.0, r64(c0 + C) * 0.3
    sc1w, sh1w = torch.zeros(G, c0 + C, dtype=torch.float64), torch.zeros(G, c0 + C, dtype=torch.float64)
    y = Yw[:, c0:].clone().requires_grad_(True)
    gamma, beta = gw[c0:].clone().requires_grad_(True), bw[c0:].clone().requires_grad_(True)
    loss = 0.0
    for gi in range(G):
        r0, n = int(tiles.h_g_row0[gi]), int(tiles.h_g_count[gi])
        v = y[r0:r0 + n].view(n, NG, CG)
        mean = v.mean(dim=(0, 2), keepdim=True)
        rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(dim=(0, 2), keepdim=True) + eps)
        z = ((v - mean) * rstd).reshape(n, C) * gamma + beta
        loss = loss + ((torch.relu(z) if relu else z) * dAw[r0:r0 + n, c0:]).sum()
        sc1w[gi, c0:] = rstd.detach().reshape(NG, 1).expand(NG, CG).reshape(C)
        sh1w[gi, c0:] = (-mean * rstd).detach().reshape(NG, 1).expand(NG, CG).reshape(C)
    dy_ref, dgamma_ref, dbeta_ref = torch.autograd.grad(loss, (y, gamma, beta))
    views = (dAw[:, c0:], Yw[:, c0:], C, sc1w[:, c0:], sh1w[:, c0:], gw[c0:], bw[c0:], relu)
    P = torch.zeros(tiles.T, 2, C, dtype=torch.float64)
    emu.gn_bwd_partial(*views, tiles, P)
    _same64(P[:, 1].sum(0), dgamma_ref, 'dgamma')
    _same64(P[:, 0].sum(0), dbeta_ref, 'dbeta')
    S = torch.stack([P[int(tiles.h_g_tile0[k]):int(tiles.h_g_tile0[k]) + int(tiles.h_g_ntiles[k])].sum(0) for k in range(G)])
    M = torch.zeros(G, 2, C, dtype=torch.float64)
    emu.gn_bwd_finalize(S.reshape(G * 2, C), tiles, C, NG, gw[c0:], M)
    dYw = torch.full((R, c0 + C), float('nan'), dtype=torch.float64)
    emu.gn_bwd_apply(*views, M, tiles, dYw[:, c0:])
    _same64(dYw[:, c0:], dy_ref, 'dY')
    assert torch.isnan(dYw[:, :c0]).all()


@pytest.mark.parametrize('pairop', [0, 1, 2])
def test_pair_bwd_spec_matches_autograd_with_ties(pairop):
    """pair_bwd (both sides, on top of a non-zero dF; the middle frame of a 3-frame sample gets both) against autograd of
    the pairwise operand; with a == b exactly in a few columns, where |a - b| has the sub-gradient 0 (torch's choice too)"""
    from mmmot_amd.backward import _aux
    from mmmot_amd.plan import BatchPlan
    emu, C = TorchOps(torch.float64), 8
    plan = BatchPlan([([3, 2, 4], None), ([1, 1], None)], 32, 'cpu', rows=(0,), use_points=False)
    aux, PT = _aux(plan), plan.pair_tiles
    g = torch.Generator().manual_seed(22)
    F = torch.randn(plan.Lt, C, generator=g, dtype=torch.float64)
    F[3, 2:5] = F[0, 2:5]     # frame 0 row 0 == frame 1 row 0 (pair 0: a_0 == b_0)
    F[6, 0:3] = F[4, 0:3]     # frame 1 row 1 == frame 2 row 1 (pair 1: a_1 == b_1)
    F[10] = F[9]              # the 1 x 1 pair: every column ties
    dX = torch.randn(PT.R, C, generator=g, dtype=torch.float64)
    dF0 = torch.randn(plan.Lt, C, generator=g, dtype=torch.float64)
    f = F.clone().requires_grad_(True)
    loss = 0.0
    for k in range(PT.G):
        N, M, r0 = int(plan.h_pg_N[k]), int(plan.h_pg_M[k]), int(PT.h_g_row0[k])
        a, b = f[int(plan.h_pg_aoff[k]):][:N].unsqueeze(1), f[int(plan.h_pg_boff[k]):][:M].unsqueeze(0)
        x = a * b if pairop == 0 else ((a - b).abs() / 2 if pairop == 1 else (a - b) / 2)
        loss = loss + (x * dX[r0:r0 + N * M].view(N, M, C)).sum()
    (ref,) = torch.autograd.grad(loss, f)
    dF = dF0.clone()
    for side, (bg, bi) in enumerate([(aux.a_grp, aux.a_idx), (aux.b_grp, aux.b_idx)]):
        emu.pair_bwd(dX, F, dF, C, PT.g_row0, plan.pg_N, plan.pg_M, plan.pg_aoff, plan.pg_boff, bg, bi, pairop, side)
    _same64(dF, dF0 + ref, 'dF')
    if pairop == 1:  # the ties contribute nothing: the 1 x 1 pair's rows keep their start value
        assert torch.equal(dF[9:11], dF0[9:11])


@pytest.mark.parametrize('nsplit', [1, 4, 7])
def test_gemm_tn_spec_shares_match_autograd(nsplit):
    """share s of gemm_tn holds the tiles [T*s/nsplit, T*(s+1)/nsplit): every share against autograd over its own rows,
    empty shares (nsplit > T = 4) exact zeros, and the shares add up to the whole gradient"""
    from mmmot_amd.plan import RowTiles
    emu, N, K = TorchOps(torch.float64), 6, 5
    tiles = RowTiles([5, 130, 1], 'cpu')
    T = tiles.T
    assert T == 4
    g = torch.Generator().manual_seed(23)
    r64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    X, dY, sc, sh = r64(tiles.R, K), r64(tiles.R, N), r64(tiles.G, K) + 1.0, r64(tiles.G, K) * 0.5
    dW, db = torch.full((nsplit, N, K), float('nan'), dtype=torch.float64), torch.full((nsplit, N), float('nan'), dtype=torch.float64)
    emu.gemm_tn(dY, tiles, N, K, dW, db, X=X, sc=sc, sh=sh, amode=1, nsplit=nsplit)
    grp = torch.repeat_interleave(torch.arange(tiles.G), torch.as_tensor(tiles.h_g_count).long())
    A = torch.relu(X * sc[grp] + sh[grp])
    W = torch.zeros(N, K, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    n_empty = 0
    for s in range(nsplit):
        lo, hi = T * s // nsplit, T * (s + 1) // nsplit
        if hi == lo:
            n_empty += 1
            assert (dW[s] == 0).all() and (db[s] == 0).all()
            continue
        r_lo, r_hi = int(tiles.h_row0[lo]), int(tiles.h_row0[hi - 1]) + int(tiles.h_nrows[hi - 1])
        gw, gb = torch.autograd.grad(((A[r_lo:r_hi] @ W.t() + bias) * dY[r_lo:r_hi]).sum(), (W, bias))
        _same64(dW[s], gw, 'share %d dW' % s)
        _same64(db[s], gb, 'share %d db' % s)
    assert n_empty == max(0, nsplit - T)
    gw, gb = torch.autograd.grad(((A @ W.t() + bias) * dY).sum(), (W, bias))
    _same64(dW.sum(0), gw, 'dW summed')
    _same64(db.sum(0), gb, 'db summed')


def test_gemm_tn_refuses_tiles_longer_than_128_rows():
    """mmmot_gemm_tn_f16 stages 128 rows of a tile: a Gram-style tiling (RowTiles(..., tile=512 / 2048)) would lose the
    rest without a word, so both backends refuse it before anything runs - in both arithmetics"""
    from mmmot_amd.ops import HipOps
    from mmmot_amd.plan import RowTiles
    long_tiles, ok_tiles = RowTiles([300], 'cpu', tile=512), RowTiles([300], 'cpu')
    assert long_tiles.T == 1 and int(long_tiles.h_nrows.max()) == 300 and int(ok_tiles.h_nrows.max()) == 128
    dY, X, dW = torch.zeros(300, 64), torch.zeros(300, 64), torch.zeros(64, 64)
    with pytest.raises(ValueError, match='128 rows'):
        TorchOps().gemm_tn(dY, long_tiles, 64, 64, dW, X=X)
    TorchOps().gemm_tn(dY, ok_tiles, 64, 64, dW, X=X)
    hip = object.__new__(HipOps)  # no library needed: the refusal comes before the first pointer is taken
    for f16 in (True, False):
        hip.tn_f16 = f16
        with pytest.raises(ValueError, match='128 rows'):
            hip.gemm_tn(dY, long_tiles, 64, 64, dW, X=X)
