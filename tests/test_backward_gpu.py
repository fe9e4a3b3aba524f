"""Training backward of the pairwise block on the device (csrc/backward.hip through the C-ABI):
* every backward kernel against its executable specification (tests/fake_ops.py);
* end to end: dF and every w_link.* gradient against torch.autograd through the ORACLE (float64 CPU restatement of
  reference modules/gcn.py:68-82, new_end.py:62-82, tracking_net.py:106-126), all pairwise ops / softmax modes, several
  samples per batch, a 3-frame sample, N x M up to 32 x 32; through the autograd.Function as well."""
import numpy as np
import pytest
import torch

from common import build_model, get_case
from fake_ops import TorchOps
from mmmot_amd.backward import affinity_autograd, affinity_backward, affinity_forward_train
from mmmot_amd.plan import BatchPlan, RowTiles
from test_backward_cpu import (HEAD_CASES, check_recorded_forward_is_the_eval_forward, check_tape_owns_its_storage,
                               reference_grads)
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def both(tiles_counts):
    return RowTiles(tiles_counts, 'cpu'), RowTiles(tiles_counts, DEV)


@pytest.mark.parametrize('C,NG', [(128, 128), (512, 1), (512, 512), (64, 4)])
def test_gn_backward_kernels(hip, C, NG):
    emu = TorchOps()
    tc, tg = both([5, 300, 128, 1])
    R, G = tc.R, tc.G
    Y, dA = rnd(R, C, seed=1), rnd(R, C, seed=2)
    sc1, sh1 = rnd(G, C, seed=3).abs() + 0.3, rnd(G, C, seed=4) * 0.2
    gamma, beta = rnd(C, seed=5) + 1.0, rnd(C, seed=6) * 0.3
    Pc, Pg = torch.zeros(tc.T, 2, C), torch.zeros(tc.T, 2, C, device=DEV)
    emu.gn_bwd_partial(dA, Y, C, sc1, sh1, gamma, beta, True, tc, Pc)
    hip.gn_bwd_partial(dA.cuda(), Y.cuda(), C, sc1.cuda(), sh1.cuda(), gamma.cuda(), beta.cuda(), True, tg, Pg)
    close(Pg, Pc, 2e-5, 'gn_bwd_partial')
    S = torch.stack([Pc[int(tc.h_g_tile0[g]):int(tc.h_g_tile0[g]) + int(tc.h_g_ntiles[g])].sum(0) for g in range(G)])
    Mc, Mg = torch.zeros(G, 2, C), torch.zeros(G, 2, C, device=DEV)
    emu.gn_bwd_finalize(S.reshape(G * 2, C), tc, C, NG, gamma, Mc)
    hip.gn_bwd_finalize(S.reshape(G * 2, C).cuda(), tg, C, NG, gamma.cuda(), Mg)
    close(Mg, Mc, 2e-6, 'gn_bwd_finalize')
    dYc, dYg = torch.zeros(R, C), torch.full((R, C), float('nan'), device=DEV)
    emu.gn_bwd_apply(dA, Y, C, sc1, sh1, gamma, beta, True, Mc, tc, dYc)
    hip.gn_bwd_apply(dA.cuda(), Y.cuda(), C, sc1.cuda(), sh1.cuda(), gamma.cuda(), beta.cuda(), True, Mc.cuda(), tg, dYg)
    close(dYg, dYc, 2e-6, 'gn_bwd_apply')


@pytest.mark.parametrize('amode', [0, 1, 2])
def test_gemm_tn(hip, amode):
    emu = TorchOps()
    N, K = 128, 192
    if amode == 2:
        plan_c = BatchPlan([([5, 7], None), ([3, 2, 4], None)], 32, 'cpu', use_points=False)
        plan_g = BatchPlan([([5, 7], None), ([3, 2, 4], None)], 32, DEV, use_points=False)
        tc, tg = plan_c.pair_tiles, plan_g.pair_tiles
        F = rnd(3 * plan_c.Lt, K, seed=7)
        pair_c = dict(row0=tc.g_row0, M=plan_c.pg_M, aoff=plan_c.pg_aoff, boff=plan_c.pg_boff)
        pair_g = dict(row0=tg.g_row0, M=plan_g.pg_M, aoff=plan_g.pg_aoff, boff=plan_g.pg_boff)
        kw_c, kw_g = dict(FA=F, FB=F, pair=pair_c, pairop=1), dict(FA=F.cuda(), FB=F.cuda(), pair=pair_g, pairop=1)
    else:
        tc, tg = both([7, 260, 128])
        X, sc, sh = rnd(tc.R, K, seed=8), rnd(tc.G, K, seed=9) + 1.0, rnd(tc.G, K, seed=10) * 0.5
        kw_c = dict(X=X, sc=sc, sh=sh) if amode else dict(X=X)
        kw_g = {k: v.cuda() for k, v in kw_c.items()}
    dY = rnd(tc.R, N, seed=11)
    for ns in (1, 3):
        dWc, dbc = torch.zeros(ns, N, K), torch.zeros(ns, N)
        dWg, dbg = torch.full((ns, N, K), float('nan'), device=DEV), torch.full((ns, N), float('nan'), device=DEV)
        emu.gemm_tn(dY, tc, N, K, dWc, dbc, amode=amode, nsplit=ns, **kw_c)
        hip.gemm_tn(dY.cuda(), tg, N, K, dWg, dbg, amode=amode, nsplit=ns, **kw_g)
        close(dWg, dWc, 2e-6, 'gemm_tn dW (nsplit %d)' % ns)
        close(dbg, dbc, 2e-6, 'gemm_tn db (nsplit %d)' % ns)
        close(dWg.sum(0), dWc.sum(0), 2e-6, 'gemm_tn dW summed')


@pytest.mark.parametrize('pairop', [0, 1, 2])
def test_pair_backward_kernels(hip, pairop):
    from mmmot_amd.backward import _aux
    emu = TorchOps()
    samples = [([5, 7], None), ([3, 2, 4], None), ([1, 1], None)]
    pc, pg = BatchPlan(samples, 32, 'cpu', use_points=False), BatchPlan(samples, 32, DEV, use_points=False)
    C = 256
    F = rnd(3 * pc.Lt, C, seed=12)
    dX = rnd(pc.pair_tiles.R, C, seed=13)
    dFc, dFg = torch.zeros(3 * pc.Lt, C), torch.zeros(3 * pc.Lt, C, device=DEV)
    ac, ag = _aux(pc), _aux(pg)
    for side, (bg_c, bi_c, bg_g, bi_g) in enumerate([(ac.a_grp, ac.a_idx, ag.a_grp, ag.a_idx), (ac.b_grp, ac.b_idx, ag.b_grp, ag.b_idx)]):
        emu.pair_bwd(dX, F, dFc, C, pc.pair_tiles.g_row0, pc.pg_N, pc.pg_M, pc.pg_aoff, pc.pg_boff, bg_c, bi_c, pairop, side)
        hip.pair_bwd(dX.cuda(), F.cuda(), dFg, C, pg.pair_tiles.g_row0, pg.pg_N, pg.pg_M, pg.pg_aoff, pg.pg_boff, bg_g, bi_g, pairop, side)
    close(dFg, dFc, 2e-6, 'pair_bwd')
    dV = rnd(pc.v_tiles.R, C, seed=14)
    dAc, dAg = torch.zeros(pc.pair_tiles.R, C), torch.full((pc.pair_tiles.R, C), float('nan'), device=DEV)
    emu.pair_expand_bwd(dV, dAc, C, pc.pair_tiles, pc.pair_tiles.g_row0, pc.pg_N, pc.pg_M, ac.vrow0)
    hip.pair_expand_bwd(dV.cuda(), dAg, C, pg.pair_tiles, pg.pair_tiles.g_row0, pg.pg_N, pg.pg_M, ag.vrow0)
    close(dAg, dAc, 1e-6, 'pair_expand_bwd')


@pytest.mark.parametrize('act,use_idx', [(0, False), (2, True)])
def test_rowdot_backward(hip, act, use_idx):
    emu = TorchOps()
    tc, tg = both([5, 300, 128])
    K, R = 128, tc.R
    X, w = rnd(R, K, seed=15), rnd(K, seed=16)
    sc, sh = rnd(tc.G, K, seed=17) + 1.0, rnd(tc.G, K, seed=18) * 0.5
    gidx = torch.randperm(2 * R, generator=torch.Generator().manual_seed(1))[:R].to(torch.int32) if use_idx else None
    gout = rnd(2 * R if use_idx else R, seed=19)
    dAc, PWc = torch.zeros(R, K), torch.zeros(tc.T, 132)
    dAg, PWg = torch.full((R, K), float('nan'), device=DEV), torch.zeros(tc.T, 132, device=DEV)
    emu.rowdot_bwd(X, K, w, 0.3, sc, sh, tc, act, gout, gidx, dAc, PWc)
    hip.rowdot_bwd(X.cuda(), K, w.cuda(), 0.3, sc.cuda(), sh.cuda(), tg, act, gout.cuda(),
                   None if gidx is None else gidx.cuda(), dAg, PWg)
    close(dAg, dAc, 2e-6, 'rowdot_bwd dA')
    close(PWg[:, :129], PWc[:, :129], 2e-5, 'rowdot_bwd partial dw / db')


@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_softmax_backward(hip, mode):
    emu = TorchOps()
    samples = [([5, 7], None), ([32, 20], None), ([1, 1], None), ([1, 9], None)]
    pc, pg = BatchPlan(samples, 32, 'cpu', use_points=False), BatchPlan(samples, 32, DEV, use_points=False)
    R = pc.pair_tiles.R
    logits, dout = rnd(R, seed=20) * 2.0, rnd(R, seed=21)
    dc, dg = torch.zeros(R), torch.full((R,), float('nan'), device=DEV)
    emu.softmax_pairs_bwd(logits, dout, dc, pc.pair_tiles.g_row0, pc.pg_N, pc.pg_M, pc.pair_tiles.G, pc.max_nm, mode)
    hip.softmax_pairs_bwd(logits.cuda(), dout.cuda(), dg, pg.pair_tiles.g_row0, pg.pg_N, pg.pg_M, pg.pair_tiles.G, pg.max_nm, mode)
    close(dg, dc, 3e-6, 'softmax_pairs_bwd')


@pytest.mark.parametrize('trunk,rtol', [('f32', 2e-4), ('f16x3', 5e-4)])
@pytest.mark.parametrize('op,sm,samples', [
    ('multiply', 'none', [[3, 4]]),
    ('minus_abs', 'dual_add', [[5, 2], [1, 6]]),
    ('minus', 'dual', [[2, 3, 2]]),
    ('multiply', 'dual_max', [[4, 4]]),
    ('minus_abs', 'single', [[1, 1], [3, 5]]),
    ('multiply', 'none', [[32, 32], [20, 31]]),
    ('minus_abs', 'dual_add', [[32, 32]]),
])
def test_backward_matches_autograd_through_the_oracle(op, sm, samples, trunk, rtol):
    c, base = get_case('s2_C_multiply_none')
    c = dict(c, aff=op, sm=sm)
    if any(len(s) > 2 for s in samples):
        c['counts'] = samples[0]
    m_cpu = build_model(c, base)
    m = build_model(c, base, device=DEV)
    m.set_trunk(trunk)
    eng = m.engine()
    assert eng.ops.name == 'hip'
    plan = BatchPlan([(s, None) for s in samples], 32, DEV, use_points=False)
    g = torch.Generator().manual_seed(3)
    F = torch.randn(3, plan.Lt, 512, generator=g) * 0.7
    R_ = plan.pair_tiles.R
    w_link, w_new, w_end = torch.randn(R_, generator=g), torch.randn(3, plan.Lt, generator=g), torch.randn(3, plan.Lt, generator=g)
    Fd = F.to(DEV)
    link, new, end, tape = affinity_forward_train(eng, plan, Fd)
    dF, grads = affinity_backward(eng, plan, Fd, tape, w_link.to(DEV), w_new.to(DEV), w_end.to(DEV))
    dF_ref, g_ref = reference_grads(m_cpu, samples, F, op, sm, w_link, w_new, w_end)
    # ReLU is not differentiable at 0: with ~1e6 pre-activations per forward, one of them can sit within fp32 rounding
    # of zero and take the other branch than in the float64 reference, which moves the gradients that flow through it
    # by a few per cent of their maximum (seen on the 32 x 32 cases; any fp32 implementation has this, and the
    # emulation run in float64 agrees to 8e-8; a flip upstream of a GroupNorm touches every channel of its gamma / beta
    # gradient a little).  So: strict L-inf for every tensor, or - when that fails - a small L2 error with a bounded
    # L-inf: a wrong formula or index shows up as an O(1) L2 error.
    gmax = max(v.abs().max().item() for v in g_ref.values())

    def check(name, got, ref):
        d = got.cpu().double().reshape(ref.shape) - ref
        rmax = ref.abs().max().item()
        linf = d.abs().max().item()
        tol = rtol * rmax + 1e-2 * rtol * (1.0 + gmax)
        if linf < tol:
            return linf / max(rmax, 1e-30), False
        l2 = (d.norm() / max(ref.norm().item(), 1e-30)).item()
        assert l2 < 5e-3 and linf < 0.1 * rmax + tol, (name, linf, rmax, l2)
        return l2, True

    res = {'dF': check('dF', dF, dF_ref)}
    for k, ref in g_ref.items():
        res[k] = check(k, grads[k], ref)
    flipped = [k for k, (_, f) in res.items() if f]
    if max(len(s_) for s_ in samples) <= 3 and max(max(s_) for s_ in samples) <= 8:
        assert not flipped, flipped  # the small cases have too few pre-activations for a flip: strict everywhere
    print('backward %s/%s %s %s: dF %.1e%s, worst parameter gradient %.1e, ReLU-flip tolerance used for %d tensors' % (
        op, sm, samples, trunk, res['dF'][0], ' (L2)' if res['dF'][1] else '',
        max(v for k, (v, _) in res.items() if k != 'dF' and g_ref[k].abs().max() > 1e-6 * gmax), len(flipped)))


def test_autograd_function_on_the_device():
    c, base = get_case('s2_C_minus_abs_dual_add')
    m = build_model(c, base, device=DEV)
    plan = BatchPlan([([6, 5], None), ([2, 9], None)], 32, DEV, use_points=False)
    F = (torch.randn(3, plan.Lt, 512, generator=torch.Generator().manual_seed(1)) * 0.7).to(DEV).requires_grad_(True)
    link, new, end = affinity_autograd(m, plan, F)
    # the training forward is the inference forward: same scores as Engine.affinity
    m.engine().dev = torch.device(DEV)  # Engine.forward sets it; affinity() is called on its own here
    l2, n2, e2 = m.engine().affinity(plan, F.detach())
    assert torch.allclose(link, l2, atol=1e-6) and torch.allclose(new, n2, atol=1e-6) and torch.allclose(end, e2, atol=1e-6)
    (link.square().sum() + 2 * new.sum() - end.sum()).backward()
    assert F.grad is not None and torch.isfinite(F.grad).all() and F.grad.abs().max() > 0
    for k, p in m.named_parameters():
        assert (p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all()) == k.startswith('w_link.'), k


# ---- second slice: fusion + training-mode w_det + pairwise block -------------------------------------------------------
def test_fusion_c_bwd_and_add_rows_kernels(hip):
    emu = TorchOps()
    tc, tg = both([40, 7])
    R, C = tc.R, 512
    Y0, Y1, dFu = rnd(R, 1024, seed=30), rnd(R, 1024, seed=31), rnd(R, C, seed=32)
    sc0, sh0, sc1, sh1 = rnd(tc.G, C, seed=33) + 1.0, rnd(tc.G, C, seed=34), rnd(tc.G, C, seed=35) + 1.0, rnd(tc.G, C, seed=36)
    outs_c = [torch.zeros(R, 1024), torch.zeros(R, 1024), torch.zeros(R, C), torch.zeros(R, C)]
    outs_g = [torch.zeros(R, 1024, device=DEV), torch.zeros(R, 1024, device=DEV), torch.zeros(R, C, device=DEV),
              torch.zeros(R, C, device=DEV)]
    emu.fusion_c_bwd(dFu, Y0, Y1, sc0, sh0, sc1, sh1, tc, *outs_c, C)
    hip.fusion_c_bwd(dFu.cuda(), Y0.cuda(), Y1.cuda(), sc0.cuda(), sh0.cuda(), sc1.cuda(), sh1.cuda(), tg, *outs_g, C)
    for a, b, what in zip(outs_g, outs_c, ('dgate0', 'dgate1', 'dn0', 'dn1')):
        close(a[:, :C], b[:, :C], 3e-6, 'fusion_c_bwd ' + what)
    A, B = rnd(R, 1024, seed=37), rnd(R, C, seed=38)
    Yg = torch.zeros(R, 1024, device=DEV)
    hip.add_rows(A.cuda()[:, 512:], B.cuda(), Yg[:, 512:], C)
    assert torch.equal(Yg[:, 512:].cpu(), A[:, 512:] + B) and (Yg[:, :512] == 0).all()


@pytest.mark.parametrize('trunk,rtol', [('f32', 3e-4), ('f16x3', 6e-4)])
@pytest.mark.parametrize('fusion,op,sm,counts', [('A', 'multiply', 'none', [4, 5]), ('B', 'minus_abs', 'dual_add', [7, 3]),
                                                 ('C', 'multiply', 'none', [6, 6]), ('C', 'minus_abs', 'dual_add', [24, 17])])
def test_head_backward_matches_autograd(fusion, op, sm, counts, trunk, rtol):
    from mmmot_amd.backward import head_backward, head_forward_train
    from test_backward_cpu import head_reference
    c, base = get_case('s2_C_multiply_none')
    c = dict(c, fusion=fusion, aff=op, sm=sm)
    m_cpu = build_model(c, base)
    m = build_model(c, base, device=DEV)
    m.set_trunk(trunk)
    eng = m.engine()
    plan = BatchPlan([(counts, None)], 32, DEV, use_points=False)
    g = torch.Generator().manual_seed(5)
    cat = torch.randn(plan.Lt, 1024, generator=g) * 0.8
    w = dict(det=torch.randn(3, plan.Lt, generator=g), link=torch.randn(plan.pair_tiles.R, generator=g),
             new=torch.randn(3, plan.Lt, generator=g), end=torch.randn(3, plan.Lt, generator=g))
    cd = cat.to(DEV)
    det, link, new, end, tape = head_forward_train(eng, m, plan, cd)
    dcat, grads = head_backward(eng, m, plan, cd, tape, *[w[k].to(DEV) for k in ('det', 'link', 'new', 'end')])
    dcat_ref, g_ref, det_ref = head_reference(m_cpu, counts, cat, fusion, op, sm, w)
    assert (det.cpu().double() - det_ref).abs().max().item() < 5e-4
    gmax = max(v.abs().max().item() for v in g_ref.values())
    worst = 0.0
    for name, got, ref in [('dcat', dcat, dcat_ref)] + [(k, grads[k], g_ref[k]) for k in g_ref]:
        d = got.cpu().double().reshape(ref.shape) - ref
        linf, rmax = d.abs().max().item(), ref.abs().max().item()
        tol = rtol * rmax + 1e-2 * rtol * (1.0 + gmax)
        if linf >= tol:  # an isolated ReLU-branch flip against the float64 reference (see the pairwise test above)
            l2 = (d.norm() / max(ref.norm().item(), 1e-30)).item()
            assert l2 < 5e-3 and linf < 0.1 * rmax + tol, (name, linf, rmax, l2)
        elif rmax > 1e-6 * gmax:
            worst = max(worst, linf / rmax)
    assert set(grads) == set(g_ref)
    print('head backward fusion %s %s/%s %s %s: worst relative gradient error %.1e over dcat + %d parameter tensors' % (
        fusion, op, sm, counts, trunk, worst, len(g_ref)))


def test_head_autograd_on_the_device():
    from mmmot_amd.backward import head_autograd
    c, base = get_case('s2_C_minus_abs_dual_add')
    m = build_model(c, base, device=DEV)
    plan = BatchPlan([([6, 5], None)], 32, DEV, use_points=False)
    cat = (torch.randn(plan.Lt, 1024, generator=torch.Generator().manual_seed(1)) * 0.8).to(DEV).requires_grad_(True)
    rv0 = m.w_det[4].running_var.clone()
    det, link, new, end = head_autograd(m, plan, cat)
    (det.sum() + link.square().sum() + 2 * new.sum() - end.sum()).backward()
    assert cat.grad is not None and torch.isfinite(cat.grad).all() and cat.grad.abs().max() > 0
    heads = ('fusion_module', 'w_det', 'w_link')
    for k, p in m.named_parameters():
        assert (p.grad is not None and torch.isfinite(p.grad).all()) == (k.split('.')[0] in heads), k
    assert not torch.equal(m.w_det[4].running_var, rv0)  # training-mode BatchNorm updated its buffers


def test_sgd_on_the_head_reduces_a_loss():
    """A few plain SGD steps on the head's parameters through head_autograd (forward + backward on the device): a
    regression loss on the link scores and a logistic loss on the det scores both go down - the gradients point the
    right way end to end (the head's packed weights are rebuilt from the updated parameters by model.refresh_head())."""
    from mmmot_amd.backward import head_autograd
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, device=DEV)
    plan = BatchPlan([([8, 7], None)], 32, DEV, use_points=False)
    g = torch.Generator().manual_seed(4)
    cat = (torch.randn(plan.Lt, 1024, generator=g) * 0.8).to(DEV)
    tgt_link = torch.randn(plan.pair_tiles.R, generator=g).to(DEV)
    tgt_det = (torch.rand(3, plan.Lt, generator=g) > 0.5).float().to(DEV)
    params = [p for k, p in m.named_parameters() if k.split('.')[0] in ('fusion_module', 'w_det', 'w_link')]
    losses = []
    for step in range(6):
        for p in params:
            p.grad = None
        det, link, new, end = head_autograd(m, plan, cat, update_running_stats=False)
        loss = (torch.nn.functional.mse_loss(link, tgt_link) +
                torch.nn.functional.binary_cross_entropy_with_logits(det, tgt_det))
        loss.backward()
        losses.append(loss.item())
        with torch.no_grad():
            for p in params:
                p.add_(p.grad, alpha=-0.02)
        m.refresh_head()  # re-pack the 3 M head parameters only
    print('head SGD losses', ['%.4f' % v for v in losses])
    assert losses[-1] < 0.9 * losses[0] and all(b < a * 1.02 for a, b in zip(losses, losses[1:]))


# ---- the head's training forward is the engine's forward, recorded (Engine.recording) ---------------------------------
def test_a_tape_owns_its_storage():
    c, base = get_case('s2_C_multiply_none')
    check_tape_owns_its_storage(build_model(c, base, device=DEV), DEV)


@pytest.mark.parametrize('counts', [[32, 32], [5, 3]])
@pytest.mark.parametrize('fusion,op,sm', HEAD_CASES)
def test_recorded_forward_is_the_eval_forward(fusion, op, sm, counts):
    c, base = get_case('s2_C_multiply_none')
    m = build_model(dict(c, fusion=fusion, aff=op, sm=sm), base, device=DEV)
    check_recorded_forward_is_the_eval_forward(m, counts, DEV)
