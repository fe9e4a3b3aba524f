"""Training of end_mode='max' models (NewEndIndicator_v2 taking maxima, reference modules/new_end.py:72-74), host side:
the executable specification of the two arg-max backward operators (tests/end_max_ref.py) against float64 autograd with
exact ties, mmmot_amd/backward.py on the operator emulation against autograd through the oracle, one whole training step
against the imported reference's (tests/golden/endmax_train_s10_C.npz, tools/gen_golden_endmax_train.py) and the
argument checks of the two launchers.  tests/test_end_max_gpu.py runs the HIP kernels."""
import pytest
import torch

from common import build_model, compare_train_step, get_case
from end_max_ref import EndMaxOps, reference_grads, top_two_gaps
from mmmot_amd.backward import _aux, affinity_backward, affinity_forward_train
from mmmot_amd.plan import BatchPlan


def test_specification_matches_autograd_with_exact_ties():
    """segment_argmax + pair_expand_max_bwd of the specification against float64 autograd through x.max(dim=-2)[0] /
    x.max(dim=-1)[0] on small integers (ties everywhere), with an all-non-positive column (relu: every row ties at 0, the
    gradient goes to row 0) and planted ties between rows 1 and 4 (different waves of the kernel) and rows 0 and count-1"""
    emu, C = EndMaxOps(torch.float64), 8
    plan = BatchPlan([([5, 7], None), ([3, 2, 4], None), ([1, 1], None)], 32, 'cpu', rows=(0,), use_points=False)
    aux, PT, VT = _aux(plan), plan.pair_tiles, plan.v_tiles
    g = torch.Generator().manual_seed(31)
    X = torch.randint(-3, 4, (PT.R, C), generator=g).double()
    X[:, 0] = -X[:, 0].abs()                       # all <= 0
    N0, M0 = 5, 7                                  # group 0 starts at row 0: row (i, j) = i * M0 + j
    X[1 * M0 + 2, 3] = X[4 * M0 + 2, 3] = 9.0      # "new" vector 2, channel 3: rows 1 and 4 of its 5
    X[0 * M0 + 1, 5] = X[0 * M0 + 4, 5] = 9.0      # "end" vector 0, channel 5: rows 1 and 4 of its 7
    X[0 * M0 + 6, 6] = X[4 * M0 + 6, 6] = 8.0      # "new" vector 6, channel 6: rows 0 and count - 1
    X[2 * M0 + 0, 7] = X[2 * M0 + 6, 7] = 8.0      # "end" vector 2, channel 7: rows 0 and count - 1
    dV = torch.randn(VT.R, C, generator=g, dtype=torch.float64)
    idx = torch.full((VT.R, C), -1, dtype=torch.int32)
    emu.segment_argmax(X, C, plan.v_segs, idx, relu=True)
    dA = torch.full((PT.R, C), float('nan'), dtype=torch.float64)
    emu.pair_expand_max_bwd(dV, idx, dA, C, PT, PT.g_row0, plan.pg_N, plan.pg_M, aux.vrow0)
    a = torch.relu(X).requires_grad_(True)
    loss = 0.0
    for k in range(PT.G):
        N, M, r0, v0 = int(plan.h_pg_N[k]), int(plan.h_pg_M[k]), int(PT.h_g_row0[k]), int(aux.vrow0[k])
        x = a[r0:r0 + N * M].view(N, M, C).permute(2, 0, 1)              # C x N x M, the reference's layout
        new, new_i = x.max(dim=-2)                                       # C x M
        end, end_i = x.max(dim=-1)                                       # C x N
        assert torch.equal(idx[v0:v0 + M].long(), new_i.t()) and torch.equal(idx[v0 + M:v0 + M + N].long(), end_i.t())
        loss = loss + (new.t() * dV[v0:v0 + M]).sum() + (end.t() * dV[v0 + M:v0 + M + N]).sum()
    (ref,) = torch.autograd.grad(loss, a)
    assert torch.equal(dA, ref)
    v0 = int(aux.vrow0[0])
    assert (idx[:, 0] == 0).all()
    assert idx[v0 + 2, 3] == 1 and idx[v0 + M0 + 0, 5] == 1 and idx[v0 + 6, 6] == 0 and idx[v0 + M0 + 2, 7] == 0
    # pair rows (1, 2) and (4, 2) both hold the 9 of channel 3: each is the maximum of its own "end" vector, only the
    # first one gets the gradient of "new" vector 2
    assert dA[4 * M0 + 2, 3] == dV[v0 + M0 + 4, 3] and dA[1 * M0 + 2, 3] == dV[v0 + 2, 3] + dV[v0 + M0 + 1, 3]


# (pairwise op, softmax mode, samples, seed of F): on these the smallest top-two gap of the maxima is >= 1e-5 of the
# tensor's maximum (asserted below), far above fp32 rounding of the normalised conv0 output (~1e-7): fp32 and float64
# pick the same rows, and the comparison is as strict as the one of tests/test_backward_cpu.py
STRICT_CASES = [
    ('multiply', 'none', [[3, 4]], 4),
    ('minus_abs', 'dual_add', [[5, 2], [1, 6]], 1),
    ('minus', 'dual', [[2, 3, 2]], 3),
    ('multiply', 'dual_max', [[4, 4]], 1),
    ('minus_abs', 'single', [[1, 1], [3, 5]], 2),
]


@pytest.mark.parametrize('op,sm,samples,seed', STRICT_CASES)
def test_backward_matches_autograd_through_the_oracle(op, sm, samples, seed):
    c, base = get_case('s2_C_multiply_none')
    c = dict(c, aff=op, sm=sm, end_mode='max')
    if any(len(s) > 2 for s in samples):
        c['counts'] = samples[0]
    m = build_model(c, base, ops=EndMaxOps())
    m.set_trunk('f32')
    eng = m.engine()
    assert eng.end_mode == 'max'
    plan = BatchPlan([(s, None) for s in samples], 32, 'cpu', use_points=False)
    g = torch.Generator().manual_seed(seed)
    F = torch.randn(3, plan.Lt, 512, generator=g) * 0.7
    R_ = plan.pair_tiles.R
    w_link, w_new, w_end = torch.randn(R_, generator=g), torch.randn(3, plan.Lt, generator=g), torch.randn(3, plan.Lt, generator=g)
    gap = top_two_gaps(m.state_dict(), F, samples, op).min().item()
    assert gap >= 1e-5, gap
    link, new, end, tape = affinity_forward_train(eng, plan, F)
    dF, grads = affinity_backward(eng, plan, F, tape, w_link, w_new, w_end)
    dF_ref, g_ref = reference_grads(m, samples, F, op, sm, w_link, w_new, w_end)
    # ... and these are not the gradients of the mean pool
    dF_avg, _ = reference_grads(m, samples, F, op, sm, w_link, w_new, w_end, end_mode='avg')
    scale = dF_ref.abs().max().item()
    assert (dF_avg - dF_ref).abs().max().item() > 1e-2 * scale
    assert (dF.double() - dF_ref).abs().max().item() < 2e-4 * scale, 'dF'
    assert set(grads) == set(g_ref)
    gmax = max(v.abs().max().item() for v in g_ref.values())
    for k, ref in g_ref.items():
        got = grads[k].double().reshape(ref.shape)
        tol = 2e-4 * ref.abs().max().item() + 2e-6 * (1.0 + gmax)
        assert (got - ref).abs().max().item() < tol, (k, (got - ref).abs().max().item(), ref.abs().max().item())
    print('end-max backward %s/%s %s seed %d: smallest top-two gap %.1e, dF error %.1e of its maximum' % (
        op, sm, samples, seed, gap, (dF.double() - dF_ref).abs().max().item() / scale))


def test_training_step_matches_the_reference_fixture():
    """model.train() forward -> TrackingLoss -> backward with end_mode='max' on the float64 operator emulation against the
    imported reference's step; the CPU tolerances of tests/test_train_vgg_cpu.py"""
    from test_train_vgg_cpu import product_train_step
    name = 'endmax_train_s10_C'
    g, outs, loss, grad_of, buffers = product_train_step(name, ops=EndMaxOps(torch.float64))
    worst = compare_train_step(g, outs, loss, grad_of, buffers, out_tol=5e-5, loss_tol=5e-6, grad_tol=2e-2, norm_tol=1e-2,
                               bn_tol=1e-5, what=name)
    print('%s: product (emulated C-ABI) vs the reference training step: %s' % (name, ' '.join('%s=%.1e' % kv for kv in worst.items())))


def test_launchers_reject_bad_arguments_without_a_gpu():
    """null pointers, C % 4, T <= 0 and misaligned pointers return MMMOT_EINVAL before any launch"""
    from mmmot_amd import _lib
    lib = _lib.load()
    d = 4096  # never dereferenced
    ok = lambda **kw: dict(dict(X=d, ldx=512, C=512, start=d, count=d, stride=d, group=d, nseg=3, sc=d, sh=d, ldsc=512, relu=1,
                                idx=d, ldo=512), **kw)
    call = lambda a: lib.mmmot_segment_argmax(a['X'], a['ldx'], a['C'], a['start'], a['count'], a['stride'], a['group'],
                                              a['nseg'], a['sc'], a['sh'], a['ldsc'], a['relu'], a['idx'], a['ldo'], None)
    for bad in (dict(X=None), dict(start=None), dict(count=None), dict(idx=None), dict(sh=None), dict(C=510), dict(C=0),
                dict(nseg=0), dict(nseg=-1), dict(X=d + 4), dict(idx=d + 8), dict(sc=d + 4), dict(sh=d + 12), dict(ldx=514),
                dict(ldo=510), dict(ldsc=6), dict(ldx=256), dict(relu=2), dict(relu=3)):
        assert call(ok(**bad)) == -1, bad
    ok = lambda **kw: dict(dict(dV=d, lddv=512, idx=d, ldi=512, dA=d, ldda=512, C=512, row0=d, nrows=d, grp=d, T=2, g0=d, gN=d,
                                gM=d, v0=d), **kw)
    call = lambda a: lib.mmmot_pair_expand_max_bwd(a['dV'], a['lddv'], a['idx'], a['ldi'], a['dA'], a['ldda'], a['C'],
                                                   a['row0'], a['nrows'], a['grp'], a['T'], a['g0'], a['gN'], a['gM'], a['v0'],
                                                   None)
    for bad in (dict(dV=None), dict(idx=None), dict(dA=None), dict(row0=None), dict(nrows=None), dict(grp=None), dict(g0=None),
                dict(gN=None), dict(gM=None), dict(v0=None), dict(C=6), dict(C=0), dict(T=0), dict(T=-3), dict(dV=d + 4),
                dict(idx=d + 4), dict(dA=d + 8), dict(lddv=510), dict(ldi=6), dict(ldda=514), dict(ldda=256)):
        assert call(ok(**bad)) == -1, bad
