"""Training of end_mode='max' models on the device (csrc/backward.hip: mmmot_segment_argmax, mmmot_pair_expand_max_bwd):
the two kernels against their executable specification bit for bit, the pairwise block's backward against float64 autograd
through the oracle, one whole training step against the imported reference's and the training pipeline in both orders."""
import pytest
import torch

from common import build_model, case_kwargs, compare_train_step, get_case
from end_max_ref import EndMaxOps, conv0_rows, reference_grads, top_two_gaps
from mmmot_amd.backward import _aux, affinity_backward, affinity_forward_train
from mmmot_amd.plan import BatchPlan
from test_kernels_gpu import hip  # noqa: F401  (a fixture)
from test_train_pipeline_gpu import bits, frames, make_pipe, sample_of  # noqa: F401  (frames is a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# one-row segments ([1,1], [1,33], [33,1]), counts below 4 and off the multiple of 4, stride M != 1 next to stride 1, two
# groups in one sample ([3,2,4]), pair tiles that cross an i boundary (5 x 7 in one tile, 32 x 32 in eight per modality row)
KERNEL_SAMPLES = [[5, 7], [3, 2, 4], [1, 1], [1, 33], [33, 1], [32, 32]]


@pytest.fixture(scope='module')
def grid_case():
    """Inputs on which fp32 arithmetic is exact: X from a shuffled grid with spacing 2^-10 (every value once), sc powers
    of two, sh multiples of 2^-10 - fmaf(x, sc, sh) equals the rounded multiply-then-add of the specification, and two
    values of one column differ by a whole grid step or tie at 0 behind the ReLU.  Planted on top: exact ties of the
    maximum between rows 1 and 4 (waves 1 and 0 of the kernel) and rows 0 and count - 1, and a column that is <= 0
    everywhere.  The specification's index table and dA are computed once and shared."""
    pc = BatchPlan([(s, None) for s in KERNEL_SAMPLES], 32, 'cpu', use_points=False)
    PT, VT, C = pc.pair_tiles, pc.v_tiles, 512
    g = torch.Generator().manual_seed(41)
    n = PT.R * C
    X = ((torch.randperm(n, generator=g).double() - n // 2) * 2.0 ** -10).float().view(PT.R, C)
    assert X.abs().max().item() < 2.0 ** 11
    sc = torch.pow(2.0, torch.randint(-1, 2, (PT.G, C), generator=g).float())
    sh = torch.randint(-200 * 1024, 200 * 1024, (PT.G, C), generator=g).float() * 2.0 ** -10
    X[:, 9] = -X[:, 9].abs()
    sh[:, 9] = -0.5
    big = 4096.0
    planted = 0
    for k in range(PT.G):
        N, M, r0 = int(pc.h_pg_N[k]), int(pc.h_pg_M[k]), int(PT.h_g_row0[k])
        if N >= 5 and M >= 5:
            row = lambda i, j: r0 + i * M + j
            X[row(1, 2), 3] = X[row(4, 2), 3] = big            # "new" vector 2: rows 1 and 4
            X[row(0, 1), 5] = X[row(0, 4), 5] = big            # "end" vector 0: rows 1 and 4
            X[row(0, M - 1), 6] = X[row(N - 1, M - 1), 6] = big  # "new" vector M - 1: rows 0 and count - 1
            X[row(2, 0), 7] = X[row(2, M - 1), 7] = big        # "end" vector 2: rows 0 and count - 1
            planted += 1
    assert planted == 6  # the three modality rows of [5, 7] and of [32, 32]
    dV = torch.randn(VT.R, C, generator=g)
    emu, aux = EndMaxOps(), _aux(pc)
    out = {}
    for Cc in (512, 64):
        idx = torch.full((VT.R, Cc), -1, dtype=torch.int32)
        emu.segment_argmax(X[:, :Cc], Cc, pc.v_segs, idx, sc=sc[:, :Cc], sh=sh[:, :Cc], relu=True)
        dA = torch.full((PT.R, Cc), float('nan'))
        emu.pair_expand_max_bwd(dV[:, :Cc], idx, dA, Cc, PT, PT.g_row0, pc.pg_N, pc.pg_M, aux.vrow0)
        assert int(idx.min()) == 0 and int(idx.max()) == 32 and torch.isfinite(dA).all()
        out[Cc] = (idx, dA)
    # the planted ties are decided for the lower index, and the specification's arithmetic is exact here
    k = next(k for k in range(PT.G) if pc.h_pg_N[k] >= 5 and pc.h_pg_M[k] >= 5)
    v0, M = int(aux.vrow0[k]), int(pc.h_pg_M[k])
    idx = out[512][0]
    assert idx[v0 + 2, 3] == 1 and idx[v0 + M + 0, 5] == 1 and idx[v0 + M - 1, 6] == 0 and idx[v0 + M + 2, 7] == 0
    assert (idx[:, 9] == 0).all()
    grp = torch.repeat_interleave(torch.arange(PT.G), torch.as_tensor(PT.h_g_count).long())
    a32 = torch.relu(X * sc[grp] + sh[grp])
    assert torch.equal(a32.double(), torch.relu(X.double() * sc[grp].double() + sh[grp].double()))
    return dict(pc=pc, X=X, sc=sc, sh=sh, dV=dV, a=a32, spec=out)


@pytest.mark.parametrize('C', [512, 64])
def test_kernels_match_the_specification_bit_for_bit(hip, grid_case, C):
    """C = 512: two channel blocks per segment; C = 64: 16 busy lanes per wave, views with a leading dimension of 512"""
    q = grid_case
    pc, pg = q['pc'], BatchPlan([(s, None) for s in KERNEL_SAMPLES], 32, DEV, use_points=False)
    PT, VT, aux = pg.pair_tiles, pg.v_tiles, _aux(pg)
    Xg, scg, shg, dVg = q['X'].to(DEV), q['sc'].to(DEV), q['sh'].to(DEV), q['dV'].to(DEV)
    idx_ref, dA_ref = q['spec'][C]
    runs = []
    for _ in range(2):
        idx = torch.full((VT.R, C), -1, dtype=torch.int32, device=DEV)
        hip.segment_argmax(Xg[:, :C], C, pg.v_segs, idx, sc=scg[:, :C], sh=shg[:, :C], relu=True)
        dA = torch.full((PT.R, C), float('nan'), device=DEV)
        hip.pair_expand_max_bwd(dVg[:, :C], idx, dA, C, PT, PT.g_row0, pg.pg_N, pg.pg_M, aux.vrow0)
        runs.append((idx.cpu(), dA.cpu()))
    assert torch.equal(runs[0][0], idx_ref), 'index table: %d of %d entries differ' % (
        int((runs[0][0] != idx_ref).sum()), idx_ref.numel())
    assert torch.equal(runs[0][1], dA_ref), 'dA'
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # consistency with the forward: the activation at the arg-max row is the value the forward's maximum pool wrote
    V = torch.full((VT.R, C), float('nan'), device=DEV)
    hip.segment_mean(Xg[:, :C], C, pg.v_segs, V, sc=scg[:, :C], sh=shg[:, :C], relu=True, take_max=True)
    segs = pc.v_segs
    rows = torch.as_tensor(segs.h_start).view(-1, 1) + runs[0][0].long() * torch.as_tensor(segs.h_stride).view(-1, 1)
    picked = q['a'][:, :C].gather(0, rows)
    assert torch.equal(picked, V.cpu())


# (pairwise op, softmax mode, samples, seed of F, strict).  strict: the smallest top-two gap of the maxima, measured on the
# float64 restatement, is >= 1e-5 of the tensor's maximum - fp32 and float64 pick the same rows and every tensor must
# agree in L-inf.  The 32 x 32 cases have gaps of 4e-8 .. 2e-6, below fp32 rounding: a maximum decided the other way moves
# one channel's gradient out of 512, which the two-tier check of tests/test_backward_gpu.py admits.
E2E_CASES = [
    ('multiply', 'none', [[3, 4]], 4, True),
    ('minus_abs', 'dual_add', [[5, 2], [1, 6]], 1, True),
    ('minus', 'dual', [[2, 3, 2]], 3, True),
    ('multiply', 'dual_max', [[4, 4]], 1, True),
    ('minus_abs', 'single', [[1, 1], [3, 5]], 2, True),
    ('multiply', 'none', [[32, 32], [20, 31]], 3, False),
    ('minus_abs', 'dual_add', [[32, 32]], 3, False),
]
_refs = {}


def e2e_reference(c, base, op, sm, samples, seed):
    """inputs, float64 gradients, gaps and conv0 activations of one case: computed once, shared by both trunks"""
    key = (op, sm, str(samples), seed)
    if key not in _refs:
        m_cpu = build_model(c, base)
        Lt, R_ = sum(sum(s) for s in samples), sum(3 * s[i] * s[i + 1] for s in samples for i in range(len(s) - 1))
        g = torch.Generator().manual_seed(seed)
        F = torch.randn(3, Lt, 512, generator=g) * 0.7
        w = (torch.randn(R_, generator=g), torch.randn(3, Lt, generator=g), torch.randn(3, Lt, generator=g))
        dF_ref, g_ref = reference_grads(m_cpu, samples, F, op, sm, *w)
        _refs[key] = (F, w, dF_ref, g_ref, top_two_gaps(m_cpu.state_dict(), F, samples, op).min().item(),
                      conv0_rows(m_cpu.state_dict(), F, samples, op))
    return _refs[key]


@pytest.mark.parametrize('trunk,rtol', [('f32', 2e-4), ('f16x3', 5e-4)])
@pytest.mark.parametrize('op,sm,samples,seed,strict', E2E_CASES)
def test_backward_matches_autograd_through_the_oracle(op, sm, samples, seed, strict, trunk, rtol):
    c, base = get_case('s2_C_multiply_none')
    c = dict(c, aff=op, sm=sm, end_mode='max')
    if any(len(s) > 2 for s in samples):
        c['counts'] = samples[0]
    F, (w_link, w_new, w_end), dF_ref, g_ref, gap, a_ref = e2e_reference(c, base, op, sm, samples, seed)
    m = build_model(c, base, device=DEV)
    m.set_trunk(trunk)
    eng = m.engine()
    assert eng.ops.name == 'hip' and eng.end_mode == 'max'
    plan = BatchPlan([(s, None) for s in samples], 32, DEV, use_points=False)
    assert plan.pair_tiles.R == w_link.numel() and plan.Lt == F.shape[1]
    Fd = F.to(DEV)
    link, new, end, tape = affinity_forward_train(eng, plan, Fd)
    dF, grads = affinity_backward(eng, plan, Fd, tape, w_link.to(DEV), w_new.to(DEV), w_end.to(DEV))
    # the device's error on what the maxima are taken of: relu(Y * sc + sh) of the tape against the float64 restatement
    NE0, PT = tape['aff_ne0'], plan.pair_tiles
    grp = torch.repeat_interleave(torch.arange(PT.G), torch.as_tensor(PT.h_g_count).long())
    a_dev = torch.relu(NE0.Y.cpu().double() * NE0.sc.cpu().double()[grp] + NE0.sh.cpu().double()[grp])
    a_err = (a_dev - a_ref).abs().max().item() / a_ref.max().item()
    print('end-max backward %s/%s %s seed %d %s: smallest top-two gap %.1e, device error on relu(gn(conv0)) %.1e' % (
        op, sm, samples, seed, trunk, gap, a_err))
    if strict:
        assert gap >= 1e-5, gap            # the condition of the strict comparison, measured in float64
        assert 4.0 * a_err <= gap, (a_err, gap)  # ... and the device decides these maxima like float64 does
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

    assert set(grads) == set(g_ref)
    res = {'dF': check('dF', dF, dF_ref)}
    for k, ref in g_ref.items():
        res[k] = check(k, grads[k], ref)
    flipped = [k for k, (_, f) in res.items() if f]
    if strict:
        assert not flipped, flipped
    print('    dF %.1e%s, worst parameter gradient %.1e, second tier used for %d tensors' % (
        res['dF'][0], ' (L2)' if res['dF'][1] else '',
        max(v for k, (v, _) in res.items() if k != 'dF' and g_ref[k].abs().max() > 1e-6 * gmax), len(flipped)))


def test_device_training_step_matches_the_reference_fixture():
    """model.train() forward -> TrackingLoss -> backward with end_mode='max' on the device against the imported
    reference's step (tools/gen_golden_endmax_train.py); the GPU tolerances of tests/test_train_vgg_gpu.py.  Measured:
    scores 1.7e-5, loss 1.5e-6, gradient slices 1.7e-2 and gradient norms 1.8e-2 of the tensor's maximum - both on the
    first trunk layers (appearance.layers.0.*: fp32 noise through 13 batch-normalised layers, the fp32 operator emulation
    on the host gives the same 1.8e-2, and there every tensor outside the image encoder is within 2e-3)."""
    from test_train_vgg_cpu import product_train_step
    name = 'endmax_train_s10_C'
    g, outs, loss, grad_of, buffers = product_train_step(name, device=DEV)
    worst = compare_train_step(g, outs, loss, grad_of, buffers, out_tol=3e-4, loss_tol=1e-4, grad_tol=3e-2, norm_tol=2e-2,
                               bn_tol=5e-5, what=name)
    print('%s: device vs the reference training step: %s' % (name, ' '.join('%s=%.1e' % kv for kv in worst.items())))


def run_two(frames, overlap):
    from mmmot_amd import TrackingNet
    from mmmot_amd.weights import init_module
    torch.manual_seed(21)
    c, base = get_case('s2_C_multiply_none')
    model = TrackingNet(**dict(case_kwargs(dict(c, end_mode='max'), base), dropblock=0, use_dropout=False))
    init_module(model, 0)
    model = model.to(DEV).train()
    assert model.engine().end_mode == 'max'
    losses = make_pipe(model, overlap=overlap).run([sample_of(frames[k:k + 2]) for k in range(2)])
    torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def test_pipeline_overlap_equals_serial_bit_for_bit(frames):
    la, pa = run_two(frames, True)
    lb, pb = run_two(frames, False)
    assert la.shape == (2,) and bool(torch.isfinite(la).all())
    assert torch.equal(bits(la), bits(lb)), (la.tolist(), lb.tolist())
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
