"""One-launch Adam step on the device (csrc/adam_step.hip behind mmmot_amd.optim.Adam):
* every path of the kernel - one element, the tails, one chunk exactly, more than one chunk; bases that are only 4-byte
  aligned and 16-byte aligned ones; both decay modes; a tensor without a gradient; a zero gradient - with p, g, m and v
  between NaN guards, bit-equal when run again and when the tensors are registered in reverse order;
* accuracy against the float64 restatement (tests/optim_ref.RefOptim), measured with torch's own fp32 single-tensor Adam
  on the CPU as the yardstick: the device within 4 x the yardstick's deviation + 2^-24 x the tensor's largest value;
* torch.optim.Adam on the device under the restated wrapper, and state_dict interchange in both directions mid-run;
* one training step of the whole TrackingNet: build_optim's wrapper step against the restated wrapper over
  torch.optim.Adam, compared through the eval forward that follows (the re-pack must see the new weights)."""
import copy

import numpy as np
import pytest
import torch

import optim_ref
from mmmot_amd import optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OPS = None  # the product backend (HipOps)
GUARD = 8  # elements; a multiple of 4, so a view behind it is 16-byte aligned and one element further is not
WD = 0.1
STEPS = 5
NONE_AT = (2, 3)  # tensor 2 has no gradient at step 3
ZERO_GRAD = 3     # tensor 3's gradient is zero at every step


def sizes():
    C = optim.chunk_elems()
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]


def hyper(it):
    return optim_ref.one_cycle(3 * it + 2, **optim_ref.SCHEDULE)  # crosses from the first phase into the second


@pytest.fixture(scope='module')
def master():
    """Start values and the gradients of every step (fp32, CPU); made once, never changed."""
    g = torch.Generator().manual_seed(5)
    ns = sizes()
    p0 = [torch.randn(n, generator=g) * 0.5 for n in ns]
    grads = [[torch.zeros(n) if i == ZERO_GRAD else torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 1, (1,), generator=g))
              for i, n in enumerate(ns)] for _ in range(STEPS)]
    return p0, grads


def guarded(n, aligned, dev):
    buf = torch.full((n + 2 * GUARD + 4,), float('nan'), device=dev)
    o = GUARD + (0 if aligned else 1)
    view = buf[o:o + n]
    assert (view.data_ptr() % 16 == 0) == aligned
    return buf, o, view


def guards_intact(buf, o, n):
    return bool(torch.isnan(buf[:o]).all() and torch.isnan(buf[o + n:]).all() and not torch.isnan(buf[o:o + n]).any())


class Run:
    """The master tensors on ``dev`` - each p, g, m, v a view between NaN guards - split into two parameter groups."""

    def __init__(self, master, aligned=True, dev=None):
        dev = dev or DEV
        self.master, self.dev = master, dev
        self.bufs, self.p, self.g, self.m, self.v = [], [], [], [], []
        for p0 in master[0]:
            n = p0.numel()
            quad = [guarded(n, aligned, dev) for _ in range(4)]
            self.bufs.append((n, quad))
            quad[0][2].copy_(p0)
            quad[2][2].zero_()
            quad[3][2].zero_()
            self.p.append(torch.nn.Parameter(quad[0][2]))
            self.g.append(quad[1][2])
            self.m.append(quad[2][2])
            self.v.append(quad[3][2])
        half = len(self.p) // 2
        self.groups = [list(range(half)), list(range(half, len(self.p)))]

    def set_grads(self, it):
        for i, p in enumerate(self.p):
            if (i, it) == NONE_AT:
                p.grad = None
            else:
                self.g[i].copy_(self.master[1][it][i])
                p.grad = self.g[i]

    def ours(self, order=1, guarded_state=True):
        opt = optim.Adam([{'params': [self.p[i] for i in g[::order]]} for g in self.groups[::order]], lr=1e-3,
                         betas=optim_ref.BETAS, eps=optim_ref.EPS, ops=OPS)
        if guarded_state:  # exp_avg / exp_avg_sq between guards too: the state as the optimizer would have made it
            for i, p in enumerate(self.p):
                opt.state[p] = {'step': 0, 'exp_avg': self.m[i], 'exp_avg_sq': self.v[i]}
        return opt

    def step_ours(self, opt, it, true_wd):
        lr, mom = hyper(it)
        for g in opt.param_groups:
            g['lr'], g['betas'], g['weight_decay'] = lr, (mom, optim_ref.BETAS[1]), 0 if true_wd else WD
        self.set_grads(it)
        opt.step(decay=[1 - WD * lr] * len(opt.param_groups) if true_wd else None)

    def torch_wrapper(self, true_wd):
        return optim_ref.TorchWrapper([[self.p[i] for i in g] for g in self.groups], WD, true_wd, True)

    def step_torch(self, w, it):
        self.set_grads(it)
        w.step(*hyper(it))

    def check_guards(self):
        torch.cuda.synchronize()  # raises on a HIP error of the launches before it
        for n, quad in self.bufs:
            for what, (buf, o, _) in zip('pgmv', quad):
                assert guards_intact(buf, o, n), '%s of the tensor of %d elements: written outside, or NaN inside' % (what, n)

    def values(self, opt=None):
        if opt is None:
            return [[t.detach().cpu().clone() for t in (self.p[i], self.m[i], self.v[i])] for i in range(len(self.p))]
        st = opt.state
        return [[p.detach().cpu().clone(), st[p]['exp_avg'].cpu().clone(), st[p]['exp_avg_sq'].cpu().clone()] for p in self.p]


def run_ours(master, aligned, true_wd, order=1):
    r = Run(master, aligned)
    opt = r.ours(order)
    for it in range(STEPS):
        r.step_ours(opt, it, true_wd)
    r.check_guards()
    assert [opt.state[p]['step'] for p in r.p] == [STEPS - 1 if i == NONE_AT[0] else STEPS for i in range(len(r.p))]
    return r.values()


@pytest.mark.parametrize('aligned', [False, True])
@pytest.mark.parametrize('true_wd', [True, False])
def test_shapes_guards_and_determinism(master, aligned, true_wd):
    a = run_ours(master, aligned, true_wd)
    b = run_ours(master, aligned, true_wd)
    c = run_ours(master, aligned, true_wd, order=-1)
    for i, (x, y, z) in enumerate(zip(a, b, c)):
        for k, what in enumerate('pmv'):
            assert torch.equal(x[k], y[k]), 'a second run differs: %s of tensor %d' % (what, i)
            assert torch.equal(x[k], z[k]), 'reverse registration differs: %s of tensor %d' % (what, i)
    assert not torch.equal(a[0][0], master[0][0])
    if true_wd:  # a zero gradient moves nothing but the decay: m and v stay zero, the update term is 0 / eps = 0
        assert not a[ZERO_GRAD][1].any() and not a[ZERO_GRAD][2].any()
        assert (a[ZERO_GRAD][0].abs() < master[0][ZERO_GRAD].abs()).all()
    else:        # added to the gradient, the decay reaches m and v
        assert a[ZERO_GRAD][1].any() and a[ZERO_GRAD][2].any()


def reference_runs(master, true_wd):
    """Per step [(p, m, v) float64 per tensor] of the float64 restatement, and of torch's fp32 CPU Adam under the restated
    wrapper (the yardstick)."""
    n = len(master[0])
    names = [str(i) for i in range(n)]
    half = n // 2
    params = {k: master[0][int(k)].double().numpy().copy() for k in names}
    ref = optim_ref.RefOptim(params, [names[:half], names[half:]], WD, true_wd, True)
    cpu = Run(master, True, 'cpu')
    w = cpu.torch_wrapper(true_wd)
    out64, out32 = [], []
    for it in range(STEPS):
        lr, mom = hyper(it)
        ref.step({k: (None if (int(k), it) == NONE_AT else master[1][it][int(k)].double().numpy()) for k in names}, lr, mom)
        out64.append([[params[k].copy(), ref.m[k].copy(), ref.v[k].copy()] for k in names])
        cpu.step_torch(w, it)
        st = w.opt.state
        out32.append([[p.detach().double().numpy().copy()] + [st[p][k].double().numpy().copy() for k in ('exp_avg', 'exp_avg_sq')]
                      for p in cpu.p])
    return out64, out32


def bounds(out64, out32):
    """4 x the yardstick's deviation from float64 + 2^-24 x the tensor's largest float64 value; per step, tensor, p/m/v."""
    return [[[4 * np.abs(b - a).max() + 2.0 ** -24 * np.abs(a).max() for a, b in zip(t64, t32)] for t64, t32 in zip(s64, s32)]
            for s64, s32 in zip(out64, out32)]


@pytest.fixture(scope='module')
def references(master):
    return {tw: reference_runs(master, tw) for tw in (True, False)}


@pytest.mark.parametrize('aligned', [False, True])
@pytest.mark.parametrize('true_wd', [True, False])
def test_accuracy_against_float64(master, references, aligned, true_wd):
    out64, out32 = references[true_wd]
    bnd = bounds(out64, out32)
    r = Run(master, aligned)
    opt = r.ours()
    worst_dev, worst_cpu, worst_ratio, bad = [0.0] * 3, [0.0] * 3, 0.0, []
    for it in range(STEPS):
        r.step_ours(opt, it, true_wd)
        got = r.values()
        for i in range(len(r.p)):
            for k, what in enumerate('pmv'):
                a = out64[it][i][k]
                scale = max(np.abs(a).max(), 1e-30)
                dev = np.abs(got[i][k].double().numpy() - a).max()
                cpu = np.abs(out32[it][i][k] - a).max()
                worst_dev[k], worst_cpu[k] = max(worst_dev[k], dev / scale), max(worst_cpu[k], cpu / scale)
                if bnd[it][i][k] > 0:
                    worst_ratio = max(worst_ratio, dev / bnd[it][i][k])
                if not dev <= bnd[it][i][k]:
                    bad.append((it, i, what, dev, bnd[it][i][k]))
    # printed before anything is asserted, so that a failure still shows the figures
    print('adam_step %s %s: worst deviation from float64 relative to the tensor\'s largest value, p / m / v: device '
          '%.2e / %.2e / %.2e, torch fp32 on the CPU %.2e / %.2e / %.2e; worst device deviation / bound %.3f' % (
              'aligned' if aligned else 'unaligned', 'true_wd' if true_wd else 'l2', *worst_dev, *worst_cpu, worst_ratio))
    r.check_guards()
    assert not bad, bad[:8]


@pytest.mark.parametrize('true_wd', [True, False])
def test_torch_adam_on_the_device_and_state_interchange(master, references, true_wd):
    bnd = bounds(*references[true_wd])

    def close(got, want, it, what):
        for i in range(len(want)):
            for k, name in enumerate('pmv'):
                d = (got[i][k].double() - want[i][k].double()).abs().max().item()
                assert d <= bnd[it][i][k], (what, it, i, name, d, bnd[it][i][k])

    # uninterrupted, ours (the optimizer's own flat state here) - and torch.optim.Adam on the device beside it
    a, b = Run(master, True), Run(master, True)
    ours, theirs = a.ours(guarded_state=False), b.torch_wrapper(true_wd)
    mid = None
    for it in range(STEPS):
        a.step_ours(ours, it, true_wd)
        b.step_torch(theirs, it)
        close(b.values(theirs.opt), a.values(ours), it, 'torch.optim.Adam on the device')
        if it == 2:
            mid = (copy.deepcopy(ours.state_dict()), copy.deepcopy(theirs.opt.state_dict()),  # the dicts hold the live tensors
                   [p.detach().clone() for p in a.p], [p.detach().clone() for p in b.p])
    final = a.values(ours)
    torch.cuda.synchronize()
    # ours -> torch: a fresh torch.optim.Adam loads our dict at step 3 and goes on
    c = Run(master, True)
    with torch.no_grad():
        for p, x in zip(c.p, mid[2]):
            p.copy_(x)
    w = c.torch_wrapper(true_wd)
    w.opt.load_state_dict(mid[0])
    for it in range(3, STEPS):
        c.step_torch(w, it)
    close(c.values(w.opt), final, STEPS - 1, 'ours -> torch')
    # torch -> ours
    d = Run(master, True)
    with torch.no_grad():
        for p, x in zip(d.p, mid[3]):
            p.copy_(x)
    opt = d.ours(guarded_state=False)
    opt.load_state_dict(mid[1])
    for it in range(3, STEPS):
        d.step_ours(opt, it, true_wd)
    close(d.values(opt), final, STEPS - 1, 'torch -> ours')
    d.check_guards()


def test_whole_model_step_matches_torch_adam_through_the_next_forward():
    from common import build_model, case_inputs, get_case
    from mmmot_amd import TrackingLoss
    from test_train_cpu import make_gts
    c, base = get_case('s2_C_multiply_none')
    dets, info, ds = case_inputs(c)
    counts = [int(x) for x in ds]
    gts = make_gts(counts, 11)
    dinfo = {k: v.to(DEV) for k, v in info.items()}
    ma, mb = build_model(c, base, device=DEV), build_model(c, base, device=DEV)
    ma.freeze_appearance = True
    ma.train()
    crit = TrackingLoss(detloss_type='bce', linkloss_type='l2', det_ratio=1.5, trans_ratio=0.001)
    det, links, new, end, trans = ma(dets.to(DEV), dinfo, ds)
    dg = lambda x: [t.to(DEV) for t in x] if isinstance(x, list) else x.to(DEV)
    crit(ds, dg(gts[0]), dg(gts[1]), dg(gts[2]), dg(gts[3]), det, links, new, end, trans).backward()
    cfg = dict(lr_scheduler=dict(optim='Adam', base_lr=optim_ref.BASE_LR), weight_decay=optim_ref.WD, fixed_wd=True)
    w = optim.build_optim(ma, cfg)
    names = {id(p): k for k, p in ma.named_parameters()}
    pb = dict(mb.named_parameters())
    n_grads = 0
    for k, p in ma.named_parameters():
        if p.grad is not None:
            pb[k].grad = p.grad.clone()
            n_grads += 1
    assert n_grads >= 76
    tw = optim_ref.TorchWrapper([[pb[names[id(p)]] for p in g['params']] for g in w.opt.param_groups], optim_ref.WD, True, True)
    with torch.no_grad():  # the training forward moved the running statistics of A's BatchNorms: B gets the same ones
        bb = dict(mb.named_buffers())
        for k, b in ma.named_buffers():
            bb[k].copy_(b)
    # the scores BEFORE the step are taken here, after the training forward and backward: the running statistics the
    # forward moved are already in them, so what changes them below is the optimizer step and nothing else
    ma.eval()
    with torch.no_grad():
        before = ma(dets.to(DEV), dinfo, ds)
        before = [before[0].clone(), before[1][0].clone(), before[2].clone(), before[3].clone()]
    assert ma.head_is_current()
    w.step()
    assert not ma.head_is_current()  # the step's version counters, not the BatchNorm update, made it stale
    tw.step(optim_ref.BASE_LR, optim_ref.BETAS[0])
    torch.cuda.synchronize()
    assert w.opt._ops().name == 'hip'
    worst = max((p.detach() - pb[k].detach()).abs().max().item() for k, p in ma.named_parameters())
    ma.eval()
    with torch.no_grad():
        oa, ob = ma(dets.to(DEV), dinfo, ds), mb(dets.to(DEV), dinfo, ds)
    torch.cuda.synchronize()
    flat = lambda o: [o[0], o[1][0], o[2], o[3]]
    diff = max((x - y).abs().max().item() for x, y in zip(flat(oa), flat(ob)))
    moved = max((x - y).abs().max().item() for x, y in zip(flat(oa), before))
    print('whole model: worst parameter difference to torch.optim.Adam %.2e; scores after the step differ by %.2e between '
          'the two optimizers and by %.2e from the scores before it' % (worst, diff, moved))
    assert diff < 1e-3
    assert moved > 0 and not any(torch.equal(x, y) for x, y in zip(flat(oa)[:2], before[:2]))
