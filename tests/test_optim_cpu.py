"""Optimizer step without a GPU (mmmot_amd/optim.py): the wrapper, the schedule and the grouping against the fixture made
by running the reference's own wrapper over torch.optim.Adam (tests/golden/optim_adam.npz, tools/gen_golden_optim.py),
``optim.Adam`` through the emulation of the kernel (tests/optim_ref.EmuOps), state interchange with torch.optim.Adam, the
version counters, the launcher's argument checks and the refusals."""
import ctypes
import types

import numpy as np
import pytest
import torch

import optim_ref
from mmmot_amd import TrackingNet, _lib, optim

SMOKE_KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True,
                appear_fpn=False, point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2',
                end_mode='avg', test_mode=2, neg_threshold=0.2, dropblock=0, use_dropout=False,
                score_fusion_arch='C', affinity_op='minus_abs', softmax_mode='dual_add')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(optim_ref.GOLDEN))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def train_cfg(true_wd=True, optim_name='Adam'):
    return dict(lr_scheduler=dict(optim=optim_name, base_lr=optim_ref.BASE_LR), weight_decay=optim_ref.WD, fixed_wd=true_wd)


def build_case(gold, true_wd, bn_wd, dtype=torch.float64):
    """The fixture's tree under optim.OptimWrapper over optim.Adam on the emulation, and its OneCycle."""
    net = optim_ref.make_tree({k: gold['init/' + k] for k in gold['names']}, dtype)
    emu = optim_ref.EmuOps(dtype)
    if bn_wd:
        w = optim.build_optim(net, train_cfg(true_wd), ops=emu)
    else:
        import functools
        w = optim.OptimWrapper.create(functools.partial(optim.Adam, betas=optim_ref.BETAS, ops=emu), optim_ref.BASE_LR,
                                      optim.get_layer_groups(net), wd=optim_ref.WD, true_wd=true_wd, bn_wd=False)
    S = optim_ref.SCHEDULE
    sched = optim.OneCycle(w, S['total_step'], S['lr_max'], list(S['moms']), S['div_factor'], S['pct_start'])
    return net, w, sched, emu


@pytest.mark.parametrize('true_wd,bn_wd', optim_ref.CASES)
def test_float64_restatement_reproduces_the_fixture(gold, true_wd, bn_wd):
    c = optim_ref.case_name(true_wd, bn_wd)
    names = list(gold['names'])
    params = {k: gold['init/' + k].copy() for k in names}
    ref = optim_ref.RefOptim(params, [list(gold['group0/' + c]), list(gold['group1/' + c])], optim_ref.WD, true_wd, bn_wd)
    worst = 0.0
    for it in range(optim_ref.SCHEDULE['total_step']):
        lr, mom = optim_ref.one_cycle(it, **optim_ref.SCHEDULE)
        grads = {k: (None if (k, it) == optim_ref.NONE_GRAD else gold['grad/' + k][it]) for k in names}
        ref.step(grads, lr, mom)
        for k in names:
            worst = max(worst, rel(params[k], gold['param/%s/%s' % (c, k)][it]))
    print('%s: worst relative difference of optim_ref from the fixture %.1e' % (c, worst))
    assert worst < 1e-12
    assert not np.array_equal(params['stem.0.weight'], gold['init/stem.0.weight'])
    assert np.array_equal(params['block.scale'], gold['init/block.scale'])  # a parent's own parameter: in no group


@pytest.mark.parametrize('true_wd,bn_wd', optim_ref.CASES)
def test_one_cycle_and_grouping_match_the_fixture(gold, true_wd, bn_wd):
    c = optim_ref.case_name(true_wd, bn_wd)
    net, w, sched, _ = build_case(gold, true_wd, bn_wd)
    by_id = {id(p): k for k, p in net.named_parameters()}
    groups = [[by_id[id(p)] for p in g['params']] for g in w.opt.param_groups]
    assert groups == [list(gold['group0/' + c]), list(gold['group1/' + c])]
    assert 'block.scale' not in sum(groups, []) and 'frozen.weight' not in sum(groups, [])
    assert 'block.norm.weight' in groups[0]  # LayerNorm counts as a non-norm leaf
    for it in range(optim_ref.SCHEDULE['total_step']):
        sched.step(it)
        assert abs(w.lr - gold['lr/' + c][it]) <= 1e-15 * gold['lr/' + c][it]
        assert abs(w.mom - gold['mom/' + c][it]) <= 1e-15 * gold['mom/' + c][it]
        assert optim_ref.one_cycle(it, **optim_ref.SCHEDULE) == (w.lr, w.mom)
        for g in w.opt.param_groups:
            assert g['lr'] == w.lr and g['betas'] == (w.mom, optim_ref.BETAS[1])


def test_grouping_of_the_full_model():
    net = TrackingNet(**SMOKE_KW)
    w = optim.build_optim(net, train_cfg(), ops=types.SimpleNamespace(name='none'))
    g = w.opt.param_groups
    assert [len(x['params']) for x in g] == [110, 106]
    ids = [id(p) for x in g for p in x['params']]
    assert len(set(ids)) == 216
    assert set(ids) == {id(p) for p in net.parameters() if p.requires_grad}
    idt = [p for k, p in net.named_parameters() if k.endswith('.idt')]
    assert len(idt) == 2 and not any(id(p) in ids for p in idt)
    assert w.true_wd and w.wd == optim_ref.WD and w.beta == 0.99 and w.mom == 0.9 and w.lr == optim_ref.BASE_LR


@pytest.mark.parametrize('true_wd,bn_wd', optim_ref.CASES)
def test_adam_through_the_emulation_follows_the_fixture(gold, true_wd, bn_wd):
    c = optim_ref.case_name(true_wd, bn_wd)
    net, w, sched, emu = build_case(gold, true_wd, bn_wd)
    worst = 0.0
    for it in range(optim_ref.SCHEDULE['total_step']):
        sched.step(it)
        w.zero_grad()
        for k, p in net.named_parameters():
            if p.requires_grad:
                p.grad = None if (k, it) == optim_ref.NONE_GRAD else torch.from_numpy(gold['grad/' + k][it].copy())
        w.step()
        for k, p in net.named_parameters():
            worst = max(worst, rel(p.detach().numpy(), gold['param/%s/%s' % (c, k)][it]))
    print('%s: worst relative difference of optim.Adam (float64 emulation) from the fixture %.1e' % (c, worst))
    assert worst < 1e-12
    assert emu.calls == optim_ref.SCHEDULE['total_step']  # one launch a step, the decay inside it: no loop of mul_
    sd = w.state_dict()
    order = [i for g in sd['param_groups'] for i in g['params']]
    steps = [int(sd['state'][i]['step']) if i in sd['state'] else -1 for i in order]
    assert steps == gold['steps/' + c].tolist()
    assert all(torch.is_tensor(s['step']) and s['step'].dim() == 0 for s in sd['state'].values())


def _interchange_tree(gold):
    net = optim_ref.make_tree({k: gold['init/' + k] for k in gold['names']})
    groups = [[p for k, p in net.named_parameters() if k in set(gold['group%d/tw0_bn1' % i])] for i in (0, 1)]
    return net, groups


def _drive(gold, net, opt, its, hyper):
    for it in its:
        lr, mom = optim_ref.one_cycle(it, **optim_ref.SCHEDULE)
        for g in opt.param_groups:
            g['lr'], g['betas'], g['weight_decay'] = lr, (mom, optim_ref.BETAS[1]), hyper
        for k, p in net.named_parameters():
            p.grad = torch.from_numpy(gold['grad/' + k][it].copy()) if p.requires_grad else None
        opt.step()


@pytest.mark.parametrize('int_step', [False, True])
def test_state_interchange_with_torch_adam(gold, int_step):
    mk_ours = lambda groups: optim.Adam([{'params': g} for g in groups], lr=1e-3, betas=optim_ref.BETAS,
                                        ops=optim_ref.EmuOps(torch.float64))
    mk_torch = lambda groups: torch.optim.Adam([{'params': g} for g in groups], lr=1e-3, betas=optim_ref.BETAS)
    first, rest = range(0, 3), range(3, 6)
    net_u, g_u = _interchange_tree(gold)  # uninterrupted: torch all the way
    _drive(gold, net_u, mk_torch(g_u), range(0, 6), 0.01)
    want = {k: p.detach().numpy() for k, p in net_u.named_parameters()}

    # ours -> torch
    net_a, g_a = _interchange_tree(gold)
    ours = mk_ours(g_a)
    _drive(gold, net_a, ours, first, 0.01)
    theirs = mk_torch(g_a)
    theirs.load_state_dict(ours.state_dict())
    _drive(gold, net_a, theirs, rest, 0.01)
    # torch -> ours, with step as torch writes it (a tensor) or as checkpoints of the reference's era have it (an int)
    net_b, g_b = _interchange_tree(gold)
    theirs = mk_torch(g_b)
    _drive(gold, net_b, theirs, first, 0.01)
    sd = theirs.state_dict()
    if int_step:
        for st in sd['state'].values():
            st['step'] = int(st['step'])
    ours = mk_ours(g_b)
    ours.load_state_dict(sd)
    assert all(type(st['step']) is int and st['step'] == 3 for st in ours.state.values())
    _drive(gold, net_b, ours, rest, 0.01)
    for k in want:
        assert rel(net_a.state_dict()[k].numpy(), want[k]) < 1e-12, k
        assert rel(net_b.state_dict()[k].numpy(), want[k]) < 1e-12, k
    assert not np.array_equal(want['head.bias'], gold['init/head.bias'])


def test_step_advances_the_version_of_what_it_wrote(gold):
    net, w, sched, _ = build_case(gold, True, True, torch.float32)
    sched.step(0)
    for k, p in net.named_parameters():
        p.grad = None if k == 'head.weight' or not p.requires_grad else torch.from_numpy(gold['grad/' + k][0]).float()
    before = {k: p._version for k, p in net.named_parameters()}
    values = {k: p.detach().clone() for k, p in net.named_parameters()}
    w.step()
    grouped = set(gold['group0/tw1_bn1']) | set(gold['group1/tw1_bn1'])
    for k, p in net.named_parameters():
        if k in grouped:  # written: head.weight by the decay alone
            assert p._version > before[k], k
            assert not torch.equal(p.detach(), values[k]), k
        else:  # frozen.weight (requires_grad=False), block.scale (in no group)
            assert p._version == before[k] and torch.equal(p.detach(), values[k]), k
    # without decoupled decay a parameter without a gradient is not written and keeps its version
    net, w, sched, _ = build_case(gold, False, True, torch.float32)
    sched.step(0)
    for k, p in net.named_parameters():
        p.grad = None if k == 'head.weight' or not p.requires_grad else torch.from_numpy(gold['grad/' + k][0]).float()
    v0 = net.head.weight._version
    w.step()
    assert net.head.weight._version == v0 and net.head.bias._version > 0


def test_a_wrapper_step_makes_the_packed_head_stale():
    from common import build_model, get_case
    from fake_ops import TorchOps
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    m.engine()
    assert m.head_is_current()
    w = optim.build_optim(m, train_cfg(), ops=optim_ref.EmuOps(torch.float32))
    for p in m.w_link.parameters():
        p.grad = torch.full_like(p, 1e-3)
    before = m.w_link.conv1[3].weight.detach().clone()
    w.step()
    assert not torch.equal(m.w_link.conv1[3].weight.detach(), before)
    assert not m.head_is_current()
    assert m.refresh_head() is m.engine() and m.head_is_current()


def test_symbol_abi_and_argument_checks_without_gpu():
    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'mmmot_adam_step')
    assert lib.mmmot_abi_version() == 10
    assert lib.mmmot_adam_chunk_elems() == optim.chunk_elems() == 4096
    from mmmot_amd import torch_ops
    assert torch_ops.ADAM_ROW.itemsize == 64
    d = 4096  # never dereferenced: the argument checks come before any launch
    ok = (0.9, 0.99, 1e-8)
    assert lib.mmmot_adam_step(None, 1, d, 1, *ok, None) == -1      # null tensor table
    assert lib.mmmot_adam_step(d, 1, None, 1, *ok, None) == -1      # null chunk table
    for T, n in [(0, 1), (-1, 1), (1, 0), (1, -5), (-2 ** 31, 1)]:
        assert lib.mmmot_adam_step(d, T, d, n, *ok, None) == -1     # zero or negative counts with non-null work
    for b in (-0.1, 1.0, 1.5, float('nan'), float('inf')):
        assert lib.mmmot_adam_step(d, 1, d, 1, b, 0.99, 1e-8, None) == -1
        assert lib.mmmot_adam_step(d, 1, d, 1, 0.9, b, 1e-8, None) == -1
    for e in (-1e-8, float('nan'), -float('inf')):
        assert lib.mmmot_adam_step(d, 1, d, 1, 0.9, 0.99, e, None) == -1
    # the host-side chunk table
    C = optim.chunk_elems()
    sizes = [1, C - 1, C, C + 1, 2 * C + 3]
    t = optim._chunk_table(sizes)
    assert t.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2]]
    with pytest.raises(RuntimeError, match='MMMOT_EINVAL'):
        optim._chunk_table([4, 0])


def test_refusals(gold):
    p = torch.nn.Parameter(torch.zeros(4))
    emu = optim_ref.EmuOps(torch.float32)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(foreach=True), dict(foreach=False)):
        with pytest.raises(ValueError):
            optim.Adam([p], lr=1e-3, ops=emu, **kw)
    with pytest.raises(ValueError):  # not fp32
        optim.Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=1e-3, ops=emu)
    with pytest.raises(ValueError):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))], lr=1e-3, ops=emu)
    with pytest.raises(ValueError):  # not contiguous
        optim.Adam([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=1e-3, ops=emu)
    with pytest.raises(ValueError):  # two devices
        optim.Adam([p, torch.nn.Parameter(torch.zeros(4, device='meta'))], lr=1e-3, ops=emu)
    with pytest.raises(ValueError):  # one tensor in two groups
        optim.Adam([{'params': [p]}, {'params': [p]}], lr=1e-3, ops=emu)
    for b in ((1.0, 0.9), (0.9, -0.1)):
        with pytest.raises(ValueError):
            optim.Adam([p], lr=1e-3, betas=b, ops=emu)
    opt = optim.Adam([p], lr=1e-3, ops=emu)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, device='meta'), torch.zeros(4, 2)[:, 0]):
        p.grad = None
        try:
            p.grad = bad
        except (RuntimeError, TypeError):
            continue  # torch itself refuses to attach such a gradient
        with pytest.raises(ValueError):
            opt.step()
    p.grad = None
    sd = opt.state_dict()
    sd['param_groups'][0]['amsgrad'] = True
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
    with pytest.raises(NotImplementedError):
        optim.build_optim(optim_ref.make_tree(), train_cfg(optim_name='AdaBound'))
    # any other inner optimizer: the wrapper does the decay loop itself
    net = optim_ref.make_tree({k: gold['init/' + k] for k in gold['names']})
    import functools
    w = optim.OptimWrapper.create(functools.partial(torch.optim.Adam, betas=optim_ref.BETAS), 1e-3,
                                  optim.get_layer_groups(net), wd=0.5, true_wd=True, bn_wd=True)
    w.step()  # no gradients: the decay alone
    assert rel(net.head.bias.detach().numpy(), gold['init/head.bias'] * (1 - 0.5 * 1e-3)) < 1e-15
    assert np.array_equal(net.block.scale.detach().numpy(), gold['init/block.scale'])


def test_a_refused_step_changes_nothing_and_replaced_storage_is_noticed(gold):
    emu = optim_ref.EmuOps(torch.float32)
    a, b = torch.nn.Parameter(torch.ones(6)), torch.nn.Parameter(torch.ones(5))
    opt = optim.Adam([a, b], lr=1e-2, ops=emu)
    a.grad, b.grad = torch.ones(6), torch.ones(5)
    opt.step()
    assert [opt.state[p]['step'] for p in (a, b)] == [1, 1] and emu.calls == 1
    # the SECOND tensor's gradient is refused: the first one's step count has not moved, nothing was launched
    b.grad = torch.ones(5, 2)[:, 0]
    va, values = a._version, a.detach().clone()
    with pytest.raises(ValueError):
        opt.step()
    assert [opt.state[p]['step'] for p in (a, b)] == [1, 1] and emu.calls == 1
    assert a._version == va and torch.equal(a.detach(), values)
    # a parameter whose storage was replaced under the same object (what module.half() does) is checked again
    b.grad = None
    b.data = torch.ones(5, dtype=torch.float16)
    with pytest.raises(ValueError):
        opt.step()
    b.data = torch.ones(3)  # another length without a gradient, decay alone: the row carries the new length
    seen = {}
    emu.adam_step = lambda ch, ptrs, scal, *k: seen.update(numel=ptrs[:, 4].tolist(), chunks=ch.tolist())
    a.grad = None
    opt.step(decay=[0.5])
    assert seen['numel'] == [6, 3]
