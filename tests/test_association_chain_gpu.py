"""The device chain association (csrc/assign_chain.hip through mmmot::associate_chains / mmmot_amd.association) against
the host oracle of tests/association_chain_ref.py: the exact assignment on continuous scores, a path that has to be
undone through a backward residual edge, the optimum on tied scores, agreement with the frame-pair kernel at T = 2,
determinism over batch position and kernel variant, outputs written in full over poisoned memory, the ``gt=`` objective,
the ortools_solve-shaped drop-in with host and device inputs and a real three-frame forward."""
import os

import numpy as np
import pytest
import torch

import association_ref as pair_ref
from association_chain_ref import feasible, lp_route, milp_route, objective, random_chain, same_assignment
from mmmot_amd import _lib
from mmmot_amd.association import (associate_chain, associate_chain_batch, chain_block_size, chains_table, pairs_table,
                                   select_chain, unpack, unpack_chain)
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import associate_layout, chain_layout

pytestmark = pytest.mark.gpu

KINDS = ('normal', 'eval', 'masked')
# 2L + 1 nodes within one wave ([1,1,1] .. [2]*8), beyond it, and L = 127 | 128 on either side of the size at which the
# automatic choice goes from the one-wave to the four-wave kernel (2L + 1 <= 256)
SPLITS = ([1, 1, 1], [3, 4, 5], [5, 1, 7], [12, 0, 12], [12, 12, 12, 12], [2] * 8, [33, 31, 34], [64, 70, 64],
          [42, 43, 42], [43, 42, 43])
_OPS = []


def ops():
    if not _OPS:
        _OPS.append(HipOps())
    return _OPS[0]


def set_variant(v):
    assert _lib.load().mmmot_set_chain_variant(v) == 0


def solve(insts, variant=0, fill=None):
    """one launch over [(split, (det, new, end, links)) ...] -> [(det, [link ...], new, end) numpy], objective [B]"""
    splits = [list(s) for s, _ in insts]
    chains, offs = chains_table(splits)
    f32 = lambda x: np.asarray(x, np.float32).reshape(-1)
    cat = lambda k: torch.from_numpy(np.concatenate([f32(sc[k]) for _, sc in insts])).cuda()
    det, new, end = cat(0), cat(1), cat(2)
    link = torch.from_numpy(np.concatenate([f32(l) for _, sc in insts for l in sc[3]] + [np.zeros(1, np.float32)])).cuda()
    total, off, max_n, max_L = chain_layout(chains, det.numel(), link.numel())
    B = len(insts)
    table = torch.cat([chains.reshape(-1), off.to(torch.int32)]).cuda()
    out = torch.empty(total, dtype=torch.float32, device='cuda')
    obj = torch.empty(B, dtype=torch.float64, device='cuda')
    if fill is not None:
        out.view(torch.uint8).fill_(fill)
        obj.view(torch.uint8).fill_(fill)
    set_variant(variant)
    try:
        ops().associate_chains(det, new, end, link, table[:11 * B], B, max_n, max_L, out, table[11 * B:], obj)
        torch.cuda.synchronize()
    finally:
        set_variant(0)
    out, obj = out.cpu(), obj.cpu().numpy()
    res = []
    for s, o in zip(splits, offs):
        d, lk, n, e = unpack_chain(out[o:o + chain_block_size(s)], s)
        res.append((d.numpy(), [x[0].numpy() for x in lk], n.numpy(), e.numpy()))
    return res, obj


def same(a, b):
    return all(same_assignment(x, y) for x, y in zip(a, b))


def check_exact(inst, got, obj, want, wobj):
    split, (det, new, end, links) = inst
    assert feasible(got, split), split
    assert same_assignment(got, want), split
    assert abs(obj - wobj) <= 1e-9 * max(1.0, abs(wobj)), (split, obj, wobj)
    assert abs(objective(got, det, new, end, links) - wobj) <= 1e-9 * max(1.0, abs(wobj))


_RANDOM = {}


def random_cases(kind):
    """40 seeds of one kind, seed k on SPLITS[k % 10] at scale (1, 10, 1e4)[k % 3], with both oracle routes: computed
    once.  The seeds were picked on the host so that the two routes return the same assignment (no tied optimum)."""
    if kind not in _RANDOM:
        cases = []
        for k in range(40):
            split = SPLITS[k % len(SPLITS)]
            rng = np.random.default_rng(1000 * KINDS.index(kind) + k)
            sc = random_chain(rng, split, (1.0, 10.0, 1e4)[k % 3], kind)
            a, oa = lp_route(sc[0], sc[1], sc[2], sc[3], split)
            b, ob = milp_route(sc[0], sc[1], sc[2], sc[3], split)
            cases.append(((split, sc), a, oa, same_assignment(a, b) and abs(oa - ob) <= 1e-12 * max(1.0, abs(oa))))
        _RANDOM[kind] = cases
    return _RANDOM[kind]


@pytest.mark.parametrize('kind', KINDS)
def test_random_scores_match_the_oracle_exactly(kind):
    cases = random_cases(kind)
    skipped = sum(1 for c in cases if not c[3])
    assert skipped == 0, 'instances with a tied optimum: %d' % skipped
    # per split one launch of its own, so that the automatic choice of the kernel follows the split's size
    auto = [None] * len(cases)
    for split in SPLITS:
        idx = [k for k, c in enumerate(cases) if c[0][0] == split]
        res, obj = solve([cases[k][0] for k in idx])
        for k, r, o in zip(idx, res, obj):
            check_exact(cases[k][0], r, o, cases[k][1], cases[k][2])
            auto[k] = (r, o)
    # the same bits from either kernel, all in one launch
    for v in (1, 2):
        res, obj = solve([c[0] for c in cases], v)
        assert same(res, [a[0] for a in auto]) and np.array_equal(obj, np.array([a[1] for a in auto])), v


def test_first_path_is_rerouted_through_a_backward_edge():
    """Three frames [1, 2, 1].  The cheapest first path is a0 -> b0 -> c0 (links 10 and 10).  The optimum keeps two
    trajectories, a0 -> b1 -> c0 and b0 alone: b0 has to leave the first path.  The second augmentation enters in(b0) from
    the source, walks the link a0 -> b0 backwards to out(a0), goes on to b1 and in(c0), walks the link b0 -> c0 backwards
    to out(b0) and ends there."""
    split = [1, 2, 1]
    det = np.array([1, 1, 1, 1], np.float32)
    new = np.array([0, 3, -9, -9], np.float32)      # b0 may start a trajectory of its own at a gain
    end = np.array([-9, 6, -9, 0], np.float32)      # and end one
    links = [np.array([[10, 9]], np.float32), np.array([[10], [9.5]], np.float32)]
    want, wobj = milp_route(det, new, end, links, split)
    # first path alone: 0 + 1 + 10 + 1 + 10 + 1 + 0 = 23; the optimum: a0 -> b1 -> c0 (21.5) plus b0 alone (10) = 31.5
    assert wobj == 31.5 and want[1][0].tolist() == [[0, 1]] and want[1][1].tolist() == [[0], [1]]
    assert want[2].tolist() == [1, 1, 0, 0] and want[3].tolist() == [0, 1, 0, 1]
    for v in (0, 1, 2):
        res, obj = solve([(split, (det, new, end, links))], v)
        check_exact((split, (det, new, end, links)), res[0], obj[0], want, wobj)


def test_all_scores_negative_and_all_strongly_positive():
    rng = np.random.default_rng(41)
    insts_neg, insts_pos = [], []
    for split in ([1, 1, 1], [3, 4, 5], [12, 0, 12], [2] * 8, [33, 31, 34], [43, 42, 43]):
        det, new, end, links = random_chain(rng, split)
        insts_neg.append((split, (-np.abs(det) - 1, -np.abs(new) - 1, -np.abs(end) - 1, [-np.abs(l) - 1 for l in links])))
        insts_pos.append((split, (np.abs(det) + 10, np.abs(new) + 1, np.abs(end) + 1, [np.abs(l) + 1 for l in links])))
    res, obj = solve(insts_neg)
    for (split, _), r, o in zip(insts_neg, res, obj):
        assert o == 0.0 and all(np.count_nonzero(x) == 0 for x in [r[0], r[2], r[3]] + r[1]), split
    res, obj = solve(insts_pos)
    for (split, sc), r, o in zip(insts_pos, res, obj):
        assert feasible(r, split) and np.all(r[0] == 1), split  # det + new + end > 0 alone: every detection is used
        _, wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split)
        assert abs(o - wobj) <= 1e-9 * max(1.0, abs(wobj))


def test_the_golden_three_frame_scores():
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 's5_3frames_B.npz'))
    split = [z['link0'].shape[1], z['link0'].shape[2], z['link1'].shape[2]]
    assert z['link1'].shape[1] == split[1] and z['det'].shape[1] == sum(split)
    insts = [(split, (z['det'][r], z['new'][r], z['end'][r], [z['link0'][r], z['link1'][r]])) for r in range(3)]
    res, obj = solve(insts)
    for inst, r, o in zip(insts, res, obj):
        _, sc = inst
        want, wobj = milp_route(sc[0], sc[1], sc[2], sc[3], split)
        check_exact(inst, r, o, want, wobj)


def test_predict_assign_chain_real_forward():
    from common import build_model, case_inputs, get_case
    from mmmot_amd.tracker_glue import predict_assign_chain
    c, base = get_case('s5_3frames_B')
    m = build_model(c, base, device='cuda')
    dets, info, ds = case_inputs(c)
    split = [int(x) for x in ds]
    assert len(split) == 3
    dinfo = {k: v.cuda() for k, v in info.items()}
    scores, assignment = predict_assign_chain(m, dets.cuda(), dinfo, ds)
    with torch.no_grad():
        det, links, new, end, _ = m(dets.cuda(), dinfo, ds)
    plain = select_chain(det, links, new, end, m.test_mode)
    assert all(torch.equal(a, b.cpu()) for a, b in zip([scores[0], scores[2], scores[3]] + scores[1],
                                                       [plain[0], plain[2], plain[3]] + plain[1]))
    assert [tuple(l.shape) for l in assignment[1]] == [(1, split[0], split[1]), (1, split[1], split[2])]
    assert all(not t.is_cuda for t in (assignment[0], assignment[2], assignment[3], *assignment[1]))
    n = lambda t: t.numpy()
    want, wobj = milp_route(n(scores[0]), n(scores[2]), n(scores[3]), [n(l) for l in scores[1]], split)
    got = (n(assignment[0]), [n(l)[0] for l in assignment[1]], n(assignment[2]), n(assignment[3]))
    assert feasible(got, split) and same_assignment(got, want)


def test_two_frames_equal_the_pair_kernel():
    rng = np.random.default_rng(53)
    for k, (N, M) in enumerate(((3, 3), (12, 100), (64, 64), (130, 128))):
        for kind in KINDS:
            det, new, end, link = pair_ref.random_instance(rng, N, M, (1.0, 10.0, 1e4)[k % 3], kind)
            a, oa = pair_ref.lsa_route(det, new, end, link, N, M)
            b, ob = lp_route(det, new, end, [link], [N, M])
            assert same_assignment((a[0], [a[1]], a[2], a[3]), b), 'a tied instance: pick another seed'
            pairs, _ = pairs_table([(N, M)])
            t = lambda x: torch.from_numpy(x.reshape(-1)).cuda()
            total, off, max_nm = associate_layout(pairs, N + M, N * M)
            out = torch.empty(total, dtype=torch.float32, device='cuda')
            obj = torch.empty(1, dtype=torch.float64, device='cuda')
            ops().associate_pairs(t(det), t(new), t(end), t(link), pairs.reshape(-1).cuda(), 1, max_nm, out,
                                  off.to(torch.int32).cuda(), obj)
            pd, pl, pn, pe = unpack(out.cpu(), N, M)
            res, cobj = solve([([N, M], (det, new, end, [link]))])
            assert same_assignment(res[0], (pd.numpy(), [pl[0][0].numpy()], pn.numpy(), pe.numpy())), (N, M, kind)
            assert abs(cobj[0] - obj.item()) <= 1e-9 * max(1.0, abs(oa)) and abs(cobj[0] - oa) <= 1e-9 * max(1.0, abs(oa))


def test_ties_reach_the_optimum_deterministically():
    rng = np.random.default_rng(5)
    insts = []
    for split in ([1, 1, 1], [3, 3, 3], [12, 12, 12], [5, 1, 7], [12, 0, 12], [2] * 8, [33, 31, 34], [43, 42, 43]):
        L = sum(split)
        c = lambda *s, v=0.5: np.full(s, v, np.float32)
        lk = lambda f: [f(a, b) for a, b in zip(split[:-1], split[1:])]
        insts.append((split, (c(L), c(L), c(L), lk(lambda a, b: c(a, b, v=2.0)))))       # any maximal set of chains
        insts.append((split, (c(L, v=0), c(L, v=0), c(L, v=0), lk(lambda a, b: c(a, b, v=0)))))  # every value exactly 0
        q = lambda *s: rng.integers(-2, 3, s).astype(np.float32)
        insts.append((split, (q(L), q(L), q(L), lk(q))))                                # small integers: tied optima
    res, obj = solve(insts)
    for (split, sc), r, o in zip(insts, res, obj):
        _, wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split)
        assert feasible(r, split), split
        assert abs(o - wobj) <= 1e-9 * max(1.0, abs(wobj)), (split, o, wobj)
        assert abs(objective(r, *sc) - wobj) <= 1e-9 * max(1.0, abs(wobj))
    again = solve(insts)
    assert same(again[0], res) and np.array_equal(again[1], obj)
    for v in (1, 2):
        got = solve(insts, v)
        assert same(got[0], res) and np.array_equal(got[1], obj), v


def test_batch_equals_chains_alone_and_shuffled():
    rng = np.random.default_rng(17)
    insts = []
    for k in range(24):
        T = (2, 3, 4, 8)[k % 4]
        split = [int(n) for n in rng.integers(0, 40 if T < 8 else 16, T)]
        split[0] = max(split[0], 1)
        insts.append((split, random_chain(rng, split, 3.0, KINDS[k % 3])))
    res, obj = solve(insts)
    for k, inst in enumerate(insts):
        alone, o = solve([inst])
        assert same(alone, [res[k]]) and o[0] == obj[k], k
        want, wobj = lp_route(*inst[1][:3], inst[1][3], inst[0])
        assert feasible(res[k], inst[0]) and abs(obj[k] - wobj) <= 1e-9 * max(1.0, abs(wobj))
    perm = rng.permutation(len(insts))
    sres, sobj = solve([insts[k] for k in perm])
    for pos, k in enumerate(perm):
        assert same([sres[pos]], [res[k]]) and sobj[pos] == obj[k]


@pytest.mark.parametrize('fill', [0xFF, 0x7B])
def test_poisoned_outputs_are_written_in_full(fill):
    rng = np.random.default_rng(23)
    insts = [(s, random_chain(rng, s, 2.0, 'eval')) for s in ([12, 12, 12], [5, 0, 64], [64, 5], [2] * 8, [40, 50, 45])]
    clean = solve(insts, fill=0)
    for v in (0, 1, 2):
        got = solve(insts, v, fill=fill)
        assert same(got[0], clean[0]) and np.array_equal(got[1], clean[1]), v


def _tensors(sc, dtype=torch.float32, device='cpu'):
    t = lambda x: torch.from_numpy(np.asarray(x)).to(dtype).to(device)
    return t(sc[0]), [t(l)[None] for l in sc[3]], t(sc[1]), t(sc[2])


def test_gt_objective():
    rng = np.random.default_rng(61)
    for split in ([2, 3, 2], [6, 5, 7], [4, 4, 4, 4], [9, 8]):
        sc = random_chain(rng, split)
        L = sum(split)
        lab = lambda *s: rng.integers(0, 2, s).astype(np.float32)
        gt = (lab(L), lab(L), lab(L), [lab(a, b) for a, b in zip(split[:-1], split[1:])])
        want, _ = milp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)
        assert same_assignment(want, lp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)[0]), 'a tied instance'
        det, links, new, end = _tensors(sc, device='cuda')
        tg = (torch.from_numpy(gt[0]).cuda(), torch.from_numpy(gt[1]).cuda(), torch.from_numpy(gt[2]).cuda(),
              [torch.from_numpy(g)[None].cuda() for g in gt[3]])
        got = associate_chain(det, links, new, end, split, gt=tg)
        # solving the shifted scores without gt is the same call
        eff = lambda g: g + g.eq(0).float().mul(-1)
        shifted = associate_chain(det - eff(tg[0]), [l - eff(g) for l, g in zip(links, tg[3])], new - eff(tg[1]),
                                  end - eff(tg[2]), split)
        n = lambda r: (r[0].cpu().numpy(), [l[0].cpu().numpy() for l in r[1]], r[2].cpu().numpy(), r[3].cpu().numpy())
        assert feasible(n(got), split) and same_assignment(n(got), n(shifted)) and same_assignment(n(got), want), split


def test_host_and_device_inputs_match_ortools_shapes():
    rng = np.random.default_rng(29)
    for split in ([1, 1, 1], [12, 12, 12], [7, 40, 3], [0, 5, 4], [5, 0, 5], [6, 6], [3, 2, 4, 1]):
        sc = random_chain(rng, split, 1.0, 'eval')
        want, _ = lp_route(sc[0], sc[1], sc[2], sc[3], split)
        for dtype in (torch.float32, torch.float64, torch.float16):
            if dtype == torch.float16:  # the oracle gets the values the solver sees
                h = [np.asarray(x, np.float16).astype(np.float32) for x in sc[:3]]
                sc16 = (h[0], h[1], h[2], [np.asarray(l, np.float16).astype(np.float32) for l in sc[3]])
                ref, _ = lp_route(sc16[0], sc16[1], sc16[2], sc16[3], split)
            else:
                ref = want
            det, links, new, end = _tensors(sc, dtype)
            host = associate_chain(det, links, new, end, [torch.tensor([s]) for s in split])
            dev = associate_chain(det.cuda(), [l.cuda() for l in links], new.cuda(), end.cuda(), split)
            for h, d in ((host[0], dev[0]), (host[2], dev[2]), (host[3], dev[3])):
                assert h.shape == det.shape and h.dtype == dtype and h.device.type == 'cpu'
                assert d.shape == det.shape and d.dtype == dtype and d.is_cuda and torch.equal(h, d.cpu())
            assert len(host[1]) == len(dev[1]) == len(split) - 1
            for t, (h, d) in enumerate(zip(host[1], dev[1])):
                assert h.shape == d.shape == (1, split[t], split[t + 1]) and h.dtype == d.dtype == dtype
                assert d.is_cuda and torch.equal(h, d.cpu())
            got = (host[0].double().numpy(), [l[0].double().numpy() for l in host[1]], host[2].double().numpy(),
                   host[3].double().numpy())
            assert same_assignment(got, ref), (split, dtype)
    # associate_chain_batch: the chains of one launch equal associate_chain one by one
    insts = [(s, random_chain(rng, s, 1.0, 'eval')) for s in ([3, 4, 2], [12, 12], [2] * 8)]
    args = [_tensors(sc, device='cuda') for _, sc in insts]
    res, obj = associate_chain_batch([a[0] for a in args], [a[1] for a in args], [a[2] for a in args],
                                     [a[3] for a in args], [s for s, _ in insts], return_objective=True)
    assert obj.shape == (3,) and obj.dtype == torch.float64
    for (s, sc), a, r, o in zip(insts, args, res, obj.cpu().numpy()):
        one = associate_chain(a[0], a[1], a[2], a[3], s)
        assert all(torch.equal(x, y) for x, y in zip([r[0], r[2], r[3]] + r[1], [one[0], one[2], one[3]] + one[1]))
        assert abs(o - lp_route(sc[0], sc[1], sc[2], sc[3], s)[1]) <= 1e-9 * max(1.0, abs(o))
