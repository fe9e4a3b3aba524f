"""Whole-sequence association on the device (mmmot_amd.association.associate_sequence, csrc/assign_sequence.hip) against
the two host oracles of the chain program, against ``associate_chain`` inside that kernel's limits, on long sequences,
on ties, over batch position and kernel variant, over poisoned outputs, with ``gt=``, with host and device inputs, and
its trajectory numbers against tests/sequence_ref.ids_of and against the pair-by-pair tracker on decisive instances.

The long cases: T = 300 and T = 1000 are both kept - ``test_long_sequences`` says what each took on an MI355X."""
import time

import numpy as np
import pytest
import torch

from association_chain_ref import feasible, lp_route, milp_route, objective, random_chain, same_assignment
from sequence_ref import ids_of, planted_sequence
from test_association_sequence_cpu import KINDS, LENGTHS, instance, pairs_of
from mmmot_amd import _lib
from mmmot_amd.association import (AssociationError, _raise_status, associate_chain_batch, associate_sequence, associate_sequence_batch, chain_block_size,
                                   pairs_table, sequences_table, unpack_chain)
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import SEQ_ROW, sequence_layout
from mmmot_amd.tracks import TrackState, assign_ids, merge_tracks

pytestmark = pytest.mark.gpu

_OPS = []
VARIANTS = (1, 2, 3, 4)  # one / four waves with the state in the workspace, one / four waves with the state in LDS


def ops():
    if not _OPS:
        _OPS.append(HipOps())
    return _OPS[0]


def solve(insts, variant=0, fill=None, tamper=None, max_T=None, max_L=None):
    """one launch over [(split, (det, new, end, links)) ...] -> [(det, [link ...], new, end) numpy], objective [B],
    per sequence its flat ids, info [B, 4]; ``fill``: the outputs are pre-filled with this byte (or NaN for 'nan');
    ``tamper(rows, max_T)``: changes the [B, 6] device table in place before it is uploaded; ``max_T`` / ``max_L``: what
    the launch is sized for when not what the sequences need"""
    splits = [list(s) for s, _ in insts]
    seqs, nts, offs, sos = sequences_table(splits)
    f32 = lambda x: np.asarray(x, np.float32).reshape(-1)
    cat = lambda k: torch.from_numpy(np.concatenate([f32(sc[k]) for _, sc in insts])).cuda()
    det, new, end = cat(0), cat(1), cat(2)
    link = torch.from_numpy(np.concatenate([f32(l) for _, sc in insts for l in sc[3]] + [np.zeros(1, np.float32)])).cuda()
    total, off, woff, units, max_n, mL, mT = sequence_layout(seqs, nts, det.numel(), link.numel())
    max_T, max_L = max_T or mT, max_L or mL
    B = len(insts)
    rows = torch.cat([seqs, off.to(torch.int32)[:, None], woff.to(torch.int32)[:, None]], 1)
    assert rows.shape == (B, SEQ_ROW)
    if tamper is not None:
        tamper(rows, max_T)
    table = torch.cat([rows.reshape(-1), nts]).cuda()
    out = torch.empty(total, dtype=torch.float32, device='cuda')
    ids = torch.empty(det.numel(), dtype=torch.int32, device='cuda')
    obj = torch.empty(B, dtype=torch.float64, device='cuda')
    info = torch.empty((B, 4), dtype=torch.int32, device='cuda')
    ws = torch.empty(units, dtype=torch.float64, device='cuda')
    if fill == 'nan':
        out.fill_(float('nan'))
        obj.fill_(float('nan'))
        ids.fill_(-77)
        info.fill_(-77)
        ws.fill_(float('nan'))
    elif fill is not None:
        for t in (out, ids, obj, info, ws):
            t.view(torch.uint8).fill_(fill)
    assert _lib.load().mmmot_set_sequence_variant(variant) == 0
    try:
        ops().associate_sequences(det, new, end, link, table[:SEQ_ROW * B], table[SEQ_ROW * B:], B, max_T, max_n, max_L, out, ids,
                                  obj, info, ws)
        torch.cuda.synchronize()
    finally:
        assert _lib.load().mmmot_set_sequence_variant(0) == 0
    out, ids = out.cpu(), ids.cpu().numpy()
    res, flat_ids = [], []
    for s, o, so in zip(splits, offs, sos):
        d, lk, n, e = unpack_chain(out[o:o + chain_block_size(s)], s)
        res.append((d.numpy(), [x[0].numpy() for x in lk], n.numpy(), e.numpy()))
        flat_ids.append(ids[so:so + sum(s)])
    return res, obj.cpu().numpy(), flat_ids, info.cpu().numpy()


def same(a, b):
    return all(same_assignment(x, y) for x, y in zip(a, b))


def check_sane(insts, res, ids, info):
    """status 0, augmentations = trajectories, passes >= augmentations, a feasible flow, the IDs of sequence_ref.ids_of"""
    for (split, _), r, i, w in zip(insts, res, ids, info):
        assert w[0] == 0 and w[2] == w[1] == int(r[2].sum()) and w[3] >= w[2], (split, w)
        assert feasible(r, split), split
        assert np.array_equal(i, np.concatenate(ids_of(r, split))), split


def check_optimal(inst, got, obj, want, wobj, agreed):
    split, (det, new, end, links) = inst
    assert abs(obj - wobj) <= 1e-9 * max(1.0, abs(wobj)), (split, obj, wobj)
    assert abs(objective(got, det, new, end, links) - wobj) <= 1e-9 * max(1.0, abs(wobj)), split
    if agreed:
        assert same_assignment(got, want), split


_CASES = []


def oracle_cases():
    """the families of the CPU suite, 6 seeds per (T, kind), and three dense T = 12, n_t = 24 instances, where a
    shortest path is often rerouted through back-edges; both oracle routes, computed once"""
    if not _CASES:
        insts = [instance(T, kind, seed) for T in LENGTHS for kind in KINDS for seed in range(6)]
        for seed in range(3):
            insts.append(([24] * 12, random_chain(np.random.default_rng(9000 + seed), [24] * 12, 1.0, 'normal')))
        for split, sc in insts:
            a, oa = lp_route(sc[0], sc[1], sc[2], sc[3], split)
            b, ob = milp_route(sc[0], sc[1], sc[2], sc[3], split)
            assert abs(oa - ob) <= 1e-9 * max(1.0, abs(oa))
            _CASES.append(((split, sc), a, oa, same_assignment(a, b)))
    return _CASES


def test_random_and_dense_scores_match_both_oracles():
    cases = oracle_cases()
    assert sum(1 for c in cases if c[3]) >= len(cases) // 2
    insts = [c[0] for c in cases]
    res, obj, ids, info = solve(insts)
    check_sane(insts, res, ids, info)
    for c, r, o in zip(cases, res, obj):
        check_optimal(c[0], r, o, c[1], c[2], c[3])
    # one pass per search when no shortest path turns back: the dense instances need more
    assert (info[-3:, 3] > info[-3:, 2] + 1).all(), info[-3:]


@pytest.mark.parametrize('variant', VARIANTS)
def test_every_kernel_variant_returns_the_same_bits(variant):
    insts = [c[0] for c in oracle_cases()]
    auto = solve(insts)
    got = solve(insts, variant)
    assert same(got[0], auto[0]) and np.array_equal(got[1], auto[1])
    assert all(np.array_equal(x, y) for x, y in zip(got[2], auto[2])) and np.array_equal(got[3], auto[3])


@pytest.mark.parametrize('variant', (3, 4))
def test_the_largest_lds_request_returns_the_same_bits(variant):
    """a launch sized for T = 4096 and L = 2304 asks for the most dynamic LDS the kernel may (154 896 bytes)"""
    rng = np.random.default_rng(93)
    insts = [(s, random_chain(rng, s, 1.0, 'normal')) for s in ([5] * 12, [18, 2, 0, 7, 3, 20, 1, 4, 9])]
    auto = solve(insts)
    got = solve(insts, variant, 'nan', max_T=4096, max_L=2304)
    assert same(got[0], auto[0]) and np.array_equal(got[1], auto[1])
    assert all(np.array_equal(x, y) for x, y in zip(got[2], auto[2])) and np.array_equal(got[3], auto[3])


def _break_T(rows, max_T):
    rows[1, 0] = max_T + 1      # more frames than the launch was sized for: refused before anything of it is read


def _break_out(rows, max_T):
    rows[1, 4] = 2 ** 31 - 64   # an output block past the end of `out`: refused after the frame scan, before any write


@pytest.mark.parametrize('tamper', [_break_T, _break_out], ids=['T', 'out'])
def test_a_sequence_outside_the_contract_gets_a_status_and_its_neighbours_are_solved(tamper):
    rng = np.random.default_rng(41)
    insts = [(s, random_chain(rng, s, 1.0, 'normal')) for s in ([3, 0, 4, 5], [4] * 9, [6, 7])]
    clean = solve(insts)
    for variant in (0, 2):
        res, obj, ids, info = solve(insts, variant, 'nan', tamper)
        assert np.isnan(obj[1]) and info[1].tolist() == [1, 0, 0, 0]
        # nothing else of it was written: its block and its ids are the pre-fill
        assert all(np.isnan(x).all() for x in [res[1][0], res[1][2], res[1][3]] + res[1][1]) and (ids[1] == -77).all()
        for k in (0, 2):
            assert same_assignment(res[k], clean[0][k]) and obj[k] == clean[1][k]
            assert np.array_equal(ids[k], clean[2][k]) and np.array_equal(info[k], clean[3][k]) and info[k, 0] == 0
        with pytest.raises(AssociationError, match='sequence 1 not solved: outside the launch contract') as e:
            _raise_status(info)
        assert e.value.index == 1 and e.value.status == 1


def _tensors(sc, dtype=torch.float32, device='cpu'):
    t = lambda x: torch.from_numpy(np.asarray(x)).to(dtype).to(device)
    return t(sc[0]), [t(l)[None] for l in sc[3]], t(sc[1]), t(sc[2])


def _numpy(r):
    return (r[0].double().cpu().numpy(), [l[0].double().cpu().numpy() for l in r[1]], r[2].double().cpu().numpy(),
            r[3].double().cpu().numpy())


def test_equals_associate_chain_inside_its_limits():
    rng = np.random.default_rng(17)
    for split in ([1, 1], [3, 4, 5], [12, 0, 12], [2] * 8, [33, 31, 34], [64, 70, 64], [128] * 8):
        sc = random_chain(rng, split, 1.0, 'eval' if len(split) % 2 else 'normal')
        res, obj, _, info = solve([(split, sc)])
        det, links, new, end = _tensors(sc, device='cuda')
        want, wobj = associate_chain_batch([det], [links], [new], [end], [split], return_objective=True)
        assert info[0, 0] == 0 and same_assignment(res[0], _numpy(want[0])), split
        assert obj[0] == wobj.cpu().numpy()[0], split  # the same sums in the same order


@pytest.mark.parametrize('T,hi', [(300, 6), (1000, 5)])
def test_long_sequences(T, hi):
    """T = 300 with n_t in 0 .. 5 and T = 1000 with n_t in 0 .. 4, kind eval, against lp_route.  On an MI355X the launch
    and its copies took 0.47 s (T = 300, 312 trajectories) and 3.8 s (T = 1000, 832 trajectories): below the 5 s at which
    the T = 1000 case would have been dropped, so both are kept."""
    rng = np.random.default_rng(T)
    split = [int(n) for n in rng.integers(0, hi, T)]
    sc = random_chain(rng, split, 1.0, 'eval')
    want, wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split)
    inst = (split, sc)
    t0 = time.perf_counter()
    res, obj, ids, info = solve([inst])
    print('T = %d, L = %d: trajectories %d, augmentations %d, passes %d, %.3f s with copies' %
          (T, sum(split), *info[0, 1:], time.perf_counter() - t0))
    check_sane([inst], res, ids, info)
    check_optimal(inst, res[0], obj[0], want, wobj, False)


def test_integer_scores_with_many_ties():
    rng = np.random.default_rng(5)
    insts = []
    for split in ([4, 4, 4], [3, 0, 5, 2], [6] * 9, [5, 3, 6, 2] * 5):
        L = sum(split)
        z = lambda *s: rng.integers(-2, 3, s).astype(np.float32)
        insts.append((split, (z(L), z(L), z(L), [z(a, b) for a, b in zip(split[:-1], split[1:])])))
    a = solve(insts)
    b = solve(insts)
    check_sane(insts, a[0], a[2], a[3])
    for (split, sc), r, o in zip(insts, a[0], a[1]):
        wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split)[1]
        assert o == wobj == objective(r, sc[0], sc[1], sc[2], sc[3]), split  # integers: exact
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def test_batch_equals_sequences_alone_and_shuffled():
    rng = np.random.default_rng(23)
    insts = [(s, random_chain(rng, s, 1.0, k)) for s, k in (([3, 4, 5], 'normal'), ([2] * 40, 'eval'), ([20, 30], 'masked'),
                                                             ([5, 0, 6, 1, 4, 0, 0, 3, 2], 'normal'), ([1, 1], 'eval'),
                                                             ([7] * 17, 'normal'))]
    whole = solve(insts)
    check_sane(insts, whole[0], whole[2], whole[3])
    order = [4, 2, 5, 0, 3, 1]
    shuffled = solve([insts[i] for i in order])
    for pos, i in enumerate(order):
        alone = solve([insts[i]])
        for got, k in ((whole, i), (shuffled, pos)):
            assert same_assignment(got[0][k], alone[0][0]) and got[1][k] == alone[1][0]
            assert np.array_equal(got[2][k], alone[2][0]) and np.array_equal(got[3][k], alone[3][0])


@pytest.mark.parametrize('fill', ['nan', 0xFF, 0x7B])
def test_poisoned_outputs_are_written_in_full(fill):
    rng = np.random.default_rng(31)
    insts = [(s, random_chain(rng, s, 1.0, 'normal')) for s in ([3, 0, 4, 5], [6] * 9, [40, 37])]
    clean = solve(insts)
    for variant in (0, 1):
        got = solve(insts, variant, fill)
        assert same(got[0], clean[0]) and np.array_equal(got[1], clean[1]) and np.array_equal(got[3], clean[3])
        assert all(np.array_equal(x, y) for x, y in zip(got[2], clean[2]))


def test_gt_objective():
    rng = np.random.default_rng(61)
    for split in ([2, 3, 2], [6, 5, 7], [4] * 9, [3, 0, 4, 2, 5, 1, 0, 2, 3, 4, 2]):
        sc = random_chain(rng, split)
        L = sum(split)
        lab = lambda *s: rng.integers(0, 2, s).astype(np.float32)
        gt = (lab(L), lab(L), lab(L), [lab(a, b) for a, b in zip(split[:-1], split[1:])])
        want, _ = lp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)
        agreed = same_assignment(want, milp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)[0])
        det, links, new, end = _tensors(sc, device='cuda')
        tg = (torch.from_numpy(gt[0]).cuda(), torch.from_numpy(gt[1]).cuda(), torch.from_numpy(gt[2]).cuda(),
              [torch.from_numpy(g)[None].cuda() for g in gt[3]])
        got = _numpy(associate_sequence(det, links, new, end, split, gt=tg))
        assert feasible(got, split)
        if agreed:
            assert same_assignment(got, want), split
        # the objective of the shifted scores at the assignment, the constant added, is the oracle's optimum
        eff = lambda g: g + (g == 0) * -1.0
        shifted = (sc[0] - eff(gt[0]), sc[1] - eff(gt[1]), sc[2] - eff(gt[2]), [l - eff(g) for l, g in zip(sc[3], gt[3])])
        const = sum(float(g.sum()) for g in (gt[0], gt[1], gt[2], *gt[3]))
        wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)[1]
        assert abs(objective(got, shifted[0], shifted[1], shifted[2], shifted[3]) + const - wobj) <= 1e-5 * max(1.0, abs(wobj))


def test_host_and_device_inputs_match_ortools_shapes():
    rng = np.random.default_rng(29)
    for split in ([1, 1, 1], [12] * 9, [7, 40, 3], [0, 5, 4], [5, 0, 5], [6, 6], [3, 2, 4, 1] * 3):
        sc = random_chain(rng, split, 1.0, 'eval')
        want, wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split)
        for dtype in (torch.float32, torch.float64):
            det, links, new, end = _tensors(sc, dtype)
            host = associate_sequence(det, links, new, end, [torch.tensor([s]) for s in split])
            dev = associate_sequence(det.cuda(), [l.cuda() for l in links], new.cuda(), end.cuda(), split)
            assert len(host) == len(dev) == 4
            for h, d in ((host[0], dev[0]), (host[2], dev[2]), (host[3], dev[3])):
                assert h.shape == det.shape and h.dtype == dtype and h.device.type == 'cpu'
                assert d.shape == det.shape and d.dtype == dtype and d.is_cuda and torch.equal(h, d.cpu())
            assert len(host[1]) == len(dev[1]) == len(split) - 1
            for t, (h, d) in enumerate(zip(host[1], dev[1])):
                assert h.shape == d.shape == (1, split[t], split[t + 1]) and h.dtype == d.dtype == dtype
                assert d.is_cuda and torch.equal(h, d.cpu())
            got = _numpy(host)
            assert feasible(got, split)
            assert abs(objective(got, sc[0], sc[1], sc[2], sc[3]) - wobj) <= 1e-9 * max(1.0, abs(wobj)), (split, dtype)


def test_return_ids_and_the_batch_call():
    rng = np.random.default_rng(37)
    insts = [(s, random_chain(rng, s, 1.0, 'eval')) for s in ([3, 4, 2], [4] * 12, [2, 0, 3, 3, 0, 1, 2, 2, 4])]
    args = [_tensors(sc, device='cuda') for _, sc in insts]
    res, obj = associate_sequence_batch([a[0] for a in args], [a[1] for a in args], [a[2] for a in args],
                                        [a[3] for a in args], [s for s, _ in insts], return_objective=True,
                                        return_ids=True)
    assert obj.shape == (3,) and obj.dtype == torch.float64 and obj.is_cuda
    for (s, sc), a, r, o in zip(insts, args, res, obj.cpu().numpy()):
        one = associate_sequence(a[0], a[1], a[2], a[3], s, return_ids=True)
        assert len(one) == len(r) == 6
        assert all(torch.equal(x, y) for x, y in zip([r[0], r[2], r[3]] + r[1], [one[0], one[2], one[3]] + one[1]))
        want = ids_of(_numpy(one), s)
        for got in (one, r):
            assert len(got[4]) == len(s) and got[5] == int(one[2].sum().item()) == 1 + max(int(w.max()) for w in want if w.size)
            for g, w in zip(got[4], want):
                assert g.dtype == torch.int64 and g.is_cuda and np.array_equal(g.cpu().numpy(), w)
        assert abs(o - lp_route(sc[0], sc[1], sc[2], sc[3], s)[1]) <= 1e-9 * max(1.0, abs(o))
    host = associate_sequence(*[x.cpu() if torch.is_tensor(x) else [l.cpu() for l in x] for x in args[0]], insts[0][0],
                              return_ids=True)
    assert all(not g.is_cuda and g.dtype == torch.int64 for g in host[4])
    plain = associate_sequence_batch([a[0] for a in args], [a[1] for a in args], [a[2] for a in args],
                                     [a[3] for a in args], [s for s, _ in insts])
    assert len(plain) == 3 and all(len(r) == 4 for r in plain)


@pytest.mark.parametrize('seed', range(3))
def test_global_ids_equal_the_pairwise_tracker_on_decisive_instances(seed):
    split, sc, _ = planted_sequence(np.random.default_rng(300 + seed))
    det, links, new, end = _tensors(sc, device='cuda')
    got = associate_sequence(det, links, new, end, split, return_ids=True)
    assert same_assignment(_numpy(got), lp_route(sc[0], sc[1], sc[2], sc[3], split)[0])
    # pair by pair over the same scores: one batched pair solve, one ID walk
    pairs = pairs_of(sc, split)
    splits = list(zip(split[:-1], split[1:]))
    f = lambda k: torch.from_numpy(np.concatenate([np.asarray(p[k], np.float32).reshape(-1) for p in pairs])).cuda()
    table, _ = pairs_table(splits)
    blocks, _ = torch.ops.mmmot.associate(f(0), f(2), f(3), f(1), table)
    tracks = [np.full(n, -1, np.int64) for n in split]
    for t, (i0, i1, start, _) in enumerate(assign_ids(TrackState(), blocks, splits, [(t, t + 1) for t in range(len(splits))])):
        merge_tracks(tracks, t + 1, i0, i1, start)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[4], tracks))
