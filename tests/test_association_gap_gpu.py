"""Whole-sequence association with skip links on the device (mmmot_amd.association.associate_sequence_gaps,
csrc/assign_sequence.hip): planted tracks recovered across missed detections, against the literal program (scipy's
milp) and the serial restatement of the search (tests/sequence_gap_ref.py), at one gap against mmmot_associate_sequences
bit for bit, over kernel variant, batch position, poisoned outputs and tampered table rows, with ``gt=``, with host and
device inputs, and what the C entry refuses."""
import numpy as np
import pytest
import torch

from sequence_gap_ref import (flat_links, gap_feasible, gap_objective, ids_of_gaps, lp_gap_route, milp_gap_route,
                              random_gap_sequence, same_gap_assignment, ssp_gap_route)
from test_association_gap_cpu import PLANTED_SEEDS, close, hidden_names, instance, planted
from test_association_sequence_gpu import solve as solve_one_gap
from mmmot_amd import _lib
from mmmot_amd.association import (AssociationError, _raise_status, associate_sequence, associate_sequence_gaps,
                                   associate_sequence_gaps_batch, gap_block_size, gap_sequences_table, unpack_gaps)
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import SEQ_ROW, sequence_gap_layout

pytestmark = pytest.mark.gpu

_OPS = []
VARIANTS = (1, 2, 3, 4)  # one / four waves with the state in the workspace, one / four waves with the state in LDS


def ops():
    if not _OPS:
        _OPS.append(HipOps())
    return _OPS[0]


def solve(insts, G, variant=0, fill=None, tamper=None, max_T=None, max_L=None, max_n=None, raw=False):
    """one launch over [(split, (det, new, end, links nested)) ...] -> [(det, [[link ...] per gap], new, end) numpy],
    objective [B], per sequence its flat ids, info [B, 4]; ``fill``: the outputs are pre-filled with this byte (or NaN
    for 'nan'); ``tamper(rows)``: changes the [B, 6] device table before it is uploaded; ``max_T`` / ``max_L`` / ``max_n``:
    what the launch is sized for when not what the sequences need; ``raw``: the flat buffers instead of the unpacked results"""
    splits = [list(s) for s, _ in insts]
    seqs, nts, offs, sos = gap_sequences_table(splits, G)
    f32 = lambda x: np.asarray(x, np.float32).reshape(-1)
    cat = lambda k: torch.from_numpy(np.concatenate([f32(sc[k]) for _, sc in insts])).cuda()
    det, new, end = cat(0), cat(1), cat(2)
    link = torch.from_numpy(np.concatenate([f32(l) for _, sc in insts for l in flat_links(sc[3])] +
                                           [np.zeros(1, np.float32)])).cuda()
    total, off, woff, units, mn, mL, mT = sequence_gap_layout(seqs, nts, G, det.numel(), link.numel())
    max_T, max_L, max_n = max_T or mT, max_L or mL, max_n or mn
    B = len(insts)
    rows = torch.cat([seqs, off.to(torch.int32)[:, None], woff.to(torch.int32)[:, None]], 1)
    assert rows.shape == (B, SEQ_ROW)
    if tamper is not None:
        tamper(rows)
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
    assert _lib.load().mmmot_set_sequence_gap_variant(variant) == 0
    try:
        ops().associate_sequences_gap(det, new, end, link, table[:SEQ_ROW * B], table[SEQ_ROW * B:], B, max_T, max_n, max_L,
                                      G, out, ids, obj, info, ws)
        torch.cuda.synchronize()
    finally:
        assert _lib.load().mmmot_set_sequence_gap_variant(0) == 0
    out, ids = out.cpu(), ids.cpu().numpy()
    if raw:
        return out.numpy(), obj.cpu().numpy(), ids, info.cpu().numpy()
    res, flat_ids = [], []
    for s, o, so in zip(splits, offs, sos):
        d, lk, n, e = unpack_gaps(out[o:o + gap_block_size(s, G)], s, G)
        res.append((d.numpy(), [[x[0].numpy() for x in row] for row in lk], n.numpy(), e.numpy()))
        flat_ids.append(ids[so:so + sum(s)])
    return res, obj.cpu().numpy(), flat_ids, info.cpu().numpy()


def same(a, b):
    """two results of ``solve``: the same bits"""
    return (all(same_gap_assignment(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1], equal_nan=True) and
            all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and np.array_equal(a[3], b[3]))


def check_against_ssp(insts, G, got):
    """status 0, the assignment, the IDs and info (tracks, augmentations, passes) of the serial restatement"""
    res, obj, ids, info = got
    for (split, sc), r, o, i, w in zip(insts, res, obj, ids, info):
        want, wobj, winfo = ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split)
        assert w.tolist() == [0, winfo['tracks'], winfo['augmentations'], winfo['passes']], (split, w, winfo)
        assert gap_feasible(r, split) and same_gap_assignment(r, want), split
        assert close(o, wobj), (split, o, wobj)
        assert np.array_equal(i, np.concatenate(ids_of_gaps(r, split))), split


def _tensors(sc, dtype=torch.float32, device='cpu'):
    t = lambda x: torch.from_numpy(np.asarray(x)).to(dtype).to(device)
    return t(sc[0]), [[t(l)[None] for l in row] for row in sc[3]], t(sc[1]), t(sc[2])


def _numpy(r):
    f = lambda x: x.double().cpu().numpy()
    return f(r[0]), [[f(l[0]) for l in row] for row in r[1]], f(r[2]), f(r[3])


@pytest.mark.parametrize('seed', PLANTED_SEEDS)
def test_recovers_hidden_tracks_across_misses(seed):
    split, sc, frames, misses = planted(seed)  # T = 30, max_n = 6, G = 3, p_miss = 0.15
    assert misses >= 1
    det, links, new, end = _tensors(sc, device='cuda')
    got = associate_sequence_gaps(det, links, new, end, split, return_ids=True)
    names = hidden_names(frames, [i.cpu().numpy() for i in got[4]])
    assert got[5] == len(names) == len({h for f in frames for h in f})
    # the links of gap 1 alone: every miss inside a track ends it and starts another
    alone = associate_sequence(det, links[0], new, end, split, return_ids=True)
    assert alone[5] > got[5]


_CASES = []


def oracle_cases():
    """(G, [instances]) per gap: T in 3, 6, 12, 40 with G in 1, 2, 3, T = 12 also with G = 8, the three score kinds"""
    if not _CASES:
        for G in (1, 2, 3):
            insts = [instance(T, G, kind, seed) for T in (3, 6, 12) for kind in ('normal', 'dense', 'ties') for seed in (0, 1)]
            for k, kind in enumerate(('normal', 'dense', 'ties')):
                rng = np.random.default_rng(4000 + 10 * G + k)
                split = [int(n) for n in rng.integers(0, 5, 40)]
                insts.append((split, random_gap_sequence(rng, split, G, kind)))
            _CASES.append((G, [i for i in insts if len(i[0]) > G]))
        insts = []
        for k, kind in enumerate(('normal', 'dense', 'ties')):
            rng = np.random.default_rng(4800 + k)
            split = [int(n) for n in rng.integers(0, 5, 12)]
            insts.append((split, random_gap_sequence(rng, split, 8, kind)))
        _CASES.append((8, insts))
    return _CASES


@pytest.mark.parametrize('case', range(4), ids=['G1', 'G2', 'G3', 'G8'])
def test_matches_the_literal_program_and_the_serial_search(case):
    G, insts = oracle_cases()[case]
    got = solve(insts, G)
    check_against_ssp(insts, G, got)
    for (split, sc), r, o in zip(insts, got[0], got[1]):
        wobj = milp_gap_route(sc[0], sc[1], sc[2], sc[3], split)[1]
        assert close(o, wobj) and close(gap_objective(r, *sc), wobj), (split, o, wobj)


def test_one_gap_is_the_sequence_kernel_bit_for_bit():
    insts = oracle_cases()[0][1]
    rng = np.random.default_rng(77)
    insts = insts + [([20] * 6, random_gap_sequence(rng, [20] * 6, 1, 'normal')), ([6] * 9, random_gap_sequence(rng, [6] * 9, 1, 'ties'))]
    res, obj, ids, info = solve(insts, 1)
    old = solve_one_gap([(s, (sc[0], sc[1], sc[2], sc[3][0])) for s, sc in insts])
    for r, w in zip(res, old[0]):
        assert same_gap_assignment(r, (w[0], [w[1]], w[2], w[3]))
    assert np.array_equal(obj, old[1]) and np.array_equal(info, old[3])
    assert all(np.array_equal(x, y) for x, y in zip(ids, old[2]))


def variant_instances():
    """small ones, empty frames, one with n_t = 20 > 16 (the four-wave lane grouping), G = 3"""
    rng = np.random.default_rng(91)
    return [(s, random_gap_sequence(rng, s, 3, k)) for s, k in (([20] * 6, 'normal'), ([3, 0, 4, 5, 0, 2], 'ties'),
                                                                 ([4] * 12, 'dense'), ([17, 3, 0, 21, 9], 'normal'))]


@pytest.mark.parametrize('variant', VARIANTS)
def test_every_kernel_variant_returns_the_same_bits(variant):
    insts = variant_instances()
    auto = solve(insts, 3)
    check_against_ssp(insts[1:3], 3, tuple(x[1:3] for x in auto))
    assert same(solve(insts, 3, variant), auto)


@pytest.mark.parametrize('variant', (3, 4))
def test_offset_table_in_the_workspace_returns_the_same_bits(variant):
    """a launch sized for T = 4096 and L = 2304 at G = 8 cannot hold the offset table in LDS beside the state"""
    rng = np.random.default_rng(93)
    insts = [(s, random_gap_sequence(rng, s, 8, 'normal')) for s in ([5] * 12, [18, 2, 0, 7, 3, 20, 1, 4, 9])]
    assert same(solve(insts, 8, variant, 'nan', max_T=4096, max_L=2304), solve(insts, 8))


def test_long_sequence():
    """T = 300, n_t <= 4, G = 3: the walk along pred over skipped frames, against the serial search and the LP"""
    rng = np.random.default_rng(300)
    split = [int(n) for n in rng.integers(0, 5, 300)]
    inst = (split, random_gap_sequence(rng, split, 3, 'eval'))
    got = solve([inst], 3)
    check_against_ssp([inst], 3, got)
    assert close(got[1][0], lp_gap_route(*inst[1], split)[1])


def batch_instances():
    rng = np.random.default_rng(23)
    return [(s, random_gap_sequence(rng, s, 2, k)) for s, k in (([3, 4, 5], 'normal'), ([2] * 40, 'eval'), ([20, 30, 4], 'ties'),
                                                                 ([5, 0, 6, 1, 4, 0, 0, 3, 2], 'normal'), ([1, 1, 1], 'eval'),
                                                                 ([7] * 17, 'dense'))]


def test_batch_equals_sequences_alone_and_shuffled():
    insts = batch_instances()  # T = 3 .. 40 in one launch
    whole = solve(insts, 2)
    check_against_ssp(insts[:1] + insts[3:5], 2, tuple(list(x[:1]) + list(x[3:5]) for x in whole))
    order = [4, 2, 5, 0, 3, 1]
    shuffled = solve([insts[i] for i in order], 2)
    for pos, i in enumerate(order):
        alone = solve([insts[i]], 2)
        for got, k in ((whole, i), (shuffled, pos)):
            assert same(tuple(x[k:k + 1] for x in got), alone)
    assert same(solve(insts, 2), whole)  # two calls: equal bits


def _break_T(rows):
    rows[1, 0] = 41             # more frames than the launch was sized for


def _break_out(rows):
    rows[1, 4] = 2 ** 31 - 64   # an output block past the end of `out`


def _break_link(rows):
    rows[1, 2] = 2 ** 31 - 64   # link blocks past the end of `link`


def _break_gap(rows):
    rows[1, 0] = 2              # max_gap = 2 >= T


@pytest.mark.parametrize('tamper', [_break_T, _break_out, _break_link, _break_gap], ids=['T', 'out', 'link', 'gap'])
def test_a_sequence_outside_the_contract_gets_a_status_and_its_neighbours_are_solved(tamper):
    insts = batch_instances()[:3]
    clean = solve(insts, 2)
    for variant in (0, 2):
        got = solve(insts, 2, variant, 'nan', tamper)
        res, obj, ids, info = got
        assert np.isnan(obj[1]) and info[1].tolist() == [1, 0, 0, 0]
        # nothing else of it was written: its block and its ids are the pre-fill
        assert all(np.isnan(x).all() for x in [res[1][0], res[1][2], res[1][3]] + flat_links(res[1][1])) and (ids[1] == -77).all()
        for k in (0, 2):
            assert same(tuple(x[k:k + 1] for x in got), tuple(x[k:k + 1] for x in clean))
        with pytest.raises(AssociationError, match='sequence 1 not solved: outside the launch contract'):
            _raise_status(info)


def test_a_frame_over_max_n_gets_a_status():
    """a launch sized for max_n = 5, below the frames of the last sequence, [20, 30, 4]"""
    insts = batch_instances()[:3]
    clean = solve(insts, 2)
    got = solve(insts, 2, fill='nan', max_n=5)
    res, obj, ids, info = got
    assert np.isnan(obj[2]) and info[2].tolist() == [1, 0, 0, 0] and (ids[2] == -77).all()
    assert all(np.isnan(x).all() for x in [res[2][0], res[2][2], res[2][3]] + flat_links(res[2][1]))
    assert same(tuple(x[:2] for x in got), tuple(x[:2] for x in clean))


@pytest.mark.parametrize('fill', ['nan', 0xFF])
def test_poisoned_outputs_are_written_in_full(fill):
    insts = variant_instances()
    clean = solve(insts, 3)
    for variant in (0, 1):
        raw = solve(insts, 3, variant, fill, raw=True)
        assert not np.isnan(raw[0]).any() and np.isin(raw[0], (0.0, 1.0)).all() and (raw[2] >= -1).all()
        assert same(solve(insts, 3, variant, fill), clean)


def test_gt_objective():
    rng = np.random.default_rng(61)
    for split, G in (([2, 3, 2], 2), ([6, 5, 7, 4], 3), ([4] * 9, 2), ([3, 0, 4, 2, 5, 1, 0, 2, 3, 4, 2], 3)):
        sc = random_gap_sequence(rng, split, G)
        L = sum(split)
        lab = lambda *s: rng.integers(0, 2, s).astype(np.float32)
        gt = (lab(L), lab(L), lab(L), [[lab(*l.shape) for l in row] for row in sc[3]])
        wobj = milp_gap_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)[1]
        det, links, new, end = _tensors(sc, device='cuda')
        tg = (torch.from_numpy(gt[0]).cuda(), torch.from_numpy(gt[1]).cuda(), torch.from_numpy(gt[2]).cuda(),
              [[torch.from_numpy(g)[None].cuda() for g in row] for row in gt[3]])
        got = _numpy(associate_sequence_gaps(det, links, new, end, split, gt=tg))
        assert gap_feasible(got, split)
        assert same_gap_assignment(got, ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)[0]), split
        # the objective of the shifted scores at the assignment, the constant added, is the oracle's optimum
        eff = lambda g: g + (g == 0) * -1.0
        shifted = (sc[0] - eff(gt[0]), sc[1] - eff(gt[1]), sc[2] - eff(gt[2]),
                   [[l - eff(g) for l, g in zip(row, grow)] for row, grow in zip(sc[3], gt[3])])
        const = sum(float(g.sum()) for g in (gt[0], gt[1], gt[2], *flat_links(gt[3])))
        assert abs(gap_objective(got, *shifted) + const - wobj) <= 1e-5 * max(1.0, abs(wobj))


def test_host_and_device_inputs_return_the_nested_shapes():
    rng = np.random.default_rng(29)
    for split, G in (([1, 1, 1], 2), ([12] * 5, 3), ([7, 40, 3], 1), ([0, 5, 4, 2], 2), ([5, 0, 5], 2), ([3, 2, 4, 1] * 3, 4)):
        sc = random_gap_sequence(rng, split, G, 'eval')
        wobj = lp_gap_route(sc[0], sc[1], sc[2], sc[3], split)[1]
        for dtype in (torch.float32, torch.float64):
            det, links, new, end = _tensors(sc, dtype)
            flat2d = [[l[0] for l in row] for row in links]  # n_t x n_{t+g} blocks
            host = associate_sequence_gaps(det, flat2d, new, end, [torch.tensor([s]) for s in split])
            dev = associate_sequence_gaps(det.cuda(), [[l.cuda() for l in row] for row in links], new.cuda(), end.cuda(), split)
            assert len(host) == len(dev) == 4 and len(host[1]) == len(dev[1]) == G
            for h, d in ((host[0], dev[0]), (host[2], dev[2]), (host[3], dev[3])):
                assert h.shape == det.shape and h.dtype == dtype and h.device.type == 'cpu'
                assert d.shape == det.shape and d.dtype == dtype and d.is_cuda and torch.equal(h, d.cpu())
            for g in range(1, G + 1):
                assert len(host[1][g - 1]) == len(dev[1][g - 1]) == len(split) - g
                for t, (h, d) in enumerate(zip(host[1][g - 1], dev[1][g - 1])):
                    assert h.shape == (split[t], split[t + g]) and d.shape == (1, split[t], split[t + g])
                    assert h.dtype == d.dtype == dtype and d.is_cuda and torch.equal(h, d.cpu()[0])
            got = _numpy(dev)
            assert gap_feasible(got, split) and close(gap_objective(got, *sc), wobj), (split, dtype)


def test_return_ids_and_the_batch_call():
    insts = batch_instances()[:4]
    args = [_tensors(sc, device='cuda') for _, sc in insts]
    res, obj = associate_sequence_gaps_batch([a[0] for a in args], [a[1] for a in args], [a[2] for a in args],
                                             [a[3] for a in args], [s for s, _ in insts], return_objective=True,
                                             return_ids=True)
    assert obj.shape == (4,) and obj.dtype == torch.float64 and obj.is_cuda
    for (s, sc), a, r, o in zip(insts, args, res, obj.cpu().numpy()):
        one = associate_sequence_gaps(a[0], a[1], a[2], a[3], s, return_ids=True)
        assert len(one) == len(r) == 6
        assert all(torch.equal(x, y) for x, y in zip([r[0], r[2], r[3]] + flat_links(r[1]), [one[0], one[2], one[3]] + flat_links(one[1])))
        want = ids_of_gaps(_numpy(one), s)
        for got in (one, r):
            assert len(got[4]) == len(s) and got[5] == int(one[2].sum().item())
            for g, w in zip(got[4], want):
                assert g.dtype == torch.int64 and g.is_cuda and np.array_equal(g.cpu().numpy(), w)
        assert close(o, lp_gap_route(sc[0], sc[1], sc[2], sc[3], s)[1])
    plain = associate_sequence_gaps_batch([a[0] for a in args], [a[1] for a in args], [a[2] for a in args],
                                          [a[3] for a in args], [s for s, _ in insts])
    assert len(plain) == 4 and all(len(r) == 4 for r in plain)


def test_the_c_entry_refuses_before_any_launch():
    lib = _lib.load()
    d = torch.zeros(64, device='cuda')
    i = torch.zeros(64, dtype=torch.int32, device='cuda')
    f64 = torch.zeros(64, dtype=torch.float64, device='cuda')
    p = lambda t: t.data_ptr()
    good = dict(det=p(d), new=p(d), end=p(d), link=p(d), seqs=p(i), nts=p(i), B=1, n_nts=4, max_T=4, max_n=4, max_L=16,
                max_gap=2, n_scores=16, n_link=64, out=p(d), n_out=64, ids=p(i), objective=p(f64), info=p(i), ws=p(f64),
                ws_units=64, stream=None)
    call = lambda **k: lib.mmmot_associate_sequences_gap(*{**good, **k}.values())
    for bad in (dict(det=None), dict(ws=None), dict(B=0), dict(max_T=1), dict(max_T=4097), dict(max_n=0), dict(max_n=513),
                dict(max_L=0), dict(max_L=65537), dict(max_gap=0), dict(max_gap=9), dict(max_gap=4), dict(n_link=-1),
                dict(ws_units=0), dict(ws=p(f64) + 4)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert lib.mmmot_set_sequence_gap_variant(5) == -1 and lib.mmmot_set_sequence_gap_variant(-1) == -1
    assert lib.mmmot_set_sequence_gap_variant(3) == 0
    try:
        assert call(max_L=2305) == -1  # the state of 2305 detections does not fit LDS
    finally:
        assert lib.mmmot_set_sequence_gap_variant(0) == 0
    assert lib.mmmot_associate_sequences_gap.argtypes == _lib.SIGNATURES['mmmot_associate_sequences_gap']
