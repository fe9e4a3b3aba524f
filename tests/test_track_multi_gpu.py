"""The ID step of several sequences in one launch (mmmot_track_ids_multi / mmmot_track_chain_ids_multi through
mmmot::track_ids_multi, mmmot::track_chain_ids_multi and mmmot_amd.tracks) against the single-state ops, which
tests/tracking_ref.py and tests/tracking_chain_ref.py pin: every stream of a multi launch equals its own sequential
single-state launches bit for bit, ids and state; empty streams are left alone; error flags stay with their stream.
Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from association_ref import random_instance
from tracking_chain_ref import load_fixture
from mmmot_amd import _lib
from mmmot_amd.association import associate, chains_table, pairs_table
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import TRACK_STATE_INTS, track_chain_layout, track_layout
from mmmot_amd.tracks import (ECONTRACT, EINFEASIBLE, TrackingError, TrackState, TrackStates, assign_chain_ids, assign_ids,
                              chain_frame_table, frame_table, queue_chain_ids_multi, queue_ids_multi, split_ids_multi,
                              stream_major)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
POISON = -0x5A5A5A5B


def solved_pair(rng, N, M):
    """a pair's solver block [det L | new L | end L | link N*M] from ``associate`` on random scores"""
    det, new, end, link = random_instance(rng, N, M, 1.0, 'eval')
    t = torch.from_numpy
    a = associate(t(det), [t(link).view(1, N, M)], t(new), t(end), [N, M])
    return np.concatenate([x.reshape(-1).numpy() for x in (a[0], a[2], a[3], a[1][0])]).astype(np.float32)


def make_streams(rng, counts_per_stream, first_frame=0):
    """per stream its consecutive pairs: [(block, (N, M), (f0, f1))]; ``counts_per_stream``: per stream the detection
    counts of its frames (k + 1 counts make k pairs)"""
    streams = []
    for counts in counts_per_stream:
        prs = []
        for t in range(len(counts) - 1):
            N, M = counts[t], counts[t + 1]
            prs.append((solved_pair(rng, N, M), (N, M), (first_frame + t, first_frame + t + 1)))
        streams.append(prs)
    return streams


def single_walk(prs, state=None, max_nm=0):
    """a stream through the single-state op, one launch per pair; returns (per pair result, state block)"""
    state = TrackState('cuda') if state is None else state
    res = []
    for blk, split, fr in prs:
        res += assign_ids(state, torch.from_numpy(blk).cuda(), [split], [fr], max_nm)
    return res, state.buf.clone()


def launch_order(streams, stream_of):
    """the groups in the order ``stream_of`` asks for: stream_of[g] takes that stream's next pair"""
    nxt = [0] * len(streams)
    groups = []
    for s in stream_of:
        groups.append(streams[s][nxt[s]])
        nxt[s] += 1
    assert nxt == [len(p) for p in streams]
    return groups


def multi(states, streams, stream_of, max_nm=0):
    groups = launch_order(streams, stream_of)
    blocks = torch.from_numpy(np.concatenate([g[0] for g in groups] + [np.zeros(0, np.float32)])).cuda()
    splits, fidx = [g[1] for g in groups], [g[2] for g in groups]
    flat = queue_ids_multi(states, blocks, splits, fidx, stream_of, max_nm).cpu().numpy()
    return flat, splits


def same_pairs(got, want):
    assert len(got) == len(want)
    for (a0, a1, s, l), (b0, b1, t, m) in zip(got, want):
        assert a0.dtype == b0.dtype and np.array_equal(a0, b0) and np.array_equal(a1, b1) and (s, l) == (t, m)


def per_stream(res, stream_of, S):
    out = [[] for _ in range(S)]
    for r, s in zip(res, stream_of):
        out[s].append(r)
    return out


def test_one_stream_equals_track_ids_bit_for_bit():
    rng = np.random.default_rng(0)
    prs = make_streams(rng, [[4, 6, 0, 3, 5, 5]])[0]
    blocks = torch.from_numpy(np.concatenate([p[0] for p in prs])).cuda()
    table, _ = pairs_table([p[1] for p in prs])
    fidx = frame_table([p[2] for p in prs], len(prs))
    one, many = TrackState('cuda'), TrackStates(1, 'cuda')
    want = torch.ops.mmmot.track_ids(blocks, table, fidx, one.buf, 0)
    got = torch.ops.mmmot.track_ids_multi(blocks, table, fidx, torch.tensor([0, len(prs)], dtype=torch.int32), many.buf, 0)
    assert got.dtype == torch.int32 and torch.equal(got, want) and torch.equal(many[0], one.buf)
    a, b = many.read(0), one.read()
    assert (a['last_id'], a['frame'], a['flags']) == (b['last_id'], b['frame'], b['flags']) and np.array_equal(a['ids'], b['ids'])


def test_four_streams_shuffled_with_an_empty_one():
    """B = 7 pairs split 3 / 0 / 2 / 2 with N, M in 0 .. 6 (N = 0 and M = 0 among them), in a shuffled launch order"""
    rng = np.random.default_rng(1)
    streams = make_streams(rng, [[3, 0, 5, 6], [2], [6, 0, 4], [1, 4, 2]])
    assert [len(s) for s in streams] == [3, 0, 2, 2]
    stream_of = [2, 0, 3, 0, 2, 3, 0]
    states = TrackStates(4, 'cuda')
    pattern = torch.arange(TRACK_STATE_INTS, dtype=torch.int32, device='cuda') * 7 - 100
    pattern[2] = 0   # the flag word, which queue_ids_multi hands back for every stream: no error on record
    states[1].copy_(pattern)   # stream 1 has no pair in the launch: neither read nor written
    flat, splits = multi(states, streams, stream_of)
    got = per_stream(split_ids_multi(flat, splits, stream_of), stream_of, 4)
    assert torch.equal(states[1], pattern)
    for s in (0, 2, 3):
        want, wstate = single_walk(streams[s])
        same_pairs(got[s], want)
        assert torch.equal(states[s], wstate)
        assert states.read(s)['flags'] == 0
    # the table's helpers
    snap = states.snapshot()
    states.reset([0, 3])
    fresh = TrackState('cuda').buf
    assert torch.equal(states[0], fresh) and torch.equal(states[3], fresh) and torch.equal(states[2], snap[2])
    states.restore(snap, [3])
    assert torch.equal(states[3], snap[3]) and torch.equal(states[0], fresh)
    states.restore(snap)
    assert torch.equal(states.buf, snap)
    states.reset()
    assert all(torch.equal(states[s], fresh) for s in range(4))
    # a second launch continues every stream: the rows work as TrackState.buf of the single op too
    flat, splits = multi(states, streams, sorted(stream_of))
    again = per_stream(split_ids_multi(flat, splits, sorted(stream_of)), sorted(stream_of), 4)
    for s in (0, 2, 3):
        same_pairs(again[s], got[s])


def test_four_wave_branch_beside_small_streams():
    """one stream with N = 130 (max_nm > 128: the four-wave kernel for all); the small streams' results are those of the
    one-wave entry"""
    rng = np.random.default_rng(2)
    streams = make_streams(rng, [[3, 5, 2], [130, 6, 131], [4, 4]])
    stream_of = [0, 1, 2, 0, 1]
    states = TrackStates(3, 'cuda')
    flat, splits = multi(states, streams, stream_of)
    got = per_stream(split_ids_multi(flat, splits, stream_of), stream_of, 3)
    for s in range(3):
        want, wstate = single_walk(streams[s])  # max_nm from each pair's own table: one wave for s = 0, 2
        same_pairs(got[s], want)
        assert torch.equal(states[s], wstate)
    # and the small streams alone, through the one-wave multi kernel
    small = TrackStates(3, 'cuda')
    flat, splits = multi(small, [streams[0], [], streams[2]], [0, 2, 0])
    alone = per_stream(split_ids_multi(flat, splits, [0, 2, 0]), [0, 2, 0], 3)
    same_pairs(alone[0], got[0])
    same_pairs(alone[2], got[2])
    assert torch.equal(small[0], states[0]) and torch.equal(small[2], states[2])


def test_infeasible_assignment_stays_with_its_stream():
    rng = np.random.default_rng(3)
    streams = make_streams(rng, [[3, 4, 2], [2, 5], [2, 1, 3], [4, 4]])
    # stream 2, first pair: a kept, non-new second-frame detection with two links
    bad = np.concatenate([[1, 1, 1], [1, 1, 0], [1, 1, 1], np.ones(2)]).astype(np.float32)
    streams[2][0] = (bad, (2, 1), streams[2][0][2])
    stream_of = [0, 1, 2, 3, 0, 2]
    states = TrackStates(4, 'cuda')
    flat, splits = multi(states, streams, stream_of)
    assert [states.read(s)['flags'] for s in range(4)] == [0, 0, EINFEASIBLE, 0]
    with pytest.raises(TrackingError, match='stream 2'):
        split_ids_multi(flat, splits, stream_of)
    flat[-4:] = 0  # read the other streams' words all the same
    got = per_stream(split_ids_multi(flat, splits, stream_of), stream_of, 4)
    for s in (0, 1, 3):
        want, wstate = single_walk(streams[s])
        same_pairs(got[s], want)
        assert torch.equal(states[s], wstate)
    # the flag is sticky, and stays per stream
    flat, splits = multi(states, [streams[0][:0], streams[1][:0], streams[2][1:], streams[3][:0]], [2])
    assert [states.read(s)['flags'] for s in range(4)] == [0, 0, EINFEASIBLE, 0]


def raw_launch(streams, seq_start, states, S, ids_fill=POISON, max_nm=0):
    """the C entry point on a stream-major table with the seq_start given and a poisoned ids buffer"""
    groups = [g for prs in streams for g in prs]
    table, _ = pairs_table([g[1] for g in groups])
    fidx = frame_table([g[2] for g in groups], len(groups))
    blocks = torch.from_numpy(np.concatenate([g[0] for g in groups])).cuda()
    total, off, need = track_layout(table, fidx, blocks.numel())
    ids = torch.full((total,), ids_fill, dtype=torch.int32, device='cuda')
    HipOps().track_ids_multi(blocks, table.reshape(-1).cuda(), off.to(torch.int32).cuda(), fidx.reshape(-1).cuda(),
                             torch.tensor(seq_start, dtype=torch.int32).cuda(), S, len(groups), max_nm or need, states,
                             ids)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), [g[1] for g in groups]


@pytest.mark.parametrize('seq_start', [[0, 3, 5, 4], [0, 3, 5, 8]], ids=['decreasing', 'past_B'])
def test_a_bad_range_is_refused_per_stream(seq_start):
    """ECONTRACT in the stream whose range is decreasing or leaves [0, B]; its ids words keep their poison and the
    other streams are served"""
    rng = np.random.default_rng(4)
    streams = make_streams(rng, [[3, 4, 2, 5], [2, 5, 3], [2, 1, 3]])
    states = TrackStates(3, 'cuda')
    ids, splits = raw_launch(streams, seq_start, states.buf, 3)
    assert [states.read(s)['flags'] for s in range(3)] == [0, 0, ECONTRACT]
    fresh = TrackState('cuda').buf.clone()
    fresh[2] = ECONTRACT
    assert torch.equal(states[2], fresh)   # nothing else of the state moved
    n01 = sum(N + M + 2 for N, M in splits[:5])
    assert (ids[n01:] == POISON).all() and (ids[:n01] != POISON).all()
    got = split_ids_multi(np.concatenate([ids[:n01], [0, 0]]), splits[:5], [0, 0, 0, 1, 1])
    for s, r in enumerate(per_stream(got, [0, 0, 0, 1, 1], 2)):
        want, wstate = single_walk(streams[s])
        same_pairs(r, want)
        assert torch.equal(states[s], wstate)


def test_results_do_not_depend_on_the_other_streams():
    """stream 1 beside two different neighbours: the same words and state"""
    rng = np.random.default_rng(5)
    a = make_streams(rng, [[3, 4, 2], [2, 5, 3, 1], [2, 1, 3]])
    b = make_streams(rng, [[6, 6, 6, 6, 6], [2], [5, 0]])
    b[1] = a[1]
    res = []
    for streams in (a, b):
        states = TrackStates(3, 'cuda')
        order = [s for s, prs in enumerate(streams) for _ in prs]
        flat, splits = multi(states, streams, order)
        res.append((per_stream(split_ids_multi(flat, splits, order), order, 3)[1], states[1].clone()))
    same_pairs(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


# ---- windows ---------------------------------------------------------------------------------------------------------
def chain_fixture(name):
    return load_fixture(os.path.join(GOLDEN, 'track_chain_ids_%s.npz' % name))[0]


def chain_single_walk(wins, state=None):
    state = TrackState('cuda') if state is None else state
    res = []
    for w in wins:
        res += assign_chain_ids(state, torch.from_numpy(w['block']).cuda(), [w['split']], [w['frames']])
    return res, state.buf.clone()


def same_windows(got, want):
    assert len(got) == len(want)
    for (ai, *ar), (bi, *br) in zip(got, want):
        assert len(ai) == len(bi) and all(np.array_equal(x, y) for x, y in zip(ai, bi)) and ar == br


def test_chains_three_streams_with_the_unstored_window():
    """S = 3 with T = 3 and T = 2 windows; stream 0 holds the window whose frame 0 continues the stored frame while its
    frame 1 keeps nothing (``stored`` = 0: window 2 of the roles3 fixture of tests/test_track_chains_gpu.py)"""
    wins0 = chain_fixture('roles3')[:4]
    res0, _ = chain_single_walk(wins0)
    assert [(start, stored) for _, start, _, stored in res0][2] == (1, 0), 'the stored = 0 window is in the input'
    t3 = chain_fixture('kitti3')[:3]
    rng = np.random.default_rng(6)
    t2 = [dict(split=list(p[1]), frames=list(p[2]), block=p[0]) for p in make_streams(rng, [[3, 4, 0, 2]])[0]]
    streams = [wins0, t3, t2]
    assert {len(w['split']) for prs in streams for w in prs} >= {2, 3}
    stream_of = []
    for k in range(max(len(s) for s in streams)):
        stream_of += [s for s in (2, 0, 1) if k < len(streams[s])]
    nxt, groups = [0, 0, 0], []
    for s in stream_of:
        groups.append(streams[s][nxt[s]])
        nxt[s] += 1
    states = TrackStates(3, 'cuda')
    blocks = torch.from_numpy(np.concatenate([w['block'] for w in groups])).cuda()
    splits = [list(w['split']) for w in groups]
    flat = queue_chain_ids_multi(states, blocks, splits, [list(w['frames']) for w in groups], stream_of).cpu().numpy()
    got = per_stream(split_ids_multi(flat, splits, stream_of, tail=3), stream_of, 3)
    for s in range(3):
        want, wstate = chain_single_walk(streams[s])
        same_windows(got[s], want)
        assert torch.equal(states[s], wstate)


def test_pair_and_window_launches_alternate_on_one_table():
    rng = np.random.default_rng(7)
    counts = [[3, 4, 2, 5, 3, 4], [2, 0, 3, 3, 1, 2]]
    # per stream: a pair (frames 0 1), a window (1 2 3), a pair (3 4), a two-frame window (4 5)
    pieces = [[0, 1], [1, 2, 3], [3, 4], [4, 5]]
    from association_chain_ref import milp_route, random_chain
    work = []
    for c in counts:
        row = []
        for fr in pieces:
            split = [c[f] for f in fr]
            det, new, end, links = random_chain(rng, split, 1.0, 'eval')
            (a_det, a_links, a_new, a_end), _ = milp_route(det, new, end, links, split)
            row.append((np.concatenate([a_det, a_new, a_end] + [l.reshape(-1) for l in a_links]).astype(np.float32),
                        split, fr))
        work.append(row)
    states, singles = TrackStates(2, 'cuda'), [TrackState('cuda'), TrackState('cuda')]
    for k, fr in enumerate(pieces):
        blocks = torch.from_numpy(np.concatenate([work[s][k][0] for s in (0, 1)])).cuda()
        splits = [work[s][k][1] for s in (0, 1)]
        as_pair = k in (0, 2)
        if as_pair:
            flat = queue_ids_multi(states, blocks, [tuple(s) for s in splits], [tuple(fr)] * 2, [0, 1]).cpu().numpy()
            got = split_ids_multi(flat, splits, [0, 1])
        else:
            flat = queue_chain_ids_multi(states, blocks, splits, [fr] * 2, [0, 1]).cpu().numpy()
            got = split_ids_multi(flat, splits, [0, 1], tail=3)
        for s in (0, 1):
            blk = torch.from_numpy(work[s][k][0]).cuda()
            if as_pair:
                same_pairs([got[s]], assign_ids(singles[s], blk, [tuple(splits[s])], [tuple(fr)]))
            else:
                same_windows([got[s]], assign_chain_ids(singles[s], blk, [splits[s]], [fr]))
            assert torch.equal(states[s], singles[s].buf)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_einval_before_any_launch():
    lib = _lib.load()
    z = torch.zeros(2 * TRACK_STATE_INTS, dtype=torch.int32, device='cuda')
    f = torch.zeros(16, device='cuda')
    p, q = z.data_ptr(), f.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    for fn in (lib.mmmot_track_ids_multi, lib.mmmot_track_chain_ids_multi):
        ok = [q, p, p, p, p, 1, 1, 4, p, p, stream]
        for i in (0, 1, 2, 3, 4, 8, 9):   # a null pointer
            bad = list(ok)
            bad[i] = None
            assert fn(*bad) == -1
        for i, v in ((5, 0), (6, 0), (7, 513), (7, -1)):  # S = 0, B = 0, max_nm = 513, max_nm < 0
            bad = list(ok)
            bad[i] = v
            assert fn(*bad) == -1
    torch.cuda.synchronize()
    assert not z.any()


def test_op_checks_and_meta_kernels():
    states = TrackStates(2, 'cuda')
    table, _ = pairs_table([(2, 3), (1, 1)])
    fidx = frame_table([(0, 1), (0, 1)], 2)
    ss = torch.tensor([0, 1, 2], dtype=torch.int32)
    blocks = torch.zeros(3 * 5 + 6 + 3 * 2 + 1, device='cuda')
    assert torch.ops.mmmot.track_ids_multi(blocks, table, fidx, ss, states.buf, 0).shape == (7 + 4,)
    m = torch.ops.mmmot.track_ids_multi(blocks.to('meta'), table, fidx, ss, states.buf.to('meta'), 0)
    assert m.device.type == 'meta' and m.dtype == torch.int32 and m.shape == (7 + 4,)
    ctab, _ = chains_table([[2, 3, 1], [1, 1]])
    cfidx = chain_frame_table([[0, 1, 2], [0, 1]], [[2, 3, 1], [1, 1]])
    cblocks = torch.zeros(3 * 6 + 6 + 3 + 3 * 2 + 1, device='cuda')
    assert torch.ops.mmmot.track_chain_ids_multi(cblocks, ctab, cfidx, ss, states.buf, 0).shape == (9 + 5,)
    m = torch.ops.mmmot.track_chain_ids_multi(cblocks.to('meta'), ctab, cfidx, ss, states.buf.to('meta'), 0)
    assert m.device.type == 'meta' and m.dtype == torch.int32 and m.shape == (9 + 5,)
    total, _, _ = track_chain_layout(ctab, cfidx)
    assert total == 14
    states.reset()
    for bad_ss in (ss[:2], ss.to(torch.int64), ss.cuda()):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.mmmot.track_ids_multi(blocks, table, fidx, bad_ss, states.buf, 0)
    for bad_states in (states.buf[0], states.buf[:, :-1], states.buf.to(torch.int64)):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.mmmot.track_ids_multi(blocks, table, fidx, ss, bad_states, 0)
    with pytest.raises(ValueError):
        torch.ops.mmmot.track_ids_multi(blocks, table, fidx, ss, states.buf, 2)   # max_nm below the table
    with pytest.raises(ValueError):
        queue_ids_multi(states, blocks, [(2, 3), (1, 1)], [(0, 1), (0, 1)], [0, 2])  # a stream the table does not have
    with pytest.raises(ValueError):
        queue_ids_multi(states, blocks, [(2, 3), (1, 1)], [(0, 1), (0, 1)], [0])
    with pytest.raises(ValueError):
        TrackStates(0, 'cuda')
    assert torch.equal(states.buf, TrackStates(2, 'cuda').buf)
    order, seq = stream_major([1, 0, 1], 3)
    assert order.tolist() == [1, 0, 2] and seq.tolist() == [0, 1, 3, 3]
