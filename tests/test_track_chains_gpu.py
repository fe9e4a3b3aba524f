"""Track IDs of windows of 2 .. 8 frames on the device (csrc/track_ids.hip through mmmot::track_chain_ids /
mmmot_amd.tracks) against the fixtures the reference produced (tests/golden/track_chain_ids_*.npz): exact IDs,
frame_start and last_id after every window and the final tracks, whatever the launch size and the kernel; two-frame
windows against mmmot::track_ids bit for bit; state and outputs written in full; the error flag; the drop-in on host and
device tensors; queue_solve_chains; and SequencePipeline(window=3) against tests/tracking_chain_ref.py.  Every
comparison is exact."""
import glob
import os

import numpy as np
import pytest
import torch

import tracking_ref
from association_chain_ref import feasible, milp_route, random_chain
from tracking_chain_ref import ChainTracker, check_final, check_window, load_fixture, tracks_of_windows
from mmmot_amd import TrackingNet
from mmmot_amd.association import chains_table
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import TRACK_STATE_HEAD, TRACK_STATE_INTS, track_chain_layout
from mmmot_amd.tracks import (TrackingError, TrackState, assign_chain_ids, assign_ids, chain_frame_table,
                              track_chain_ids, window_starts)
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'track_chain_ids_*.npz')))
NAMES = [os.path.basename(f)[len('track_chain_ids_'):-4] for f in FIXTURES]
PAIR_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'track_ids_*.npz')))
PAIR_NAMES = [os.path.basename(f)[len('track_ids_'):-4] for f in PAIR_FIXTURES]


def fixture(name):
    return load_fixture(os.path.join(GOLDEN, 'track_chain_ids_%s.npz' % name))


def launch(state, grp, max_n=0):
    blocks = torch.from_numpy(np.concatenate([w['block'] for w in grp])).cuda()
    got = assign_chain_ids(state, blocks, [w['split'] for w in grp], [w['frames'] for w in grp], max_n)
    assert len(got) == len(grp)
    return got


def walk(wins, B, max_n=0, state=None, check=True, tracks=None):
    """the sequence through assign_chain_ids in launches of B windows; returns the state"""
    state = TrackState('cuda') if state is None else state
    for g in range(0, len(wins), B):
        grp = wins[g:g + B]
        for w, (ids, start, last, stored) in zip(grp, launch(state, grp, max_n)):
            if check:
                check_window(w, ids, start, last)
            if tracks is not None and stored:
                tracks.update(list(zip(w['frames'], ids))[start:])
    return state


@pytest.mark.parametrize('variant', ['auto', 'four_waves'])
@pytest.mark.parametrize('B', [1, 4, 0], ids=['B1', 'B4', 'whole'])
@pytest.mark.parametrize('path', FIXTURES, ids=NAMES)
def test_fixture_sequences_equal_the_reference(path, B, variant):
    wins, z = load_fixture(path)
    tracks = {}
    state = walk(wins, B or len(wins), 0 if variant == 'auto' else 512, tracks=tracks)
    s = state.read()
    assert s['flags'] == 0 and s['last_id'] == int(z['last_id'][-1])
    check_final(z, tracks)


@pytest.mark.parametrize('path', PAIR_FIXTURES, ids=PAIR_NAMES)
def test_two_frame_windows_equal_track_ids_bit_for_bit(path):
    pairs, _ = tracking_ref.load_fixture(path)
    for B in (1, 3, len(pairs)):
        a, b = TrackState('cuda'), TrackState('cuda')
        for g in range(0, len(pairs), B):
            grp = pairs[g:g + B]
            blocks = torch.from_numpy(np.concatenate([p['block'] for p in grp])).cuda()
            want = assign_ids(a, blocks, [(p['N'], p['M']) for p in grp], [(p['f0'], p['f1']) for p in grp])
            got = assign_chain_ids(b, blocks, [[p['N'], p['M']] for p in grp], [[p['f0'], p['f1']] for p in grp])
            for (i0, i1, s, l), (ids, start, last, stored) in zip(want, got):
                assert np.array_equal(ids[0], i0) and np.array_equal(ids[1], i1) and (start, last) == (s, l)
                assert stored == int(not s or (i1 >= 0).any())
            assert torch.equal(a.buf, b.buf)


def pairs_of(w):
    """a window's assignment as T - 1 pair blocks [det N+M | new | end | link]: what mmmot::track_ids walks"""
    st = np.concatenate([[0], np.cumsum(w['split'])])
    res = []
    for t in range(w['T'] - 1):
        d = slice(st[t], st[t + 2])
        blk = np.concatenate([w['det'][d], w['new'][d], w['end'][d], w['links'][t].reshape(-1)]).astype(np.float32)
        res.append((blk, (w['split'][t], w['split'][t + 1]), (w['frames'][t], w['frames'][t + 1])))
    return res


def test_pair_and_window_launches_alternate_on_one_state():
    """kitti3 cut into mixed pieces: some windows through window launches, the others pair by pair through
    mmmot::track_ids on the SAME state, give the tracks and the last ID of the all-window walk.  (A window walked as
    pairs must keep a detection in every frame: only there the two kernels' storing rules agree - the quirk.)"""
    wins, z = fixture('kitti3')
    want = {}
    want_state = walk(wins, len(wins), tracks=want)
    as_pairs = {1, 2, 6, 9, 10, 11, 12, 15, 18}
    st = lambda w: np.concatenate([[0], np.cumsum(w['split'])])
    for i in as_pairs:
        assert all((wins[i]['det'][a:b] == 1).any() for a, b in zip(st(wins[i])[:-1], st(wins[i])[1:]))
    state, tracks, i = TrackState('cuda'), {}, 0
    while i < len(wins):
        if i in as_pairs:
            prs = pairs_of(wins[i])
            blocks = torch.from_numpy(np.concatenate([p[0] for p in prs])).cuda()
            for (_, _, (f0, f1)), (i0, i1, s, _) in zip(prs, assign_ids(state, blocks, [p[1] for p in prs],
                                                                          [p[2] for p in prs])):
                if not s:
                    tracks[f0] = i0
                tracks[f1] = i1
            i += 1
        else:
            j = i
            while j < len(wins) and j not in as_pairs and j - i < 3:
                j += 1
            for w, (ids, start, _, stored) in zip(wins[i:j], launch(state, wins[i:j])):
                if stored:
                    tracks.update(list(zip(w['frames'], ids))[start:])
            i = j
    assert sorted(tracks) == sorted(want) and all(np.array_equal(tracks[f], want[f]) for f in want)
    assert torch.equal(state.buf, want_state.buf)
    check_final(z, tracks)


def test_pair_launches_continue_a_window_sequence():
    """the same frames through both kernels: a window launch, then PAIR launches that continue from the frame it stored
    (and back) give the tracks of the restatement walking the same mixed pieces"""
    rng = np.random.default_rng(21)
    counts = [int(rng.integers(4, 9)) for _ in range(9)]
    pieces = [[0, 1, 2], [2, 3], [3, 4], [4, 5, 6, 7], [7, 8]]
    state, ct = TrackState('cuda'), ChainTracker()
    for fr in pieces:
        split = [counts[f] for f in fr]
        det, new, end, links = random_chain(rng, split, 1.0, 'eval')
        (a_det, a_links, a_new, a_end), _ = milp_route(det, new, end, links, split)
        assert feasible((a_det, a_links, a_new, a_end), split)
        block = torch.from_numpy(np.concatenate([a_det, a_new, a_end] + [l.reshape(-1) for l in a_links])
                                 .astype(np.float32)).cuda()
        wi, ws, _ = ct.window(a_det, a_links, a_new, split, fr)
        if len(fr) == 2:
            i0, i1, s, l = assign_ids(state, block, [tuple(split)], [tuple(fr)])[0]
            got = [i0, i1]
        else:
            got, s, l, _ = assign_chain_ids(state, block, [split], [fr])[0]
        assert all(np.array_equal(x, y) for x, y in zip(got, wi)) and (s, l) == (ws, ct.last_id)
    assert state.read()['frame'] == 8 and ct.last_id > 8


@pytest.mark.parametrize('name', NAMES)
def test_state_after_one_launch_equals_state_after_single_launches(name):
    wins, _ = fixture(name)
    one = walk(wins, len(wins), check=False).buf.cpu()
    many = walk(wins, 1, check=False).buf.cpu()
    mixed = walk(wins, 3, 512, check=False).buf.cpu()
    assert torch.equal(one, many) and torch.equal(one, mixed)


@pytest.mark.parametrize('fill', [0xFF, 0x7B])
@pytest.mark.parametrize('max_n', [0, 512])
def test_workspace_poison_ids_and_state_written_in_full(fill, max_n):
    """the raw entry point over poisoned buffers: every output int and the whole state block are written"""
    ops = HipOps()
    for name in ('roles5', 'waves'):
        wins, _ = fixture(name)
        table, _ = chains_table([w['split'] for w in wins])
        fidx = chain_frame_table([w['frames'] for w in wins], [w['split'] for w in wins])
        blocks = torch.from_numpy(np.concatenate([w['block'] for w in wins])).cuda()
        total, off, need = track_chain_layout(table, fidx, blocks.numel())
        res = []
        for f in (0, fill):
            ids = torch.empty(total, dtype=torch.int32, device='cuda')
            state = torch.empty(TRACK_STATE_INTS, dtype=torch.int32, device='cuda')
            ids.view(torch.uint8).fill_(f)
            state.view(torch.uint8).fill_(f)
            state[:TRACK_STATE_HEAD] = torch.tensor([0, -1, 0, 0], dtype=torch.int32)  # a new sequence; the IDs stay poisoned
            ops.track_chain_ids(blocks, table.reshape(-1).cuda(), off.to(torch.int32).cuda(), fidx.reshape(-1).cuda(),
                                len(wins), max_n or need, state, ids)
            torch.cuda.synchronize()
            res.append((ids.cpu(), state.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert torch.equal(res[1][1], walk(wins, len(wins)).buf.cpu())
        o = 0
        for w in wins:  # and they are the reference's
            L = sum(w['split'])
            r = res[1][0][o:o + L + 3].numpy()
            st = np.concatenate([[0], np.cumsum(w['split'])])
            check_window(w, [r[a:b] for a, b in zip(st[:-1], st[1:])], int(r[L]), int(r[L + 1]))
            assert r[L + 2] in (0, 1)
            o += L + 3
        assert o == total


def edited(kind, t):
    """a feasible solver output of a T = 4 window (from the fixture) edited in ONE place at frame t"""
    wins, _ = fixture('t8')
    w = wins[0]
    T = 4
    split = w['split'][:T]
    st = np.concatenate([[0], np.cumsum(split)])
    L8, L = sum(w['split']), int(st[-1])
    det, new = w['det'][:L].copy(), w['new'][:L].copy()
    end = w['end'][:L].copy()
    links = [l.copy() for l in w['links'][:T - 1]]
    end[st[T - 1]:] = det[st[T - 1]:]  # cut behind frame 3: its kept detections end there (still a solver output)
    assert feasible((det, links, new, end), split) and L8 > L
    cols = [j for j in range(split[t]) if det[st[t] + j] == 1 and new[st[t] + j] == 0]
    assert cols, 'the fixture has a linked detection in frame %d' % t
    j = cols[0]
    i = int(np.flatnonzero(links[t - 1][:, j] == 1)[0])
    if kind == 'no_link':
        links[t - 1][i, j] = 0
    elif kind == 'two_links':
        links[t - 1][(i + 1) % split[t - 1], j] = 1
        assert split[t - 1] > 1
    else:  # linked from a rejected row
        det[st[t - 1] + i] = 0
    return split, np.concatenate([det, new, end] + [l.reshape(-1) for l in links]).astype(np.float32)


@pytest.mark.parametrize('t', [1, 3], ids=['t1', 'tlast'])
@pytest.mark.parametrize('kind', ['no_link', 'two_links', 'rejected_row'])
def test_infeasible_assignment_sets_the_flag_and_raises(kind, t):
    """an error return, not a device fault: the flag is set, TrackingError is raised, and later windows stay valid"""
    split, block = edited(kind, t)
    state = TrackState('cuda')
    with pytest.raises(TrackingError):
        assign_chain_ids(state, torch.from_numpy(block).cuda(), [split], [[0, 1, 2, 3]])
    assert state.read()['flags'] == 1
    # a launch of [bad window | good windows]: the flag comes back, and the good windows' outputs are those of the
    # restatement walking them behind the bad window's last ID
    wins, _ = fixture('roles3')
    blocks = torch.from_numpy(np.concatenate([block] + [w['block'] for w in wins])).cuda()
    state.reset()
    table, _ = chains_table([split] + [w['split'] for w in wins])
    fidx = chain_frame_table([[100, 101, 102, 103]] + [w['frames'] for w in wins], [split] + [w['split'] for w in wins])
    ids = torch.ops.mmmot.track_chain_ids(blocks, table, fidx, state.buf, 0).cpu().numpy()
    assert state.read()['flags'] == 1
    o = sum(split) + 3
    bad_last = int(ids[o - 2])
    ct = ChainTracker()
    ct.stored, ct.last_id, ct.stored_ids = 103, bad_last, np.zeros(0, np.int64)  # the bad window is a discontinuity
    for w in wins:
        L = sum(w['split'])
        wi, ws, wst = ct.window(w['det'], w['links'], w['new'], w['split'], w['frames'])
        assert np.array_equal(ids[o:o + L], np.concatenate(wi)) and tuple(ids[o + L:o + L + 3]) == (ws, ct.last_id, wst)
        o += L + 3
    assert o == len(ids)
    state.reset()
    assert torch.equal(state.buf.cpu(), TrackState('cuda').buf.cpu())
    walk(wins, 4)


def test_drop_in_raises_on_an_infeasible_window():
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    with pytest.raises(TrackingError):
        track_chain_ids(TrackState('cuda'), t([1, 1, 1]), [torch.ones(1, 1, 1), torch.zeros(1, 1, 1)], t([1, 0, 0]),
                        t([0, 0, 1]), [1, 1, 1], (0, 1, 2))


def test_table_checks_come_before_any_launch():
    state = TrackState('cuda')
    blocks = torch.zeros(3 * 7 + 6 + 6, device='cuda')
    ok = ([[2, 3, 2]], [[0, 1, 2]])
    assign_chain_ids(state, blocks, *ok)
    state.reset()
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, [[2, 513, 2]], [[0, 1, 2]])
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, [[2]], [[0]])                          # T = 1
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, [[1] * 9], [list(range(9))])            # T = 9
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks[:20], *ok)                               # the blocks are shorter than the table says
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, ok[0], [[0, 1, 2], [2, 3, 4]])          # frame indices for another number of windows
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, ok[0], [[0, 1]])                        # .. of frames
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, ok[0], [[0, -1, 2]])
    with pytest.raises(ValueError):
        assign_chain_ids(state, blocks, *ok, max_n=2)
    table, _ = chains_table(ok[0])
    fidx = chain_frame_table(ok[1], ok[0])
    for bad_state in (state.buf[:-1], state.buf.to(torch.int64), state.buf.cpu()):
        with pytest.raises((ValueError, RuntimeError)):
            torch.ops.mmmot.track_chain_ids(blocks, table, fidx, bad_state, 0)
    with pytest.raises(ValueError):
        torch.ops.mmmot.track_chain_ids(blocks, table.to(torch.int64), fidx, state.buf, 0)
    with pytest.raises(ValueError):
        torch.ops.mmmot.track_chain_ids(blocks, table, fidx[:, :2].contiguous(), state.buf, 0)
    assert torch.equal(state.buf.cpu(), TrackState('cuda').buf.cpu())


@pytest.mark.parametrize('name', ['roles5', 'kitti3'])
def test_track_chain_ids_host_and_device_tensors(name):
    wins, z = fixture(name)
    host, dev = TrackState('cuda'), TrackState('cuda')
    t = torch.from_numpy
    for w in wins:
        sp = w['split']
        args = (t(w['det']), [t(l).view(1, *l.shape) for l in w['links']], t(w['new']), t(w['end']))
        split = [torch.tensor([n]) for n in sp]
        a, sa = track_chain_ids(host, *args, split, w['frames'])
        cu = (args[0].cuda(), [l.cuda() for l in args[1]], args[2].cuda(), args[3].cuda())
        b, sb = track_chain_ids(dev, *cu, split, w['frames'])
        assert sa == sb == w['frame_start'] and len(a) == len(b) == len(w['emitted']) == w['T'] - sa
        for x, y, e, n in zip(a, b, w['emitted'], sp[sa:]):
            assert x.dtype == torch.int64 and x.device.type == 'cpu' and x.shape == (n,) and torch.equal(x, y)
            assert np.array_equal(x.numpy()[x.numpy() >= 0], e)
    assert torch.equal(host.buf.cpu(), dev.buf.cpu()) and host.read()['last_id'] == wins[-1]['last_id']


def test_queue_solve_chains_with_empty_frames():
    """frames without detections inside a window go to the device with it; the IDs come from the kernel and one state"""
    from mmmot_amd.tracker_glue import ChainResult, queue_solve_chains
    rng = np.random.default_rng(3)
    t = lambda x: torch.from_numpy(x).cuda()
    state, ref = TrackState('cuda'), ChainTracker()
    wins = [([4, 0, 3], [0, 1, 2]), ([3, 5, 0], [2, 3, 4]), ([0, 2, 2], [4, 5, 6])]
    sels = []
    for split, _ in wins:
        det, new, end, links = random_chain(rng, split, 1.0, 'eval')
        sels.append((t(det), [t(l).view(1, *l.shape) for l in links], t(new), t(end)))

    def check(res, with_ids):
        for (split, fr), sel, r in zip(wins, sels, res):
            assert isinstance(r, ChainResult)
            for x, y in zip((r.scores[0], r.scores[2], r.scores[3], *r.scores[1]), (sel[0], sel[2], sel[3], *sel[1])):
                assert x.device.type == 'cpu' and torch.equal(x, y.cpu())
            a = r.assignment
            assert feasible((a[0].numpy(), [l[0].numpy() for l in a[1]], a[2].numpy(), a[3].numpy()), split)
            if with_ids:
                wi, ws, wst = ref.window(a[0].numpy(), [l[0].numpy() for l in a[1]], a[2].numpy(), split, fr)
                ids, start, last, stored = r.ids
                assert all(np.array_equal(x, y) for x, y in zip(ids, wi)) and (start, last, stored) == (ws, ref.last_id, wst)
            else:
                assert r.ids is None
    # window after window on one state, then all three in one launch on a new one: the same results
    one = [queue_solve_chains([sel], [split], track=state, frame_idx=[fr]).fetch()[0] for sel, (split, fr) in zip(sels, wins)]
    check(one, True)
    ref, state2 = ChainTracker(), TrackState('cuda')
    many = queue_solve_chains(sels, [s for s, _ in wins], track=state2, frame_idx=[f for _, f in wins]).fetch()
    check(many, True)
    assert torch.equal(state.buf, state2.buf)
    plain = queue_solve_chains(sels, [s for s, _ in wins]).fetch()
    check(plain, False)
    for a, b in zip(plain, many):
        assert all(torch.equal(x, y) for x, y in zip((a[1][0], a[1][2], a[1][3], *a[1][1]), (b[1][0], b[1][2], b[1][3], *b[1][1])))


def test_queue_solve_chains_answers_an_empty_window_on_the_host():
    from mmmot_amd.tracker_glue import queue_solve_chains
    rng = np.random.default_rng(4)
    t = lambda x: torch.from_numpy(x).cuda()
    state, ref = TrackState('cuda'), ChainTracker()
    wins = [([2, 3, 1], [0, 1, 2]), ([0, 0, 0], [3, 4, 5]), ([0, 2], [5, 6])]
    sels = []
    for split, _ in wins:
        det, new, end, links = random_chain(rng, split, 1.0, 'eval')
        sels.append((t(det), [t(l).view(1, *l.shape) for l in links], t(new), t(end)))
    res = queue_solve_chains(sels, [s for s, _ in wins], track=state, frame_idx=[f for _, f in wins]).fetch()
    assert res[1].assignment[0].numel() == 0 and [tuple(l.shape) for l in res[1].assignment[1]] == [(1, 0, 0)] * 2
    for (split, fr), r in zip(wins, res):
        a = r.assignment
        wi, ws, wst = ref.window(a[0].numpy(), [l[0].numpy() for l in a[1]], a[2].numpy(), split, fr)
        assert all(np.array_equal(x, y) for x, y in zip(r.ids[0], wi)) and r.ids[1:] == (ws, ref.last_id, wst)
    only = queue_solve_chains(sels[1:2], [wins[1][0]]).fetch()   # nothing on the device at all
    assert only[0].ids is None and only[0].scores[0].numel() == 0


# ---- end to end: SequencePipeline(window=3) --------------------------------------------------------------------------
KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True, appear_fpn=False,
          point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg', test_mode=2,
          neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='A', affinity_op='multiply',
          softmax_mode='none')
S = 64
_FEEDS, _MODEL = [], []


def feeds():
    if not _FEEDS:
        from mmmot_amd.pipeline import FrameFeed
        from mmmot_amd.synth import make_frame
        _FEEDS.extend(FrameFeed(*make_frame(300 + t, 20000, 4 + t % 4)) for t in range(11))
    return _FEEDS


def model():
    if not _MODEL:
        m = TrackingNet(**KW)
        init_module(m, seed=0)
        _MODEL.append(m.eval().cuda())
    return _MODEL[0]


def flat_of(r):
    sc, a = r
    return [sc[0], sc[2], sc[3], *sc[1], a[0], a[2], a[3], *a[1]]


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        fx, fy = flat_of(x), flat_of(y)
        assert len(fx) == len(fy) and all(torch.equal(p, q) for p, q in zip(fx, fy))


def same_tracks(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == np.int64 and np.array_equal(x, y), (x, y)


def ref_window_tracks(res, fs, window):
    wins = [list(range(s, s + k)) for s, k in window_starts(len(fs), window)]
    assert len(res) == len(wins)
    return tracks_of_windows([(a[0].numpy(), [l[0].numpy() for l in a[1]], a[2].numpy()) for _, a in res], wins,
                             [len(f.dets['bbox']) for f in fs])


def test_sequence_pipeline_window_3_in_two_orders():
    from mmmot_amd.pipeline import SequencePipeline
    fs, m = feeds(), model()
    counts = [len(f.dets['bbox']) for f in fs]
    runs = {'run': lambda p, **k: p.run(fs, **k),
            'offline': lambda p, **k: p.run_offline(fs, frames_per_encode=4, windows_per_forward=2, **k)}
    results, tracks = {}, {}
    for name, run in runs.items():
        pipe = SequencePipeline(m, S, associate=True, track=True, window=3)
        seen, scored, assigned = [], [], []
        got = run(pipe, on_tracks=lambda t, ids: seen.append((t, ids.copy())), on_scores=lambda t, sc: scored.append(t),
                  on_assign=lambda t, a: assigned.append(t))
        assert len(got) == 5 and scored == assigned == [2, 4, 6, 8, 10]   # the index of each window's last frame
        for (s, k), (sc, a) in zip(window_starts(len(fs), 3), got):
            split = counts[s:s + k]
            assert sc[0].numel() == sum(split) and [tuple(l.shape) for l in a[1]] == [(1, x, y) for x, y in
                                                                                      zip(split[:-1], split[1:])]
            assert feasible((a[0].numpy(), [l[0].numpy() for l in a[1]], a[2].numpy(), a[3].numpy()), split)
        assert len(pipe.tracks) == len(fs) and all(len(x) == n for x, n in zip(pipe.tracks, counts))
        want = ref_window_tracks(got, fs, 3)
        same_tracks(pipe.tracks, want)
        last = {}
        for t, ids in seen:   # the callback saw every stored frame, and its last emission is what stands
            last[t] = ids
        tr = ChainTracker()
        stored = set()
        for (s, k), (_, a) in zip(window_starts(len(fs), 3), got):
            _, start, st = tr.window(a[0].numpy(), [l[0].numpy() for l in a[1]], a[2].numpy(), counts[s:s + k],
                                     list(range(s, s + k)))
            if st:
                stored.update(range(s + start, s + k))
        assert set(last) == stored and all(np.array_equal(last[t], pipe.tracks[t]) for t in last)
        results[name], tracks[name] = got, [x.copy() for x in pipe.tracks]
        # scores and assignments do not depend on the ID step
        same_results(run(SequencePipeline(m, S, associate=True, window=3)), got)
        # a second run on the same pipeline starts a new sequence
        run(pipe)
        same_tracks(pipe.tracks, tracks[name])
    same_results(results['run'], results['offline'])
    same_tracks(tracks['run'], tracks['offline'])
    assert any((x >= 0).any() for x in tracks['run'])
    # scores alone without associate: the same scores
    plain = SequencePipeline(m, S, window=3).run(fs)
    for sc, (want, _) in zip(plain, results['run']):
        assert all(torch.equal(x, y) for x, y in zip((sc[0], sc[2], sc[3], *sc[1]), (want[0], want[2], want[3], *want[1])))


def test_window_2_is_the_default_pipeline():
    from mmmot_amd.pipeline import SequencePipeline
    fs, m = feeds()[:6], model()
    a = SequencePipeline(m, S, associate=True, track=True)
    b = SequencePipeline(m, S, associate=True, track=True, window=2)
    ra, rb = a.run(fs), b.run(fs)
    same_results(ra, rb)
    same_tracks(a.tracks, b.tracks)
    same_results(a.run_offline(fs, frames_per_encode=4), b.run_offline(fs, frames_per_encode=4, windows_per_forward=2))
    same_tracks(a.tracks, b.tracks)
    assert a.stats == b.stats


def posed(fs):
    """the feeds with a camera that drives and turns: a pose per frame and the IMU calibration the alignment needs"""
    from mmmot_amd.pipeline import FrameFeed
    from mmmot_amd.synth import KITTI_IMU2VELO, ego_poses
    out = []
    for f, pose in zip(fs, ego_poses(len(fs), 1)):
        info = dict(f.info)
        info['calib/Tr_imu_to_velo'] = KITTI_IMU2VELO
        out.append(FrameFeed(f.img.numpy(), f.sweep.numpy(), info, f.dets, pose=pose))
    return out


def test_posed_sequence_window_3_equals_a_host_composition():
    """each window's frame k aligned to its frame 0 by the k accumulated steps: against mmmot_amd.points.align_points
    per frame and model.forward per window"""
    from mmmot_amd import ego
    from mmmot_amd.pipeline import SequencePipeline
    from mmmot_amd.points import align_points
    from mmmot_amd.tracker_glue import scores_for_solver
    fs, m = posed(feeds()[:6]), model()
    pipe = SequencePipeline(m, S, window=3)
    got = pipe.run(fs)
    assert len(got) == 3 and [len(g[1]) for g in got] == [2, 2, 1]   # frames (0 1 2) (2 3 4) (4 5)
    off = SequencePipeline(m, S, window=3).run_offline(fs, frames_per_encode=4, windows_per_forward=2)
    still = SequencePipeline(m, S, window=3).run(feeds()[:6])
    moved = False
    prep = SequencePipeline(m, S, overlap=False, window=3)
    for (s, k), g, o, q in zip(window_starts(len(fs), 3), got, off, still):
        fr = [prep.prepare(f) for f in fs[s:s + k]]
        R, T, pts = [], [], [fr[0]['points']]
        for j in range(1, k):
            r, t = ego.pair_motion(fs[s + j - 1].pose, fs[s + j].pose)
            R.append(r)
            T.append(t)
            pts.append(align_points(R, T, fs[s + j].info['calib/Tr_imu_to_velo'], fr[j]['points']))
        info = {'points': torch.cat(pts).unsqueeze(0),
                'points_split': torch.from_numpy(SequencePipeline._window_split(fr).astype(np.float32)).unsqueeze(0)}
        with torch.no_grad():
            out = m(torch.cat([f['crops'] for f in fr]), info, [torch.tensor([f['n']]) for f in fr])
        want = scores_for_solver(out[0], out[1], out[2], out[3], m.test_mode)
        for a, b, c in zip((g[0], g[2], g[3], *g[1]), (want[0], want[2], want[3], *want[1]), (o[0], o[2], o[3], *o[1])):
            assert torch.equal(a, b) and torch.equal(a, c)
        moved = moved or any(not torch.equal(a, b) for a, b in zip((g[0], *g[1]), (q[0], *q[1])))
    assert moved, 'the poses change the scores'


def test_window_argument_refusals():
    from mmmot_amd import ego
    from mmmot_amd.pipeline import SequencePipeline
    m = model()
    assert ego.MAX_CHAIN == 4
    with pytest.raises(ValueError, match='window'):
        SequencePipeline(m, S, window=6).run(posed(feeds()[:7]))
    with pytest.raises(ValueError, match='window'):
        SequencePipeline(m, S, window=6).run_offline(posed(feeds()[:7]))
    with pytest.raises(ValueError, match='reuse_appearance'):
        SequencePipeline(m, S, window=3, reuse_appearance=True).run(feeds()[:4])
    assert len(SequencePipeline(m, S, window=6).run(feeds()[:7])) == 2   # without poses a window of 6 is fine
