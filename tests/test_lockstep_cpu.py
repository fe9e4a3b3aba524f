"""The host side of the lockstep order (mmmot_amd.pipeline.LockstepPipeline), without a device: the stream-major
reordering of a multi-state ID launch and its inverse, ``seq_start`` with empty streams, the per-stream reading of a
hand-off buffer whose pairs were partly answered on the host, the schedule of sequences of different lengths, and the
refusals that come before anything touches the device."""
import numpy as np
import pytest
import torch

from mmmot_amd.pipeline import LockstepPipeline, lockstep_stage, lockstep_steps
from mmmot_amd.tracker_glue import HandOff, PairResult, multi_ids_reader
from mmmot_amd.tracks import ECONTRACT, EINFEASIBLE, TrackingError, split_ids, split_ids_multi, stream_major


def test_stream_major_order_and_seq_start():
    order, seq = stream_major([2, 0, 3, 0, 2, 3, 0], 4)
    assert order.tolist() == [1, 3, 6, 0, 4, 2, 5]            # stable: a stream's groups keep their order
    assert seq.dtype == np.int32 and seq.tolist() == [0, 3, 3, 5, 7]   # stream 1 is empty: [3, 3)
    inv = np.argsort(order)
    assert np.array_equal(order[inv], np.arange(7)) and np.array_equal(np.asarray([2, 0, 3, 0, 2, 3, 0])[order],
                                                                      [0, 0, 0, 2, 2, 3, 3])
    order, seq = stream_major([], 3)
    assert order.size == 0 and seq.tolist() == [0, 0, 0, 0]
    order, seq = stream_major([1, 1], 2)                       # already stream-major, the first stream empty
    assert order.tolist() == [0, 1] and seq.tolist() == [0, 0, 2]
    for bad in ([0, 4], [-1]):
        with pytest.raises(ValueError):
            stream_major(bad, 4)


def ids_buffer(rng, splits, stream_of, S, tail=2, flags=None):
    """what a multi-state launch hands back for groups given in any order: [the groups' words stream-major | S flags],
    and per group (in the order given) its own words"""
    words = [rng.integers(-1, 40, sum(s) + tail).astype(np.int32) for s in splits]
    order, _ = stream_major(stream_of, S)
    fl = np.zeros(S, np.int32) if flags is None else np.asarray(flags, np.int32)
    return np.concatenate([words[g] for g in order] + [fl]), words


def test_split_ids_multi_is_the_inverse_of_the_reordering():
    rng = np.random.default_rng(0)
    splits = [(3, 2), (0, 4), (1, 1), (5, 0), (2, 2), (0, 0), (4, 3)]
    stream_of = [2, 0, 3, 0, 2, 3, 0]
    flat, words = ids_buffer(rng, splits, stream_of, 4)
    got = split_ids_multi(flat, splits, stream_of)
    assert len(got) == 7
    for (N, M), w, (i0, i1, start, last) in zip(splits, words, got):
        assert i0.dtype == np.int64 and np.array_equal(i0, w[:N]) and np.array_equal(i1, w[N:N + M])
        assert (start, last) == (int(w[N + M]), int(w[N + M + 1]))
    # one stream: the reading of the single-state buffer
    one = np.concatenate(words + [np.zeros(1, np.int32)])
    for a, b in zip(split_ids_multi(one, splits, [0] * 7), split_ids(one, splits)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # windows: three trailing words, per-frame lists
    wsplits = [[2, 3, 1], [1, 1], [0, 2, 2, 1]]
    flat, words = ids_buffer(rng, wsplits, [1, 0, 1], 2, tail=3)
    for s, w, (ids, start, last, stored) in zip(wsplits, words, split_ids_multi(flat, wsplits, [1, 0, 1], tail=3)):
        assert [len(i) for i in ids] == s and np.array_equal(np.concatenate(ids), w[:sum(s)])
        assert (start, last, stored) == tuple(int(x) for x in w[sum(s):])


@pytest.mark.parametrize('flag', [EINFEASIBLE, ECONTRACT])
def test_split_ids_multi_names_the_stream(flag):
    rng = np.random.default_rng(1)
    splits, stream_of = [(1, 2), (2, 2), (3, 1)], [0, 2, 1]
    flat, _ = ids_buffer(rng, splits, stream_of, 3, flags=[0, 0, flag])
    with pytest.raises(TrackingError, match='stream 2'):
        split_ids_multi(flat, splits, stream_of)
    flat[-1] = 0
    assert len(split_ids_multi(flat, splits, stream_of)) == 3


def test_hand_off_unpacks_per_stream_with_pairs_answered_on_the_host():
    """four pairs of streams 0 .. 3, pairs 1 and 3 with an empty frame: their (scores, assignment) were made on the host
    at queue time, the buffer holds [det | new | end | link of pairs 0 and 2 | their solver blocks | the ids of ALL
    pairs, in the order the ID launch got them: solved pairs first, host pairs behind | 4 flags]"""
    rng = np.random.default_rng(2)
    splits = [(3, 2), (0, 4), (2, 2), (3, 0)]
    stream_of = [3, 1, 0, 2]
    full, host = [0, 2], [1, 3]
    f32 = lambda n: rng.standard_normal(n).astype(np.float32)
    det, new, end = ({p: f32(sum(splits[p])) for p in full} for _ in range(3))
    link = {p: f32(splits[p][0] * splits[p][1]) for p in full}
    blocks = {p: rng.integers(0, 2, 3 * sum(splits[p]) + splits[p][0] * splits[p][1]).astype(np.float32) for p in full}
    S, K = sum(sum(splits[p]) for p in full), sum(link[p].size for p in full)
    head = np.concatenate([x[p] for x in (det, new, end, link, blocks) for p in full])
    order = full + host
    o_splits, o_streams = [splits[p] for p in order], [stream_of[p] for p in order]
    tail, words = ids_buffer(rng, o_splits, o_streams, 4)
    done = [None] * 4
    for p in host:
        done[p] = (('scores', p), ('assignment', p))
    flat = torch.from_numpy(np.concatenate([head, tail.view(np.float32)]))
    pending = HandOff((splits, S, K, tail.size), flat, done,
                      ids_reader=lambda f, _: multi_ids_reader(f, o_splits, o_streams, order))
    res = pending.fetch()
    assert len(res) == 4 and all(isinstance(r, PairResult) for r in res)
    for p in host:
        assert res[p].scores == ('scores', p) and res[p].assignment == ('assignment', p)
    for p in full:
        N, M = splits[p]
        sc, a = res[p].scores, res[p].assignment
        assert np.array_equal(sc[0].numpy(), det[p]) and np.array_equal(sc[2].numpy(), new[p])
        assert np.array_equal(sc[3].numpy(), end[p]) and np.array_equal(sc[1][0].numpy().reshape(-1), link[p])
        assert sc[1][0].shape == (1, N, M) and a[1][0].shape == (1, N, M)
        b = blocks[p]
        assert np.array_equal(np.concatenate([a[0].numpy(), a[2].numpy(), a[3].numpy(), a[1][0].numpy().reshape(-1)]), b)
    for k, p in enumerate(order):   # every pair gets its own words back, whatever its place in the launch
        N, M = splits[p]
        i0, i1, start, last = res[p].ids
        w = words[k]
        assert np.array_equal(i0, w[:N]) and np.array_equal(i1, w[N:N + M]) and (start, last) == (int(w[N + M]), int(w[N + M + 1]))
    # a flag of stream 2 (pair 3) fails the whole fetch, naming it
    tail[-2] = EINFEASIBLE
    pending.flat = torch.from_numpy(np.concatenate([head, tail.view(np.float32)]))
    with pytest.raises(TrackingError, match='stream 2'):
        pending.fetch()


def test_schedule_of_sequences_that_end_apart():
    """stream 1 finishes two steps before the others; stream 3 has one frame and stream 4 none: in no step"""
    lens = [5, 3, 5, 1, 0]
    steps = lockstep_steps(lens)
    assert steps == [[0, 1, 2], [0, 1, 2], [0, 2], [0, 2]]
    assert sum(len(s) for s in steps) == sum(n - 1 for n in lens if n >= 2)
    assert [lockstep_stage(lens, t) for t in range(6)] == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 2], [0, 2], []]
    # every frame of a sequence with a pair is prepared exactly once, before the step that scores it
    for s, n in enumerate(lens):
        assert sum(s in lockstep_stage(lens, t) for t in range(6)) == (n if n >= 2 else 0)
    assert lockstep_steps([1, 0]) == [] and lockstep_steps([]) == [] and lockstep_steps([2]) == [[0]]
    # the seq_start of a step in which stream 1 is gone: an empty range for it
    _, seq = stream_major(steps[2], 3)
    assert seq.tolist() == [0, 1, 1, 2]


def test_frames_without_detections_are_left_out_and_put_back():
    """the pair path runs over the frames that hold a detection (the reference's dataset skips the others): the kept
    feeds, callbacks that speak of the sequence's own frame indices, and the tracks back at those indices"""
    from types import SimpleNamespace
    from mmmot_amd.pipeline import _skip_empty, _spread_tracks
    counts = [3, 1, 0, 5, 0, 2]
    feeds = [SimpleNamespace(dets={'bbox': np.zeros((n, 4))}, t=t) for t, n in enumerate(counts)]
    seen = []
    cbs = (lambda t, x: seen.append(('scores', t, x)), None, lambda t, x: seen.append(('tracks', t, x)))
    kept, idx, (on_scores, on_assign, on_tracks) = _skip_empty(feeds, cbs)
    assert [f.t for f in kept] == idx == [0, 1, 3, 5] and on_assign is None
    on_scores(2, 'a')   # kept frame 2 is the sequence's frame 3
    on_tracks(3, 'b')
    assert seen == [('scores', 3, 'a'), ('tracks', 5, 'b')]
    tracks = _spread_tracks([np.arange(n) for n in (3, 1, 5, 2)], idx, len(feeds))
    assert [len(x) for x in tracks] == counts and all(x.dtype == np.int64 for x in tracks)
    # nothing to leave out: the very same objects
    full = feeds[:2]
    assert _skip_empty(full, cbs) == (full, [0, 1], cbs) and _skip_empty(full, cbs)[0] is full
    assert _skip_empty(feeds[2:3], cbs)[:2] == ([], [])


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError, match='SequencePipeline'):
        LockstepPipeline(None, window=3)
    with pytest.raises(ValueError, match='associate'):
        LockstepPipeline(None, track=True)
