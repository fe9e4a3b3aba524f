"""Selection + packed host copy for the reference solver (reference tracking_model.py:72-75)."""
import numpy as np
import pytest
import torch

from mmmot_amd.association import pairs_table
from mmmot_amd.tracker_glue import ChainResult, PairResult, scores_for_solver, unpack_chain_hand_off, unpack_hand_off
from mmmot_amd.tracks import ECONTRACT, EINFEASIBLE, TrackingError, split_ids


def test_selection_matches_reference_indexing():
    g = torch.Generator().manual_seed(3)
    N, M = 4, 6
    det, new, end = (torch.rand(3, N + M, generator=g) for _ in range(3))
    link = [torch.rand(3, N, M, generator=g)]
    for tm in (0, 1, 2):
        d, l, n, e = scores_for_solver(det, link, new, end, tm)
        assert torch.equal(d, det[tm]) and torch.equal(n, new[tm]) and torch.equal(e, end[tm])
        assert len(l) == 1 and l[0].shape == (1, N, M) and torch.equal(l[0], link[0][tm:tm + 1])
        assert d.device.type == 'cpu'


def test_hand_off_layout_unpacks_per_pair():
    """[det | new | end | link of every pair | per-pair solver block | int32 ids viewed as float32 | flags], the buffer
    a queued hand-off copies to the host: every field of every pair against slices taken independently"""
    splits = [(3, 5), (4, 2), (1, 6)]
    rng = np.random.default_rng(11)
    f32 = lambda n: rng.standard_normal(n).astype(np.float32)
    det, new, end = ([f32(N + M) for N, M in splits] for _ in range(3))
    link = [f32(N * M) for N, M in splits]
    blocks = [rng.integers(0, 2, 3 * (N + M) + N * M).astype(np.float32) for N, M in splits]
    ids = [rng.integers(-1, 40, N + M + 2).astype(np.int32) for N, M in splits]
    S, K = sum(N + M for N, M in splits), sum(N * M for N, M in splits)
    head = np.concatenate(det + new + end + link + blocks)
    table, offs = pairs_table(splits)
    assert head.size == 3 * S + K + offs[-1] + blocks[-1].size

    def check(res, want_ids):
        assert len(res) == len(splits)
        for p, (r, (N, M), o) in enumerate(zip(res, splits, offs)):
            L, so, lo = N + M, int(table[p, 2]), int(table[p, 3])
            assert isinstance(r, PairResult) and len(r.scores) == 4 and len(r.assignment) == 4
            for got, base in ((r.scores[0], 0), (r.scores[2], S), (r.scores[3], 2 * S)):
                assert got.dtype == torch.float32 and np.array_equal(got.numpy(), head[base + so:base + so + L])
            assert len(r.scores[1]) == 1 and r.scores[1][0].shape == (1, N, M)
            assert np.array_equal(r.scores[1][0].numpy().reshape(-1), head[3 * S + lo:3 * S + lo + N * M])
            assert np.array_equal(r.scores[0].numpy(), det[p]) and np.array_equal(r.scores[1][0].numpy().reshape(-1), link[p])
            assert np.array_equal(r.scores[2].numpy(), new[p]) and np.array_equal(r.scores[3].numpy(), end[p])
            b = head[3 * S + K + o:3 * S + K + o + 3 * L + N * M]
            assert np.array_equal(b, blocks[p])
            a_det, a_link, a_new, a_end = r.assignment
            assert np.array_equal(a_det.numpy(), b[0:L]) and np.array_equal(a_new.numpy(), b[L:2 * L])
            assert np.array_equal(a_end.numpy(), b[2 * L:3 * L])
            assert len(a_link) == 1 and a_link[0].shape == (1, N, M) and np.array_equal(a_link[0].numpy().reshape(-1), b[3 * L:])
            if want_ids is None:
                assert r.ids is None
            else:
                assert len(r.ids) == 4 and r.ids[0].dtype == np.int64 and r.ids[1].dtype == np.int64
                assert all(np.array_equal(x, y) for x, y in zip(r.ids, want_ids[p]))

    check(unpack_hand_off(torch.from_numpy(head.copy()), splits, S, K, 0), None)
    tail = np.concatenate(ids + [np.zeros(1, np.int32)])            # the error flags ride last
    flat = np.concatenate([head, tail.view(np.float32)])
    check(unpack_hand_off(torch.from_numpy(flat.copy()), splits, S, K, tail.size), split_ids(tail, splits))
    for flag in (EINFEASIBLE, ECONTRACT):
        tail[-1] = flag
        with pytest.raises(TrackingError):
            unpack_hand_off(torch.from_numpy(np.concatenate([head, tail.view(np.float32)])), splits, S, K, tail.size)


@pytest.mark.parametrize('with_ids', [False, True])
def test_pair_buffer_reads_as_two_frame_windows(with_ids):
    """a packed pair buffer is the buffer of two-frame windows: ``unpack_hand_off`` and ``unpack_chain_hand_off`` on the
    same bytes give the same scores and assignment, element for element; the ID tail of a pair has two trailing words"""
    splits = [(3, 4), (0, 2), (5, 1)]
    rng = np.random.default_rng(5)
    S, K = sum(N + M for N, M in splits), sum(N * M for N, M in splits)
    head = rng.standard_normal(3 * S + K + sum(3 * (N + M) + N * M for N, M in splits)).astype(np.float32)
    tail = np.zeros(0, np.int32)
    if with_ids:
        tail = np.concatenate([rng.integers(-1, 40, N + M + 2) for N, M in splits] + [np.zeros(1)]).astype(np.int32)
    flat = torch.from_numpy(np.concatenate([head, tail.view(np.float32)]))
    pairs = unpack_hand_off(flat, splits, S, K, tail.size)
    wins = unpack_chain_hand_off(flat, [list(s) for s in splits], S, K, 0)   # the pair tail is not a window's: not read
    assert len(pairs) == len(wins) == len(splits)
    for p, w, (N, M) in zip(pairs, wins, splits):
        assert isinstance(p, PairResult) and isinstance(w, ChainResult) and isinstance(p, ChainResult)
        for a, b in ((p.scores, w.scores), (p.assignment, w.assignment)):
            assert len(a) == len(b) == 4 and len(a[1]) == len(b[1]) == 1 and a[1][0].shape == b[1][0].shape == (1, N, M)
            for x, y in zip((a[0], a[1][0], a[2], a[3]), (b[0], b[1][0], b[2], b[3])):
                assert x.shape == y.shape and torch.equal(x, y)
            assert a[0].numel() == a[2].numel() == a[3].numel() == N + M
        assert w.ids is None and (p.ids is None) == (not with_ids)
    if with_ids:
        assert [len(p.ids) for p in pairs] == [4] * 3
        assert all(np.array_equal(x, y) for p, i in zip(pairs, split_ids(tail, splits)) for x, y in zip(p.ids, i))
