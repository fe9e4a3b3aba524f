"""The whole-sequence association with skip links without a GPU: the serial restatement of the kernel's search
(tests/sequence_gap_ref.py, ``ssp_gap_route``) against the literal program through scipy's milp, against
``sequence_ref.ssp_route`` at one gap, the planted generator, the hand-made cases, the layout helpers and every refusal
of the Python layer (all of them happen before any launch)."""
import numpy as np
import pytest
import torch

from sequence_gap_ref import (assemble_gaps, gap_feasible, gap_objective, ids_of_gaps, lp_gap_route, milp_gap_route,
                              planted_gap_sequence, random_gap_sequence, same_gap_assignment, ssp_gap_route)
from sequence_ref import ssp_route
from mmmot_amd import association as A
from mmmot_amd import torch_ops

KINDS = ('normal', 'dense', 'ties')
LENGTHS = (3, 6, 12)
GAPS = (1, 2, 3)
SEEDS = 6
PLANTED_SEEDS = (500, 501, 502, 503)  # the seeds of the GPU suite's planted instances


def random_split(rng, T):
    """n_t in 0 .. 4, empty frames included, at least one detection"""
    while True:
        split = [int(n) for n in rng.integers(0, 5, T)]
        if rng.random() < 0.5:
            split[int(rng.integers(0, T))] = 0
        if sum(split) > 0:
            return split


def instance(T, G, kind, seed):
    rng = np.random.default_rng(1000000 * LENGTHS.index(T) + 10000 * G + 1000 * KINDS.index(kind) + seed)
    split = random_split(rng, T)
    return split, random_gap_sequence(rng, split, min(G, T - 1), kind)


def planted(seed, T=30, max_n=6, G=3, p_miss=0.15):
    return planted_gap_sequence(np.random.default_rng(seed), T, max_n, G, p_miss)


def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('G', GAPS)
@pytest.mark.parametrize('T', LENGTHS)
def test_ssp_gap_route_matches_the_literal_program(T, G, kind):
    for seed in range(SEEDS):
        split, sc = instance(T, G, kind, seed)
        want, wobj = milp_gap_route(sc[0], sc[1], sc[2], sc[3], split)
        got, obj, info = ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split)
        assert info['status'] == 0 and gap_feasible(got, split), (split, info)
        assert close(obj, wobj), (split, obj, wobj)
        assert close(gap_objective(got, *sc), wobj), split
        assert info['augmentations'] == info['tracks'] and info['passes'] >= info['augmentations']
        assert close(lp_gap_route(sc[0], sc[1], sc[2], sc[3], split)[1], wobj), split
        # the kernel's shorter sweeps give the result of full sweeps
        short = ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split, ranges=True)
        assert same_gap_assignment(short[0], got) and short[1] == obj and short[2] == info, split


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T', LENGTHS)
def test_one_gap_is_ssp_route(T, kind):
    for seed in range(SEEDS):
        split, sc = instance(T, 1, kind, seed)
        got, obj, info = ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split)
        want, wobj, winfo = ssp_route(sc[0], sc[1], sc[2], sc[3][0], split)
        assert info == winfo and (obj == wobj or (obj != obj and wobj != wobj)), split
        assert same_gap_assignment(got, (want[0], [want[1]], want[2], want[3])), split


def hidden_names(frames, ids):
    """the trajectory number of every hidden track, asserting that the ids are the hidden tracks up to renumbering"""
    names = {}
    for f, i in zip(frames, ids):
        for h, x in zip(f, i):
            assert x >= 0 and names.setdefault(h, x) == x
    assert len(set(names.values())) == len(names)
    return names


@pytest.mark.parametrize('seed', PLANTED_SEEDS + (510, 511))
@pytest.mark.parametrize('T,G', [(30, 3), (12, 2), (12, 3)])
def test_planted_instances_are_recovered_and_have_misses(seed, T, G):
    split, sc, frames, misses = planted(seed, T, 6, G)
    assert misses >= 1, 'the generator must drop at least one detection for this seed'
    assert len(split) == T and split == [len(f) for f in frames]
    want, wobj = milp_gap_route(sc[0], sc[1], sc[2], sc[3], split)
    got, obj, info = ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split)
    assert info['status'] == 0 and close(obj, wobj)
    assert same_gap_assignment(got, want), split  # the optimum is unique: identical on every planted instance
    names = hidden_names(frames, ids_of_gaps(got, split))
    assert info['tracks'] == len(names)
    # without the skip links every miss inside a track splits it
    alone, _, ainfo = ssp_gap_route(sc[0], sc[1], sc[2], sc[3][:1], split)
    assert ainfo['tracks'] > info['tracks']


def test_planted_misses_are_bounded():
    for seed in range(20):
        split, _, frames, misses = planted(seed, 40, 6, 3, 0.4)
        seen = {}
        for t, f in enumerate(frames):
            for h in f:
                assert t - seen.get(h, t) <= 3, 'a track was dropped for more than G - 1 frames'
                seen[h] = t
        assert misses > 0 and all(len(set(f)) == len(f) for f in frames)


def test_gt_objective():
    rng = np.random.default_rng(7)
    for split, G in (([2, 3, 2], 2), ([4, 0, 4, 3], 3), ([3] * 9, 2)):
        sc = random_gap_sequence(rng, split, G)
        L = sum(split)
        lab = lambda *s: rng.integers(0, 2, s).astype(np.float32)
        gt = (lab(L), lab(L), lab(L), [[lab(*l.shape) for l in row] for row in sc[3]])
        want, wobj = milp_gap_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)
        got, obj, info = ssp_gap_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)
        assert info['status'] == 0 and gap_feasible(got, split)
        assert abs(obj - wobj) <= 1e-5 * max(1.0, abs(wobj))  # the shifted scores are formed in fp32, as on the device


def test_one_trajectory_across_an_empty_frame_by_hand():
    split = [1, 0, 1]
    det, new, end = np.array([2, 2], np.float32), np.array([0, -1], np.float32), np.array([-1, 0], np.float32)
    links = [[np.zeros((1, 0), np.float32), np.zeros((0, 1), np.float32)], [np.array([[3]], np.float32)]]
    for route in (ssp_gap_route, milp_gap_route):
        r = route(det, new, end, links, split)
        assert r[0][0].tolist() == [1, 1] and r[0][2].tolist() == [1, 0] and r[0][3].tolist() == [0, 1]
        assert r[0][1][1][0].tolist() == [[1]] and r[1] == 7.0
        assert [i.tolist() for i in ids_of_gaps(r[0], split)] == [[0], [], [0]]
    one, obj, info = ssp_gap_route(det, new, end, links[:1], split)
    assert info['tracks'] == 2 and obj == 2.0 and one[2].tolist() == [1, 1] and one[3].tolist() == [1, 1]
    assert [i.tolist() for i in ids_of_gaps(one, split)] == [[0], [], [1]]


def test_layout_helpers_by_hand():
    split = [2, 0, 3, 1]
    assert A.gap_link_sizes(split, 1) == [(2, 0), (0, 3), (3, 1)]
    assert A.gap_link_sizes(split, 3) == [(2, 0), (0, 3), (3, 1), (2, 3), (0, 1), (2, 1)]
    assert A.gap_block_size(split, 3) == 18 + 3 + 6 + 2
    seqs, nts, offs, sos = A.gap_sequences_table([split, [1] * 5, [4, 5, 2]], 2)
    assert seqs.dtype == torch.int32 and nts.dtype == torch.int32
    assert seqs.tolist() == [[4, 0, 0, 0], [5, 6, 9, 4], [3, 11, 16, 9]]
    assert nts.tolist() == split + [1] * 5 + [4, 5, 2]
    assert offs == [0, 27, 27 + 22] and sos == [0, 6, 11]
    # one gap: the table of sequences_table
    a, b = A.gap_sequences_table([split, [4, 5, 2]], 1), A.sequences_table([split, [4, 5, 2]])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    total, off, woff, units, max_n, max_L, max_T = torch_ops.sequence_gap_layout(seqs, nts, 2, 22, 54)
    assert total == 27 + 22 + 33 + 38 and off.tolist() == offs and (max_n, max_L, max_T) == (5, 11, 5)
    per = [(2 * T + 1) // 2 + (53 * L + 7) // 8 for T, L in ((4, 6), (5, 5), (3, 11))]
    assert woff.tolist() == [0, per[0], per[0] + per[1]] and units == sum(per)
    one = torch_ops.sequence_gap_layout(*A.gap_sequences_table([split], 1)[:2], 1)
    ref = torch_ops.sequence_layout(*A.sequences_table([split])[:2])
    assert one[0] == ref[0] and one[4:] == ref[4:] and one[3] == ref[3] + 2
    meta = torch.ops.mmmot.associate_sequences_gap(*[torch.empty(22, device='meta')] * 3, torch.empty(54, device='meta'),
                                                   seqs, nts, 2)
    assert [tuple(m.shape) for m in meta] == [(total,), (22,), (3,), (3, 4)]
    assert [m.dtype for m in meta] == [torch.float32, torch.int32, torch.float64, torch.int32]
    # unpack: a block whose values name their place
    block = torch.arange(A.gap_block_size(split, 3), dtype=torch.float32)
    det, links, new, end = A.unpack_gaps(block, split, 3)
    assert det.tolist() == list(range(6)) and new.tolist() == list(range(6, 12)) and end.tolist() == list(range(12, 18))
    assert [[tuple(l.shape) for l in row] for row in links] == [[(1, 2, 0), (1, 0, 3), (1, 3, 1)], [(1, 2, 3), (1, 0, 1)],
                                                                [(1, 2, 1)]]
    assert links[0][2].reshape(-1).tolist() == [18, 19, 20] and links[1][0].reshape(-1).tolist() == list(range(21, 27))
    assert links[2][0].reshape(-1).tolist() == [27, 28]
    like = torch.zeros(6, dtype=torch.float64)
    shaped = A.unpack_gaps(block, split, 2, like, [[(2, 0), (0, 3), (3, 1)], [(2, 3), (0, 1)]])
    assert shaped[0].dtype == torch.float64 and shaped[1][1][0].shape == (2, 3) and shaped[1][1][0].dtype == torch.float64
    sc = random_gap_sequence(np.random.default_rng(1), split, 2)
    assert assemble_gaps(*sc).size == A.gap_block_size(split, 2)


def test_layout_refusals():
    seqs, nts, _, _ = A.gap_sequences_table([[2, 3, 1], [1, 1, 1, 1]], 2)
    lay = torch_ops.sequence_gap_layout
    with pytest.raises(ValueError, match='max_gap must be in 1 .. 8'):
        lay(seqs, nts, 9)
    with pytest.raises(ValueError, match='max_gap must be in 1 .. 8'):
        lay(seqs, nts, 0)
    with pytest.raises(ValueError, match='more than max_gap = 3 frames'):
        lay(seqs, nts, 3)
    with pytest.raises(ValueError, match='CPU int32'):
        lay(seqs.long(), nts, 2)
    with pytest.raises(ValueError, match='past the end of the link'):
        lay(seqs, nts, 2, 10, 10 + 5)
    assert lay(seqs, nts, 2, 10, 11 + 5)[0] == 18 + 11 + 12 + 5


def test_python_refusals_happen_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError('a refusal must come before any launch')
    monkeypatch.setattr(A, 'gap_sequences_table', no_launch)  # what every launch is preceded by
    z = lambda *s: torch.zeros(*s)
    blocks = lambda split, G: [[z(1, split[t], split[t + g]) for t in range(len(split) - g)] for g in range(1, G + 1)]
    split = [2, 3, 1, 2]
    with pytest.raises(ValueError, match='1 .. 8 gaps, got 0'):
        A.associate_sequence_gaps(z(8), [], z(8), z(8), split)
    with pytest.raises(ValueError, match='1 .. 8 gaps, got 9'):
        A.associate_sequence_gaps(z(12), blocks([1] * 12, 9), z(12), z(12), [1] * 12)
    with pytest.raises(ValueError, match='max_gap = 4 needs more than 4 frames, got 4'):
        A.associate_sequence_gaps(z(8), blocks(split, 3) + [[]], z(8), z(8), split)
    with pytest.raises(ValueError, match='gap 2 needs 2 link blocks, got 1'):
        A.associate_sequence_gaps(z(8), [blocks(split, 2)[0], blocks(split, 2)[1][:1]], z(8), z(8), split)
    bad = blocks(split, 2)
    bad[1][1] = z(1, 2, 3)
    with pytest.raises(ValueError, match=r'link block \(gap 2, frame 1\) must be 3 x 2'):
        A.associate_sequence_gaps(z(8), bad, z(8), z(8), split)
    with pytest.raises(ValueError, match='det / new / end scores do not match'):
        A.associate_sequence_gaps(z(8), blocks(split, 2), z(7), z(8), split)
    with pytest.raises(ValueError, match='at least 2'):
        A.associate_sequence_gaps(z(3), [[]], z(3), z(3), [3])
    with pytest.raises(ValueError, match='gt does not match'):
        A.associate_sequence_gaps(z(8), blocks(split, 2), z(8), z(8), split,
                                  gt=(z(8), z(8), z(8), blocks(split, 1)))
    with pytest.raises(ValueError, match='no sequences'):
        A.associate_sequence_gaps_batch([], [], [], [], [])
    with pytest.raises(ValueError, match='needs a detection'):
        A.associate_sequence_gaps_batch([z(0)], [blocks([0, 0, 0], 2)], [z(0)], [z(0)], [[0, 0, 0]])
    with pytest.raises(ValueError, match='the same 2 gaps'):
        A.associate_sequence_gaps_batch([z(8), z(8)], [blocks(split, 2), blocks(split, 1)], [z(8), z(8)], [z(8), z(8)],
                                        [split, split])
    # both 2-D and 1 x n x m blocks are taken; an empty sequence is answered on the host
    r = A.associate_sequence_gaps(z(0), blocks([0, 0, 0], 2), z(0), z(0), [0, 0, 0], return_ids=True)
    assert r[0].numel() == 0 and [len(row) for row in r[1]] == [2, 1] and len(r[4]) == 3 and r[5] == 0
    r = A.associate_sequence_gaps(z(0), [[z(0, 0), z(0, 0)], [z(0, 0)]], z(0), z(0), [0, 0, 0])
    assert r[1][1][0].shape == (0, 0)
