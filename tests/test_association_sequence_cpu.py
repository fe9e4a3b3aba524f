"""The whole-sequence association without a GPU: the serial restatement of the kernel's search (tests/sequence_ref.py,
``ssp_route``) against the two host oracles of the chain program, the ID numbering against the tracker's bookkeeping on
decisive instances, the assembly convention on hand-made pairs, the table builder and every refusal of the Python
layer (all of them happen before any launch)."""
import numpy as np
import pytest
import torch

from association_chain_ref import feasible, lp_route, milp_route, random_chain, same_assignment
from sequence_ref import assemble, ids_of, planted_sequence, ssp_route
from tracking_ref import tracks_of
from mmmot_amd import association as A
from mmmot_amd import torch_ops

KINDS = ('normal', 'eval', 'masked')
LENGTHS = (2, 3, 9, 17, 40)
SEEDS = 34  # 5 lengths x 3 kinds x 34 seeds = 510 instances


def random_split(rng, T):
    """n_t in 0 .. 6, empty frames included, at least one detection"""
    while True:
        split = [int(n) for n in rng.integers(0, 7, T)]
        if rng.random() < 0.5:
            split[int(rng.integers(0, T))] = 0
        if sum(split) > 0:
            return split


def instance(T, kind, seed):
    rng = np.random.default_rng(100000 * LENGTHS.index(T) + 1000 * KINDS.index(kind) + seed)
    split = random_split(rng, T)
    return split, random_chain(rng, split, (1.0, 10.0, 1e4)[seed % 3], kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('T', LENGTHS)
def test_ssp_route_matches_both_oracles(T, kind):
    agreed = 0
    for seed in range(SEEDS):
        split, sc = instance(T, kind, seed)
        a, oa = lp_route(sc[0], sc[1], sc[2], sc[3], split)
        b, ob = milp_route(sc[0], sc[1], sc[2], sc[3], split)
        got, obj, info = ssp_route(sc[0], sc[1], sc[2], sc[3], split)
        assert info['status'] == 0 and feasible(got, split), (split, info)
        assert abs(obj - oa) <= 1e-9 * max(1.0, abs(oa)), (split, obj, oa)
        assert abs(obj - ob) <= 1e-9 * max(1.0, abs(ob)), (split, obj, ob)
        assert info['augmentations'] == info['tracks'] and info['passes'] >= info['augmentations']
        if same_assignment(a, b):
            agreed += 1
            assert same_assignment(got, a), split
    assert agreed >= SEEDS // 2, 'too few instances on which the oracles agree: %d' % agreed


def test_ssp_route_gt_objective():
    rng = np.random.default_rng(7)
    for split in ([2, 3, 2], [4, 0, 4, 3], [3] * 9):
        sc = random_chain(rng, split)
        L = sum(split)
        lab = lambda *s: rng.integers(0, 2, s).astype(np.float32)
        gt = (lab(L), lab(L), lab(L), [lab(a, b) for a, b in zip(split[:-1], split[1:])])
        want, wobj = lp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)
        got, obj, info = ssp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)
        assert info['status'] == 0 and feasible(got, split)
        assert abs(obj - wobj) <= 1e-5 * max(1.0, abs(wobj))  # the shifted scores are formed in fp32, as on the device
        if same_assignment(want, milp_route(sc[0], sc[1], sc[2], sc[3], split, gt=gt)[0]):
            assert same_assignment(got, want), split


def pairs_of(sc, split):
    """the sequence's scores cut into its pairs: pair t = (det, link, new, end) over frames t and t + 1"""
    det, new, end, links = sc
    st = np.concatenate([[0], np.cumsum(split)])
    return [(det[st[t]:st[t + 2]], links[t], new[st[t]:st[t + 2]], end[st[t]:st[t + 2]]) for t in range(len(split) - 1)]


@pytest.mark.parametrize('seed', range(5))
def test_ids_equal_the_pairwise_tracker_on_decisive_instances(seed):
    split, sc, hidden = planted_sequence(np.random.default_rng(300 + seed))
    got, _ = lp_route(sc[0], sc[1], sc[2], sc[3], split)
    assert same_assignment(got, ssp_route(sc[0], sc[1], sc[2], sc[3], split)[0])
    ids = ids_of(got, split)
    pair_assign = []
    for (d, l, n, e), a, b in zip(pairs_of(sc, split), split[:-1], split[1:]):
        r, _ = lp_route(d, n, e, [l], [a, b])
        pair_assign.append((r[0], r[1][0], r[2]))
    want = tracks_of(pair_assign, split)
    assert all(np.array_equal(x, y) for x, y in zip(ids, want))
    # and they are the hidden tracks up to their names
    names = {}
    for f, i in zip(hidden, ids):
        for h, x in zip(f, i):
            assert x >= 0 and names.setdefault(h, x) == x
    assert len(set(names.values())) == len(names)


def test_ids_of_by_hand():
    # frame 0: two kept; frame 1: one continues detection 1, one new, one rejected; frame 2: continues the new one
    det = np.array([1, 1, 1, 1, 0, 1.0])
    new = np.array([1, 1, 0, 1, 0, 0.0])
    links = [np.array([[0, 0, 0], [1, 0, 0.0]]), np.array([[0], [1], [0.0]])]
    ids = ids_of((det, links, new, None), [2, 3, 1])
    assert [i.tolist() for i in ids] == [[0, 1], [1, 2, -1], [2]]
    assert all(i.dtype == np.int64 for i in ids)


def test_assemble_by_hand():
    counts = [2, 1, 3]
    # pair rows carry a value that names (pair, kind, position)
    row = lambda p, kind, n: np.arange(n, dtype=np.float32) + 100 * p + 10 * kind
    pairs = []
    for p in range(2):
        n = counts[p] + counts[p + 1]
        link = (np.arange(counts[p] * counts[p + 1], dtype=np.float32) + 1000 * (p + 1)).reshape(1, counts[p], counts[p + 1])
        pairs.append((row(p, 1, n), [link], row(p, 2, n), row(p, 3, n)))
    det, links, new, end = assemble(pairs, counts)
    assert det.tolist() == [10, 11, 12, 111, 112, 113]        # frame 0: pair 0 first half; then second halves
    assert new.tolist() == [20, 21, 22, 121, 122, 123]
    assert end.tolist() == [30, 31, 130, 131, 132, 133]       # first halves; the last frame: pair 1's second half
    assert [l.shape for l in links] == [(2, 1), (1, 3)]
    assert links[0].reshape(-1).tolist() == [1000, 1001] and links[1].reshape(-1).tolist() == [2000, 2001, 2002]
    torch_rows = [(torch.from_numpy(d), [torch.from_numpy(l[0])], torch.from_numpy(n), torch.from_numpy(e))
                  for d, l, n, e in pairs]
    again = assemble(torch_rows, counts)
    assert np.array_equal(again[0], det) and np.array_equal(again[3], end)


def test_tables():
    seqs, nts, offs, sos = A.sequences_table([[2, 0, 3], [1] * 9, [4, 5]])
    assert seqs.dtype == torch.int32 and nts.dtype == torch.int32
    assert seqs.tolist() == [[3, 0, 0, 0], [9, 5, 0, 3], [2, 14, 8, 12]]
    assert nts.tolist() == [2, 0, 3] + [1] * 9 + [4, 5]
    assert offs == [0, 15, 15 + 27 + 8] and sos == [0, 5, 14]
    total, off, woff, units, max_n, max_L, max_T = torch_ops.sequence_layout(seqs, nts, 23, 28)
    assert total == 15 + 35 + 47 and off.tolist() == offs and max_n == 5 and max_L == 9 and max_T == 9
    per = [(53 * L + 7) // 8 for L in (5, 9, 9)]
    assert woff.tolist() == [0, per[0], per[0] + per[1]] and units == sum(per)
    meta = torch.ops.mmmot.associate_sequences(torch.empty(23, device='meta'), torch.empty(23, device='meta'),
                                               torch.empty(23, device='meta'), torch.empty(28, device='meta'), seqs, nts)
    assert [tuple(m.shape) for m in meta] == [(total,), (23,), (3,), (3, 4)]
    assert [m.dtype for m in meta] == [torch.float32, torch.int32, torch.float64, torch.int32]


def test_layout_refusals():
    seqs, nts, _, _ = A.sequences_table([[2, 3], [1, 1, 1]])
    lay = torch_ops.sequence_layout
    with pytest.raises(ValueError, match='CPU int32'):
        lay(seqs.long(), nts)
    with pytest.raises(ValueError, match='flat array'):
        lay(seqs, nts.long())
    with pytest.raises(ValueError, match='no sequences'):
        lay(seqs[:0], nts)
    with pytest.raises(ValueError, match='past the end of the score'):
        lay(seqs, nts, 7, 100)
    with pytest.raises(ValueError, match='past the end of the link'):
        lay(seqs, nts, 8, 7)
    bad = seqs.clone()
    bad[1, 3] = 3
    with pytest.raises(ValueError, match='past the end of nts'):
        lay(bad, nts)
    bad = seqs.clone()
    bad[0, 0] = 1
    with pytest.raises(ValueError, match='2 <= T'):
        lay(bad, nts)
    bad = seqs.clone()
    bad[0, 1] = -1
    with pytest.raises(ValueError, match='negative offset'):
        lay(bad, nts)
    with pytest.raises(ValueError, match='0 <= n_t'):
        lay(seqs, torch.tensor([2, 513, 1, 1, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match='1 <= L'):
        lay(seqs, torch.tensor([2, 3, 0, 0, 0], dtype=torch.int32))


def test_python_refusals_happen_before_any_launch():
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match='at least 2'):
        A.associate_sequence(z(3), [], z(3), z(3), [3])
    with pytest.raises(ValueError, match='at most 4096 frames'):
        A.associate_sequence(z(4097), [z(1, 1, 1)] * 4096, z(4097), z(4097), [1] * 4097)
    with pytest.raises(ValueError, match='0 <= n_t <= 512'):
        A.associate_sequence(z(514), [z(1, 513, 1)], z(514), z(514), [513, 1])
    with pytest.raises(ValueError, match='at most 65536 detections'):
        A.sequence_of([512] * 129)
    with pytest.raises(ValueError, match='do not match'):
        A.associate_sequence(z(5), [z(1, 2, 3)], z(5), z(4), [2, 3])
    with pytest.raises(ValueError, match='do not match'):
        A.associate_sequence(z(5), [z(1, 2, 2)], z(5), z(5), [2, 3])
    with pytest.raises(ValueError, match='do not match'):
        A.associate_sequence(z(6), [z(1, 2, 3)], z(6), z(6), [2, 3, 1])
    with pytest.raises(ValueError, match='gt does not match'):
        A.associate_sequence(z(5), [z(1, 2, 3)], z(5), z(5), [2, 3], gt=(z(5), z(5), z(4), [z(1, 2, 3)]))
    with pytest.raises(ValueError, match='no sequences'):
        A.associate_sequence_batch([], [], [], [], [])
    with pytest.raises(ValueError, match='needs a detection'):
        A.associate_sequence_batch([z(0)], [[z(1, 0, 0)]], [z(0)], [z(0)], [[0, 0]])
    with pytest.raises(ValueError, match='fewer than 2\\^31'):
        A.sequences_table([[512] * 128] * 130)
    # an empty sequence is answered on the host, as associate_chain answers it
    r = A.associate_sequence(z(0), [z(1, 0, 0), z(1, 0, 0)], z(0), z(0), [0, 0, 0], return_ids=True)
    assert r[0].numel() == 0 and len(r[1]) == 2 and len(r[4]) == 3 and r[5] == 0


def test_association_error_names_the_sequence():
    e = A.AssociationError(3, 3)
    assert isinstance(e, RuntimeError) and e.index == 3 and e.status == 3 and 'pass bound' in str(e)
    info = np.zeros((4, 4), np.int32)
    A._raise_status(info)
    info[2, 0] = 4
    with pytest.raises(A.AssociationError, match='sequence 2'):
        A._raise_status(info)
