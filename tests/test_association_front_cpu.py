"""The host front end of the association solvers without a GPU: the launch seam of mmmot_amd.association is replaced by
a recorder and the device of the host round trip by 'cpu'.  For each of the eight public functions (pairs, chains,
sequences, sequences with skip links; single and batch) the recorded operator, ``max_gap``, score tensors and tables
are compared with hand-built ones, the returned tensors with the slices of an output block whose values name their
place, and the single-instance function with its batch function at B = 1.  Empty cases and refusals launch nothing."""
import pytest
import torch

from mmmot_amd import association as A
from mmmot_amd import pipeline

F32, F64 = torch.float32, torch.float64


class Recorder:
    """stands in for the launch seam: keeps every call and answers with outputs of the operator's sizes - the output
    block arange, arange IDs, a zero objective and a zero info"""

    def __init__(self):
        self.calls = []

    def __call__(self, op, det, new, end, link, tables, max_gap=None):
        self.calls.append(dict(op=op, det=det, new=new, end=end, link=link, tables=tuple(tables), max_gap=max_gap))
        B = tables[0].shape[0]
        assert det.numel() == new.numel() == end.numel() and all(t.dim() == 1 for t in (det, new, end, link))
        out = torch.arange(3 * det.numel() + link.numel(), dtype=F32)
        obj = torch.zeros(B, dtype=F64)
        if op in ('associate', 'associate_chains'):
            assert max_gap is None
            return out, obj
        assert op in ('associate_sequences', 'associate_sequences_gap') and (max_gap is None) == (op == 'associate_sequences')
        return out, torch.arange(det.numel(), dtype=torch.int32), obj, torch.zeros(B, 4, dtype=torch.int32)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(A, '_launch', r)
    monkeypatch.setattr(A, 'DEVICE', 'cpu')
    return r


def instance(split, G=1, base=0.0, dtype=F32, nested=False, flat_links=False):
    """(det, links, new, end) with distinct values: det base + 1 .., new base + 101 .., end base + 201 .., the link
    blocks base + 301 .. in layout order (all of gap 1, then all of gap 2, ..)"""
    L = sum(split)
    det, new, end = (base + k + 1 + torch.arange(L, dtype=dtype) for k in (0, 100, 200))
    links, o = [], base + 301
    for g in range(1, G + 1):
        row = []
        for t in range(len(split) - g):
            a, b = split[t], split[t + g]
            blk = (o + torch.arange(a * b, dtype=dtype)).view((a, b) if flat_links else (1, a, b))
            row.append(blk)
            o += a * b
        links.append(row)
    return det, (links if nested else links[0]), new, end


def gt_of(scores, nested):
    """a gt tuple of the scores' shapes: 1 where the score's integer value is divisible by 3, else 0"""
    f = lambda t: (t.to(torch.int64) % 3 == 0).to(t.dtype)
    det, links, new, end = scores
    return f(det), f(new), f(end), ([[f(l) for l in row] for row in links] if nested else [f(l) for l in links])


def flat_links(links, nested):
    blocks = [l for row in links for l in row] if nested else list(links)
    return torch.cat([l.reshape(-1).to(F32) for l in blocks] + [torch.zeros(0)])


def augmented(x, g):
    """the loss-augmented score, the reference expression"""
    return x - (g + (g == 0) * -1)


def expected_parts(insts, nested, gts=None):
    """the four tensors the operator must be given: the instances' det, new, end and links joined per part"""
    gts = gts or [None] * len(insts)
    parts = []
    for (det, links, new, end), gt in zip(insts, gts):
        p = [det.reshape(-1).to(F32), new.reshape(-1).to(F32), end.reshape(-1).to(F32), flat_links(links, nested)]
        if gt is not None:
            g = [gt[0].reshape(-1).to(F32), gt[1].reshape(-1).to(F32), gt[2].reshape(-1).to(F32), flat_links(gt[3], nested)]
            p = [augmented(x, y) for x, y in zip(p, g)]
        parts.append(p)
    return [torch.cat([p[k] for p in parts]) for k in range(4)]


def expected_result(o, scores, split, G, nested):
    """what the instance whose block starts at ``o`` of the arange output returns, shaped and typed like its scores"""
    det, links, new, end = scores
    L = sum(split)
    take = lambda start, like: torch.arange(start, start + like.numel(), dtype=F32).view(like.size()).to(like.dtype)
    rows, k = [], o + 3 * L
    for row in (links if nested else [links]):
        got = []
        for l in row:
            got.append(take(k, l))
            k += l.numel()
        rows.append(got)
    return (take(o, det), rows if nested else rows[0], take(o + L, new), take(o + 2 * L, end)), k


def same(a, b):
    """equal element for element, with equal nesting, shapes, dtypes and devices"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return (torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype
                and a.device == b.device and torch.equal(a, b))
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def check_call(call, op, max_gap, parts, tables):
    assert call['op'] == op and call['max_gap'] == max_gap
    for name, want in zip(('det', 'new', 'end', 'link'), parts):
        got = call[name]
        assert got.dtype == F32 and got.shape == want.shape and torch.equal(got, want), name
    assert len(call['tables']) == len(tables)
    for got, want in zip(call['tables'], tables):
        assert got.dtype == torch.int32 and got.device.type == 'cpu' and torch.equal(got, want)


def check_results(results, insts, splits, G, nested, ids=False):
    o, so = 0, 0
    for res, scores, split in zip(results, insts, splits):
        want, o = expected_result(o, scores, split, G, nested)
        assert isinstance(res, tuple) and len(res) == (6 if ids else 4)
        assert same(tuple(res[:4]), want)
        if ids:
            per_frame = list(torch.arange(so, so + sum(split), dtype=torch.int64).split(split))
            assert same(res[4], per_frame) and res[5] == 0 and type(res[5]) is int
        so += sum(split)


def columns(insts):
    return [[i[0] for i in insts], [i[1] for i in insts], [i[2] for i in insts], [i[3] for i in insts]]


# ---- pairs ---------------------------------------------------------------------------------------------------------
PAIR_SPLITS = [(2, 3), (1, 2)]


def pair_instances():
    return [instance(list(s), base=1000.0 * i, dtype=(F64, F32)[i]) for i, s in enumerate(PAIR_SPLITS)]


def test_pairs_by_hand():
    assert A.pairs_table(PAIR_SPLITS)[0].tolist() == [[2, 3, 0, 0], [1, 2, 5, 6]] and A.pairs_table(PAIR_SPLITS)[1] == [0, 21]
    det, links, new, end = instance([2, 3])
    assert det.tolist() == [1, 2, 3, 4, 5] and new[0] == 101 and end[4] == 205
    assert links[0].tolist() == [[[301, 302, 303], [304, 305, 306]]]


def test_associate(rec):
    one = pair_instances()[0]
    res = A.associate(one[0], one[1], one[2], one[3], [2, 3])
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate', None, expected_parts([one], False), (A.pairs_table([(2, 3)])[0],))
    check_results([res], [one], [(2, 3)], 1, False)
    batch = A.associate_batch(*columns([one]), [[2, 3]])
    assert len(rec.calls) == 2 and isinstance(batch, list) and same(batch, [res])
    for k in ('det', 'new', 'end', 'link'):
        assert torch.equal(rec.calls[0][k], rec.calls[1][k])


def test_associate_batch(rec):
    insts = pair_instances()
    res, obj = A.associate_batch(*columns(insts), [[torch.tensor([2]), torch.tensor([3])], (1, 2)], return_objective=True)
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate', None, expected_parts(insts, False), (A.pairs_table(PAIR_SPLITS)[0],))
    check_results(res, insts, PAIR_SPLITS, 1, False)
    assert res[1][0].tolist() == [21, 22, 23] and res[1][1][0].reshape(-1).tolist() == [30, 31]  # the second block: 21 ..
    assert obj.dtype == F64 and obj.shape == (2,)
    assert same(A.associate_batch(*columns(insts), PAIR_SPLITS), res)


def test_associate_launches_nothing_for_empty_frames_and_refusals(rec):
    det, new, end = torch.tensor([1.0, -1.0, 0.5]), torch.tensor([0.5, 0.5, -2.0]), torch.tensor([0.0, 1.0, 1.0])
    got = A.associate(det, [torch.zeros(1, 0, 3)], new, end, [0, 3])
    assert got[0].tolist() == [1, 1, 0] and same(got[0], got[2]) and same(got[0], got[3]) and got[1][0].shape == (1, 0, 3)
    got = A.associate(det, [torch.zeros(1, 3, 0)], new, end, [3, 0])
    assert got[0].tolist() == [1, 1, 0] and got[1][0].shape == (1, 3, 0)
    one = pair_instances()[0]
    with pytest.raises(NotImplementedError, match='associate: the gt'):
        A.associate(one[0], one[1], one[2], one[3], [2, 3], gt=gt_of(one, False))
    with pytest.raises(ValueError, match='det_split must have 2 entries, got 3'):
        A.associate(one[0], one[1], one[2], one[3], [2, 3, 1])
    with pytest.raises(ValueError, match=r'associate: scores do not match det_split \[2, 2\]'):
        A.associate(one[0], one[1], one[2], one[3], [2, 2])
    with pytest.raises(ValueError, match='associate_batch: no pairs'):
        A.associate_batch([], [], [], [], [])
    with pytest.raises(ValueError, match='associate_batch: every pair needs detections in both frames'):
        A.associate_batch(*columns([one, (det, [torch.zeros(1, 0, 3)], new, end)]), [(2, 3), (0, 3)])
    assert rec.calls == []


# ---- chains --------------------------------------------------------------------------------------------------------
CHAIN_SPLITS = [[2, 0, 3], [1, 2]]


def chain_instances():
    return [instance(CHAIN_SPLITS[0], base=0.0, dtype=F64, flat_links=True), instance(CHAIN_SPLITS[1], base=1000.0)]


def test_associate_chain(rec):
    one = chain_instances()[0]
    assert [tuple(l.shape) for l in one[1]] == [(2, 0), (0, 3)]
    res = A.associate_chain(one[0].view(1, 5), one[1], one[2].view(1, 5), one[3].view(1, 5), [2, 0, 3])
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate_chains', None, expected_parts([one], False), (A.chains_table([[2, 0, 3]])[0],))
    shaped = (one[0].view(1, 5), one[1], one[2].view(1, 5), one[3].view(1, 5))
    check_results([res], [shaped], [[2, 0, 3]], 1, False)
    assert res[0].shape == (1, 5) and res[0].dtype == F64 and isinstance(res[1], list) and res[1][1].shape == (0, 3)
    assert same(A.associate_chain_batch(*columns([shaped]), [[2, 0, 3]]), [res])
    # gt: every score drops by gt + (gt == 0) * -1
    gt = gt_of(one, False)
    with_gt = A.associate_chain(one[0], one[1], one[2], one[3], [2, 0, 3], gt=gt)
    assert len(rec.calls) == 3
    parts = expected_parts([one], False, [gt])
    assert parts[0].tolist() == [2, 3, 2, 5, 6] and parts[1].tolist() == [102, 101, 104, 105, 104]
    check_call(rec.calls[2], 'associate_chains', None, parts, (A.chains_table([[2, 0, 3]])[0],))
    check_results([with_gt], [one], [[2, 0, 3]], 1, False)
    assert same(A.associate_chain_batch(*columns([one]), [[2, 0, 3]], gts=[gt]), [with_gt])
    assert all(torch.equal(rec.calls[2][k], rec.calls[3][k]) for k in ('det', 'new', 'end', 'link'))


def test_associate_chain_batch(rec):
    insts = chain_instances()
    gts = [None, gt_of(insts[1], False)]
    res, obj = A.associate_chain_batch(*columns(insts), CHAIN_SPLITS, gts=gts, return_objective=True)
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate_chains', None, expected_parts(insts, False, gts), (A.chains_table(CHAIN_SPLITS)[0],))
    assert rec.calls[0]['link'].tolist() == [1302.0, 1301.0]  # 1301 + 1 (gt 0) and 1302 - 1 (gt 1); the first chain has no link
    check_results(res, insts, CHAIN_SPLITS, 1, False)
    assert res[1][0].tolist() == [15, 16, 17] and res[1][1][0].reshape(-1).tolist() == [24, 25]  # the second block: 15 ..
    assert obj.dtype == F64 and obj.shape == (2,)


def test_chain_launches_nothing_for_empty_chains_and_refusals(rec):
    z = lambda *s: torch.zeros(*s, dtype=F64)
    got = A.associate_chain(z(0), [z(1, 0, 0), z(1, 0, 0)], z(0), z(0), [0, 0, 0])
    assert same(got, (z(0), [z(1, 0, 0), z(1, 0, 0)], z(0), z(0)))
    one = chain_instances()[1]
    with pytest.raises(ValueError, match='associate_chain: det_split must have at least 2 entries, got 1'):
        A.associate_chain(one[0], one[1], one[2], one[3], [3])
    with pytest.raises(ValueError, match='associate_chain: scores do not match det_split'):
        A.associate_chain(one[0], one[1], one[2], one[3], [2, 2])
    with pytest.raises(ValueError, match='associate_chain: at most 8 frames, got 9'):
        A.associate_chain(z(9), [z(1, 1, 1)] * 8, z(9), z(9), [1] * 9)
    with pytest.raises(ValueError, match='associate_chain: gt does not match the scores'):
        A.associate_chain(one[0], one[1], one[2], one[3], [1, 2], gt=(one[0], one[2], one[3], []))
    with pytest.raises(ValueError, match='associate_chain_batch: no chains'):
        A.associate_chain_batch([], [], [], [], [])
    with pytest.raises(ValueError, match='associate_chain_batch: every chain needs a detection'):
        A.associate_chain_batch(*columns([one, (z(0), [z(1, 0, 0)], z(0), z(0))]), [[1, 2], [0, 0]])
    with pytest.raises(ValueError, match='associate_chain: scores do not match det_split'):
        A.associate_chain_batch(*columns([one, one]), [[1, 2], [2, 1, 1]])
    assert rec.calls == []


# ---- whole sequences -----------------------------------------------------------------------------------------------
SEQ_SPLITS = [[2, 3, 1, 2], [1, 1, 1]]


def sequence_instances(G=1, nested=False):
    return [instance(SEQ_SPLITS[0], G, base=0.0, nested=nested),
            instance(SEQ_SPLITS[1], G, base=1000.0, dtype=F64, nested=nested)]


def test_associate_sequence(rec):
    one = sequence_instances()[0]
    res = A.associate_sequence(one[0], one[1], one[2], one[3], SEQ_SPLITS[0])
    assert len(rec.calls) == 1 and len(res) == 4
    check_call(rec.calls[0], 'associate_sequences', None, expected_parts([one], False), A.sequences_table(SEQ_SPLITS[:1])[:2])
    check_results([res], [one], SEQ_SPLITS[:1], 1, False)
    gt = gt_of(one, False)
    res = A.associate_sequence(one[0], one[1], one[2], one[3], torch.tensor(SEQ_SPLITS[0]), gt=gt, return_ids=True)
    check_call(rec.calls[1], 'associate_sequences', None, expected_parts([one], False, [gt]),
               A.sequences_table(SEQ_SPLITS[:1])[:2])
    check_results([res], [one], SEQ_SPLITS[:1], 1, False, ids=True)
    assert [i.tolist() for i in res[4]] == [[0, 1], [2, 3, 4], [5], [6, 7]]
    assert same(A.associate_sequence_batch(*columns([one]), SEQ_SPLITS[:1], gts=[gt], return_ids=True), [res])
    assert len(rec.calls) == 3 and all(torch.equal(rec.calls[1][k], rec.calls[2][k]) for k in ('det', 'new', 'end', 'link'))


def test_associate_sequence_batch(rec):
    insts = sequence_instances()
    gts = [gt_of(insts[0], False), None]
    res, obj = A.associate_sequence_batch(*columns(insts), SEQ_SPLITS, gts=gts, return_objective=True, return_ids=True)
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate_sequences', None, expected_parts(insts, False, gts), A.sequences_table(SEQ_SPLITS)[:2])
    check_results(res, insts, SEQ_SPLITS, 1, False, ids=True)
    # the second sequence's block starts at 3 * 8 + 6 + 3 + 2 = 35, its IDs at 8
    assert res[1][0].tolist() == [35, 36, 37] and res[1][0].dtype == F64 and res[1][1][1].reshape(-1).tolist() == [45]
    assert [i.tolist() for i in res[1][4]] == [[8], [9], [10]]
    assert obj.dtype == F64 and obj.shape == (2,)
    plain = A.associate_sequence_batch(*columns(insts), SEQ_SPLITS, gts=gts)
    assert same(plain, [r[:4] for r in res])


def test_sequence_launches_nothing_for_empty_sequences_and_refusals(rec):
    z = lambda *s: torch.zeros(*s)
    got = A.associate_sequence(z(0), [z(1, 0, 0)] * 2, z(0), z(0), [0, 0, 0], return_ids=True)
    assert same(got, (z(0), [z(1, 0, 0)] * 2, z(0), z(0), [torch.zeros(0, dtype=torch.int64)] * 3, 0))
    assert same(A.associate_sequence(z(0), [z(1, 0, 0)] * 2, z(0), z(0), [0, 0, 0]), got[:4])
    one = sequence_instances()[1]
    with pytest.raises(ValueError, match='associate_sequence: det_split must have at least 2 entries, got 1'):
        A.associate_sequence(one[0], one[1], one[2], one[3], [3])
    with pytest.raises(ValueError, match='associate_sequence: every frame needs 0 <= n_t <= 512'):
        A.associate_sequence(one[0], one[1], one[2], one[3], [1, 513, 1])
    with pytest.raises(ValueError, match='associate_chain: scores do not match det_split'):
        A.associate_sequence(one[0], one[1], one[2], one[3], [1, 1, 2])
    with pytest.raises(ValueError, match='associate_sequence_batch: no sequences'):
        A.associate_sequence_batch([], [], [], [], [])
    with pytest.raises(ValueError, match='associate_sequence_batch: every sequence needs a detection'):
        A.associate_sequence_batch(*columns([one, (z(0), [z(1, 0, 0)], z(0), z(0))]), [[1, 1, 1], [0, 0]])
    assert rec.calls == []


def test_status_word_raises_after_the_one_launch(rec, monkeypatch):
    one = sequence_instances()[0]

    def failing(*a, **k):
        out, ids, obj, info = rec(*a, **k)
        info[0, 0] = 3
        return out, ids, obj, info
    monkeypatch.setattr(A, '_launch', failing)
    with pytest.raises(A.AssociationError, match='sequence 0 not solved: pass bound hit') as e:
        A.associate_sequence(one[0], one[1], one[2], one[3], SEQ_SPLITS[0])
    assert e.value.status == 3 and len(rec.calls) == 1
    nested = sequence_instances(2, True)[0]
    with pytest.raises(A.AssociationError):
        A.associate_sequence_gaps_batch(*columns([nested]), SEQ_SPLITS[:1])
    assert len(rec.calls) == 2


# ---- whole sequences with skip links -------------------------------------------------------------------------------
def test_associate_sequence_gaps(rec):
    one = sequence_instances(2, True)[0]
    assert [[tuple(l.shape) for l in row] for row in one[1]] == [[(1, 2, 3), (1, 3, 1), (1, 1, 2)], [(1, 2, 1), (1, 3, 2)]]
    res = A.associate_sequence_gaps(one[0], one[1], one[2], one[3], SEQ_SPLITS[0])
    assert len(rec.calls) == 1 and len(res) == 4
    tables = A.gap_sequences_table(SEQ_SPLITS[:1], 2)[:2]
    check_call(rec.calls[0], 'associate_sequences_gap', 2, expected_parts([one], True), tables)
    check_results([res], [one], SEQ_SPLITS[:1], 2, True)
    assert isinstance(res[1][0], list) and res[1][1][1].shape == (1, 3, 2)
    assert res[1][1][0].reshape(-1).tolist() == [24 + 11, 24 + 12]  # 3 L = 24, 11 links of gap 1 in front
    gt = gt_of(one, True)
    res = A.associate_sequence_gaps(one[0], one[1], one[2], one[3], SEQ_SPLITS[0], gt=gt, return_ids=True)
    check_call(rec.calls[1], 'associate_sequences_gap', 2, expected_parts([one], True, [gt]), tables)
    check_results([res], [one], SEQ_SPLITS[:1], 2, True, ids=True)
    assert same(A.associate_sequence_gaps_batch(*columns([one]), SEQ_SPLITS[:1], gts=[gt], return_ids=True), [res])
    assert len(rec.calls) == 3 and all(torch.equal(rec.calls[1][k], rec.calls[2][k]) for k in ('det', 'new', 'end', 'link'))


def test_one_gap_goes_to_the_gap_operator(rec):
    one = sequence_instances(1, True)[0]
    two_d = (one[0], [[l[0] for l in one[1][0]]], one[2], one[3])  # n x m blocks are taken as 1 x n x m ones are
    res = A.associate_sequence_gaps(*two_d[:4], SEQ_SPLITS[0], return_ids=True)
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate_sequences_gap', 1, expected_parts([one], True), A.sequences_table(SEQ_SPLITS[:1])[:2])
    check_results([res], [two_d], SEQ_SPLITS[:1], 1, True, ids=True)
    assert res[1][0][0].shape == (2, 3)
    plain = sequence_instances()[0]
    same_blocks = A.associate_sequence(plain[0], plain[1], plain[2], plain[3], SEQ_SPLITS[0], return_ids=True)
    assert rec.calls[1]['op'] == 'associate_sequences' and rec.calls[1]['max_gap'] is None
    assert same(same_blocks[1], [l.view(1, *l.shape) for l in res[1][0]]) and same(same_blocks[4], res[4])


def test_associate_sequence_gaps_batch(rec):
    insts = sequence_instances(2, True)
    gts = [None, gt_of(insts[1], True)]
    res, obj = A.associate_sequence_gaps_batch(*columns(insts), SEQ_SPLITS, gts=gts, return_objective=True, return_ids=True)
    assert len(rec.calls) == 1
    check_call(rec.calls[0], 'associate_sequences_gap', 2, expected_parts(insts, True, gts),
               A.gap_sequences_table(SEQ_SPLITS, 2)[:2])
    check_results(res, insts, SEQ_SPLITS, 2, True, ids=True)
    # the second sequence's block starts at 24 + 11 + 8 = 43: 9 scores, two links of gap 1, one of gap 2
    assert res[1][0].tolist() == [43, 44, 45] and res[1][1][1][0].reshape(-1).tolist() == [54] and res[1][1][1][0].dtype == F64
    assert [i.tolist() for i in res[1][4]] == [[8], [9], [10]]
    assert obj.dtype == F64 and obj.shape == (2,)
    assert same(A.associate_sequence_gaps_batch(*columns(insts), SEQ_SPLITS, gts=gts), [r[:4] for r in res])


def test_gaps_launch_nothing_for_empty_sequences_and_refusals(rec):
    z = lambda *s: torch.zeros(*s)
    links = [[z(1, 0, 0), z(0, 0)], [z(1, 0, 0)]]
    got = A.associate_sequence_gaps(z(0), links, z(0), z(0), [0, 0, 0], return_ids=True)
    assert same(got, (z(0), links, z(0), z(0), [torch.zeros(0, dtype=torch.int64)] * 3, 0))
    insts = sequence_instances(2, True)
    with pytest.raises(ValueError, match='associate_sequence_gaps: max_gap = 2 needs more than 2 frames, got 2'):
        A.associate_sequence_gaps(z(2), [[z(1, 1)], []], z(2), z(2), [1, 1])
    with pytest.raises(ValueError, match=r'associate_sequence_gaps: link block \(gap 1, frame 0\) must be 2 x 3'):
        A.associate_sequence_gaps(insts[0][0], [[z(3, 2)] + insts[0][1][0][1:], insts[0][1][1]], insts[0][2], insts[0][3],
                                  SEQ_SPLITS[0])
    with pytest.raises(ValueError, match='associate_sequence_gaps_batch: no sequences'):
        A.associate_sequence_gaps_batch([], [], [], [], [])
    with pytest.raises(ValueError, match='associate_sequence_gaps_batch: every sequence needs a detection'):
        A.associate_sequence_gaps_batch(*columns([insts[0], (z(0), links, z(0), z(0))]), [SEQ_SPLITS[0], [0, 0, 0]])
    with pytest.raises(ValueError, match='associate_sequence_gaps_batch: every sequence needs the blocks of the same 2 gaps'):
        A.associate_sequence_gaps_batch(*columns([insts[0], sequence_instances(1, True)[1]]), SEQ_SPLITS)
    assert rec.calls == []


# ---- the offline pipeline's solve ------------------------------------------------------------------------------------
def global_rows(split):
    """per consecutive pair (det, link, new, end) flat rows with distinct values, as ``run_global`` selects them"""
    rows = []
    for p, (a, b) in enumerate(zip(split[:-1], split[1:])):
        base = 1000.0 * p
        sizes = ((1, a + b), (301, a * b), (101, a + b), (201, a + b))
        rows.append(tuple(base + k + torch.arange(n, dtype=F32) for k, n in sizes))
    return rows


def test_solve_global_chooses_the_operator_by_max_gap(rec, monkeypatch):
    split = SEQ_SPLITS[0]
    rows = global_rows(split)
    res = pipeline.solve_global(rows, split)
    assert len(rec.calls) == 1
    det = torch.tensor([1., 2., 3., 4., 5., 1004., 2002., 2003.])
    new = det + 100
    end = torch.tensor([201., 202., 1201., 1202., 1203., 2201., 2202., 2203.])
    link = torch.cat([r[1] for r in rows])
    check_call(rec.calls[0], 'associate_sequences', None, [det, new, end, link], A.sequences_table([split])[:2])
    assert res.max_gap == 1 and res.n_tracks == 0 and res.gap_assignment == []
    assert res.assignment[0].tolist() == list(range(8)) and res.assignment[1][2].reshape(-1).tolist() == [33, 34]
    assert [i.tolist() for i in res.ids] == [[0, 1], [2, 3, 4], [5], [6, 7]]
    gap2 = [5000.0 + torch.arange(2, dtype=F32), 6000.0 + torch.arange(6, dtype=F32)]
    res = pipeline.solve_global(rows, split, gap2, 2)
    assert len(rec.calls) == 2
    check_call(rec.calls[1], 'associate_sequences_gap', 2, [det, new, end, torch.cat([link] + gap2)],
               A.gap_sequences_table([split], 2)[:2])
    assert res.max_gap == 2 and [a.reshape(-1).tolist() for a in res.gap_assignment[0]] == [[35, 36], list(range(37, 43))]

    def failing(*a, **k):
        out, ids, obj, info = rec(*a, **k)
        info[0, 0] = 2
        return out, ids, obj, info
    monkeypatch.setattr(A, '_launch', failing)
    with pytest.raises(A.AssociationError, match='augmentation bound hit'):
        pipeline.solve_global(rows, split)


def test_layout_helpers_share_one_walk():
    split = [2, 0, 3]
    assert A.chain_block_size(split) == A.gap_block_size(split, 1) == 15 and A.chain_block_size((2, 3)) == 21
    block = torch.arange(21, dtype=F32)
    det, links, new, end = A.unpack(block, 2, 3)
    assert det.tolist() == [0, 1, 2, 3, 4] and end.tolist() == list(range(10, 15)) and links[0].shape == (1, 2, 3)
    assert links[0].reshape(-1).tolist() == list(range(15, 21)) and links[0].data_ptr() == block[15:].data_ptr()  # a view
    chain = A.unpack_chain(block[:15], split)
    gaps = A.unpack_gaps(block[:15], split, 1)
    assert same(chain, (gaps[0], gaps[1][0], gaps[2], gaps[3])) and [tuple(l.shape) for l in chain[1]] == [(1, 2, 0), (1, 0, 3)]
    shaped = A.unpack(block, 2, 3, torch.zeros(5, 1, dtype=F64), (2, 3))
    assert shaped[0].shape == (5, 1) and shaped[1][0].shape == (2, 3) and shaped[1][0].dtype == F64
    assert A.chains_table([split, [1, 2]])[0].tolist() == [[3, 0, 0, 2, 0, 3] + [0] * 5, [2, 5, 0, 1, 2] + [0] * 6]
    assert A.chains_table([split, [1, 2]])[1] == [0, 15]
