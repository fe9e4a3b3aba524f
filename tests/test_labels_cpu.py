"""Training labels without a GPU: the NumPy restatement of tests/labels_ref.py equals the fixtures of the imported
reference (tools/gen_golden_labels.py: crafted cases, 200 random chains and 60 random frames); the host helpers of
mmmot_amd.labels (layout, shapes, dtypes, refusals) work on CPU tensors over a fake operator that answers from the
restatement; the library exports both entry points and rejects bad arguments before any launch."""
import os

import numpy as np
import pytest
import torch

import labels_ref
from mmmot_amd import _lib, labels
from mmmot_amd.association import chain_block_size, chains_table, unpack_chain

GOLDEN = labels_ref.GOLDEN


# ---- the restatement against the reference ----------------------------------------------------------------------------
def test_restatement_equals_the_generate_gt_fixture():
    names = []
    for name, split, cls, ids, block in labels_ref.gt_fixture():
        got = labels_ref.block_of(labels_ref.generate_gt(cls, ids, split))
        assert got.dtype == block.dtype == np.float32 and np.array_equal(got, block), name
        names.append(split)
    assert [1, 1] in names and [3, 0] in names and [0, 2] in names and [5, 7] in names
    assert any(len(s) == 3 and s[1] == 0 for s in names) and any(len(s) == 8 for s in names)


def test_restatement_equals_the_match_fixture():
    z = np.load(os.path.join(GOLDEN, 'labels_match.npz'))
    assert int(z['car']) == labels.CAR and int(z['dontcare']) == labels.DONTCARE
    seen = set()
    for name, det, gt, gid, gname, want_id, want_cls in labels_ref.match_fixture():
        got_id, got_cls = labels_ref.match_dets(det, gt, gid, gname)
        assert np.array_equal(got_id, want_id) and np.array_equal(got_cls, want_cls), name
        seen |= set(int(c) for c in want_cls)
    assert seen == {-1, 0, 1}


def test_restatement_equals_the_reference_on_random_chains():
    """200 seeded chains (T <= 8, n <= 12) that the imported reference was run on when the fixture was made"""
    count, frames = 0, set()
    for k, split, cls, ids, block in labels_ref.gt_fixture_random():
        got = labels_ref.block_of(labels_ref.generate_gt(cls, ids, split))
        assert got.shape == block.shape and np.array_equal(got, block), (k, split)
        count += 1
        frames.add(len(split))
    assert count == 200 and frames == set(range(2, 9))


def test_restatement_equals_the_reference_on_random_frames():
    """60 seeded frames (n_det, n_gt <= 12, float64 and float32 boxes) run through the imported reference"""
    count, dtypes = 0, set()
    for k, det, gt, gid, gname, want_id, want_cls in labels_ref.match_fixture_random():
        got = labels_ref.match_dets(det, gt, gid, gname)
        assert np.array_equal(got[0], want_id) and np.array_equal(got[1], want_cls), (k, det.shape, gt.shape)
        count += 1
        dtypes.add(det.dtype.type)
    assert count == 60 and dtypes == {np.float32, np.float64}


# ---- host helpers over a fake operator --------------------------------------------------------------------------------
def fake_generate_gt(ids, cls, chains):
    """mmmot::generate_gt answered from the restatement (CPU tensors)"""
    assert ids.dtype == cls.dtype == torch.int32 and chains.dtype == torch.int32 and chains.shape[1] == 11
    blocks = []
    for row in chains.tolist():
        T, so, split = row[0], row[1], row[3:3 + row[0]]
        cut = np.cumsum(split)[:-1]
        L = sum(split)
        c, i = cls[so:so + L].numpy(), ids[so:so + L].numpy()
        blocks.append(labels_ref.block_of(labels_ref.generate_gt(np.split(c, cut), np.split(i, cut), split)))
    return torch.from_numpy(np.concatenate(blocks))


def fake_match_dets(det_xywh, gt_xywh, gt_id, gt_name, frames, car, dontcare, max_iou):
    assert det_xywh.dtype == gt_xywh.dtype == torch.float64 and gt_id.dtype == gt_name.dtype == torch.int32
    res = torch.empty((2, det_xywh.shape[0]), dtype=torch.int32)
    for do, nd, go, ng in frames.tolist():
        i, c = labels_ref.match_xywh(det_xywh[do:do + nd].numpy(), gt_xywh[go:go + ng].numpy(), gt_id[go:go + ng].numpy(),
                                     gt_name[go:go + ng].numpy(), car, dontcare, max_iou)
        res[0, do:do + nd], res[1, do:do + nd] = torch.from_numpy(i).int(), torch.from_numpy(c).int()
    return res


@pytest.fixture
def fake_op(monkeypatch):
    monkeypatch.setattr(labels, '_op_generate_gt', fake_generate_gt)
    monkeypatch.setattr(labels, '_op_match_dets', fake_match_dets)
    monkeypatch.setattr(labels, '_DEVICE', 'cpu')


def test_generate_gt_drop_in_shapes_and_dtypes(fake_op):
    for name, split, cls, ids, block in labels_ref.gt_fixture():
        L = sum(split)
        t = lambda v: torch.from_numpy(v).view(1, -1, 1)
        for dtype in (torch.float32, torch.float64):
            score = torch.zeros(L, dtype=dtype)
            got = labels.generate_gt(score, [t(c) for c in cls], [t(i) for i in ids], [torch.tensor([n]) for n in split])
            gt_det, gt_link, gt_new, gt_end = got
            for x in (gt_det, gt_new, gt_end):
                assert x.shape == score.shape and x.dtype == dtype
            assert [tuple(l.shape) for l in gt_link] == [(1, a, b) for a, b in zip(split[:-1], split[1:])]
            assert all(l.dtype == dtype for l in gt_link)
            flat = torch.cat([gt_det, gt_new, gt_end] + [l.reshape(-1) for l in gt_link])
            assert np.array_equal(flat.numpy().astype(np.float32), block), name
            # the solver's order
            s = labels.as_solver_gt(got)
            assert s[0] is gt_det and s[1] is gt_new and s[2] is gt_end and isinstance(s[3], list) and len(s[3]) == len(gt_link)
            assert all(a is b for a, b in zip(s[3], gt_link))


def test_generate_gt_empty_sample_is_answered_on_the_host():
    got = labels.generate_gt(torch.zeros(0), [torch.zeros(1, 0, 1, dtype=torch.long)] * 3,
                             [torch.zeros(1, 0, 1, dtype=torch.long)] * 3, [torch.tensor([0])] * 3)
    assert got[0].numel() == got[2].numel() == got[3].numel() == 0
    assert [tuple(l.shape) for l in got[1]] == [(1, 0, 0), (1, 0, 0)]


def test_generate_gt_batch_uses_the_chain_table(fake_op):
    cases = list(labels_ref.gt_fixture())
    splits = [c[1] for c in cases]
    t = lambda v: torch.from_numpy(v)
    block, offs, per = labels.generate_gt_batch([[t(x) for x in c[2]] for c in cases], [[t(x) for x in c[3]] for c in cases],
                                                splits)
    chains, want_offs = chains_table(splits)
    assert list(offs) == list(want_offs) and block.dtype == torch.float32
    assert block.numel() == sum(chain_block_size(s) for s in splits)
    for (name, split, _, _, want), o, lab in zip(cases, offs, per):
        assert np.array_equal(block[o:o + chain_block_size(split)].numpy(), want), name
        ref = unpack_chain(torch.from_numpy(want), split)
        assert all(torch.equal(a, b) for a, b in zip([lab[0], lab[2], lab[3]] + lab[1], [ref[0], ref[2], ref[3]] + ref[1]))
    like = torch.zeros(1, dtype=torch.float64)
    _, _, per64 = labels.generate_gt_batch([[t(x) for x in c[2]] for c in cases], [[t(x) for x in c[3]] for c in cases],
                                           splits, like=like)
    assert all(x.dtype == torch.float64 for lab in per64 for x in [lab[0], lab[2], lab[3]] + lab[1])


def test_generate_gt_refusals(fake_op):
    one = lambda *v: torch.tensor(v, dtype=torch.long).view(1, -1, 1)
    ok = dict(det_score=torch.zeros(3), det_cls=[one(1, 1), one(1)], det_id=[one(1, 2), one(2)], det_split=[2, 1])
    labels.generate_gt(**ok)
    with pytest.raises(ValueError):  # ids outside int32, on the host
        labels.generate_gt(**dict(ok, det_id=[one(1, 2 ** 31), one(2)]))
    with pytest.raises(ValueError):
        labels.generate_gt(**dict(ok, det_id=[one(1, -2 ** 31 - 1), one(2)]))
    with pytest.raises(ValueError):  # a frame that does not match the split
        labels.generate_gt(**dict(ok, det_cls=[one(1, 1, 1), one(1)]))
    with pytest.raises(ValueError):
        labels.generate_gt(**dict(ok, det_score=torch.zeros(4)))
    with pytest.raises(ValueError):
        labels.generate_gt(**dict(ok, det_id=[one(1, 2)]))
    with pytest.raises(ValueError):  # one frame is not a chain
        labels.generate_gt(torch.zeros(2), [one(1, 1)], [one(1, 2)], [2])
    with pytest.raises(ValueError):  # more than 8 frames
        labels.generate_gt(torch.zeros(9), [one(1)] * 9, [one(1)] * 9, [1] * 9)
    wide = torch.ones(1, 513, 1, dtype=torch.long)
    with pytest.raises(ValueError, match='mmmot::generate_gt: every frame needs'):  # the refusal names this operator
        labels.generate_gt(torch.zeros(514), [wide, one(1)], [wide, one(1)], [513, 1])
    with pytest.raises(ValueError):  # floating-point ids
        labels.generate_gt(**dict(ok, det_id=[one(1, 2).float(), one(2).float()]))
    with pytest.raises(ValueError):
        labels.generate_gt_batch([], [], [])
    with pytest.raises(ValueError):  # an empty sample in a batch
        labels.generate_gt_batch([[one(), one()]], [[one(), one()]], [[0, 0]])


def test_match_dets_drop_in(fake_op):
    frames = list(labels_ref.match_fixture())
    for name, det, gt, gid, gname, want_id, want_cls in frames:
        for wrap in (lambda a: a, torch.from_numpy):
            rid, rcls = labels.match_dets(wrap(det), wrap(gt), wrap(gid), wrap(gname))
            assert rid.dtype == rcls.dtype == torch.long and tuple(rid.shape) == tuple(rcls.shape) == (len(det), 1)
            assert np.array_equal(rid.numpy().reshape(-1), want_id) and np.array_equal(rcls.numpy().reshape(-1), want_cls)
    crafted = frames  # all of them in one call
    res = labels.match_dets_batch([f[1] for f in crafted], [f[2] for f in crafted], [f[3] for f in crafted],
                                  [f[4] for f in crafted])
    assert len(res) == len(crafted)
    for f, (rid, rcls) in zip(crafted, res):
        assert np.array_equal(rid.numpy().reshape(-1), f[5]) and np.array_equal(rcls.numpy().reshape(-1), f[6]), f[0]
    # no detection: nothing to launch
    rid, rcls = labels.match_dets(np.zeros((0, 4)), crafted[0][2], crafted[0][3], crafted[0][4])
    assert tuple(rid.shape) == tuple(rcls.shape) == (0, 1) and rid.dtype == torch.long


def test_match_dets_width_and_height_in_the_input_dtype(fake_op, monkeypatch):
    seen = {}

    def spy(det_xywh, gt_xywh, *a):
        seen['det'], seen['gt'] = det_xywh.clone(), gt_xywh.clone()
        return fake_match_dets(det_xywh, gt_xywh, *a)
    monkeypatch.setattr(labels, '_op_match_dets', spy)
    det = np.array([[0.1, 0.2, 50.3, 40.7]], np.float32)
    gt = np.array([[1.1, 0.9, 49.6, 41.2]], np.float32)
    labels.match_dets(det, gt, np.array([5]), np.array([0]))
    for got, src in ((seen['det'], det), (seen['gt'], gt)):
        want = np.concatenate([src[:, :2], src[:, 2:] - src[:, :2]], 1)  # float32 subtraction, then widened
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want.astype(np.float64))


def test_match_dets_refusals(fake_op):
    det, gt = np.zeros((2, 4)), np.zeros((3, 4))
    with pytest.raises(ValueError):
        labels.match_dets(np.zeros((2, 3)), gt, np.zeros(3, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        labels.match_dets(det, gt, np.zeros(2, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        labels.match_dets(det, gt, np.array([1, 2, 2 ** 31]), np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        labels.match_dets(np.zeros((513, 4)), gt, np.zeros(3, np.int64), np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        labels.match_dets_batch([], [], [], [])


# ---- operators and the library ----------------------------------------------------------------------------------------
def test_meta_kernels_and_no_cpu_kernel():
    chains, _ = chains_table([[3, 4, 2], [5, 2]])
    ids = torch.empty(16, dtype=torch.int32, device='meta')
    out = torch.ops.mmmot.generate_gt(ids, ids, chains)
    assert out.shape == (3 * 9 + 20 + 3 * 7 + 10,) and out.dtype == torch.float32 and out.device.type == 'meta'
    frames = torch.tensor([[0, 3, 0, 2], [3, 4, 2, 0]], dtype=torch.int32)
    box = torch.empty((7, 4), dtype=torch.float64, device='meta')
    code = torch.empty(2, dtype=torch.int32, device='meta')
    res = torch.ops.mmmot.match_dets(box, box[:2], code, code, frames, 0, -1, 0.5)
    assert res.shape == (2, 7) and res.dtype == torch.int32 and res.device.type == 'meta'
    with pytest.raises(NotImplementedError):  # no CPU kernel, no fallback
        torch.ops.mmmot.generate_gt(torch.zeros(9, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), chains[:1])
    with pytest.raises(NotImplementedError):
        torch.ops.mmmot.match_dets(torch.zeros((7, 4), dtype=torch.float64), torch.zeros((2, 4), dtype=torch.float64),
                                   torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), frames, 0, -1, 0.5)


def test_match_layout_rejections():
    from mmmot_amd.torch_ops import match_layout
    f = lambda *rows: torch.tensor(rows, dtype=torch.int32)
    assert match_layout(f([0, 3, 0, 2], [3, 4, 2, 0]), 7, 2) == 4
    assert match_layout(f([0, 0, 0, 0])) == 1 and match_layout(f([0, 512, 0, 512])) == 512
    for bad in (f([0, 513, 0, 1]), f([0, 1, 0, 513]), f([-1, 1, 0, 1]), f([0, 1, 0, -1]), f([0, 3, 0, 2], [2, 4, 2, 0])):
        with pytest.raises(ValueError):
            match_layout(bad)
    with pytest.raises(ValueError):
        match_layout(f([0, 3, 0, 2]), 2, 2)
    with pytest.raises(ValueError):
        match_layout(f([0, 3, 0, 2]), 3, 1)
    with pytest.raises(ValueError):
        match_layout(f([0, 3, 0, 2]).long())
    with pytest.raises(ValueError):
        match_layout(f([0, 3, 0, 2])[:0])


def test_entry_points_exported_and_reject_bad_arguments():
    lib = _lib.load()
    assert hasattr(lib, 'mmmot_generate_gt') and hasattr(lib, 'mmmot_match_dets')
    assert lib.mmmot_abi_version() == 10
    d = 4096  # never dereferenced: the argument checks come before any launch
    f = lib.mmmot_generate_gt
    args = [d, d, d, 1, 8, 16, d, d, None]
    for k in (0, 1, 2, 6, 7):  # each pointer NULL in turn
        bad = list(args)
        bad[k] = None
        assert f(*bad) == -1, k
    for B, n, L in ((0, 8, 16), (-3, 8, 16), (1, 0, 16), (1, 513, 1024), (1, 8, 7), (1, 8, 0), (1, 512, 1025), (1, 8, 65)):
        bad = list(args)
        bad[3], bad[4], bad[5] = B, n, L
        assert f(*bad) == -1, (B, n, L)
    g = lib.mmmot_match_dets
    args = [d, d, d, d, d, 1, 0, -1, 0.5, 8, d, d, None]
    for k in (0, 1, 2, 3, 4, 10, 11):
        bad = list(args)
        bad[k] = None
        assert g(*bad) == -1, k
    for NF, n in ((0, 8), (-1, 8), (1, 0), (1, 513)):
        bad = list(args)
        bad[5], bad[9] = NF, n
        assert g(*bad) == -1, (NF, n)
    bad = list(args)
    bad[0] = d + 4  # fp64 boxes need 8-byte alignment
    assert g(*bad) == -1
