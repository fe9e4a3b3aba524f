"""PoolLevels (mmmot_amd/plan.py): the leveled segment tables of every user equal the formulas they were built from before
there was one builder - restated here in plain numpy, because the chunking fixes the summation order and so the bits - and
the runner pools level by level."""
import types

import numpy as np
import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd.plan import BatchPlan, CropPlan, PoolLevels
from mmmot_amd.tape import chunked_segments, colsum
from mmmot_amd.train_vgg import _pool_levels


def table(start, count, stride, div):
    n = len(start)
    full = lambda v: None if v is None else np.broadcast_to(np.asarray(v, np.int64), (n,))
    return dict(h_start=np.asarray(start, np.int64), h_count=np.asarray(count, np.int64), h_stride=full(stride), h_div=full(div))


def assert_levels(levels, want):
    assert len(levels.levels) == len(want)
    for seg, w in zip(levels.levels, want):
        assert seg.n == len(w['h_start'])
        for name, arr in w.items():
            got = getattr(seg, name)
            assert (got is None) == (arr is None), name
            if arr is not None:
                assert got.shape == arr.shape and (got == arr).all(), name
        assert (seg.h_group == 0).all()


def map_pool_formula(L, hw, chunk, longer_than):
    """L maps of hw rows: one level with the default divisor, or chunks of every map, then a map's chunk sums over hw"""
    if hw <= longer_than:
        return [table(np.arange(L) * hw, np.full(L, hw), 1, None)]
    S = -(-hw // chunk)
    l, c = np.repeat(np.arange(L), S), np.tile(np.arange(S), L)
    return [table(l * hw + c * chunk, np.minimum(chunk, hw - c * chunk), 1, 1),
            table(np.arange(L) * S, np.full(L, S), 1, hw)]


def strided_sum_formula(start, count, stride, chunk=128, longer_than=512):
    start, count = np.asarray(start, np.int64), np.asarray(count, np.int64)
    if count.max() <= longer_than:
        return [table(start, count, stride, 1)]
    nch = -(-count // chunk)
    s1 = np.concatenate([start[i] + stride * chunk * np.arange(nch[i]) for i in range(len(start))])
    c1 = np.concatenate([np.minimum(chunk, count[i] - chunk * np.arange(nch[i])) for i in range(len(start))])
    return [table(s1, c1, stride, 1), table(np.concatenate([[0], np.cumsum(nch)[:-1]]), nch, 1, 1)]


def colsum_formula(rows, chunk=128):
    out = []
    while rows > 2 * chunk:
        n = -(-rows // chunk)
        start = np.arange(n) * chunk
        out.append(table(start, np.minimum(chunk, rows - start), 1, 1))
        rows = n
    return out + [table([0], [rows], 1, 1)]


@pytest.mark.parametrize('hw,nlev', [(49, 1), (784, 2)])
def test_crop_pool_tables(hw, nlev):
    want = map_pool_formula(3, hw, 256, 256)
    assert len(want) == nlev
    if nlev == 2:  # four chunks, the last of 16 rows, divided by 784 at the end
        assert want[0]['h_count'][:4].tolist() == [256, 256, 256, 16] and (want[1]['h_div'] == 784).all()
    plan = BatchPlan([([1, 2], None)], 32, 'cpu', rows=(0,), use_points=False)
    assert_levels(plan.crop_segments(hw), want)
    assert_levels(CropPlan(3, 32, 'cpu').crop_segments(hw), want)
    assert plan.crop_segments(hw) is plan.crop_segments(hw)


@pytest.mark.parametrize('hw,nlev', [(196, 1), (784, 2)])
def test_training_head_pool_tables(hw, nlev):
    want = map_pool_formula(3, hw, 128, 512)
    assert len(want) == nlev
    if nlev == 2:  # seven chunks, the last of 16
        assert want[0]['h_count'][:7].tolist() == [128] * 6 + [16] and (want[1]['h_count'] == 7).all()
    cache = {}
    assert_levels(_pool_levels(cache, 3, hw, 'cpu'), want)
    assert _pool_levels(cache, 3, hw, 'cpu') is _pool_levels(cache, 3, hw, 'cpu')


def test_chunked_segments_tables():
    start, count = [0, 1, 1200], [600, 600, 3]
    want = strided_sum_formula(start, count, 2)
    assert [len(w['h_start']) for w in want] == [5 + 5 + 1, 3]
    assert_levels(chunked_segments(np.array(start), np.array(count), 2, 'cpu'), want)
    want = strided_sum_formula([0, 1], [40, 40], 2)
    assert len(want) == 1
    assert_levels(chunked_segments(np.array([0, 1]), np.array([40, 40]), 2, 'cpu'), want)


@pytest.mark.parametrize('rows,ns', [(256, [1]), (257, [3, 1]), (33000, [258, 3, 1])])
def test_colsum_levels(rows, ns):
    want = colsum_formula(rows)
    assert [len(w['h_start']) for w in want] == ns
    eng = types.SimpleNamespace(ops=TorchOps(torch.float64))
    X = torch.arange(rows * 8, dtype=torch.float64).view(rows, 8)[:, :4]  # a column slice: summed as it lies, no folding
    assert torch.equal(colsum(eng, X), X.sum(0))                          # integers: exact in any order
    assert_levels(eng._colsum_segs[(rows, 'cpu')], want)


TWO_LEVEL = {
    'crop pool': lambda: (CropPlan(3, 32, 'cpu').crop_segments(784), np.arange(3) * 784, [784] * 3, 1, [784] * 3),
    'training head': lambda: (_pool_levels({}, 3, 784, 'cpu'), np.arange(3) * 784, [784] * 3, 1, [784] * 3),
    'strided sums': lambda: (chunked_segments(np.array([0, 1, 1200]), np.array([600, 600, 3]), 2, 'cpu'), [0, 1, 1200],
                             [600, 600, 3], 2, [1] * 3),
}


@pytest.mark.parametrize('which', sorted(TWO_LEVEL))
def test_runner_equals_the_plain_pool(which):
    levels, start, count, stride, div = TWO_LEVEL[which]()
    assert len(levels.levels) == 2
    C = 8
    X = torch.randn(3 * 784, C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    out = torch.full((3, C), float('nan'), dtype=torch.float64)
    levels.pool(TorchOps(torch.float64), X, C, out)
    rows = [X[s:s + (n - 1) * stride + 1:stride] / d for s, n, d in zip(start, count, div)]
    want, absum = torch.stack([r.sum(0) for r in rows]), torch.stack([r.abs().sum(0) for r in rows])
    # two summation orders of n terms in float64: each within n * 2^-53 * sum |x| of the exact sum
    assert ((out - want).abs() <= 2 * max(count) * 2.0 ** -53 * absum).all()


def test_runner_describes_the_input_to_the_first_level_only():
    calls = []

    class Recorder:
        def segment_mean(self, X, C, segs, out, **kw):
            calls.append((X, segs, out, kw))

    levels = PoolLevels.chunked([0], [33000], 1, 'cpu', chunk=128, longer_than=256, div=1, repeat=True)
    X, out, bufs = torch.zeros(33000, 4), torch.zeros(1, 4), []

    def partial(rows):
        bufs.append(torch.zeros(rows, 4))
        return bufs[-1]

    levels.pool(Recorder(), X, 4, out, partial=partial, hl16=2, relu=True)
    assert [c[1] for c in calls] == levels.levels and [b.shape[0] for b in bufs] == [258, 3]
    assert calls[0][3] == dict(use_group=False, hl16=2, relu=True)
    assert calls[1][3] == calls[2][3] == dict(use_group=False)
    assert calls[0][0] is X and calls[0][2] is bufs[0] and calls[1][0] is bufs[0] and calls[1][2] is bufs[1]
    assert calls[2][0] is bufs[1] and calls[2][2] is out
