"""The relations the shared pool skeleton (csrc/segpool.h) exists to guarantee, at the smallest shapes that can break them:
counts around the 4-wave split and the 16-row stride of the mean, one and two channel blocks (C = 4: one busy lane; C = 260:
a second block with one busy lane), two groups with their own sc / sh, a stride-3 segment.  The dropout pool with nothing
dropped against the plain pool is tests/test_pointnet_dropout_gpu.py (same counts); the arg-max kernels against their
specification on plan-shaped segments are tests/test_end_max_gpu.py."""
import numpy as np
import pytest
import torch

from mmmot_amd.plan import PoolLevels, Segments
from test_kernels_gpu import hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POOL_COUNTS = [1, 3, 4, 5, 13, 16, 17, 65]
STRIDED = (17, 3)  # one more segment: 17 rows with stride 3


def exact_case(C):
    """Segments of POOL_COUNTS rows (stride 1) and the STRIDED one behind them, alternating between two groups, on inputs
    with exact fp32 arithmetic: X on a shuffled grid of spacing 2^-10 below 2^11, sc powers of two, sh multiples of 2^-10,
    so fmaf(x, sc, sh) is the rounded multiply-then-add torch does on the host.  Column 1 of every segment of at least 5
    rows holds an exact tie of the maximum between rows 1 and 4 (waves 1 and 0)."""
    cnt = np.asarray(POOL_COUNTS + [STRIDED[0]])
    stride = np.asarray([1] * len(POOL_COUNTS) + [STRIDED[1]])
    span = (cnt - 1) * stride + 1
    start = np.concatenate([[0], np.cumsum(span)[:-1]])
    grp = np.arange(len(cnt)) % 2
    R = int(span.sum())
    g = torch.Generator().manual_seed(17)
    X = ((torch.randperm(R * C, generator=g).double() - R * C // 2) * 2.0 ** -10).float().view(R, C)
    sc = torch.pow(2.0, torch.randint(-1, 2, (2, C), generator=g).float())
    sh = torch.randint(-200 * 1024, 200 * 1024, (2, C), generator=g).float() * 2.0 ** -10
    sc[:, 1] = 1.0
    tied = [s for s in range(len(cnt)) if cnt[s] >= 5]
    for s in tied:
        X[start[s] + 1 * stride[s], 1] = X[start[s] + 4 * stride[s], 1] = 4096.0
    rowgrp = torch.as_tensor(np.repeat(grp, span))
    a = torch.relu(X * sc[rowgrp] + sh[rowgrp])
    assert torch.equal(a.double(), torch.relu(X.double() * sc[rowgrp].double() + sh[rowgrp].double()))
    return X, sc, sh, a, (start, cnt, stride, grp), tied


@pytest.mark.parametrize('C', [4, 260])
def test_argmax_rows_hold_what_the_max_pool_wrote(hip, C):
    X, sc, sh, a, (start, cnt, stride, grp), tied = exact_case(C)
    sg = Segments(start, cnt, stride, grp, DEV)
    Xg, scg, shg = X.cuda(), sc.cuda(), sh.cuda()
    V = torch.full((sg.n, C), float('nan'), device=DEV)
    hip.segment_mean(Xg, C, sg, V, sc=scg, sh=shg, relu=True, take_max=True)
    idx = torch.full((sg.n, C), -1, dtype=torch.int32, device=DEV)
    hip.segment_argmax(Xg, C, sg, idx, sc=scg, sh=shg, relu=True)
    idx = idx.cpu().long()
    assert (idx >= 0).all() and (idx < torch.as_tensor(cnt).view(-1, 1)).all()
    assert (idx[tied, 1] == 1).all()  # the tie goes to the lower index, not to the lower wave
    rows = torch.as_tensor(start).view(-1, 1) + idx * torch.as_tensor(stride).view(-1, 1)
    assert torch.equal(a.gather(0, rows), V.cpu())
    first = torch.stack([torch.where(a[s0:s0 + (n - 1) * st + 1:st] == V.cpu()[s], torch.arange(n).view(-1, 1), n).min(0)[0]
                         for s, (s0, n, st) in enumerate(zip(start, cnt, stride))])  # the FIRST row at the maximum
    assert torch.equal(idx, first)


@pytest.mark.parametrize('C', [4, 260])
def test_runner_is_the_explicit_launches(hip, C):
    """PoolLevels.pool on a two-level table = the two segment_mean launches, the prologue on the first level only"""
    levels = PoolLevels.chunked([0, 200], [65, 17], [1, 3], DEV, chunk=16, longer_than=16)
    assert [lv.n for lv in levels.levels] == [5 + 2, 2] and levels.levels[0].h_count.tolist() == [16] * 4 + [1, 16, 1]
    X, sc, sh = rnd(256, C, seed=5).cuda(), (rnd(1, C, seed=6) * 0.5 + 1.0).cuda(), (rnd(1, C, seed=7) * 0.3).cuda()
    got = torch.full((2, C), float('nan'), device=DEV)
    levels.pool(hip, X, C, got, sc=sc, sh=sh, relu=True)
    part, want = torch.empty(7, C, device=DEV), torch.empty(2, C, device=DEV)
    hip.segment_mean(X, C, levels.levels[0], part, use_group=False, sc=sc, sh=sh, relu=True)
    hip.segment_mean(part, C, levels.levels[1], want, use_group=False)
    assert torch.equal(got, want)
    ref = torch.stack([torch.relu(X[s:s + (n - 1) * st + 1:st].double() * sc.double() + sh.double()).mean(0)
                       for s, n, st in ((0, 65, 1), (200, 17, 3))])
    # fp32 sums of n <= 65 non-negative terms: within 2 n 2^-24 of their exact sum (the terms' own rounding included)
    assert ((got.double().cpu() - ref.cpu()).abs() <= 2 * 65 * 2.0 ** -24 * ref.cpu()).all()
