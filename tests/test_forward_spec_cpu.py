"""The entries of tests/fake_ops.py that tests/test_forward_kernels_gpu.py leans on and that no other CPU test pins, against
direct float64 torch expressions: segment_mean(take_max=True), rowdot with each activation and with the threshold, and
softmax_pairs in its four modes on logits far from zero (offset +200, spread over +-60), where the specification itself
has to stay finite."""
import numpy as np
import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd.plan import RowTiles, Segments

emu = TorchOps(torch.float64)


def rnd64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def far_logits(NM, seed=0):
    """one block of N x M logits per group: +200, spread uniformly over +-60 (fp32 values)"""
    g = torch.Generator().manual_seed(seed)
    R = sum(n * m for n, m in NM)
    return (200.0 + (torch.rand(R, generator=g) * 2.0 - 1.0) * 60.0).float()


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('div', [False, True])
def test_segment_max(norm, relu, div):
    """maximum over the rows of a (strided) segment after the optional affine and ReLU; a divisor does not enter it"""
    C = 12
    start, count, stride, group = [0, 3, 40, 2], [3, 37, 1, 13], [1, 1, 1, 3], [0, 1, 1, 0]
    X = -rnd64(41, C + 4, seed=1).abs() - 0.5                      # all negative: the maximum is not 0 by accident
    sc, sh = rnd64(2, C, seed=2), rnd64(2, C, seed=3)
    sg = Segments(start, count, stride, group, 'cpu', div=[7, 7, 7, 7] if div else None)
    out = torch.full((4, C), float('nan'), dtype=torch.float64)
    emu.segment_mean(X, C, sg, out, sc=sc if norm else None, sh=sh if norm else None, relu=relu, take_max=True)
    for s in range(4):
        rows = torch.stack([X[start[s] + t * stride[s], :C] for t in range(count[s])])
        if norm:
            rows = rows * sc[group[s]] + sh[group[s]]
        if relu:
            rows = rows.clamp(min=0.0)
        assert torch.equal(out[s], rows.amax(0)), (s, norm, relu, div)
    if not norm and not relu:
        assert (out < 0).all()


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('norm', [False, True])
def test_rowdot_activations(act, norm):
    K = 20
    tl = RowTiles([3, 130], 'cpu')
    R = tl.R
    X, w = rnd64(R, K + 4, seed=4), rnd64(K, seed=5)
    sc, sh = rnd64(2, K, seed=6), rnd64(2, K, seed=7)
    out = torch.full((R,), float('nan'), dtype=torch.float64)
    emu.rowdot(X, K, w, 0.25, tl, out, sc=sc if norm else None, sh=sh if norm else None, act=act)
    grp = torch.repeat_interleave(torch.arange(2), torch.tensor([3, 130]))
    A = X[:, :K]
    if norm:
        A = (A * sc[grp] + sh[grp]).clamp(min=0.0)
    s = (A * w).sum(1) + 0.25
    want = s if act == 0 else s.clamp(min=0.0) if act == 1 else 1.0 / (1.0 + torch.exp(-s))
    assert (out - want).abs().max().item() < 1e-13


def test_rowdot_threshold_and_output_map():
    """scores below the threshold leave as score - 1 (the reference's 'not a detection' marker), the others unchanged; omap
    scatters the rows"""
    K = 8
    tl = RowTiles([50], 'cpu')
    X, w = rnd64(50, K, seed=8), rnd64(K, seed=9)
    s = 1.0 / (1.0 + torch.exp(-((X * w).sum(1) - 0.1)))
    thr = 0.5
    assert (s < thr).any() and (s >= thr).any() and (s - thr).abs().min().item() > 1e-6
    out = torch.full((50,), float('nan'), dtype=torch.float64)
    emu.rowdot(X, K, w, -0.1, tl, out, act=2, use_thr=True, thr=thr)
    assert (out - torch.where(s < thr, s - 1.0, s)).abs().max().item() < 1e-13
    omap = torch.randperm(60, generator=torch.Generator().manual_seed(10))[:50].int()
    out2 = torch.full((60,), float('nan'), dtype=torch.float64)
    emu.rowdot(X, K, w, -0.1, tl, out2, act=2, omap=omap)
    assert (out2[omap.long()] - s).abs().max().item() < 1e-13
    assert int(torch.isnan(out2).sum()) == 10


@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_softmax_pairs_far_from_zero(mode):
    """exp(260) overflows float32 and exp(-120) underflows it: the specification has to subtract the maxima, and does - in
    float64 and in float32 (the yardstick of the device test) alike"""
    NM = [(5, 7), (1, 1), (1, 9), (3, 300), (64, 1)]
    x32 = far_logits(NM, seed=11)
    assert x32.min().item() < 145.0 and x32.max().item() > 255.0
    row0 = torch.tensor(np.concatenate([[0], np.cumsum([n * m for n, m in NM])[:-1]]))
    gN, gM = torch.tensor([n for n, _ in NM]), torch.tensor([m for _, m in NM])
    outs = {}
    for dtype in (torch.float64, torch.float32):
        x = x32.to(dtype)
        out = torch.full_like(x, float('nan'))
        emu.softmax_pairs(x, out, row0, gN, gM, len(NM), 400, mode)
        assert torch.isfinite(out).all() and out.min().item() >= 0.0 and out.max().item() <= 1.0
        outs[dtype] = out
    assert (outs[torch.float32].double() - outs[torch.float64]).abs().max().item() < 1e-6
    for g, (n, m) in enumerate(NM):
        x = x32.double()[int(row0[g]):int(row0[g]) + n * m].view(n, m)
        e_r = torch.exp(x - x.amax(1, keepdim=True))
        e_c = torch.exp(x - x.amax(0, keepdim=True))
        p, q = e_r / e_r.sum(1, keepdim=True), e_c / e_c.sum(0, keepdim=True)
        want = p if mode == 1 else p * q if mode == 2 else (p + q) / 2 if mode == 3 else torch.maximum(p, q)
        got = outs[torch.float64][int(row0[g]):int(row0[g]) + n * m].view(n, m)
        assert (got - want).abs().max().item() < 1e-14, (g, mode)
        if mode == 1:
            assert (got.sum(1) - 1.0).abs().max().item() < 1e-13
