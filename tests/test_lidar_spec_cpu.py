"""The entries of tests/fake_ops.py that tests/test_lidar_kernels_gpu.py leans on - gemm_ares, gram_rows,
gn_finalize_gram(_dbias), pn_mlp64, pointnet_layer1, skippool_head, and gn_finalize over half tiles - against plain
float64 statements that share no code with them: v = relu(X * sc + sh) @ W.T + bias (+ dbias[det]) is materialised row by
row from the detection sizes alone (no tile table), and torch.var / mean / F.group_norm / F.layer_norm / F.linear are
taken of it.  The half tiles are derived here from the detection sizes too, so a specification that walked the tile
table wrongly would not be compared with itself."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fake_ops import TorchOps
from mmmot_amd.pack import from_hl16, hl16_weight_shift, to_hl16
from mmmot_amd.plan import HalfTiles, RowTiles

F64 = torch.float64
emu = TorchOps(F64)
EPS = 1e-5
# two samples; detections with an empty second half (1, 64), a partial one (65, 130: a second tile of 2 rows), full tiles
DETS = [[1, 65, 130, 64], [3, 257]]


def rnd64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def same(got, ref, what, rtol=1e-12):
    assert got.shape == ref.shape, what
    err = (got.double() - ref).abs().max().item()
    assert err <= rtol * max(ref.abs().max().item(), 1e-30), '%s: error %.3e' % (what, err)


def layer(K, N, dets=DETS, seed=0, far=1.0):
    """inputs of one PointNet layer and, from the detection sizes alone: the row -> sample / detection maps, the 64-row
    half tiles [(first row, rows)] (two per 128-row tile of a detection, the second possibly empty) and v"""
    flat = [c for d in dets for c in d]
    counts = [sum(d) for d in dets]
    R, G, L = sum(flat), len(dets), len(flat)
    row_grp = torch.repeat_interleave(torch.arange(G), torch.tensor(counts))
    row_det = torch.repeat_interleave(torch.arange(L), torch.tensor(flat))
    X = rnd64(R, K, seed=seed) + 0.5
    sc, sh = rnd64(G, K, seed=seed + 1).abs() + 0.5, rnd64(G, K, seed=seed + 2)
    W = rnd64(N, K, seed=seed + 3) * K ** -0.5
    shift = hl16_weight_shift(W.float())
    W16 = to_hl16(W * 2.0 ** shift)
    Wq = from_hl16(W16).double() * 2.0 ** -shift          # the weights the hl16 entries see
    bias, dbias = rnd64(N, seed=seed + 4) * far, rnd64(L, N, seed=seed + 5) * far
    osc, osh = rnd64(G, N, seed=seed + 6).abs() + 0.5, rnd64(G, N, seed=seed + 7)
    a = torch.relu(X * sc[row_grp] + sh[row_grp])
    halves, r = [], 0
    for c in flat:
        for t0 in range(0, c, 128):
            n = min(128, c - t0)
            halves += [(r + t0, min(n, 64)), (r + t0 + 64, max(n - 64, 0))]
        r += c
    return dict(dets=dets, K=K, N=N, R=R, G=G, L=L, flat=flat, counts=counts, row_grp=row_grp, row_det=row_det, X=X, sc=sc, sh=sh, W=W,
                W16=W16, osv=2.0 ** -shift, Wq=Wq, bias=bias, dbias=dbias, osc=osc, osh=osh, a=a, halves=halves)


def det_tiles(d, **kw):
    t = RowTiles(d['counts'], 'cpu', sub_counts=d['dets'], **kw)
    tile_det = torch.from_numpy(np.repeat(np.arange(d['L']), t.h_sub_ntiles)).int()
    return t, tile_det


@pytest.mark.parametrize('K,N', [(64, 128), (128, 256)])
@pytest.mark.parametrize('with_bias,with_dbias', [(True, True), (True, False), (False, True), (False, False)])
def test_gemm_ares_half_tile_statistics_and_column_sums(K, N, with_bias, with_dbias):
    d = layer(K, N, seed=10)
    tiles, tile_det = det_tiles(d)
    assert 2 * tiles.T == len(d['halves'])
    v = d['a'] @ d['Wq'].t()
    if with_bias:
        v = v + d['bias']
    if with_dbias:
        v = v + d['dbias'][d['row_det']]
    w = torch.relu(v * d['osc'][d['row_grp']] + d['osh'][d['row_grp']])
    part, cs = torch.full((2 * tiles.T, 2, N), 7.0, dtype=F64), torch.full((2 * tiles.T, N), 7.0, dtype=F64)
    emu.gemm_ares(d['W16'], d['osv'], tiles, N, K, d['X'], d['sc'], d['sh'], bias=d['bias'] if with_bias else None,
                  dbias=d['dbias'] if with_dbias else None, tile_dbrow=tile_det if with_dbias else None, part=part,
                  osc=d['osc'], osh=d['osh'], colsum=cs)
    empty = 0
    for i, (r0, n) in enumerate(d['halves']):
        if n == 0:  # the half-tile contract: an empty half gives sum 0, M2 0 and column sum 0
            assert (part[i] == 0).all() and (cs[i] == 0).all(), 'empty half %d' % i
            empty += 1
            continue
        vh = v[r0:r0 + n]
        same(part[i, 0], vh.sum(0), 'sum of half %d' % i)
        same(part[i, 1], torch.var(vh, 0, unbiased=False) * n, 'M2 of half %d' % i, 1e-9)
        same(cs[i], w[r0:r0 + n].sum(0), 'column sum of half %d' % i)
    assert empty >= 3


def group_norm_rows(v, gamma, beta):
    """nn.GroupNorm(N, N) over the rows of one sample: [P][N] -> [P][N]"""
    return F.group_norm(v.t().unsqueeze(0), v.shape[1], gamma, beta, EPS)[0].t()


def test_half_tile_statistics_feed_gn_finalize():
    """part of gemm_ares through gn_finalize over HalfTiles (empty halves among them) is F.group_norm of v"""
    K, N = 64, 128
    d = layer(K, N, seed=20)
    tiles, tile_det = det_tiles(d)
    half = HalfTiles(tiles, 'cpu')
    v = d['a'] @ d['Wq'].t() + d['dbias'][d['row_det']]
    part = torch.zeros(half.T, 2, N, dtype=F64)
    emu.gemm_ares(d['W16'], d['osv'], tiles, N, K, d['X'], d['sc'], d['sh'], dbias=d['dbias'], tile_dbrow=tile_det, part=part)
    gamma, beta = rnd64(N, seed=21).abs() + 0.5, rnd64(N, seed=22)
    s, h = torch.zeros(d['G'], N, dtype=F64), torch.zeros(d['G'], N, dtype=F64)
    emu.gn_finalize(part, half, N, N, gamma, beta, EPS, s, h)
    for g in range(d['G']):
        vg = v[d['row_grp'] == g]
        same(vg * s[g] + h[g], group_norm_rows(vg, gamma, beta), 'group %d' % g, 1e-10)


@pytest.mark.parametrize('K', [64, 128])
def test_gram_rows(K):
    d = layer(K, 128, seed=30)
    tiles, _ = det_tiles(d, tile=200)  # super-tiles of up to 200 rows inside a detection
    Gm, S = torch.zeros(tiles.T, K * K, dtype=F64), torch.zeros(tiles.T, K, dtype=F64)
    emu.gram_rows(d['X'], K, d['sc'], d['sh'], tiles, Gm, S)
    t, r = 0, 0
    for c in d['flat']:
        for t0 in range(0, c, 200):
            a = d['a'][r + t0:r + min(c, t0 + 200)]
            same(Gm[t].view(K, K), torch.einsum('rk,rl->kl', a, a), 'Gram matrix of super-tile %d' % t)
            same(S[t], a.sum(0), 'column sums of super-tile %d' % t)
            t += 1
        r += c
    assert t == tiles.T


@pytest.mark.parametrize('N', [64, 70, 192])
@pytest.mark.parametrize('with_bias', [True, False])
def test_gn_finalize_gram(N, with_bias):
    """scale / shift from the moments of the input are GroupNorm(N, N) of the materialised v (outputs rounded to fp32)"""
    K = 128
    d = layer(K, N, seed=40)
    tiles = RowTiles(d['counts'], 'cpu', tile=100)
    Gm, S = torch.zeros(tiles.T, K * K, dtype=F64), torch.zeros(tiles.T, K, dtype=F64)
    emu.gram_rows(d['X'], K, d['sc'], d['sh'], tiles, Gm, S)
    gamma, beta = rnd64(N, seed=41).abs() + 0.5, rnd64(N, seed=42)
    s, h = torch.zeros(d['G'], N, dtype=F64), torch.zeros(d['G'], N, dtype=F64)
    emu.gn_finalize_gram(Gm, S, tiles, K, d['W'], d['bias'] if with_bias else None, N, gamma, beta, EPS, None, s, h)
    v = d['a'] @ d['W'].t() + (d['bias'] if with_bias else 0.0)
    for g in range(d['G']):
        vg = v[d['row_grp'] == g]
        same(vg * s[g] + h[g], group_norm_rows(vg, gamma, beta), 'group %d' % g, 1e-6)
        same(s[g], gamma / torch.sqrt(torch.var(vg, 0, unbiased=False) + EPS), 'scale of group %d' % g, 1e-6)


@pytest.mark.parametrize('N', [64, 100])
def test_gn_finalize_gram_dbias(N):
    """the same with a gathered per-detection bias whose spread is larger than that of W a"""
    K = 64
    d = layer(K, N, seed=50, far=5.0)
    tiles, tile_det = det_tiles(d, tile=100)
    Gm, S = torch.zeros(tiles.T, K * K, dtype=F64), torch.zeros(tiles.T, K, dtype=F64)
    emu.gram_rows(d['X'], K, d['sc'], d['sh'], tiles, Gm, S)
    gamma, beta = rnd64(N, seed=51).abs() + 0.5, rnd64(N, seed=52)
    s, h = torch.zeros(d['G'], N, dtype=F64), torch.zeros(d['G'], N, dtype=F64)
    emu.gn_finalize_gram_dbias(Gm, S, tiles, tile_det, K, d['W'], d['dbias'], N, gamma, beta, EPS, None, s, h)
    wa = d['a'] @ d['W'].t()
    v = wa + d['dbias'][d['row_det']]
    assert d['dbias'].std(0).median() > 2 * wa.std(0).median()
    for g in range(d['G']):
        vg = v[d['row_grp'] == g]
        same(vg * s[g] + h[g], group_norm_rows(vg, gamma, beta), 'group %d' % g, 1e-6)


@pytest.mark.parametrize('N', [64, 128])
@pytest.mark.parametrize('with_bias', [True, False])
def test_pn_mlp64(N, with_bias):
    d = layer(64, N, seed=60)
    tiles = RowTiles(d['counts'], 'cpu')
    Y, part = torch.zeros(d['R'], N, dtype=F64), torch.zeros(tiles.T, 2, N, dtype=F64)
    emu.pn_mlp64(d['W16'], d['osv'], tiles, N, d['X'], d['sc'], d['sh'], d['bias'] if with_bias else None, Y, part)
    v = d['a'] @ d['Wq'].t() + (d['bias'] if with_bias else 0.0)
    same(Y, v, 'Y')
    t, r = 0, 0
    for c in d['counts']:
        for t0 in range(0, c, 128):
            vt = v[r + t0:r + min(c, t0 + 128)]
            same(part[t, 0], vt.sum(0), 'sum of tile %d' % t)
            same(part[t, 1], torch.var(vt, 0, unbiased=False) * vt.shape[0], 'M2 of tile %d' % t, 1e-9)
            t += 1
        r += c
    assert t == tiles.T


@pytest.mark.parametrize('K', [3, 4])
def test_pointnet_layer1(K):
    counts = [130, 1, 64]
    tiles = RowTiles(counts, 'cpu')
    X = rnd64(sum(counts), K, seed=70) * 10 + 30
    W, b = rnd64(64, K, seed=71), rnd64(64, seed=72)
    Y, part = torch.zeros(sum(counts), 64, dtype=F64), torch.zeros(tiles.T, 2, 64, dtype=F64)
    emu.pointnet_layer1(X, W, b, Y, part, tiles)
    v = F.linear(X, W, b)
    same(Y, v, 'Y')
    bounds = [(0, 128), (128, 130), (130, 131), (131, 195)]
    assert tiles.T == len(bounds)
    for t, (lo, hi) in enumerate(bounds):
        same(part[t, 0], v[lo:hi].sum(0), 'sum of tile %d' % t)
        same(part[t, 1], torch.var(v[lo:hi], 0, unbiased=False) * (hi - lo), 'M2 of tile %d' % t, 1e-8)


def head(C, C4, seed=0):
    r = lambda *s, k: rnd64(*s, seed=seed + k)
    return dict(g0=r(C, k=1).abs() + 0.5, b0=r(C, k=2), w1=r(C4, C, k=3) * C ** -0.5, c1=r(C4, k=4), g2=r(C4, k=5).abs() + 0.5,
                b2=r(C4, k=6), w4=r(128, C4, k=7) * C4 ** -0.5, c4=r(128, k=8), g5=r(128, k=9).abs() + 0.5, b5=r(128, k=10))


@pytest.mark.parametrize('C,C4', [(64, 64), (320, 128)])
def test_skippool_head(C, C4):
    hd, R = head(C, C4, seed=80), 5
    P = rnd64(R + 2, C + 3, seed=81) * 3 + 1
    out = torch.full((R + 2, 130), 9.0, dtype=F64)
    emu.skippool_head(P, C, hd, EPS, out, R)
    x = F.layer_norm(P[:R, :C], (C,), hd['g0'], hd['b0'], EPS)
    x = torch.relu(F.layer_norm(F.linear(x, hd['w1'], hd['c1']), (C4,), hd['g2'], hd['b2'], EPS))
    x = torch.relu(F.layer_norm(F.linear(x, hd['w4'], hd['c4']), (128,), hd['g5'], hd['b5'], EPS))
    same(out[:R, :128], x, 'skippool head')
    assert (out[R:] == 9.0).all() and (out[:, 128:] == 9.0).all()


def test_a_wrong_tile_to_detection_map_is_noticed():
    """the bias row of a tile comes from tile_dbrow / tile_det and from nowhere else: with the map of the neighbouring
    detection the specification is far from the direct statistics - a kernel that read the wrong table entry (the tile's
    own index, the entry of the tile before) cannot agree with it"""
    K, N = 64, 64
    d = layer(K, N, seed=90, far=5.0)
    tiles, tile_det = det_tiles(d)
    v = d['a'] @ d['Wq'].t() + d['dbias'][d['row_det']]
    wrong = (tile_det + 1) % d['L']
    for tab, ok in ((tile_det, True), (wrong, False), (torch.arange(tiles.T).int() % d['L'], False)):
        part = torch.zeros(2 * tiles.T, 2, N, dtype=F64)
        emu.gemm_ares(d['W16'], d['osv'], tiles, N, K, d['X'], d['sc'], d['sh'], dbias=d['dbias'], tile_dbrow=tab, part=part)
        direct = torch.stack([v[r0:r0 + n].sum(0) for r0, n in d['halves']])
        err = (part[:, 0] - direct).abs().max().item() / direct.abs().max().item()
        assert (err < 1e-12) == ok and (ok or err > 1e-2), (ok, err)
    gt, gdet = det_tiles(d, tile=100)
    Gm, S = torch.zeros(gt.T, K * K, dtype=F64), torch.zeros(gt.T, K, dtype=F64)
    emu.gram_rows(d['X'], K, d['sc'], d['sh'], gt, Gm, S)
    gamma, beta = torch.ones(N, dtype=F64), torch.zeros(N, dtype=F64)
    v = d['a'] @ d['W'].t() + d['dbias'][d['row_det']]
    for tab, ok in ((gdet, True), ((gdet + 1) % d['L'], False)):
        s, h = torch.zeros(d['G'], N, dtype=F64), torch.zeros(d['G'], N, dtype=F64)
        emu.gn_finalize_gram_dbias(Gm, S, gt, tab, K, d['W'], d['dbias'], N, gamma, beta, EPS, None, s, h)
        ref = torch.stack([1.0 / torch.sqrt(torch.var(v[d['row_grp'] == g], 0, unbiased=False) + EPS) for g in range(d['G'])])
        err = (s - ref).abs().max().item() / ref.abs().max().item()
        assert (err < 1e-6) == ok and (ok or err > 1e-2), (ok, err)
