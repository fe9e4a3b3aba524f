"""Every launch branch of the head's forward kernels (csrc/gemm_rows.hip, csrc/small_kernels.hip) against the float64
specification in tests/fake_ops.py (TorchOps(torch.float64) on float64 copies of the fp32 inputs; the entries nothing
else pins are pinned by tests/test_forward_spec_cpu.py).

Conventions: those of tests/test_backward_kernels_gpu.py, whose guarded-buffer helpers are used here -
* outputs with a leading dimension are column slices of a NaN buffer with guard rows; outputs without one (part and
  colsum of gemm_rows, sc / sh of gn_finalize, the rowdot, fusion_combine and softmax outputs) lie between NaN guards.
  Where a launch must leave part of the output alone (rowdot with an output map, fusion_combine rows outside the tiles)
  the view starts from a sentinel value and those elements must still hold it;
* inputs with a leading dimension are column slices of NaN buffers: a read beside the operand poisons the result;
* every launch runs twice on fresh buffers, the two results are equal bit for bit, nothing around them changes;
* no element is excluded from a comparison.  The rowdot threshold is put into a gap of the float64 scores so that every
  row is at least 1e-4 away from it (asserted on the CPU before the launch).

Tolerances, as a fraction of the reference's maximum (test_kernels_gpu.close): those of tests/test_kernels_gpu.py where
the reduction is no longer than there - gemm Y 3e-6, tile sums and column sums (a sum over the <= 128 rows of a tile,
like the tile sums) 1e-5, tile M2 1e-4, segment_mean 2e-6, rowdot 2e-6 (K <= 512), row_layernorm 3e-6 (C <= 512),
affine_act 1e-6, fusion_combine 3e-6, gn_finalize 1e-6 (groups of <= 3 tiles).  Beyond that range no number is fixed in
advance: the same specification evaluated in torch float32 on the host is the yardstick, and the device may be at most 4
times as far from float64 as that evaluation is, relative to the largest output (the convention of
test_pointnet_dropout_gpu.py::test_segment_mean_dropout_masked; 4 allows for another summation order).  Should the host
evaluation be exact, the kernel's existing tolerance holds.

Measured on an MI355X (device error / host-fp32 error, relative to the largest output, worst over the cases of a test):
  rowdot K = 1028 (10 cases)                         device 7.1e-8 .. 1.1e-7    host 1.6e-7 .. 2.4e-7
  gn_finalize, groups of 63 / 257 / 700 tiles        device 2.3e-8 .. 5.1e-8    host 3.5e-8 .. 2.9e-7
      per-channel kernel, 700 tiles around a mean of 100: 2.8e-8 .. 4.3e-8 - that of the general kernel on the same
      statistics (2.3e-8 .. 5.1e-8), so (Q - S mean) / n in fp64 costs nothing measurable and the kernel stays as it is
  row_layernorm C = 1024                             device 1.1e-7 .. 1.5e-7    host 1.3e-7 .. 1.9e-7
  softmax_pairs, logits 200 +- 60, modes 1 .. 4      device 1.0e-7 .. 2.7e-7    host the same figures
In none of these cases is the device further from float64 than the host evaluation.

Empty segments (count 0) are not tested: no plan produces one (every frame has a detection, every detection a point, every
pooling chunk a row - mmmot_amd/plan.py raises otherwise), and include/mmmot_hip.h says so for mmmot_segment_mean."""
import functools

import numpy as np
import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd.pack import from_hl16, hl16_weight_shift, to_hl16
from mmmot_amd.plan import HalfTiles, RowTiles, Segments
from test_backward_kernels_gpu import DEV, flat, put, slab, twice
from test_forward_spec_cpu import far_logits
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu
F64 = torch.float64
emu = TorchOps(F64)


def both(counts, **kw):
    return RowTiles(counts, 'cpu', **kw), RowTiles(counts, DEV, **kw)


def dbl(*ts):
    return [None if t is None else t.double() for t in ts]


def einval(fn, *a, **kw):
    """the launcher returns MMMOT_EINVAL (the operator layer raises on a status, naming it)"""
    with pytest.raises(RuntimeError, match=r'status -1 \(MMMOT_EINVAL'):
        fn(*a, **kw)


def yardstick(what, got, ref, host32, fallback):
    """the device at most 4 x as far from the float64 reference as the host's float32 evaluation of the same specification,
    relative to the largest output; `fallback`: the kernel's existing tolerance, if the host evaluation is exact"""
    got, ref = got.detach().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), '%s: non-finite values' % what
    top = max(ref.abs().max().item(), 1e-6)
    dev_err = (got - ref).abs().max().item() / top
    host_err = (host32.double() - ref).abs().max().item() / top
    print('%s: device error %.3e, host fp32 error %.3e (relative to the largest output)' % (what, dev_err, host_err))
    if host_err == 0.0:
        close(got, ref, fallback, what)
    else:
        assert dev_err <= 4.0 * host_err, '%s: device error %.3e, host fp32 error %.3e' % (what, dev_err, host_err)


def sentinel(value, *shape):
    """make() of `twice`: a flat guarded output that starts from `value` (elements the launch must leave alone)"""
    def make():
        buf, v = flat(*shape)
        v.fill_(value)
        return [(buf, v)]
    return make


# ---- gemm_rows --------------------------------------------------------------------------------------------------------
@pytest.fixture
def tile_kernel(hip):
    """pins mmmot_gemm_rows to the tile kernel (the wide kernel of csrc/gemm_wide.hip has a pass of its own, tests/test_wide_kernels_gpu.py)"""
    assert hip.lib.mmmot_set_gemm_rows_variant(1) == 0
    yield
    assert hip.lib.mmmot_set_gemm_rows_variant(0) == 0


# one row, one row short of a tile, one row more than a tile (a last tile of one row), four groups
GEMM_COUNTS = [[1], [127], [129], [5, 300, 128, 1]]
PAIR_NM = {1: (1, 1), 5: (1, 5), 127: (127, 1), 128: (4, 32), 129: (43, 3), 300: (20, 15)}  # rows of a group = N x M


def check_part(P, ref, what):
    close(P[:, 0], ref[:, 0], 1e-5, what + ' tile sums')
    close(P[:, 1], ref[:, 1], 1e-4, what + ' tile M2')


def check_gemm(hip, what, counts, N, K, amode, pairop, f16, seed):
    """Y alone; part alone (Y = NULL); Y + part + sigmoid; dbias + rowidx with ReLU and part; colsum with osc / osh"""
    tc, tg = both(counts)
    R, T, G = tc.R, tc.T, tc.G
    W = rnd(N, K, seed=seed, scale=K ** -0.5)
    bias = rnd(N, seed=seed + 1, scale=0.2)
    dbias = rnd(7, N, seed=seed + 2)
    rowidx = ((torch.arange(R) * 5 + 3) % 7).int()
    osc, osh = rnd(G, N, seed=seed + 3).abs() + 0.5, rnd(G, N, seed=seed + 4) * 0.5
    if amode == 2:
        NM = [PAIR_NM[c] for c in counts]
        aoff, boff, o = [], [], 1
        for n, m in NM:
            aoff.append(o)
            boff.append(o + n)
            o += n + m
        F = rnd(o + 2, K, seed=seed + 5)
        tab = lambda t, dev: dict(row0=t.g_row0, M=torch.tensor([m for _, m in NM], dtype=torch.int32, device=dev),
                                  aoff=torch.tensor(aoff, dtype=torch.int32, device=dev),
                                  boff=torch.tensor(boff, dtype=torch.int32, device=dev))
        Fg = put(F)
        assert Fg.stride(0) > K
        kw_c = dict(FA=F.double(), FB=F.double(), pair=tab(tc, 'cpu'), amode=2, pairop=pairop)
        kw_g = dict(FA=Fg, FB=Fg, pair=tab(tg, DEV), amode=2, pairop=pairop)
    else:
        X = rnd(R, K, seed=seed + 5) + (3.0 if amode == 0 else 0.0)  # non-zero mean: the tile-centred second moment
        kw_c, kw_g = dict(X=X.double()), dict(X=put(X))
        if amode == 1:
            sc, sh = rnd(G, K, seed=seed + 6).abs() + 0.5, rnd(G, K, seed=seed + 7)
            kw_c.update(sc=sc.double(), sh=sh.double(), amode=1)
            kw_g.update(sc=put(sc), sh=put(sh), amode=1)
    if f16:
        shift = hl16_weight_shift(W)
        W16 = to_hl16(W.double() * 2.0 ** shift)
        Wc, Wg = W16, W16.to(DEV)
        kw_c.update(w_hl16=True, oscale=2.0 ** -shift)
        kw_g.update(w_hl16=True, oscale=2.0 ** -shift)
    else:
        Wc, Wg = W.double(), W.to(DEV)

    def spec(**extra):
        Y, part = torch.zeros(R, N, dtype=F64), torch.zeros(T, 2, N, dtype=F64)
        cs = torch.zeros(T, N, dtype=F64)
        emu.gemm(Wc, tc, N, K, bias=bias.double(), Y=Y, part=part, osc=osc.double(), osh=osh.double(), colsum=cs,
                 **extra, **kw_c)
        return Y, part, cs
    v0, p0, c0 = spec()
    v1, p1, _ = spec(dbias=dbias.double(), rowidx=rowidx)
    kw_g.update(bias=put(bias))
    gemm = lambda **kw: hip.gemm(Wg, tg, N, K, **kw, **kw_g)
    (Y,) = twice(what + ' Y', lambda: [slab(R, N)], lambda Y: gemm(Y=Y))
    close(Y, v0, 3e-6, what + ' Y alone')
    (P0,) = twice(what + ' part', lambda: [flat(T, 2, N)], lambda P: gemm(part=P))
    check_part(P0, p0, what + ' part alone:')
    Y, P = twice(what + ' Y part act', lambda: [slab(R, N), flat(T, 2, N)], lambda Y, P: gemm(Y=Y, part=P, act=2))
    close(Y, torch.sigmoid(v0), 3e-6, what + ' sigmoid(Y) with part')
    assert torch.equal(P, P0), what + ': the statistics depend on whether Y is stored'
    dbg, rig = put(dbias), rowidx.to(DEV)
    Y, P = twice(what + ' dbias', lambda: [slab(R, N), flat(T, 2, N)],
                 lambda Y, P: gemm(Y=Y, part=P, act=1, dbias=dbg, rowidx=rig))
    close(Y, torch.relu(v1), 3e-6, what + ' relu(Y) with dbias and part')
    check_part(P, p1, what + ' dbias + act + part:')
    oscg, oshg = put(osc), put(osh)
    (CS,) = twice(what + ' colsum', lambda: [flat(T, N)], lambda CS: gemm(colsum=CS, osc=oscg, osh=oshg))
    close(CS, c0, 1e-5, what + ' column sums')


@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16x3'])
@pytest.mark.parametrize('amode', [0, 1, 2], ids=['plain', 'norm_relu', 'pair'])
@pytest.mark.parametrize('BN', [64, 128], ids=['BN64', 'BN128'])
def test_gemm_rows_every_instantiation(hip, tile_kernel, BN, amode, f16):
    """gemm_rows_kernel<BN, AMODE, F16>, all twelve: BN = 64 at N = 64 / 192 (N % 128 != 0; WM = 4 in the colsum reduction,
    the per-lane stores of the narrow f16 instantiation with an activation), BN = 128 at N = 128 / 384; one K stage (fp32
    K = 32, f16 K = 64: no prefetch), an odd number of stages (fp32 K = 96 / 160, f16 K = 192); PAIR with each pairop on
    the four-group tiling (and in turn on the others); every operand a strided slice"""
    bk = 64 if f16 else 32
    for N in ((64, 192) if BN == 64 else (128, 384)):
        for ki, K in enumerate((64, 192) if f16 else (32, 96, 160)):
            assert K % bk == 0 and ((K // bk) % 2 == 1)
            for ci, counts in enumerate(GEMM_COUNTS):
                ops = (0,) if amode != 2 else (0, 1, 2) if len(counts) == 4 and ki == 0 else ((ci + ki) % 3,)
                for pairop in ops:
                    check_gemm(hip, 'gemm <%d, %d, %s> N %d K %d %s op %d' % (BN, amode, f16, N, K, counts, pairop), counts,
                               N, K, amode, pairop, f16, seed=1000 + 10 * ci)


# ---- segment_mean -----------------------------------------------------------------------------------------------------
# 12 / 13 / 16 / 17: either side of `t + 12 < count`, where a wave leaves the 16-row unrolled loop; 1 .. 3: waves without a row
SEG_COUNTS = [1, 2, 3, 4, 5, 12, 13, 16, 17, 63, 65, 257]


def seg_tables(div):
    """the ragged segments, then one strided segment (50 rows, every third); alternating groups; -> (cpu, device, rows)"""
    start = np.concatenate([[0], np.cumsum(SEG_COUNTS)]).astype(np.int64)
    count, stride = np.array(SEG_COUNTS + [50]), np.array([1] * len(SEG_COUNTS) + [3])
    n = len(count)
    dv = None if div is None else np.full(n, div)
    mk = lambda dev: Segments(start, count, stride, np.arange(n) % 2, dev, div=dv)
    return mk('cpu'), mk(DEV), int(start[-1]) + 49 * 3 + 1


def put_hl16(x16):
    """hl16 rows (fp16 halves in fp32-typed storage) as a strided slice, bit for bit; ld % 8 == 0 as the format needs"""
    buf, v = slab(x16.shape[0], x16.shape[1], off=8, extra=8)
    v.view(torch.int32).copy_(x16.view(torch.int32))
    return v


@pytest.mark.parametrize('hl16,C', [(False, 4), (False, 132), (False, 516), (True, 64), (True, 384), (True, 512)],
                         ids=['f32-C4', 'f32-C132', 'f32-C516', 'hl16-C64', 'hl16-C384', 'hl16-C512'])
def test_segment_mean_and_max(hip, hl16, C):
    """mean and maximum (flag bit 2) x with / without sc, sh x with / without ReLU x with / without seg_div (which must not
    enter a maximum), and the maximum of all-negative rows (the accumulators start at -3.0e38; waves without a row of a
    short segment contribute that).  C = 4 / 132 / 516: a last 256-channel block with idle lanes; hl16 rows with a
    prologue, with the maximum, or with C = 64 / 384 take the general kernel, hl16 C = 512 without one the unit-per-lane
    kernel"""
    _, _, R = seg_tables(None)
    n = len(SEG_COUNTS) + 1
    X, neg = rnd(R, C, seed=300) * 2 + 0.5, -rnd(R, C, seed=301).abs() * 2 - 0.5
    sc, sh = rnd(2, C, seed=302), rnd(2, C, seed=303)
    scg, shg = put(sc), put(sh)

    def operand(x):
        if not hl16:
            return x.double(), put(x)
        x16 = to_hl16(x)
        return from_hl16(x16).double(), put_hl16(x16)
    (Xc, Xg), (negc, negg) = operand(X), operand(neg)
    assert (negc < 0).all()
    for take_max in (False, True):
        for norm in (False, True):
            for relu in (False, True):
                for div in (None, 7):
                    sg_c, sg_g, _ = seg_tables(div)
                    what = 'segment_%s hl16=%s C=%d norm=%s relu=%s div=%s' % ('max' if take_max else 'mean', hl16, C, norm, relu, div)
                    ref = torch.zeros(n, C, dtype=F64)
                    emu.segment_mean(Xc, C, sg_c, ref, sc=sc.double() if norm else None, sh=sh.double() if norm else None,
                                     relu=relu, take_max=take_max)
                    (out,) = twice(what, lambda: [slab(n, C)], lambda o: hip.segment_mean(
                        Xg, C, sg_g, o, sc=scg if norm else None, sh=shg if norm else None, relu=relu, hl16=hl16,
                        take_max=take_max))
                    close(out, ref, 2e-6, what)
    sg_c, sg_g, _ = seg_tables(None)
    ref = torch.zeros(n, C, dtype=F64)
    emu.segment_mean(negc, C, sg_c, ref, take_max=True)
    assert (ref < 0).all()
    (out,) = twice('maximum of negative rows', lambda: [slab(n, C)],
                   lambda o: hip.segment_mean(negg, C, sg_g, o, hl16=hl16, take_max=True))
    close(out, ref, 2e-6, 'segment maximum of all-negative rows')
    assert (out < 0).all()


# ---- rowdot -----------------------------------------------------------------------------------------------------------
def gap_threshold(s):
    """a threshold in the widest gap between the middle half of the scores: every score at least 1e-4 away (asserted)"""
    v = s.sort()[0]
    lo, hi = len(v) // 4, 3 * len(v) // 4
    i = lo + int((v[lo + 1:hi + 1] - v[lo:hi]).argmax())
    thr = float((v[i] + v[i + 1]) / 2)
    assert (s - thr).abs().min().item() >= 1e-4 and (s < thr).any() and (s >= thr).any()
    return thr


@pytest.mark.parametrize('K', [4, 64, 100, 128, 132, 384, 1028])
def test_rowdot(hip, K):
    """K <= 128: two rows per wave (K = 4 / 64 / 100: dead lanes in the half wave; tiles of 3, 73 and 1 rows: an upper half
    wave without a row), K = 132 / 384 / 1028: the general loop with a partly filled last trip; each activation with and
    without the normalisation table, the threshold, the output map"""
    tc, tg = both([3, 201, 1])
    assert tc.h_nrows.tolist() == [3, 128, 73, 1]
    R, b = tc.R, 0.3
    X, w = rnd(R, K, seed=400), rnd(K, seed=401, scale=K ** -0.5)
    sc, sh = rnd(3, K, seed=402), rnd(3, K, seed=403)
    Xg, wg, scg, shg = put(X), put(w), put(sc), put(sh)

    def judge(what, out, ref, host):
        if K <= 512:
            close(out, ref, 2e-6, what)
        else:
            yardstick(what, out, ref, host, 2e-6)

    def spec(dtype, n_out, fill, norm, **kw):
        out = torch.full((n_out,), fill, dtype=dtype)
        t = lambda v: v.to(dtype)
        emu.rowdot(t(X), K, t(w), b, tc, out, sc=t(sc) if norm else None, sh=t(sh) if norm else None, **kw)
        return out
    for norm in (False, True):
        tab = dict(sc=scg, sh=shg) if norm else {}
        for act in (0, 1, 2):
            what = 'rowdot K=%d norm=%s act=%d' % (K, norm, act)
            (out,) = twice(what, lambda: [flat(R)], lambda o: hip.rowdot(Xg, K, wg, b, tg, o, act=act, **tab))
            judge(what, out, spec(F64, R, 0.0, norm, act=act), spec(torch.float32, R, 0.0, norm, act=act))
        what = 'rowdot K=%d norm=%s threshold' % (K, norm)
        thr = gap_threshold(spec(F64, R, 0.0, norm, act=2))
        (out,) = twice(what, lambda: [flat(R)],
                       lambda o: hip.rowdot(Xg, K, wg, b, tg, o, act=2, use_thr=True, thr=thr, **tab))
        ref = spec(F64, R, 0.0, norm, act=2, use_thr=True, thr=thr)
        assert (ref < 0).any() and (ref > 0).any()
        judge(what, out, ref, spec(torch.float32, R, 0.0, norm, act=2, use_thr=True, thr=thr))
        what = 'rowdot K=%d norm=%s output map' % (K, norm)
        omap = torch.randperm(R + 10, generator=torch.Generator().manual_seed(404))[:R].int()
        omg = omap.to(DEV)
        (out,) = twice(what, sentinel(-0.75, R + 10), lambda o: hip.rowdot(Xg, K, wg, b, tg, o, act=2, omap=omg, **tab))
        ref = spec(F64, R + 10, -0.75, norm, act=2, omap=omap)
        assert int((ref == -0.75).sum()) == 10  # (a sigmoid is positive: no score can equal the sentinel)
        assert torch.equal(out.cpu() == -0.75, ref == -0.75), what + ': an element outside the map was written'
        judge(what, out, ref, spec(torch.float32, R + 10, -0.75, norm, act=2, omap=omap))


# ---- gn_finalize ------------------------------------------------------------------------------------------------------
GN_NT = [1, 63, 257, 700]  # tiles per group


def ragged_subs(nt):
    """detection sizes that tile into exactly nt tiles, partial tiles in the middle of the group"""
    subs, t, k = [], 0, 0
    while t < nt:
        s = (1, 129, 64, 128, 300, 5)[k % 6]
        k += 1
        if t + -(-s // 128) > nt:
            s = 7
        subs.append(s)
        t += -(-s // 128)
    return subs


@functools.lru_cache(maxsize=None)
def gn_tables(kind):
    """'plain': consecutive 128-row tiles, tile_nrows NULL; 'ragged': detection-aligned tiles, tile_nrows passed; 'half': the
    64-row halves of the ragged tiles, empty ones among them"""
    if kind == 'plain':
        tc, tg = both([100, 63 * 128 - 5, 257 * 128 - 127, 700 * 128 - 60])
        assert not tg.ragged
    else:
        subs = [ragged_subs(nt) for nt in GN_NT]
        tc, tg = both([sum(s) for s in subs], sub_counts=subs)
        assert tg.ragged and (tc.h_nrows[:-1] < 128).sum() > 100
    assert tc.h_g_ntiles.tolist() == GN_NT
    if kind == 'half':
        tc, tg = HalfTiles(tc, 'cpu'), HalfTiles(tc, DEV)
        assert tc.h_g_ntiles.tolist() == [2 * nt for nt in GN_NT] and (tc.h_nrows == 0).sum() > 100
        assert (tc.h_nrows[1:-1][tc.h_nrows[1:-1] == 0]).size > 0  # empty halves in the middle of a list
    return tc, tg


def gn_spec(part, tiles, C, NG, gamma, beta, eps, dtype):
    """TorchOps.gn_finalize with the arithmetic in `dtype` (that entry always works in float64)"""
    CG = C // NG
    sc, sh = torch.zeros(tiles.G, C, dtype=dtype), torch.zeros(tiles.G, C, dtype=dtype)
    for g in range(tiles.G):
        t0, nt, cnt = int(tiles.h_g_tile0[g]), int(tiles.h_g_ntiles[g]), int(tiles.h_g_count[g])
        p = part[t0:t0 + nt, :, :C].to(dtype)
        n_t = torch.as_tensor(tiles.h_nrows[t0:t0 + nt]).to(dtype).view(nt, 1)
        s1 = p[:, 0].sum(0).view(NG, CG).sum(1) / (cnt * CG)
        dev = torch.where(n_t > 0, p[:, 0] / n_t.clamp(min=1) - s1.repeat_interleave(CG), torch.zeros_like(p[:, 0]))
        m2 = (p[:, 1] + n_t * dev * dev).sum(0).view(NG, CG).sum(1)
        rstd = 1.0 / torch.sqrt(m2 / (cnt * CG) + eps)
        scv = gamma.to(dtype) * rstd.repeat_interleave(CG)
        sc[g], sh[g] = scv, beta.to(dtype) - s1.repeat_interleave(CG) * scv
    return sc, sh


GN_CASES = [(C, NG, kind) for C, NG in [(96, 2), (12, 4), (24, 24), (512, 1), (64, 64), (1024, 1024)]
            for kind in ('plain', 'ragged') + (('half',) if NG == C and C % 16 == 0 else ())]


@pytest.mark.parametrize('C,NG,kind', GN_CASES, ids=['C%d-NG%d-%s' % c for c in GN_CASES])
def test_gn_finalize_long_tile_lists(hip, C, NG, kind):
    """groups of 1, 63, 257 and 700 tiles.  General kernel: CG = 48 and 3 (the incremental (tile, channel) walk with a CG that
    does not divide 256), (24, 24): NG == C with C % 16 != 0 (CG = 1), (512, 1): CG > 256 and nt * CG > 4096 (further trips
    of the 16-element loop).  Per-channel kernel (64, 64), (1024, 1024): nt > 256 (a second ti += 256 trip), nt % 64 != 0
    (the clamp of the look-ahead loads), tile_nrows NULL / given / half tiles with empty entries.  Synthetic statistics as
    in test_gn_finalize (tile means spread by 3, a tiny within-tile M2), once around 0 and once around a common mean of
    100 - the per-channel kernel's (Q - S mean) / n cancels there.  The one-tile group keeps the 1e-6 of test_gn_finalize;
    the long groups are judged by the host-fp32 yardstick."""
    tc, tg = gn_tables(kind)
    T, G = tc.T, tc.G
    n_t = torch.as_tensor(tc.h_nrows).double().view(-1, 1)
    gamma, beta = rnd(C, seed=501).abs() + 0.5, rnd(C, seed=502)
    gg, bg = put(gamma), put(beta)
    for off in (0.0, 100.0):
        what = 'gn_finalize C=%d NG=%d %s tiles, mean %g' % (C, NG, kind, off)
        g = torch.Generator().manual_seed(500)
        part = torch.zeros(T, 2, C)
        part[:, 0] = ((torch.randn(T, C, generator=g, dtype=F64) * 3 + off) * n_t).float()
        part[:, 1] = (torch.rand(T, C, generator=g, dtype=F64) * n_t * 0.01).float()
        pbuf = torch.full((T + 2, 2, C + 12), float('nan'), device=DEV)  # a guard tile either side, ldp > C
        pg = pbuf[1:T + 1, :, 4:4 + C]
        pg.copy_(part)
        sc, sh = torch.zeros(G, C, dtype=F64), torch.zeros(G, C, dtype=F64)
        emu.gn_finalize(part, tc, C, NG, gamma, beta, 1e-5, sc, sh)
        s64, h64 = gn_spec(part, tc, C, NG, gamma, beta, 1e-5, F64)
        assert torch.equal(s64, sc) and torch.equal(h64, sh)
        s32, h32 = gn_spec(part, tc, C, NG, gamma, beta, 1e-5, torch.float32)
        scg, shg = twice(what, lambda: [flat(G, C), flat(G, C)],
                         lambda s, h: hip.gn_finalize(pg, tg, C, NG, gg, bg, 1e-5, s, h))
        close(scg[:1], sc[:1], 1e-6, what + ': scale of the short group')
        close(shg[:1], sh[:1], 1e-6, what + ': shift of the short group')
        yardstick(what + ': scale of the long groups', scg[1:], sc[1:], s32[1:], 1e-6)
        yardstick(what + ': shift of the long groups', shg[1:], sh[1:], h32[1:], 1e-6)


# ---- row_layernorm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [64, 192, 1024])
def test_row_layernorm(hip, C):
    """1, 3 and 16 values per lane; with and without ReLU; R = 1, a multiple of 4 and not (the last workgroup partly idle);
    strided input and output.  C = 1024 is longer than the rows of test_kernels_gpu.py: the host-fp32 yardstick"""
    gamma, beta = rnd(C, seed=601), rnd(C, seed=602)
    gg, bg = put(gamma), put(beta)
    for R in (1, 8, 37):
        X = rnd(R, C, seed=600) * 3 + 5
        Xg = put(X)
        for relu in (0, 1):
            what = 'row_layernorm C=%d R=%d relu=%d' % (C, R, relu)
            ref = torch.zeros(R, C, dtype=F64)
            emu.row_layernorm(X.double(), C, gamma.double(), beta.double(), 1e-5, relu, ref, R)
            (Y,) = twice(what, lambda: [slab(R, C)], lambda Y: hip.row_layernorm(Xg, C, gg, bg, 1e-5, relu, Y, R))
            if C <= 512:
                close(Y, ref, 3e-6, what)
            else:
                host = torch.zeros(R, C)
                emu.row_layernorm(X, C, gamma, beta, 1e-5, relu, host, R)
                yardstick(what, Y, ref, host, 3e-6)
            assert relu == 0 or (Y >= 0).all()
            assert relu == 1 or (Y < 0).any()


# ---- affine_act -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts', [[1, 130], [1] * 256], ids=['T3', 'T256'])
@pytest.mark.parametrize('C', [4, 132])
def test_affine_act(hip, C, counts):
    """T < 256: eight workgroups share a tile; T >= 256: gridDim.y = 1 (256 one-row tiles); each activation; C = 4: one
    f32x4 per row"""
    tc, tg = both(counts)
    R, G = tc.R, tc.G
    X, sc, sh = rnd(R, C, seed=700), rnd(G, C, seed=701), rnd(G, C, seed=702)
    Xg, scg, shg = put(X), put(sc), put(sh)
    for act in (0, 1, 2):
        what = 'affine_act C=%d T=%d act=%d' % (C, tc.T, act)
        ref = torch.zeros(R, C, dtype=F64)
        emu.affine_act(X.double(), C, sc.double(), sh.double(), tc, act, ref)
        (Y,) = twice(what, lambda: [slab(R, C)], lambda Y: hip.affine_act(Xg, C, scg, shg, tg, act, Y))
        close(Y, ref, 1e-6, what)


# ---- fusion_combine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('C', [4, 132])
def test_fusion_combine(hip, C, mode):
    """a one-row tile, C = 4, and Lt five rows larger than the tiles cover: those rows keep what they held in all three planes
    (the ends of the image and LiDAR planes lie in the middle of F)"""
    tc, tg = both([1, 140])
    R, G = tc.R, tc.G
    Lt, N = R + 5, (2 * C if mode == 2 else C)
    cat = rnd(Lt, 2 * C, seed=800)
    Y0, Y1 = rnd(Lt, N, seed=801), rnd(Lt, N, seed=802)
    s0, h0, s1, h1 = (rnd(G, C, seed=803 + i) for i in range(4))
    ref = torch.zeros(3, R, C, dtype=F64)
    emu.fusion_combine(mode, *dbl(cat[:R], Y0[:R], Y1[:R] if mode else None, s0, h0, s1 if mode else None,
                                  h1 if mode else None), tc, ref, R, C)
    catg, Y0g, Y1g = cat.to(DEV), put(Y0), put(Y1)
    s0g, h0g, s1g, h1g = put(s0), put(h0), put(s1), put(h1)
    what = 'fusion_combine mode %d C=%d' % (mode, C)
    (F,) = twice(what, sentinel(-7.0, 3, Lt, C), lambda F: hip.fusion_combine(
        mode, catg, Y0g, Y1g if mode else None, s0g, h0g, s1g if mode else None, h1g if mode else None, tg, F, Lt, C))
    assert (F[:, R:] == -7.0).all(), what + ': rows outside the tiles were written'
    close(F[:, :R], ref, 3e-6, what)


# ---- softmax_pairs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_softmax_pairs_far_logits(hip, mode):
    """logits at +200 spread over +-60: exp() of a logit overflows, so a kernel that forgot a row or column maximum fails;
    (3, 300): M > 256, a second trip of the column loop; launched with max_nm = 8192, the largest the 64 KB of LDS take
    (mode 1: with the groups' own maximum)"""
    NM = [(5, 7), (1, 1), (1, 9), (3, 300), (130, 70), (64, 1)]
    row0 = np.concatenate([[0], np.cumsum([n * m for n, m in NM])]).astype(np.int32)
    R, G = int(row0[-1]), len(NM)
    x = far_logits(NM, seed=900)
    r0 = torch.tensor(row0[:-1])
    gN, gM = torch.tensor([n for n, _ in NM], dtype=torch.int32), torch.tensor([m for _, m in NM], dtype=torch.int32)
    max_nm = 303 if mode == 1 else 8192
    ref, host = torch.zeros(R, dtype=F64), torch.zeros(R)
    emu.softmax_pairs(x.double(), ref, r0, gN, gM, G, max_nm, mode)
    emu.softmax_pairs(x, host, r0, gN, gM, G, max_nm, mode)
    assert torch.isfinite(ref).all() and torch.isfinite(host).all()
    xg, r0g, gNg, gMg = put(x), r0.to(DEV), gN.to(DEV), gM.to(DEV)
    (out,) = twice('softmax mode %d' % mode, lambda: [flat(R)],
                   lambda o: hip.softmax_pairs(xg, o, r0g, gNg, gMg, G, max_nm, mode))
    yardstick('softmax_pairs mode %d, logits 200 +- 60' % mode, out, ref, host, 3e-6)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_launchers_refuse_what_the_forward_kernels_cannot_take(hip):
    """each launcher first takes a small valid call, then - over outputs filled with 5 - the same call with ONE argument it
    must refuse: MMMOT_EINVAL, and after a synchronise nothing was written"""
    lib, s = hip.lib, torch.cuda.current_stream().cuda_stream
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    t = RowTiles([5], DEV)
    X, W, Wbig = z(16, 1088), z(256, 256), z(256, 256)
    vec, tab = z(1088), z(2, 1088)
    rowidx = torch.zeros(16, dtype=torch.int32, device=DEV)
    Y, Yodd, part, colsum = z(16, 256), z(16, 258), z(1, 2, 64), z(1, 64)
    out, F = z(16, 1088), z(3, 16, 64)
    sg = Segments([0], [5], [1], [0], DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    outputs = [Y, Yodd, part, colsum, out, F]

    def seg(C=8, relu=0, hl16=0):
        return lib.mmmot_segment_mean(X.data_ptr(), 1088, C, sg.start.data_ptr(), sg.count.data_ptr(), sg.stride.data_ptr(),
                                      None, None, 1, None, None, 0, relu, out.data_ptr(), 1088, hl16, s)
    valid = [
        lambda: hip.gemm(W, t, 64, 64, X=X[:, :64], Y=Y[:, :64], part=part, bias=vec[:64]),
        lambda: hip.gemm(W, t, 64, 64, X=X[:, :64], Y=Y[:, :64], w_hl16=True, dbias=tab[:, :64], rowidx=rowidx,
                         colsum=colsum, osc=tab[:, :64], osh=tab[:, :64]),
        lambda: hip.row_layernorm(X[:, :64], 64, vec, vec, 1e-5, 1, out[:, :64], 5),
        lambda: hip.row_layernorm(X[:, :1024], 1024, vec, vec, 1e-5, 1, out[:, :1024], 5),
        lambda: hip.softmax_pairs(X[0], out[0], zero, one, one, 1, 8192, 1),
        lambda: hip.fusion_combine(1, X[:, :128].contiguous(), Y[:, :64], Y[:, 64:128], tab[:, :64], tab[:, :64], tab[:, :64],
                                   tab[:, :64], t, F, 16, 64),
        lambda: hip.affine_act(X[:, :8], 8, tab[:, :8], tab[:, :8], t, 1, out[:, :8]),
    ]
    for call in valid:
        call()
    assert seg() == 0 and seg(relu=3) == 0 and seg(hl16=1) == 0
    torch.cuda.synchronize()
    for o in outputs:
        o.fill_(5.0)
    g = lambda N, K, **kw: einval(hip.gemm, Wbig, t, N, K, **kw)
    g(96, 64, X=X[:, :64], Y=Y[:, :96])                                                     # N % 64
    g(64, 48, X=X[:, :48], Y=Y[:, :64])                                                     # K % 32
    g(64, 96, X=X[:, :96], Y=Y[:, :64], w_hl16=True)                                        # K % 64 under w_hl16 (96 % 32 == 0)
    g(64, 64, X=X[:, :64], Y=Y[:, :64], dbias=tab[:, :64])                                  # dbias without rowidx
    g(64, 64, X=X[:, :64], colsum=colsum)                              # colsum without osc / osh
    g(64, 64, X=X[:, :64], Y=Y[:, 1:65], w_hl16=True)                                       # Y not 16-byte aligned under w_hl16
    g(64, 64, X=X[:, :64], Y=Yodd[:, :64], w_hl16=True)                                     # ldy % 4 under w_hl16
    g(64, 64, X=X[:, 1:65], Y=Y[:, :64])                                                    # X not 16-byte aligned
    assert seg(relu=4) == -1 and seg(hl16=3) == -1 and seg(C=12, hl16=1) == -1 and seg(C=6) == -1
    einval(hip.row_layernorm, X[:, :96], 96, vec, vec, 1e-5, 1, out[:, :96], 5)             # C % 64
    einval(hip.row_layernorm, X[:, :1088], 1088, vec, vec, 1e-5, 1, out[:, :1088], 5)       # C > 1024
    einval(hip.softmax_pairs, X[0], out[0], zero, one, one, 1, 8193, 1)                     # 2 * 8193 floats of LDS > 64 KB
    einval(hip.softmax_pairs, X[0], out[0], zero, one, one, 1, 8192, 0)                     # mode 0
    einval(hip.fusion_combine, 1, X[:, :128].contiguous(), Y[:, :64], None, tab[:, :64], tab[:, :64], tab[:, :64], tab[:, :64],
           t, F, 16, 64)                                                                    # mode B without Y1
    einval(hip.affine_act, X[:, :8], 8, tab[:, 1:9], tab[:, :8], t, 1, out[:, :8])          # sc not 16-byte aligned
    einval(hip.rowdot, X[:, :6], 6, vec, 0.0, t, out[0])                                    # K % 4
    torch.cuda.synchronize()
    for o in outputs:
        assert (o == 5.0).all(), 'a refused call wrote to an output'
