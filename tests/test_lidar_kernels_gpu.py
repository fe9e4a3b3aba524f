"""Every launch branch of the LiDAR encoder's forward kernels (csrc/gemm_ares.hip, gemm_wres.hip, gemm_wreg.hip, pn_mlp64.hip,
gram.hip; pointnet_layer1 and skippool_head of csrc/small_kernels.hip) against the float64 specification in
tests/fake_ops.py (TorchOps(torch.float64) on float64 copies of the fp32 inputs; tests/test_lidar_spec_cpu.py pins those
entries against torch.var / F.group_norm / F.layer_norm of the materialised product).

Conventions: those of tests/test_backward_kernels_gpu.py and tests/test_forward_kernels_gpu.py, whose helpers are used -
* every operand with a leading dimension (X, sc / sh, osc / osh, dbias, P, Y, out) is a column slice of a NaN buffer (row
  stride > row length): a read beside the operand poisons the result;
* every output lies between NaN guards (outputs without a leading dimension: part, colsum, Gout, Sout, sc, sh) or is a
  guarded column slice; where the contract says "not touched" (the blocks of Gout below the block diagonal at K = 128)
  the view starts from a sentinel and must still hold it;
* every launch runs twice on fresh buffers, the two results are bit-equal, nothing around them changes;
* no element is excluded from a comparison;
* the normalised activations relu(X * sc + sh) stay below 100, far from the kernels' clamp at 65 000 (asserted on the CPU
  in Layer and in the pn_mlp64 / Gram tests), so the clamp never takes part;
* the CU count comes from mmmot_device_info (n_cu below); MANY is sized from it.

Tile sets, detection-aligned (RowTiles(counts, sub_counts=dets)), two samples with their own sc / sh / osc / osh:
  EDGE  detections of 1, 31, 32, 33, 63, 64 | 65, 127, 128, 129, 257 rows: empty second halves, half-tile and wave
        boundaries, a last tile of one row; T = 14 tiles
  MANY  16 n_cu + 3 detections of 1 / 2 / 3 rows (one tile each): T exceeds n_cu (persistent grids of gemm_ares_kernel and
        gemm_wres64_kernel), 2 n_cu (pn_mlp64's grid; T * nh >= 2 n_cu of the register kernel; T <= 2 n_cu of the pipelined
        Gram kernel) and 16 n_cu (2T >= 32 n_cu of the independent-wave kernel)

Case -> branch (the conditions are one function, mmmot_ares_choose of csrc/ares_choice.h; tests/test_ares_choice_cpu.py
asks it for the kernel of each of these cases without a GPU):
  gemm_ares_kernel<2, 1 / 2 / 3>  test_gemm_ares_edge[K128-N256] modes 1, 2, 3 (K = 128, mode 2 with N % 512 != 0 never goes
                                  to the register kernel); [K128-N1024] modes 1, 3 and mode 2 under variants 1 and 0
                                  (T * nh = 28 < 2 n_cu); test_gemm_ares_many[K128-N256] modes 1, 3 and [K128-N512] mode 2
                                  variant 1 with T > n_cu (tile switch, table words two tiles ahead); ..._n4096
  gemm_ares_kernel<1, 1 / 2 / 3>  test_gemm_ares_edge[K64-N768] modes 1, 2, 3 (N > 512: not weight-resident);
                                  [K64-N256], [K64-N512] under variant 1 (N % 256 == 0: stream_only); ..._many[K64-N768]
  gemm_wres64_kernel<1 / 2 / 3>   test_gemm_ares_edge[K64-N128 / N384 / N512 / N256]: modes 1, 3 under variant 0 / 3, mode 2
                                  under variant 3 and under 0 (2T = 28 < 32 n_cu); ..._many[K64-N128] modes 1, 3 and mode 2
                                  variant 3 with T > n_cu
  gemm_wres64i_kernel             test_gemm_ares_edge[K64-N128 / N256 / N384 / N512] mode 2 under variant 2 (every wave 0 or 1
                                  items, empty halves written as zeros); ..._many[K64-N128] mode 2 automatic (runs of
                                  items per wave, table rebuilt per detection); ..._without_a_group_table
  gemm_wreg128_kernel             test_gemm_ares_edge[K128-N512 / N1024 / N1536] mode 2 under variant 2 (nh = 1, 2, 3);
                                  ..._many[K128-N512] automatic (T >= 2 n_cu); ..._n4096 (nh = 8); ..._without_a_group_table
  absent operands                 every EDGE case runs with / without bias x with / without dbias (the ares_zeros
                                  stand-in); tile_group = NULL in ..._without_a_group_table (mmmot_gemm_ares called with
                                  _lib.GemmAresArgs directly); N = 4096 without bias rows reads all of ares_zeros
  fallback of the register kernel test_gemm_ares_odd_lddb_falls_back_to_the_streaming_kernel (lddb = 525)
  pn_mlp64_kernel<64>, <128>      test_pn_mlp64[N64 / N128]: plain tiles of 1 / 31 / 32 / 33 / 127 / 128 / 129 rows (7 groups) with and
                                  without bias; 2 n_cu + 5 one-row groups and one of 129 rows: T > gridDim.x (grid-stride
                                  loop, prefetch of tile t + gridDim.x, a workgroup whose second tile is its last)
  gram_rows_kernel<64>            test_gram_rows[K64]
  gram_rows128_kernel             test_gram_rows[K128] variant 1 on both tilings; automatic with T = 2 n_cu + 3
  gram_rows128p_kernel            test_gram_rows[K128] variant 2 on both tilings; automatic with T = 7
  gram_reduce_kernel              test_gn_finalize_gram*: groups of 1, 4, 5, 13, 16, 17, 29, 33, 70 super-tiles: for wave ph
                                  the unrolled loop runs while ph + 12 < nt - not at all (nt <= 12), once for some waves
                                  (13: ph = 0 only; 16, 17: all four), twice (29: ph = 0; 33: all; 70: four trips), each with
                                  a tail of 0 .. 3 trips of the single loop
  gn_finalize_gram_kernel<64/128> test_gn_finalize_gram[K64 / K128 x N]: N = 64, 192, 512 whole 64-channel workgroups; N = 70: a
                                  last quad of two channels (nb + q < N clamp); N = 100: a last workgroup of 36 channels
  gn_finalize_gram_dbias_kernel   test_gn_finalize_gram_dbias[N]: chunks of 32 super-tiles - one (nt <= 32), two (33: a second
                                  chunk of one super-tile), three (70: 32 + 32 + 6); N = 70 / 100: live = false lanes
  pointnet_layer1_kernel<3>, <4>  test_pointnet_layer1[K3 / K4]
  skippool_head_kernel<2>         test_skippool_head R = 1, 3, 255 (a last workgroup with one row)
  skippool_head_kernel<8>         test_skippool_head R = 256, 257, 263 (last workgroups of 8, 1 and 7 rows)
  C = 64 / 320 / 512: 1, 5 (not a power of two) and 8 values per lane; C4 = 64 / 128

Tolerances, as a fraction of the reference's maximum (test_kernels_gpu.close): those of tests/test_kernels_gpu.py - tile sums
and column sums 1e-5, M2 1e-4, pn_mlp64 / pointnet_layer1 Y 2e-6, Gram partials 2e-6, Gram-route scale / shift 5e-6,
skippool head 2e-5, the pooled output of the composite 2e-5.  Where the inputs leave the range of those tests no number is
fixed: the same specification evaluated in torch float32 on the host is the yardstick and the device may be at most 4 x as
far from float64 (test_forward_kernels_gpu.yardstick) - the M2 of gemm_ares under bias rows of 50 +- 30 around a product
of spread 1, the M2 of pointnet_layer1 on coordinates at 30 +- 10, and the Gram-route scale / shift of the groups of 33 and
70 super-tiles (judged by both).

Measured on an MI355X (device error / host-fp32 error, relative to the largest output):
  gemm_ares half-tile M2, bias 50 +- 30      K128-N256 2.1e-7 / 1.7e-6   K64-N128 1.7e-7 / 1.1e-6   K64-N768 2.0e-7 / 2.2e-6
                                             (modes 1 and 3 alike: the kernels centre the raw accumulators, the bias never
                                             enters the second moment)
  pointnet_layer1 tile M2, 30 +- 10          K = 3  9.7e-8 / 1.5e-7      K = 4  8.6e-8 / 1.6e-7
  Gram route, groups of 33 / 70 super-tiles  device 3.2e-8 .. 1.4e-7, host 2.5e-8 .. 2.9e-7 over the 50 comparisons; the
                                             device is at most 1.6 x the host figure (gn_finalize_gram_dbias N = 64, scale:
                                             3.9e-8 against 2.5e-8 - both are the fp32 rounding of the outputs)

Mutations (one line each) and the case that catches them, argued from the code:
* gram_reduce_kernel without the `t += 16` loop body's second half (u = 2, 3 dropped) or with `t + 12 < nt` -> `t + 16 < nt`
  and no tail: groups of 13 .. 70 super-tiles lose partials - test_gn_finalize_gram* groups 3 .. 8 (scale off by percents);
* gn_finalize_gram_dbias_kernel without the barrier before re-staging Sl: a fast wave overwrites super-tile column sums a slow
  one still reads - only groups of more than 32 super-tiles (33, 70) can show it; they are compared bit for bit between
  two launches and against float64;
* past-the-end rows masked by multiplying with 0 instead of assigning 0 (stage_a of gemm_wres64 / pn_mlp64, conv_val of the
  register kernel, convert of the independent-wave kernel): the clamped "row 0" read is finite, so the product is 0 all
  the same - unless the row is read one too far: every X slice is followed by NaN guard rows and the last detection
  of EDGE ends in a one-row tile, NaN * 0 = NaN reaches sums and column sums of the last tile;
* m0 / m1 of an empty half swapped, or the consumer's relu(0 * m1 + m0) summed over masked rows: EDGE has eight empty second
  halves whose column sums must be exactly 0 against the float64 0 with osh up to 2 (1e-5 of the maximum is far below);
* ldsc used for ldosc (epi_consts, cb_dma, consts_of): osc / osh are [G][N + 12] slices, sc / sh [G][K + 12] - group 1 would
  read row 1 at the wrong offset (NaN guard columns or other values): every mode 2 / 3 case;
* lddb taken as N: dbias is a [L][N + 12] slice - every case with dbias;
* tile_dbrow indexed by the half tile or by the group: shown on the CPU by
  test_lidar_spec_cpu.py::test_a_wrong_tile_to_detection_map_is_noticed (errors of more than 1e-2).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd import _lib
from mmmot_amd.pack import from_hl16, hl16_weight_shift, to_hl16
from mmmot_amd.plan import HalfTiles, RowTiles, Segments
from test_backward_kernels_gpu import DEV, NAN, flat, put, slab, twice, untouched  # noqa: F401
from test_forward_kernels_gpu import einval, sentinel, yardstick  # noqa: F401
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu
F64 = torch.float64
F32 = torch.float32
emu = TorchOps(F64)
emu32 = TorchOps(F32)
EPS = 1e-5

EDGE = [[1, 31, 32, 33, 63, 64], [65, 127, 128, 129, 257]]


def n_cu(hip):
    cu = ctypes.c_int(0)
    assert hip.lib.mmmot_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, 0) == 0
    assert cu.value > 0
    return cu.value


def many_dets(ncu):
    n = 16 * ncu + 3
    sizes = [(1, 2, 3)[i % 3] for i in range(n)]
    return [sizes[:n // 2 + 1], sizes[n // 2 + 1:]]


@pytest.fixture
def knobs(hip):
    """the variant knobs, back to automatic afterwards whatever happened"""
    try:
        yield hip.lib
    finally:
        assert hip.lib.mmmot_set_gemm_ares_variant(0) == 0
        assert hip.lib.mmmot_set_gram128_variant(0) == 0


class DetTiles:
    """a detection-aligned tiling on the host (.c) and on the device (.g) with its tile -> detection table"""

    def __init__(self, dets, tile=128):
        self.dets, self.flat = dets, [c for d in dets for c in d]
        self.counts, self.L = [sum(d) for d in dets], len(self.flat)
        self.c = RowTiles(self.counts, 'cpu', sub_counts=dets, tile=tile)
        self.g = RowTiles(self.counts, DEV, sub_counts=dets, tile=tile)
        self.R, self.T, self.G = self.c.R, self.c.T, self.c.G
        self.tile_det = torch.from_numpy(np.repeat(np.arange(self.L), self.c.h_sub_ntiles)).int()
        self.tile_det_g = self.tile_det.to(DEV)
        self.row_grp = torch.repeat_interleave(torch.arange(self.G), torch.tensor(self.counts))
        self.row_det = torch.repeat_interleave(torch.arange(self.L), torch.tensor(self.flat))


@functools.lru_cache(maxsize=None)
def tiling(name, ncu, tile=128):
    if name == 'EDGE':
        t = DetTiles(EDGE, tile)
        assert t.T == 14 and (t.c.h_nrows <= 64).sum() == 8 and t.c.h_nrows[-1] == 1
        return t
    if name == 'ONE':  # EDGE as a single group (tile_group = NULL)
        return DetTiles([EDGE[0] + EDGE[1]], tile)
    t = DetTiles(many_dets(ncu), tile)
    assert t.T == 16 * ncu + 3 and 2 * t.T >= 32 * ncu and t.T > 2 * ncu and max(t.flat) <= 3
    return t


class Layer:
    """fp32 inputs of one layer on a tiling (.g: strided device copies between NaN), asserted far below the 65 000 clamp"""

    def __init__(self, tl, K, N, seed, far=False, dbias_extra=8):
        G, L, R = tl.G, tl.L, tl.R
        self.K, self.N = K, N
        self.X = rnd(R, K, seed=seed) + 0.5
        self.sc, self.sh = rnd(G, K, seed=seed + 1).abs() + 0.5, rnd(G, K, seed=seed + 2)
        self.W = rnd(N, K, seed=seed + 3, scale=K ** -0.5)
        shift = hl16_weight_shift(self.W)
        self.W16, self.osv = to_hl16(self.W.double() * 2.0 ** shift), 2.0 ** -shift
        self.Wq = (from_hl16(self.W16).double() * self.osv).float()  # the weights the hl16 kernels multiply with, as fp32
        assert torch.equal(self.Wq.double(), from_hl16(self.W16).double() * self.osv)
        if far:  # |mean| >> std: bias rows spread far wider than W a
            self.bias, self.dbias = rnd(N, seed=seed + 4) * 30 + 50, rnd(L, N, seed=seed + 5) * 30
        else:
            self.bias, self.dbias = rnd(N, seed=seed + 4), rnd(L, N, seed=seed + 5)
        self.osc, self.osh = rnd(G, N, seed=seed + 6).abs() + 0.5, rnd(G, N, seed=seed + 7)
        self.gamma, self.beta = rnd(N, seed=seed + 8).abs() + 0.5, rnd(N, seed=seed + 9)
        a = torch.relu(self.X.double() * self.sc.double()[tl.row_grp] + self.sh.double()[tl.row_grp])
        assert a.max().item() < 100.0 and (a == 0).any() and (a > 0).any()
        self.a = a
        dbuf, dview = slab(L, N, extra=dbias_extra)
        dview.copy_(self.dbias)
        self.g = dict(X=put(self.X), sc=put(self.sc), sh=put(self.sh), W16=self.W16.to(DEV), bias=put(self.bias), dbias=dview,
                      osc=put(self.osc), osh=put(self.osh), W=self.W.to(DEV), Wq=self.Wq.to(DEV), gamma=put(self.gamma),
                      beta=put(self.beta))
        assert self.g['X'].stride(0) > K and self.g['osc'].stride(0) != self.g['sc'].stride(0)

    def v(self, tl, bias=True, dbias=True, W=None):
        """the materialised product in float64"""
        v = self.a @ (self.Wq if W is None else W).double().t()
        if bias:
            v = v + self.bias.double()
        if dbias:
            v = v + self.dbias.double()[tl.row_det]
        return v


# ---- mmmot_gemm_ares --------------------------------------------------------------------------------------------------
def ares_spec(tl, d, bias, dbias, dtype=F64):
    """(part [2T][2][N], colsum [2T][N]) of the specification with the arithmetic in `dtype`"""
    e = emu if dtype is F64 else emu32
    c = lambda t: t.to(dtype)
    part, cs = torch.zeros(2 * tl.T, 2, d.N, dtype=dtype), torch.zeros(2 * tl.T, d.N, dtype=dtype)
    e.gemm_ares(d.W16, d.osv, tl.c, d.N, d.K, c(d.X), c(d.sc), c(d.sh), bias=c(d.bias) if bias else None,
                dbias=c(d.dbias) if dbias else None, tile_dbrow=tl.tile_det if dbias else None, part=part, osc=c(d.osc),
                osh=c(d.osh), colsum=cs)
    return part, cs


def ares_run(hip, what, tl, d, mode, bias, dbias):
    """the launch of `mode` (bit 0: part, bit 1: colsum) twice -> (part or None, colsum or None)"""
    g = d.g
    kw = dict(bias=g['bias'] if bias else None, dbias=g['dbias'] if dbias else None, tile_dbrow=tl.tile_det_g if dbias else None)
    if mode & 2:
        kw.update(osc=g['osc'], osh=g['osh'])
    make = lambda: ([flat(2 * tl.T, 2, d.N)] if mode & 1 else []) + ([flat(2 * tl.T, d.N)] if mode & 2 else [])

    def launch(*o):
        hip.gemm_ares(g['W16'], d.osv, tl.g, d.N, d.K, g['X'], g['sc'], g['sh'], part=o[0] if mode & 1 else None,
                      colsum=o[-1] if mode & 2 else None, **kw)
    outs = twice(what, make, launch)
    return (outs[0] if mode & 1 else None), (outs[-1] if mode & 2 else None)


def ares_check(what, P, CS, ref):
    if P is not None:
        close(P[:, 0], ref[0][:, 0], 1e-5, what + ' half-tile sums')
        close(P[:, 1], ref[0][:, 1], 1e-4, what + ' half-tile M2')
    if CS is not None:
        close(CS, ref[1], 1e-5, what + ' column sums')


def ares_modes(hip, lib, what, tl, d, plan, bias, dbias):
    """plan: [(mode, variants)]; every (mode, variant) against float64, the column sums of a mode bit-equal over its variants
    (include/mmmot_hip.h: "Results do not depend on it, bit for bit" / "Bit for bit the same column sums")"""
    ref = ares_spec(tl, d, bias, dbias)
    for mode, variants in plan:
        first = None
        for v in variants:
            assert lib.mmmot_set_gemm_ares_variant(v) == 0
            w = '%s bias=%s dbias=%s mode %d variant %d' % (what, bias, dbias, mode, v)
            P, CS = ares_run(hip, w, tl, d, mode, bias, dbias)
            ares_check(w, P, CS, ref)
            if CS is not None:
                if first is None:
                    first = CS
                assert torch.equal(CS, first), w + ': column sums differ from those of variant %d' % variants[0]
    assert lib.mmmot_set_gemm_ares_variant(0) == 0


ALL3 = [(1, (0,)), (2, (0,)), (3, (0,))]
K64_LE512 = [(1, (0, 3)), (2, (3, 2, 0)), (3, (0, 3))]                 # wres64<1,2,3>, wres64i
K64_STREAM = [(1, (1, 3)), (2, (1, 3, 2, 0)), (3, (1, 3))]             # + gemm_ares_kernel<1, .> under variant 1
EDGE_CASES = {
    'K128-N256': (128, 256, ALL3),
    'K128-N1024': (128, 1024, [(1, (0,)), (2, (1, 2, 0)), (3, (0,))]),
    'K128-N512': (128, 512, [(2, (1, 2))]),
    'K128-N1536': (128, 1536, [(2, (1, 2))]),
    'K64-N768': (64, 768, [(1, (0,)), (2, (0, 2, 3)), (3, (0,))]),
    'K64-N256': (64, 256, K64_STREAM),
    'K64-N512': (64, 512, K64_STREAM),
    'K64-N128': (64, 128, K64_LE512),
    'K64-N384': (64, 384, K64_LE512),
}


@pytest.mark.parametrize('case', list(EDGE_CASES))
def test_gemm_ares_edge(hip, knobs, case):
    K, N, plan = EDGE_CASES[case]
    tl = tiling('EDGE', 0)
    ncu = n_cu(hip)
    assert tl.T * (N // 512) < 2 * ncu and 2 * tl.T < 32 * ncu and tl.T <= ncu  # the automatic choices the table names
    d = Layer(tl, K, N, seed=1100)
    for bias, dbias in ((True, True), (True, False), (False, True), (False, False)):
        ares_modes(hip, knobs, 'gemm_ares EDGE ' + case, tl, d, plan, bias, dbias)


MANY_CASES = {
    'K64-N128': (64, 128, True, True, [(1, (0,)), (2, (0, 3)), (3, (0,))]),
    'K128-N512': (128, 512, False, True, [(2, (0, 1))]),
    'K128-N256': (128, 256, True, False, [(1, (0,)), (3, (0,))]),
    'K64-N768': (64, 768, False, False, [(3, (0,))]),
}


@pytest.mark.parametrize('case', list(MANY_CASES))
def test_gemm_ares_many(hip, knobs, case):
    K, N, bias, dbias, plan = MANY_CASES[case]
    tl = tiling('MANY', n_cu(hip))
    ares_modes(hip, knobs, 'gemm_ares MANY ' + case, tl, Layer(tl, K, N, seed=1200), plan, bias, dbias)


def test_gemm_ares_n4096_on_one_short_tile_without_bias_rows(hip, knobs):
    """N = 4096: the whole of the zero stand-in is read (ares_zeros[4096]); one tile of 5 rows; K = 128 mode 2 on the
    streaming kernel and on the register kernel (nh = 8), K = 64 on the streaming kernel"""
    tl = DetTiles([[5]])
    for K in (128, 64):
        plan = [(1, (0,)), (2, (1, 2) if K == 128 else (0,)), (3, (0,))]
        ares_modes(hip, knobs, 'gemm_ares N4096 K%d' % K, tl, Layer(tl, K, 4096, seed=1300), plan, False, False)


def test_gemm_ares_odd_lddb_falls_back_to_the_streaming_kernel(hip, knobs):
    """lddb = 525: the register kernel's 16-byte LDS-DMA pieces cannot fetch such rows, mmmot_ares_choose passes it over and
    the streaming kernel serves variant 2 - the same bits as variant 1, and the float64 values"""
    tl = tiling('EDGE', 0)
    d = Layer(tl, 128, 512, seed=1400, dbias_extra=9)
    assert d.g['dbias'].stride(0) == 525
    ares_modes(hip, knobs, 'gemm_ares odd lddb', tl, d, [(2, (1, 2, 0))], True, True)


def ares_args(tl, d, part=None, colsum=None, bias=True, dbias=True, group=True):
    g, a = d.g, _lib.GemmAresArgs()
    a.X, a.ldx = g['X'].data_ptr(), g['X'].stride(0)
    a.sc, a.sh, a.ldsc = g['sc'].data_ptr(), g['sh'].data_ptr(), g['sc'].stride(0)
    a.W, a.bias = g['W16'].data_ptr(), g['bias'].data_ptr() if bias else None
    if dbias:
        a.dbias, a.tile_dbrow, a.lddb = g['dbias'].data_ptr(), tl.tile_det_g.data_ptr(), g['dbias'].stride(0)
    a.tile_row0, a.tile_nrows = tl.g.row0.data_ptr(), tl.g.nrows.data_ptr()
    a.tile_group = tl.g.group.data_ptr() if group else None
    a.part = None if part is None else part.data_ptr()
    if colsum is not None:
        a.osc, a.osh, a.ldosc, a.colsum = g['osc'].data_ptr(), g['osh'].data_ptr(), g['osc'].stride(0), colsum.data_ptr()
    a.T, a.N, a.K, a.oscale = tl.T, d.N, d.K, float(d.osv)
    return a


def test_gemm_ares_without_a_group_table(hip, knobs):
    """tile_group = NULL: one group, row 0 of sc / sh / osc / osh - on each of the five kernels"""
    tl = tiling('ONE', 0)
    assert tl.G == 1
    for K, N, plan in ((64, 128, [(1, 0), (2, 3), (2, 2), (3, 0)]), (128, 512, [(1, 0), (2, 1), (2, 2), (3, 0)]), (64, 768, [(2, 0)])):
        d = Layer(tl, K, N, seed=1500)
        ref = ares_spec(tl, d, True, True)
        for mode, v in plan:
            assert knobs.mmmot_set_gemm_ares_variant(v) == 0
            what = 'gemm_ares tile_group=NULL K%d N%d mode %d variant %d' % (K, N, mode, v)
            make = lambda: ([flat(2 * tl.T, 2, N)] if mode & 1 else []) + ([flat(2 * tl.T, N)] if mode & 2 else [])

            def launch(*o):
                a = ares_args(tl, d, part=o[0] if mode & 1 else None, colsum=o[-1] if mode & 2 else None, group=False)
                _lib.check(hip.lib.mmmot_gemm_ares(ctypes.byref(a), hip._stream()), 'mmmot_gemm_ares')
            outs = twice(what, make, launch)
            ares_check(what, outs[0] if mode & 1 else None, outs[-1] if mode & 2 else None, ref)


FAR = {}


@pytest.mark.parametrize('K,N', [(128, 256), (64, 128), (64, 768)], ids=['K128-N256', 'K64-N128', 'K64-N768'])
def test_gemm_ares_bias_rows_far_wider_than_the_product(hip, knobs, K, N):
    """bias 50 +- 30 per channel, dbias +- 30 per detection, W a of spread ~1: the half-tile M2 is a small difference of large
    values for a kernel that centred v instead of the raw accumulators.  Sums at 1e-5; M2 by the host-fp32 yardstick"""
    tl = tiling('EDGE', 0)
    d = Layer(tl, K, N, seed=1600, far=True)
    v = d.v(tl)
    assert (v.mean(0).abs() / (d.a @ d.Wq.double().t()).std(0)).median() > 20
    ref, host = ares_spec(tl, d, True, True), ares_spec(tl, d, True, True, F32)
    for mode in (1, 3):
        what = 'gemm_ares far bias K%d N%d mode %d' % (K, N, mode)
        P, CS = ares_run(hip, what, tl, d, mode, True, True)
        close(P[:, 0], ref[0][:, 0], 1e-5, what + ' half-tile sums')
        yardstick(what + ' half-tile M2', P[:, 1], ref[0][:, 1], host[0][:, 1], 1e-4)
        if CS is not None:
            close(CS, ref[1], 1e-5, what + ' column sums')


# ---- mmmot_pn_mlp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [64, 128], ids=['N64', 'N128'])
def test_pn_mlp64(hip, N):
    ncu = n_cu(hip)
    for counts in ([1, 31, 32, 33, 127, 128, 129], [1] * (2 * ncu + 5) + [129]):
        tc, tg = RowTiles(counts, 'cpu'), RowTiles(counts, DEV)
        R, T, G = tc.R, tc.T, tc.G
        assert len(counts) == 7 or T > 2 * ncu
        X = rnd(R, 64, seed=2000) + 0.3
        W = rnd(N, 64, seed=2001, scale=0.125)
        bias = rnd(N, seed=2002)
        sc, sh = rnd(G, 64, seed=2003).abs() + 0.5, rnd(G, 64, seed=2004)
        grp = torch.repeat_interleave(torch.arange(G), torch.tensor(counts))
        assert torch.relu(X * sc[grp] + sh[grp]).max().item() < 100.0
        shift = hl16_weight_shift(W)
        W16, osv = to_hl16(W.double() * 2.0 ** shift), 2.0 ** -shift
        Xg, scg, shg, W16g, bg = put(X), put(sc), put(sh), W16.to(DEV), put(bias)
        for with_bias in (True, False):
            what = 'pn_mlp64 N=%d T=%d bias=%s' % (N, T, with_bias)
            Yr, pr = torch.zeros(R, N, dtype=F64), torch.zeros(T, 2, N, dtype=F64)
            emu.pn_mlp64(W16, osv, tc, N, X.double(), sc.double(), sh.double(), bias.double() if with_bias else None, Yr, pr)
            Y, P = twice(what, lambda: [slab(R, N), flat(T, 2, N)],
                         lambda Y, P: hip.pn_mlp64(W16g, osv, tg, N, Xg, scg, shg, bg if with_bias else None, Y, P))
            close(Y, Yr, 2e-6, what + ' Y')
            close(P[:, 0], pr[:, 0], 1e-5, what + ' tile sums')
            close(P[:, 1], pr[:, 1], 1e-4, what + ' tile M2')


# ---- mmmot_gram_rows --------------------------------------------------------------------------------------------------
def flat64(*shape, fill=None):
    """test_backward_kernels_gpu.flat for float64 outputs; `fill`: the sentinel the view starts from"""
    n, g = int(np.prod(shape)), 8 * int(shape[-1])
    buf = torch.full((n + 2 * g,), NAN, dtype=F64, device=DEV)
    v = buf[g:g + n].view(*shape)
    if fill is not None:
        v.fill_(fill)
    return buf, v


def upper_blocks(K):
    """[K * K] mask of the 32 x 32 blocks on and above the block diagonal (all of them at K = 64: the kernel writes every one)"""
    if K == 64:
        return torch.ones(K * K, dtype=torch.bool)
    blk = torch.arange(K) // 32
    return (blk[:, None] <= blk[None, :]).reshape(K * K)


def gram_run(hip, what, tl, K, Xg, scg, shg):
    return twice(what, lambda: [flat64(tl.T, K * K, fill=-7.0), flat64(tl.T, K)],
                 lambda Gm, S: hip.gram_rows(Xg, K, scg, shg, tl.g, Gm, S))


@pytest.mark.parametrize('K', [64, 128], ids=['K64', 'K128'])
def test_gram_rows(hip, knobs, K):
    """super-tiles of 1, 3, 4 | 127, 128 | 129, 1025 rows (T = 7) and 2 n_cu + 3 super-tiles of 1 .. 3 rows; K = 128 under
    both pinned forms and the automatic choice, bit-equal; Gout starts from -7: the blocks below the block diagonal keep it"""
    ncu = n_cu(hip)
    up = upper_blocks(K)
    small = many_dets(ncu)
    for dets in ([[1, 3, 4], [127, 128], [129, 1025]], [small[0][:ncu + 2], small[1][:ncu + 1]]):
        tl = DetTiles(dets, tile=2048)
        assert tl.T == tl.L and (tl.T == 7 or tl.T == 2 * ncu + 3)
        X = rnd(tl.R, K, seed=3000) * 2.0 + 0.7
        sc, sh = rnd(tl.G, K, seed=3001).abs() + 0.5, rnd(tl.G, K, seed=3002) * 0.5
        assert torch.relu(X * sc[tl.row_grp] + sh[tl.row_grp]).max().item() < 100.0
        Ge, Se = torch.zeros(tl.T, K * K, dtype=F64), torch.zeros(tl.T, K, dtype=F64)
        emu.gram_rows(X.double(), K, sc.double(), sh.double(), tl.c, Ge, Se)
        Xg, scg, shg = put(X), put(sc), put(sh)
        first = None
        for v in ((0,) if K == 64 else (1, 2, 0)):
            assert knobs.mmmot_set_gram128_variant(v) == 0
            what = 'gram_rows K=%d T=%d variant %d' % (K, tl.T, v)
            Gm, S = gram_run(hip, what, tl, K, Xg, scg, shg)
            Gc = Gm.cpu()
            assert (Gc[:, ~up] == -7.0).all(), what + ': a block below the block diagonal was written'
            close(Gc[:, up], Ge[:, up], 2e-6, what + ' Gram partials')
            close(S, Se, 2e-6, what + ' column sums')
            if first is None:
                first = (Gm, S)
            assert torch.equal(Gm, first[0]) and torch.equal(S, first[1]), what + ': differs from variant 1'


# ---- mmmot_gn_finalize_gram / _dbias ----------------------------------------------------------------------------------
GRAM_NT = [1, 4, 5, 13, 16, 17, 29, 33, 70]  # super-tiles per group
GRAM = {}


def gram_groups():
    """nine groups of GRAM_NT one-detection super-tiles, most of 1 .. 5 rows, every seventh of 150 or 600 rows.  The group of one
    super-tile has 150 rows: over a single row the variance is 0 and the Gram route's E[a a^T] - m m^T is nothing but the
    fp32 rounding of the products, of the order of eps itself (measured: the scale of such a group 1.5 % off).  That is
    harmless - v * sc + sh = beta + sc * (v - mean) and v - mean is 0 there - but it is no test of the kernel"""
    dets, k = [], 0
    for nt in GRAM_NT:
        d = []
        for _ in range(nt):
            d.append((150, 1, 2, 3, 1, 5, 2, 1, 4, 3, 1, 2, 1, 600)[k % 14])
            k += 1
        dets.append(d)
    return dets


def gram_partials(hip, K):
    """(tiling, inputs, float64 partials of the specification, device partials written over 0xFF bytes), once per K"""
    if K not in GRAM:
        tl = DetTiles(gram_groups(), tile=1024)
        assert tl.c.h_g_ntiles.tolist() == GRAM_NT and tl.T == tl.L
        X = rnd(tl.R, K, seed=4000) * 2.0 + 0.7
        sc, sh = rnd(tl.G, K, seed=4001).abs() + 0.5, rnd(tl.G, K, seed=4002) * 0.5
        a = torch.relu(X.double() * sc.double()[tl.row_grp] + sh.double()[tl.row_grp])
        assert a.max().item() < 100.0
        Ge, Se = torch.zeros(tl.T, K * K, dtype=F64), torch.zeros(tl.T, K, dtype=F64)
        emu.gram_rows(X.double(), K, sc.double(), sh.double(), tl.c, Ge, Se)
        Gp = torch.empty(tl.T, K * K, dtype=F64, device=DEV)
        Sp = torch.empty(tl.T, K, dtype=F64, device=DEV)
        Gp.view(torch.uint8).fill_(0xFF)  # the lower blocks at K = 128 stay poisoned
        Sp.view(torch.uint8).fill_(0xFF)
        hip.gram_rows(put(X), K, put(sc), put(sh), tl.g, Gp, Sp)
        if K == 128:
            assert torch.isnan(Gp[:, ~upper_blocks(K).to(DEV)]).all()
        GRAM[K] = (tl, a, Ge, Se, Gp, Sp)
    return GRAM[K]


def direct_scale_shift(tl, v, gamma, beta, dtype=F64):
    v, gamma, beta = v.to(dtype), gamma.to(dtype), beta.to(dtype)
    s = torch.stack([gamma / torch.sqrt(torch.var(v[tl.row_grp == g], 0, unbiased=False) + EPS) for g in range(tl.G)])
    h = torch.stack([beta - v[tl.row_grp == g].mean(0) * s[g] for g in range(tl.G)])
    return s, h


def judge_gram(what, got, spec, direct, host):
    """every group against the specification and the direct statistics at 5e-6; the groups of 33 and 70 super-tiles (longer
    than any group of tests/test_kernels_gpu.py) also by the host-fp32 yardstick"""
    for name, g, s, dr, h in zip(('scale', 'shift'), got, spec, direct, host):
        close(g, s, 5e-6, '%s %s against the specification' % (what, name))
        close(g, dr, 5e-6, '%s %s against the statistics of v' % (what, name))
        yardstick('%s %s of the groups of 33 / 70 super-tiles' % (what, name), g[7:], dr[7:], h[7:], 5e-6)


@pytest.mark.parametrize('N', [64, 70, 100, 192, 512])
@pytest.mark.parametrize('K', [64, 128], ids=['K64', 'K128'])
def test_gn_finalize_gram(hip, K, N):
    tl, a, Ge, Se, Gp, Sp = gram_partials(hip, K)
    G = tl.G
    W = rnd(N, K, seed=4100, scale=K ** -0.5)
    bias, gamma, beta = rnd(N, seed=4101), rnd(N, seed=4102).abs() + 0.5, rnd(N, seed=4103)
    Wg, bg, gg, beg = W.to(DEV), put(bias), put(gamma), put(beta)
    for with_bias in (True, False):
        what = 'gn_finalize_gram K=%d N=%d bias=%s' % (K, N, with_bias)
        v = a @ W.double().t() + (bias.double() if with_bias else 0.0)
        spec = torch.zeros(G, N, dtype=F64), torch.zeros(G, N, dtype=F64)
        emu.gn_finalize_gram(Ge, Se, tl.c, K, W, bias if with_bias else None, N, gamma, beta, EPS, None, *spec)
        direct = direct_scale_shift(tl, v, gamma, beta)
        host = direct_scale_shift(tl, a.float() @ W.t() + (bias if with_bias else 0.0), gamma, beta, F32)
        work = torch.full((G, K * K + K), NAN, dtype=F64, device=DEV)  # poisoned
        got = twice(what, lambda: [flat(G, N), flat(G, N)], lambda s, h: hip.gn_finalize_gram(
            Gp, Sp, tl.g, K, Wg, bg if with_bias else None, N, gg, beg, EPS, work, s, h))
        judge_gram(what, got, spec, direct, host)


@pytest.mark.parametrize('N', [64, 70, 100, 192, 512])
def test_gn_finalize_gram_dbias(hip, N):
    """a strided dbias whose spread over the detections is, in every channel, larger than that of W a in any channel (asserted)"""
    K = 64
    tl, a, Ge, Se, Gp, Sp = gram_partials(hip, K)
    G = tl.G
    W = rnd(N, K, seed=4200, scale=K ** -0.5)
    dbias = rnd(tl.L, N, seed=4201) * 5.0 + 1.5
    gamma, beta = rnd(N, seed=4202).abs() + 0.5, rnd(N, seed=4203)
    wa = a @ W.double().t()
    assert dbias.std(0).min() > wa.std(0).max()
    v = wa + dbias.double()[tl.row_det]
    what = 'gn_finalize_gram_dbias N=%d' % N
    spec = torch.zeros(G, N, dtype=F64), torch.zeros(G, N, dtype=F64)
    emu.gn_finalize_gram_dbias(Ge, Se, tl.c, tl.tile_det, K, W, dbias, N, gamma, beta, EPS, None, *spec)
    direct = direct_scale_shift(tl, v, gamma, beta)
    host = direct_scale_shift(tl, a.float() @ W.t() + dbias[tl.row_det], gamma, beta, F32)
    Wg, dg, gg, beg = W.to(DEV), put(dbias), put(gamma), put(beta)
    assert dg.stride(0) == N + 12
    work = torch.full((G, K * K + K), NAN, dtype=F64, device=DEV)  # poisoned
    got = twice(what, lambda: [flat(G, N), flat(G, N)], lambda s, h: hip.gn_finalize_gram_dbias(
        Gp, Sp, tl.g, tl.tile_det_g, K, Wg, dg, N, gg, beg, EPS, work, s, h))
    judge_gram(what, got, spec, direct, host)


# ---- mmmot_pointnet_layer1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 4], ids=['K3', 'K4'])
def test_pointnet_layer1(hip, K):
    """tiles of 1 / 31 / 32 / 33 / 128 rows (and 128 + 1), coordinates at 30 +- 10: the tile M2 is judged by the host-fp32
    yardstick"""
    counts = [1, 31, 32, 33, 128, 129]
    tc, tg = RowTiles(counts, 'cpu'), RowTiles(counts, DEV)
    R, T = tc.R, tc.T
    assert tc.h_nrows.tolist() == [1, 31, 32, 33, 128, 128, 1]
    X = rnd(R, K, seed=5000) * 10 + 30
    W, b = rnd(64, K, seed=5001), rnd(64, seed=5002)
    Yr, pr = torch.zeros(R, 64, dtype=F64), torch.zeros(T, 2, 64, dtype=F64)
    emu.pointnet_layer1(X.double(), W.double(), b.double(), Yr, pr, tc)
    Yh, ph = torch.zeros(R, 64), torch.zeros(T, 2, 64)
    emu32.pointnet_layer1(X, W, b, Yh, ph, tc)
    buf, Xg = flat(R, K)
    Xg.copy_(X)
    Wg, bg = W.to(DEV), put(b)
    what = 'pointnet_layer1 K=%d' % K
    Y, P = twice(what, lambda: [flat(R, 64), flat(T, 2, 64)], lambda Y, P: hip.pointnet_layer1(Xg, Wg, bg, Y, P, tg))
    close(Y, Yr, 2e-6, what + ' Y')
    close(P[:, 0], pr[:, 0], 1e-5, what + ' tile sums')
    yardstick(what + ' tile M2', P[:, 1], pr[:, 1], ph[:, 1], 1e-4)


# ---- mmmot_skippool_head ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,C4', [(64, 64), (64, 128), (320, 64), (320, 128), (512, 64), (512, 128)])
def test_skippool_head(hip, C, C4):
    """R = 1, 3, 255: the latency form (two rows per workgroup); 256, 257, 263: the batch form (eight); P a strided slice, out a
    guarded column slice; rows 100 .. 136 of a batch-form launch bit-equal to the latency form on those rows alone"""
    hd = dict(g0=rnd(C, seed=1).abs() + 0.5, b0=rnd(C, seed=2), w1=rnd(C4, C, seed=3, scale=C ** -0.5), c1=rnd(C4, seed=4),
              g2=rnd(C4, seed=5).abs() + 0.5, b2=rnd(C4, seed=6), w4=rnd(128, C4, seed=7, scale=C4 ** -0.5),
              c4=rnd(128, seed=8), g5=rnd(128, seed=9).abs() + 0.5, b5=rnd(128, seed=10))
    hg = {k: v.to(DEV) for k, v in hd.items()}
    h64 = {k: v.double() for k, v in hd.items()}
    Pall = rnd(263, C, seed=11) * 3 + 1
    for R in (1, 3, 255, 256, 257, 263):
        what = 'skippool_head C=%d C4=%d R=%d' % (C, C4, R)
        P = Pall[:R]
        ref = torch.zeros(R, 128, dtype=F64)
        emu.skippool_head(P.double(), C, h64, EPS, ref, R)
        Pg = put(P)
        assert Pg.stride(0) > C
        (out,) = twice(what, lambda: [slab(R, 128)], lambda o: hip.skippool_head(Pg, C, hg, EPS, o, R))
        close(out, ref, 2e-5, what)
        if R >= 256:
            Fg = put(P[100:137])
            (few,) = twice(what + ' rows 100 .. 136 alone', lambda: [slab(37, 128)], lambda o: hip.skippool_head(Fg, C, hg, EPS, o, 37))
            assert torch.equal(few, out[100:137]), what + ': the batch form differs from the latency form'


# ---- composite: one conv5-shaped layer three ways ----------------------------------------------------------------------
def test_norm_relu_pool_three_routes(hip):
    """K = 128, N = 256 on EDGE: per-detection mean of relu(GroupNorm(v)) by (a) the Gram route - gram_rows, gn_finalize_gram,
    the column-sum pass, segment_mean over half tiles; (b) the statistics pass - part, gn_finalize over HalfTiles, the same
    consumer; (c) the materialised product of mmmot_gemm_rows - each against float64 group_norm -> relu -> mean"""
    K, N = 128, 256
    tl = tiling('EDGE', 0)
    d = Layer(tl, K, N, seed=6000)
    g = d.g
    v = d.v(tl, bias=True, dbias=False)
    ref = torch.zeros(tl.L, N, dtype=F64)
    r = 0
    for i, c in enumerate(tl.flat):
        grp = int(tl.row_grp[r])
        vg = v[tl.row_grp == grp]
        y = torch.nn.functional.group_norm(vg.t().unsqueeze(0), N, d.gamma.double(), d.beta.double(), EPS)[0].t()
        lo = r - int(tl.c.h_g_row0[grp])
        ref[i] = torch.relu(y[lo:lo + c]).mean(0)
        r += c
    det_grp = [gi for gi, dd in enumerate(tl.dets) for _ in dd]
    hc, hg = HalfTiles(tl.c, 'cpu'), HalfTiles(tl.g, DEV)
    half_segs = Segments(2 * tl.c.h_sub_tile0, 2 * tl.c.h_sub_ntiles, [1] * tl.L, det_grp, DEV, div=tl.flat)

    def consumer(what, osc, osh):
        (cs,) = twice(what + ' column sums', lambda: [flat(hc.T, N)], lambda cs: hip.gemm_ares(
            g['W16'], d.osv, tl.g, N, K, g['X'], g['sc'], g['sh'], bias=g['bias'], osc=osc, osh=osh, colsum=cs))
        (out,) = twice(what + ' pooled', lambda: [slab(tl.L, N)], lambda o: hip.segment_mean(cs, N, half_segs, o))
        close(out, ref, 2e-5, what)
    # (a) statistics from the Gram matrix of the input (fp32 weights equal to the dequantised hl16 ones)
    gt, gg = RowTiles(tl.counts, 'cpu', tile=1024), RowTiles(tl.counts, DEV, tile=1024)
    Gp, Sp = torch.full((gg.T, K * K), NAN, dtype=F64, device=DEV), torch.full((gg.T, K), NAN, dtype=F64, device=DEV)
    hip.gram_rows(g['X'], K, g['sc'], g['sh'], gg, Gp, Sp)
    work = torch.full((gg.G, K * K + K), NAN, dtype=F64, device=DEV)
    scn, shn = twice('Gram route scale / shift', lambda: [flat(tl.G, N), flat(tl.G, N)], lambda s, h: hip.gn_finalize_gram(
        Gp, Sp, gg, K, g['Wq'], g['bias'], N, g['gamma'], g['beta'], EPS, work, s, h))
    consumer('Gram route', put(scn), put(shn))
    # (b) statistics pass over the half tiles
    (part,) = twice('statistics pass', lambda: [flat(hc.T, 2, N)], lambda p: hip.gemm_ares(
        g['W16'], d.osv, tl.g, N, K, g['X'], g['sc'], g['sh'], bias=g['bias'], part=p))
    scn, shn = twice('statistics-pass scale / shift', lambda: [flat(tl.G, N), flat(tl.G, N)],
                     lambda s, h: hip.gn_finalize(part, hg, N, N, g['gamma'], g['beta'], EPS, s, h))
    consumer('statistics-pass route', put(scn), put(shn))
    # (c) materialised
    pc, pg = RowTiles(tl.counts, 'cpu'), RowTiles(tl.counts, DEV)
    Y, part = twice('materialised product', lambda: [slab(tl.R, N), flat(pc.T, 2, N)], lambda Y, p: hip.gemm(
        g['W16'], pg, N, K, X=g['X'], bias=g['bias'], Y=Y, part=p, sc=g['sc'], sh=g['sh'], amode=1, w_hl16=True, oscale=d.osv))
    scn, shn = twice('materialised scale / shift', lambda: [flat(tl.G, N), flat(tl.G, N)],
                     lambda s, h: hip.gn_finalize(part, pg, N, N, g['gamma'], g['beta'], EPS, s, h))
    scn, shn = put(scn), put(shn)
    starts = np.concatenate([[0], np.cumsum(tl.flat)])[:-1]
    det_segs = Segments(starts, tl.flat, [1] * tl.L, det_grp, DEV)
    (out,) = twice('materialised route', lambda: [slab(tl.L, N)],
                   lambda o: hip.segment_mean(Y, N, det_segs, o, sc=scn, sh=shn, relu=True))
    close(out, ref, 2e-5, 'materialised route')


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_launchers_refuse_what_the_lidar_kernels_cannot_take(hip):
    """each launcher first takes a small valid call, then - over outputs filled with 5 - the same call with ONE argument it
    must refuse: MMMOT_EINVAL, and after a synchronise nothing was written"""
    z = lambda *shape, **kw: torch.zeros(*shape, device=DEV, **kw)
    tl = DetTiles([[5]])
    t = tl.g
    X, Xodd, W16 = z(16, 140), z(16, 133), z(4224 * 128)
    tab, vec = z(2, 4240), z(4240)
    part, colsum, Y, out = z(2, 2, 4224), z(2, 4224), z(16, 140), z(16, 140)
    Gm, S, work, sc, sh = z(1, 128 * 128, dtype=F64), z(1, 128, dtype=F64), z(1, 128 * 128 + 128, dtype=F64), z(1, 512), z(1, 512)
    P = z(16, 1024)
    hd = {k: z(*s) for k, s in dict(g0=(1024,), b0=(1024,), w1=(256, 1024), c1=(256,), g2=(256,), b2=(256,), w4=(128, 256),
                                    c4=(128,), g5=(128,), b5=(128,)).items()}
    head = lambda C, C4: dict(hd, w1=hd['w1'].view(-1)[:C4 * C].view(C4, C))
    outputs = [part, colsum, Y, out, Gm, S, sc, sh]
    det = tl.tile_det_g
    ares = lambda N, K, Xv, **kw: hip.gemm_ares(W16, 1.0, t, N, K, Xv, tab[:, :K], tab[:, :K], **kw)
    full = dict(bias=vec, dbias=tab[:, :128], tile_dbrow=det, part=part, osc=tab[:, :128], osh=tab[:, :128], colsum=colsum)
    # valid calls
    ares(128, 64, X[:, :64], **full)
    ares(256, 128, X[:, :128], **dict(full, dbias=tab[:, :256], osc=tab[:, :256], osh=tab[:, :256]))
    hip.pn_mlp64(W16, 1.0, t, 64, X[:, :64], tab[:, :64], tab[:, :64], vec, Y[:, :64], part)
    hip.gram_rows(X[:, :64], 64, tab[:, :64], tab[:, :64], t, Gm, S)
    hip.gn_finalize_gram(Gm, S, t, 64, W16, vec, 64, vec, vec, EPS, work, sc, sh)
    hip.gn_finalize_gram_dbias(Gm, S, t, det, 64, W16, tab[:, :64], 64, vec, vec, EPS, work, sc, sh)
    hip.pointnet_layer1(X.view(-1)[:15].view(5, 3), W16[:192].view(64, 3), vec, Y.view(-1)[:320].view(5, 64), part, t)
    hip.skippool_head(P[:, :64], 64, head(64, 64), EPS, out[:, :128], 5)
    torch.cuda.synchronize()
    for o in outputs:
        o.fill_(5.0)
    einval(ares, 128, 96, X[:, :96], **full)                                                   # K not in {64, 128}
    einval(ares, 192, 64, X[:, :64], **full)                                                   # N % 128
    einval(ares, 384, 128, X[:, :128], **dict(full, dbias=tab[:, :384], osc=tab[:, :384], osh=tab[:, :384]))  # K = 128: N % 256
    einval(ares, 4224, 128, X[:, :128], **dict(full, dbias=tab[:, :4224], osc=tab[:, :4224], osh=tab[:, :4224]))  # N > 4096
    einval(ares, 128, 64, Xodd[:, :64], **full)                                                # ldx % 4
    einval(ares, 128, 64, X[:, 1:65], **full)                                                  # X 4 bytes off a 16-byte boundary
    einval(ares, 128, 64, X[:, :64], **dict(full, tile_dbrow=None))                            # dbias without tile_dbrow
    einval(ares, 128, 64, X[:, :64], **dict(full, osc=None, osh=None))                         # colsum without osc / osh
    einval(ares, 128, 64, X[:, :64], **dict(full, part=None, colsum=None))                     # neither output
    pn = lambda N, Xv, Yv: hip.pn_mlp64(W16, 1.0, t, N, Xv, tab[:, :64], tab[:, :64], vec, Yv, part)
    einval(pn, 96, X[:, :64], Y[:, :96])                                                       # N not in {64, 128}
    einval(pn, 64, Xodd[:, :64], Y[:, :64])                                                    # ldx % 4
    einval(pn, 64, X[:, 1:65], Y[:, :64])                                                      # X misaligned
    einval(pn, 64, X[:, :64], Y.view(-1)[:16 * 60].as_strided((16, 64), (60, 1)))              # ldy < N
    gr = lambda K, Xv: hip.gram_rows(Xv, K, tab[:, :K], tab[:, :K], t, Gm, S)
    einval(gr, 96, X[:, :96])                                                                  # K not in {64, 128}
    einval(gr, 64, Xodd[:, :64])                                                               # ldx % 4
    einval(gr, 64, X[:, 1:65])                                                                 # X misaligned
    einval(hip.gn_finalize_gram, Gm, S, t, 96, W16, vec, 64, vec, vec, EPS, work, sc, sh)      # K not in {64, 128}
    einval(hip.gn_finalize_gram_dbias, Gm, S, t, det, 128, W16, tab[:, :64], 64, vec, vec, EPS, work, sc, sh)  # K != 64
    einval(hip.gn_finalize_gram_dbias, Gm, S, t, det, 64, W16, tab.view(-1)[:120].as_strided((2, 64), (60, 1)), 64, vec, vec,
           EPS, work, sc, sh)                                                                  # lddb < N
    einval(hip.pointnet_layer1, X.view(-1)[:25].view(5, 5), W16[:320].view(64, 5), vec, Y.view(-1)[:320].view(5, 64), part, t)  # K = 5
    einval(hip.skippool_head, P[:, :96], 96, head(96, 64), EPS, out[:, :128], 5)               # C % 64
    einval(hip.skippool_head, P[:, :576], 576, head(576, 64), EPS, out[:, :128], 5)            # C > 512
    einval(hip.skippool_head, P[:, :64], 64, head(64, 192), EPS, out[:, :128], 5)              # C4 > 128
    torch.cuda.synchronize()
    for o in outputs:
        assert (o == 5.0).all(), 'a refused call wrote to an output'
