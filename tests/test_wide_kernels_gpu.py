"""Every launch branch of the wide pair-block GEMM (csrc/gemm_wide.hip, gemm_wide_kernel<NH, AMODE, PAIROP>) against the
float64 statement of the same layer, and against the tile kernel of csrc/gemm_rows.hip bit for bit.

Case -> branch (the conditions are one function, mmmot_wide_choose of csrc/wide_choice.h; tests/test_wide_choice_cpu.py
pins it without a GPU; every case here first asks mmmot_gemm_rows_choice which kernel, NH, items and grid its launch gets):
  <1 | 2, NORM_RELU, -> and <1 | 2, PAIR, multiply | minus_abs | minus>, K = 256 | 512, N = 512 (ntn = 2)
      test_instantiations[op-K]: Y and part / Y only (no statistics passes) / part only (Y = NULL: no LDS staging) x bias /
      bias = NULL; NORM_RELU groups of 300, 5, 128, 1, 33, 127 rows (8 tiles, one item per workgroup), PAIR (5, 64), (3, 160),
      (1, 32), (7, 96) (14 tiles: two items per workgroup under the limit of 16); ldx = K + 64,
      ldsc = K + 12, ldf = K + 256 at K = 256, ldy = N + 12, FA != FB, NaN in every unused column and row
  item chains (grid limit 8 ntn: every workgroup walks all its items; 16 ntn: chains of unequal length)
      test_chain_norm_relu[K-N]: 53 tiles in 19 groups of scale / shift magnitudes 2^-3 .. 2^5, T odd (the last NH = 2
      item has an empty second tile: ok = false, nrows = 0); on the host: every workgroup walks >= 3 items, >= half of
      the item -> successor steps change group (uniform rows of buffer ub ^ 1, top1 from the successor)
      test_chain_pair[op-K]: 49 tiles in 5 groups, K = 256 with ldf = 512 (half the uniform-row DMAs, 16 steps), aoff / boff
      with NaN rows between the groups, bias
      test_chain_padding_items[T]: T = 1 (seven of eight items are padding, has_next = false on the first item), T = 9 and
      17 (8 k + 1: a last group of items that is one tile and seven paddings; NH = 2: an empty second tile as well)
  strides and NULLs: every case above (ldx, ldsc, ldf, ldy, NaN rows of FA / FB); test_without_a_tile_group: tile_group =
      NULL with one group, NORM_RELU (mmmot_gemm_rows refuses a PAIR launch without tile_group: asserted)
  the fp16 clamp (MM_F16_CLAMP = 65000, top = 0 for rows past a tile's end): test_clamp[norm_relu | multiply | minus]:
      0.1 % .. 5 % of the A elements clamped (asserted on the host), ragged last tiles
  the automatic choice (variant 0): test_automatic_choice: PAIR, N = 1024, Y = NULL; T one below / at n_cu / 2 items (tile
      kernel / NH = 1) and one below / at 24 n_cu items (NH = 1 / NH = 2); around 24 n_cu also bit-equal to variants 1, 3, 4
      and float64 on eight sampled tiles
  what the kernel declines: test_declined[...]: under variant 3 the choice reports wide = 0 and the result matches float64
      (fp32 weights, K = 128 / 384 / 1024, N = 128 / 384, PLAIN, dbias, colsum, activation, pair_uniform32 = 0 on aligned
      and on ragged pair tiles); ldf % 4 and ldy % 4 with Y are refused by mmmot_gemm_rows itself (MMMOT_EINVAL, asserted);
      K > ldf and ldsc < K describe overlapping rows and are pinned by the CPU test only

Every case: Y is a [R][N] column slice (ldy = N + 12) of a NaN buffer with a guard row before and after, part the first T
rows of a NaN [T + 16][2][N] buffer (the padding items of the largest group stay inside it); every guard must still be NaN
and every element inside written.  The float64 statement is TorchOps(torch.float64).gemm on the same tiling over
A = clamp(op(a_i, b_j), -65000, +65000) (PAIR) / min(relu(x * sc + sh), 65000) (NORM_RELU), the hl16 weights decoded
exactly.  Y and part are bit-equal across variant 3, variant 4 and variant 1, with and without the grid limit, and on a
repeat of the same launch.  Comparisons are made per group, relative to the group's own largest value, so that a group
of small scale is judged as strictly as one of large scale.

Tolerances: those of tests/test_kernels_gpu.py (close: a fraction of the reference's largest value, here of the group's) -
Y 3e-6, tile sums 1e-5, tile M2 1e-4.  No case needs more: the clamped cases (A up to 65000 beside A of order 1) and the
M2 of the 2600-row group stay below 1e-6 as well, so none is judged by the host-float32 yardstick of
tests/test_forward_kernels_gpu.py.

Measured on an MI355X (worst over the family, relative to the largest value of the group): Y / tile sums / tile M2
  NORM_RELU                 6.3e-7 / 6.3e-7 / 6.4e-7
  PAIR multiply             8.0e-7 / 3.9e-7 / 2.9e-7
  PAIR minus_abs            7.3e-7 / 1.5e-7 / 5.9e-7
  PAIR minus                6.9e-7 / 1.7e-7 / 3.2e-7
  chained (all four)        6.8e-7 / 2.7e-7 / 5.7e-7   (NORM_RELU, 2600-row group included, the worst)
  clamped NORM_RELU         4.1e-7 / 1.4e-7 / 2.1e-7   (the host's float32 evaluation of the statement: 4.0e-7 / 1.2e-7 / 1.7e-7)
  clamped multiply          5.0e-7 / 3.9e-7 / 1.5e-7   (host float32: 5.2e-7 / 3.7e-7 / 2.1e-7)
  clamped minus             5.6e-7 / 4.0e-7 / 1.9e-7   (host float32: 5.6e-7 / 3.3e-7 / 1.9e-7)

Reverted on purpose in a scratch copy (never committed), each of these fails the cases named:
* read_u reading buffer ub instead of ub ^ 1 for the successor's steps: every test_chain_* case but T = 1, test_instantiations of the
  PAIR operations (14 tiles under the limit of 16 walk two items), test_clamp[multiply | minus], test_automatic_choice;
* the `t2 < a.T` guard dropped: the NaN rows behind part are written - every case with padding items or an odd T under NH = 2
  (test_instantiations, test_chain_*, test_clamp, test_without_a_tile_group, test_automatic_choice);
* top1 always from scur: every test_chain_* case but the padding ones, test_instantiations of the PAIR operations,
  test_clamp[multiply | minus] (a ragged tile next to a full one in the same chain);
* the wrapper not passing pair_uniform32: every PAIR case - the choice reports the tile kernel.
"""
import ctypes
import functools

import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd.pack import hl16_weight_shift, to_hl16
from mmmot_amd.plan import RowTiles
from test_backward_kernels_gpu import DEV, NAN, untouched
from test_forward_kernels_gpu import einval
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
CLAMP = 65000.0                      # MM_F16_CLAMP of csrc/common.h
NORM = 'norm_relu'
OPS = {NORM: None, 'multiply': 0, 'minus_abs': 1, 'minus': 2}
TOL_Y, TOL_SUM, TOL_M2 = 3e-6, 1e-5, 1e-4
PART_GUARD = 16                      # rows behind part: NH * 8 - 1 padding tiles at the most
WORST = {}


def n_cu(hip):
    cu = ctypes.c_int(0)
    assert hip.lib.mmmot_device_info(torch.cuda.current_device(), ctypes.byref(cu), None, 0) == 0
    assert cu.value > 0
    return cu.value


@pytest.fixture
def knobs(hip):
    """(set variant, set grid limit); both back to automatic afterwards whatever happened"""
    try:
        yield hip.lib.mmmot_set_gemm_rows_variant, hip.lib.mmmot_set_gemm_wide_grid_limit
    finally:
        assert hip.lib.mmmot_set_gemm_rows_variant(0) == 0
        assert hip.lib.mmmot_set_gemm_wide_grid_limit(0) == 0


def wide_plan(T, N, nh, ncu, limit=0):
    """(items, grid) of the wide kernel's launch - the geometry tests/test_wide_choice_cpu.py pins as literals"""
    ntn = N // 256
    g = 8 * ntn
    items = -(-(-(-T // nh)) // 8) * g
    grid = max((2 // nh) * ncu // g * g, g)
    if limit > 0 and grid > limit:
        grid = max(limit // g * g, g)
    return items, min(grid, items)


def nan_slice(t, extra, rows_before=1, rows_after=1):
    """a 2-D host tensor on the device as the leading columns of a NaN buffer with `extra` more columns and NaN rows around"""
    buf = torch.full((t.shape[0] + rows_before + rows_after, t.shape[1] + extra), NAN, device=DEV)
    v = buf[rows_before:rows_before + t.shape[0], :t.shape[1]]
    v.copy_(t)
    return v


class NoGroup:
    """a device tiling handed over without its tile -> group table (tile_group = NULL)"""

    def __init__(self, t):
        self.row0, self.nrows, self.group, self.T = t.row0, t.nrows, None, t.T


class Case:
    """one layer: host inputs, device copies in NaN buffers, the float64 / float32 statement, guarded launches"""

    def __init__(self, op, K, N, tiling, bias=True, seed=0, mags=None, plant=None, ldf=None, no_group=False):
        self.op, self.K, self.N, self.pairop = op, K, N, OPS[op]
        self.pair = op != NORM
        W = rnd(N, K, seed=seed + 1, scale=K ** -0.5)
        shift = hl16_weight_shift(W)
        self.W16, self.osc = to_hl16(W.double() * 2.0 ** shift), 2.0 ** -shift
        self.W16g = self.W16.to(DEV)
        self.bias = rnd(N, seed=seed + 2) if bias else None
        self.biasg = self.bias.to(DEV) if bias else None
        if self.pair:
            NM = tiling
            self.counts = [n * m for n, m in NM]
            self.M = torch.tensor([m for _, m in NM])
            na, nb = sum(n for n, _ in NM), sum(m for _, m in NM)
            G = len(NM)
            FA, FB = torch.full((na + 2 * G + 3, K), NAN), torch.full((nb + 3 * G + 2, K), NAN)  # NaN rows between the groups
            a, b, oa, ob = rnd(na, K, seed=seed + 3), rnd(nb, K, seed=seed + 4), 2, 3
            if plant:
                plant(a, b)
            self.aoff, self.boff = [], []
            for n, m in NM:
                self.aoff.append(oa)
                self.boff.append(ob)
                FA[oa:oa + n] = a[:n]
                FB[ob:ob + m] = b[:m]
                a, b, oa, ob = a[n:], b[m:], oa + n + 2, ob + m + 3
            self.FA, self.FB = FA, FB
            ldf = K if ldf is None else ldf
            self.FAg, self.FBg = nan_slice(FA, ldf - K, 0, 0), nan_slice(FB, ldf - K, 0, 0)
        else:
            self.counts = list(tiling)
            G, R = len(self.counts), sum(self.counts)
            self.X = rnd(R, K, seed=seed + 3)
            mags = torch.ones(G) if mags is None else torch.tensor(mags, dtype=F32)
            self.sc = (rnd(G, K, seed=seed + 4).abs() + 0.5) * mags[:, None]
            self.sh = rnd(G, K, seed=seed + 5) * mags[:, None]
            if plant:
                plant(self.sc, self.sh)
            self.Xg = nan_slice(self.X, 64)
            self.scg, self.shg = nan_slice(self.sc, 12, 0, 0), nan_slice(self.sh, 12, 0, 0)
        self.c, self.g = RowTiles(self.counts, 'cpu'), RowTiles(self.counts, DEV)
        self.R, self.T, self.G = self.c.R, self.c.T, self.c.G
        self.gtiles = NoGroup(self.g) if no_group else self.g
        self.g_row0 = torch.as_tensor(self.c.h_g_row0).long()
        if self.pair:
            mk = lambda dev: dict(row0=torch.tensor(self.c.h_g_row0).to(dev), M=self.M.int().to(dev),
                                  aoff=torch.tensor(self.aoff, dtype=torch.int32).to(dev),
                                  boff=torch.tensor(self.boff, dtype=torch.int32).to(dev), uniform32=True)
            self.pt_c, self.pt_g = mk('cpu'), mk(DEV)

    # ---- the statement ---------------------------------------------------------------------------------------------
    def operand(self, dtype, rows=None, clamp=True):
        """A of the given rows (all rows by default) evaluated in dtype: op / normalise, then the fp16 clamp"""
        rows = torch.arange(self.R) if rows is None else rows
        grp = torch.searchsorted(self.g_row0, rows, right=True) - 1
        if self.pair:
            q = rows - self.g_row0[grp]
            i, j = q // self.M[grp], q % self.M[grp]
            a = self.FA[torch.tensor(self.aoff)[grp] + i].to(dtype)
            b = self.FB[torch.tensor(self.boff)[grp] + j].to(dtype)
            A = a * b if self.pairop == 0 else ((a - b) / 2).abs() if self.pairop == 1 else (a - b) / 2
            return A.clamp(-CLAMP, CLAMP) if clamp else A
        A = torch.relu(self.X[rows].to(dtype) * self.sc[grp].to(dtype) + self.sh[grp].to(dtype))
        return A.clamp(max=CLAMP) if clamp else A

    def statement(self, dtype, tiles=None):
        """(Y, part) of TorchOps(dtype).gemm over the clamped operand; tiles: a list of tile indices (each becomes a
        group of its own) instead of the whole tiling"""
        if tiles is None:
            tl, A = self.c, self.operand(dtype)
        else:
            tl = RowTiles([int(self.c.h_nrows[t]) for t in tiles], 'cpu')
            A = self.operand(dtype, torch.cat([torch.arange(int(self.c.h_row0[t]), int(self.c.h_row0[t] + self.c.h_nrows[t]))
                                               for t in tiles]))
        Y, part = torch.zeros(tl.R, self.N, dtype=dtype), torch.zeros(tl.T, 2, self.N, dtype=dtype)
        TorchOps(dtype).gemm(self.W16, tl, self.N, self.K, X=A, bias=None if self.bias is None else self.bias.to(dtype), Y=Y,
                             part=part, amode=0, w_hl16=True, oscale=self.osc)
        return Y, part

    @functools.lru_cache(maxsize=None)
    def ref(self):
        return self.statement(F64)

    # ---- launches --------------------------------------------------------------------------------------------------
    def kwargs(self, Y, part):
        kw = dict(bias=self.biasg, Y=Y, part=part, w_hl16=True, oscale=self.osc)
        if self.pair:
            kw.update(FA=self.FAg, FB=self.FBg, pair=self.pt_g, amode=2, pairop=self.pairop)
        else:
            kw.update(X=self.Xg, sc=self.scg, sh=self.shg, amode=1)
        return kw

    def launch(self, hip, knobs, variant, limit, expect, want_y=True, want_part=True):
        """one guarded launch under (variant, limit) after asserting the choice: expect = 0 (tile kernel) or NH; ->
        (Y, part) on the host, None for an absent output"""
        assert knobs[0](variant) == 0 and knobs[1](limit) == 0
        ybuf = torch.full((self.R + 2, self.N + 12), NAN, device=DEV) if want_y else None
        Y = ybuf[1:self.R + 1, :self.N] if want_y else None
        pbuf = torch.full((self.T + PART_GUARD, 2, self.N), NAN, device=DEV) if want_part else None
        part = pbuf[:self.T] if want_part else None
        kw = self.kwargs(Y, part)
        wide, nh, items, grid = hip.gemm_choice(self.W16g, self.gtiles, self.N, self.K, **kw)
        what = '%s K%d N%d variant %d limit %d' % (self.op, self.K, self.N, variant, limit)
        if expect:
            assert (wide, nh) == (1, expect), '%s: (wide, nh) = %s' % (what, (wide, nh))
            assert (items, grid) == wide_plan(self.T, self.N, nh, n_cu(hip), limit), '%s: items, grid = %s' % (what, (items, grid))
        else:
            assert (wide, nh) == (0, 0), '%s: (wide, nh) = %s' % (what, (wide, nh))
        hip.gemm(self.W16g, self.gtiles, self.N, self.K, **kw)
        torch.cuda.synchronize()
        out = []
        for buf, v, name in ((ybuf, Y, 'Y'), (pbuf, part, 'part')):
            if v is None:
                out.append(None)
                continue
            untouched(buf, v, '%s %s' % (what, name))
            assert not torch.isnan(v).any(), '%s: %d elements of %s not written' % (what, int(torch.isnan(v).sum()), name)
            out.append(v.cpu())
        return tuple(out)

    def bitwise(self, hip, knobs, limits=(), want_y=True, want_part=True, expect=(1, 2)):
        """variant 3, its repeat, variant 4 and variant 1, variants 3 and 4 under every grid limit as well: all bit-equal;
        -> the first result.  expect: NH reported under variants 3 and 4 (0: the tile kernel)"""
        first = self.launch(hip, knobs, 3, 0, expect[0], want_y, want_part)
        runs = [(3, 0, expect[0]), (4, 0, expect[1]), (1, 0, 0)] + [(v, l, e) for l in limits for v, e in ((3, expect[0]), (4, expect[1]))]
        for v, l, e in runs:
            got = self.launch(hip, knobs, v, l, e, want_y, want_part)
            for a, b, name in zip(first, got, ('Y', 'part')):
                assert a is None or torch.equal(a, b), '%s K%d N%d: %s under variant %d, limit %d differs from variant 3' % (
                    self.op, self.K, self.N, name, v, l)
        return first

    # ---- comparison ------------------------------------------------------------------------------------------------
    def judge(self, family, Y, part):
        """per group against float64, relative to the group's largest value: the project's tolerances"""
        Yr, pr = self.ref()
        errs = []
        for g in range(self.G):
            r0, r1 = int(self.c.h_g_row0[g]), int(self.c.h_g_row0[g] + self.c.h_g_count[g])
            t0, t1 = int(self.c.h_g_tile0[g]), int(self.c.h_g_tile0[g] + self.c.h_g_ntiles[g])
            for name, tol, got, ref in (('Y', TOL_Y, Y, Yr), ('sums', TOL_SUM, part, pr), ('M2', TOL_M2, part, pr)):
                if got is None:
                    continue
                sl = (slice(r0, r1),) if name == 'Y' else (slice(t0, t1), 0 if name == 'sums' else 1)
                top = max(ref[sl].abs().max().item(), 1e-6)
                err = (got[sl].double() - ref[sl]).abs().max().item() / top
                WORST[family, name] = max(WORST.get((family, name), 0.0), err)
                what = '%s %s K%d N%d group %d %s' % (family, self.op, self.K, self.N, g, name)
                try:
                    close(got[sl], ref[sl], tol, what)
                except AssertionError as e:
                    errs.append(str(e))
        assert not errs, '\n'.join(errs)


def report(family):
    for (f, name), err in sorted(WORST.items()):
        if f == family:
            print('worst %s %s: device %.3e' % (f, name, err))


# ---- (a) instantiations ---------------------------------------------------------------------------------------------
NORM_COUNTS = [300, 5, 128, 1, 33, 127]
PAIR_NM = [(5, 64), (3, 160), (1, 32), (7, 96)]


@functools.lru_cache(maxsize=None)
def small_case(op, K, bias):
    if op == NORM:
        return Case(op, K, 512, NORM_COUNTS, bias=bias, seed=400, mags=[1, 4, 0.5, 2, 8, 0.25])
    return Case(op, K, 512, PAIR_NM, bias=bias, seed=410, ldf=512)      # K = 256: ldf = K + 256, NaN behind the slice


@pytest.mark.parametrize('K', [256, 512])
@pytest.mark.parametrize('op', list(OPS))
def test_instantiations(hip, knobs, op, K):
    """all eight instantiations at K = 256 (16 steps, half the uniform-row DMAs) and K = 512, N = 512, one item per
    workgroup: Y and part, Y only, part only (Y = NULL) x bias, bias = NULL"""
    for bias in (True, False):
        c = small_case(op, K, bias)
        assert c.T == (8 if op == NORM else 14)
        for want_y, want_part in ((True, True), (True, False), (False, True)):
            Y, part = c.bitwise(hip, knobs, limits=(16,), want_y=want_y, want_part=want_part)
            c.judge(op, Y, part)
    # the helper's statement is fake_ops' own where nothing is clamped
    c = small_case(op, K, True)
    Y, part = torch.zeros(c.R, c.N, dtype=F64), torch.zeros(c.T, 2, c.N, dtype=F64)
    kw = dict(FA=c.FA.double(), FB=c.FB.double(), pair=c.pt_c, amode=2, pairop=c.pairop) if c.pair else \
        dict(X=c.X.double(), sc=c.sc.double(), sh=c.sh.double(), amode=1)
    TorchOps(F64).gemm(c.W16, c.c, c.N, K, bias=c.bias, Y=Y, part=part, w_hl16=True, oscale=c.osc, **kw)
    assert torch.equal(Y, c.ref()[0]) and torch.equal(part, c.ref()[1])
    report(op)


# ---- (b) chains under the grid limit -------------------------------------------------------------------------------
CHAIN_COUNTS = [128] * 9 + [300, 5, 1, 33, 127, 1000, 129, 640, 31, 2600]
CHAIN_MAGS = [2.0 ** ((5 * g) % 9 - 3) for g in range(len(CHAIN_COUNTS))]          # neighbours differ by 2^5 or 2^-4
CHAIN_NM = [(40, 32), (9, 160), (33, 64), (12, 96), (1, 32)]


def chains(tiles, N, nh, grid):
    """per workgroup the groups of the items it walks (both row tiles of an NH = 2 item): the item order of the kernel"""
    ntn = N // 256
    nitems = wide_plan(tiles.T, N, nh, 1 << 20)[0]
    out = []
    for b in range(grid):
        for half in range(nh):
            walk = []
            for it in range(b, nitems, grid):
                t = nh * ((it & 7) + 8 * (it // (8 * ntn))) + half
                walk.append(int(tiles.h_group[min(t, tiles.T - 1)]))
            out.append(walk)
    return out


def assert_chained(tiles, N, nh):
    walks = chains(tiles, N, nh, 8 * (N // 256))
    assert min(len(w) for w in walks) >= 3
    steps = [(a, b) for w in walks for a, b in zip(w, w[1:])]
    assert 2 * sum(a != b for a, b in steps) >= len(steps), 'fewer than half of the item -> successor steps change group'


@functools.lru_cache(maxsize=None)
def chain_case(op, K, N):
    if op == NORM:
        return Case(op, K, N, CHAIN_COUNTS, seed=420, mags=CHAIN_MAGS)
    return Case(op, K, N, CHAIN_NM, seed=430, ldf=512)


@pytest.mark.parametrize('N', [256, 512])
@pytest.mark.parametrize('K', [256, 512])
def test_chain_norm_relu(hip, knobs, K, N):
    """A_NORM_RELU items chained: the successor's scale / shift rows DMA'd into buffer ub ^ 1 belong to another group with
    another magnitude on most steps; T = 53 is odd (NH = 2: the last item's second tile is empty and reads tile T - 1)"""
    c = chain_case(NORM, K, N)
    assert c.T == 53 and c.G == 19
    for nh in (1, 2):
        assert_chained(c.c, N, nh)
        assert wide_plan(c.T, N, nh, n_cu(hip), 8 * (N // 256))[1] == 8 * (N // 256)
    Y, part = c.bitwise(hip, knobs, limits=(8 * (N // 256), 16 * (N // 256)))
    c.judge('chained ' + NORM, Y, part)
    report('chained ' + NORM)


@pytest.mark.parametrize('K', [256, 512])
@pytest.mark.parametrize('op', ['multiply', 'minus_abs', 'minus'])
def test_chain_pair(hip, knobs, op, K):
    """A_PAIR items chained, every pairop: 49 tiles (odd) of five groups with their own aoff / boff, FA and FB different
    tensors with NaN rows between the groups' rows, K = 256 inside ldf = 512, bias"""
    c = chain_case(op, K, 512)
    assert c.T == 49
    for nh in (1, 2):
        assert min(len(w) for w in chains(c.c, 512, nh, 16)) >= 3
    Y, part = c.bitwise(hip, knobs, limits=(16, 32))
    c.judge('chained ' + op, Y, part)
    report('chained ' + op)


@pytest.mark.parametrize('counts', [[77], [128] * 8 + [5], [128] * 3 + [640, 1, 128 * 7 + 1]], ids=['T1', 'T9', 'T17'])
def test_chain_padding_items(hip, knobs, counts):
    """T = 1: one tile and seven padding items per column tile, has_next = false on every workgroup's first item (NH = 2:
    an empty second tile).  T = 8 k + 1 under the limit: the last item of workgroup 0's chain is real, that of the
    seven others is padding (they prefetch tile T - 1 and must write nothing)"""
    for op in (NORM, 'minus_abs'):
        tiling = counts if op == NORM else [(max(c // 32, 1), 32) for c in counts[:-1]] + [(-(-counts[-1] // 32), 32)]
        c = Case(op, 256, 512, tiling, seed=440, mags=None if op != NORM else [2.0 ** g for g in range(len(counts))])
        assert c.T == {1: 1, 9: 9, 6: 17}[len(counts)]
        Y, part = c.bitwise(hip, knobs, limits=(16,))
        c.judge('chained ' + op, Y, part)


# ---- (c) tile_group = NULL -------------------------------------------------------------------------------------------
def test_without_a_tile_group(hip, knobs):
    """tile_group = NULL with one group: NORM_RELU reads scale / shift row 0; a PAIR launch without the table is refused"""
    c = Case(NORM, 512, 256, [300], seed=450, no_group=True)
    Y, part = c.bitwise(hip, knobs, limits=(8,))
    c.judge(NORM, Y, part)
    p = Case('multiply', 512, 256, [(3, 64)], seed=451, no_group=True)
    assert knobs[0](3) == 0
    Y = torch.zeros(p.R, p.N, device=DEV)
    einval(hip.gemm, p.W16g, p.gtiles, p.N, p.K, **p.kwargs(Y, None))
    einval(hip.gemm_choice, p.W16g, p.gtiles, p.N, p.K, **p.kwargs(Y, None))


# ---- (d) the clamp --------------------------------------------------------------------------------------------------
def plant_norm(sc, sh):
    sc[:, ::25] = 1.0e5                       # 4 % of the columns: relu(x * 1e5 + sh) > 65000 for x > 0.65


def plant_multiply(a, b):
    a[:, ::25] *= 400.0                       # a * b * 160000: beyond +-65000 for |a b| > 0.41
    b[:, ::25] *= 400.0


def plant_minus(a, b):
    b[:, ::25] *= 2.0e5                       # (a - b) / 2 ~ -1e5 b: below -65000 for b > 0.65


@pytest.mark.parametrize('op,plant', [(NORM, plant_norm), ('multiply', plant_multiply), ('minus', plant_minus)],
                         ids=[NORM, 'multiply', 'minus'])
def test_clamp(hip, knobs, op, plant):
    """A beyond MM_F16_CLAMP on a planted 0.1 % .. 5 % of the elements, next to rows past a ragged tile's end (top = 0)"""
    tiling = [130, 33, 300] if op == NORM else [(5, 32), (9, 96), (3, 160)]      # last tiles of 2, 33, 44 / 32, 96, 96 rows
    c = Case(op, 512, 512, tiling, seed=460, plant=plant)
    raw = c.operand(F64, clamp=False)
    over, under = (raw > CLAMP).double().mean().item(), (raw < -CLAMP).double().mean().item()
    print('%s: %.2f %% of A above +clamp, %.2f %% below -clamp' % (op, 100 * over, 100 * under))
    assert 1e-3 <= over + under <= 5e-2
    assert under > 1e-3 if op == 'minus' else over > 1e-3
    assert (c.operand(F64).abs().max().item() == CLAMP) and (c.c.h_nrows % 128 != 0).any()
    Y, part = c.bitwise(hip, knobs, limits=(16,))
    c.judge('clamped ' + op, Y, part)
    report('clamped ' + op)


# ---- (e) the automatic choice ----------------------------------------------------------------------------------------
def test_automatic_choice(hip, knobs):
    """variant 0, PAIR, N = 1024 (four column tiles), statistics only: the tile kernel below n_cu / 2 items, NH = 1 from
    there, NH = 2 from 24 n_cu items on; items = ((T + 1) / 2) * 4"""
    ncu = n_cu(hip)
    lo, hi = -(-(ncu // 2) // 4), -(-(24 * ncu) // 4)                # pairs of tiles at the two thresholds
    res = {}
    for T, nh in ((2 * lo - 2, 0), (2 * lo - 1, 1), (2 * hi - 2, 1), (2 * hi - 1, 2)):
        if T < 1:
            continue
        c = Case('multiply', 512, 1024, [(T, 128)], seed=470 + nh, bias=True)
        assert c.T == T
        _, part = c.launch(hip, knobs, 0, 0, nh, want_y=False)
        if T >= 2 * hi - 2:
            for v, e in ((1, 0), (3, 1), (4, 2)):
                assert torch.equal(c.launch(hip, knobs, v, 0, e, want_y=False)[1], part), 'T = %d: variant %d differs' % (T, v)
            sample = sorted({0, T - 1} | {(k * (T - 1)) // 7 for k in range(1, 7)})
            assert len(sample) == 8
            ref = c.statement(F64, sample)[1]
            close(part[sample, 0], ref[:, 0], TOL_SUM, 'automatic choice T = %d: tile sums' % T)
            close(part[sample, 1], ref[:, 1], TOL_M2, 'automatic choice T = %d: tile M2' % T)
        res[T] = nh
    assert sorted(set(res.values())) == [0, 1, 2]


# ---- (f) what the kernel must decline -----------------------------------------------------------------------------------
def _declined(hip, knobs, what, N, K, counts, ref_kw, dev_kw, pair=None, w_hl16=True, colsum=False):
    emu = TorchOps(F64)
    cpu, gpu = RowTiles(counts, 'cpu'), RowTiles(counts, DEV)
    W = rnd(N, K, seed=481, scale=K ** -0.5)
    if w_hl16:
        shift = hl16_weight_shift(W)
        W, osc = to_hl16(W.double() * 2.0 ** shift), 2.0 ** -shift
    else:
        osc = 1.0
    bias = rnd(N, seed=482)
    Y, part, cs = torch.zeros(cpu.R, N, dtype=F64), torch.zeros(cpu.T, 2, N, dtype=F64), torch.zeros(cpu.T, N, dtype=F64)
    if pair:
        ref_kw, dev_kw = dict(ref_kw, pair=pair('cpu', cpu)), dict(dev_kw, pair=pair(DEV, cpu))
    emu.gemm(W, cpu, N, K, bias=bias, Y=Y, part=part, colsum=cs if colsum else None, w_hl16=w_hl16, oscale=osc, **ref_kw)
    assert knobs[0](3) == 0
    ybuf, pbuf = torch.full((cpu.R + 2, N + 12), NAN, device=DEV), torch.full((cpu.T + 1, 2, N), NAN, device=DEV)
    Yg, pg = ybuf[1:cpu.R + 1, :N], pbuf[:cpu.T]
    csg = torch.full((cpu.T, N), NAN, device=DEV) if colsum else None
    kw = dict(bias=bias.to(DEV), Y=Yg, part=pg, colsum=csg, w_hl16=w_hl16, oscale=osc, **dev_kw)
    assert hip.gemm_choice(W.to(DEV), gpu, N, K, **kw)[:2] == (0, 0), '%s: not declined' % what
    hip.gemm(W.to(DEV), gpu, N, K, **kw)
    untouched(ybuf, Yg, what + ' Y')
    untouched(pbuf, pg, what + ' part')
    close(Yg, Y, TOL_Y, what + ' Y')
    close(pg[:, 0], part[:, 0], TOL_SUM, what + ' tile sums')
    close(pg[:, 1], part[:, 1], TOL_M2, what + ' tile M2')
    if colsum:
        close(csg, cs, TOL_SUM, what + ' column sums')


DECLINED = {
    'fp32-weights': dict(w_hl16=False), 'K128': dict(K=128), 'K384': dict(K=384), 'K1024': dict(K=1024), 'N128': dict(N=128),
    'N384': dict(N=384), 'plain': dict(amode=0), 'dbias': dict(dbias=True), 'colsum': dict(colsum=True), 'act': dict(act=1),
}


@pytest.mark.parametrize('name', list(DECLINED))
def test_declined(hip, knobs, name):
    """one fall-through condition at a time from an otherwise eligible NORM_RELU layer: the choice under variant 3 says
    tile kernel, and the tile kernel's result matches float64"""
    d = dict(dict(N=256, K=512, amode=1, w_hl16=True, dbias=False, colsum=False, act=0), **DECLINED[name])
    counts = [130, 33]
    R, K, N = sum(counts), d['K'], d['N']
    X, sc, sh = rnd(R, K, seed=483), rnd(2, K, seed=484).abs() + 0.5, rnd(2, K, seed=485)
    ref_kw, dev_kw = dict(X=X, amode=d['amode'], act=d['act']), dict(X=nan_slice(X, 64), amode=d['amode'], act=d['act'])
    if d['amode'] == 1:
        ref_kw.update(sc=sc, sh=sh)
        dev_kw.update(sc=nan_slice(sc, 12, 0, 0), sh=nan_slice(sh, 12, 0, 0))
    if d['dbias']:
        db, idx = rnd(5, N, seed=486), (torch.arange(R) * 5 // R).int()
        ref_kw.update(dbias=db, rowidx=idx)
        dev_kw.update(dbias=db.to(DEV), rowidx=idx.to(DEV))
    if d['colsum']:
        osc, osh = rnd(2, N, seed=487).abs() + 0.5, rnd(2, N, seed=488)
        ref_kw.update(osc=osc, osh=osh)
        dev_kw.update(osc=osc.to(DEV), osh=osh.to(DEV))
    _declined(hip, knobs, name, N, K, counts, ref_kw, dev_kw, w_hl16=d['w_hl16'], colsum=d['colsum'])


@pytest.mark.parametrize('NM', [[(5, 64), (3, 32)], [(5, 7), (130, 3)]], ids=['aligned', 'ragged'])
def test_declined_without_the_uniform_rows_guarantee(hip, knobs, NM):
    """pair_uniform32 = 0: the tile kernel, on tiles that would have qualified and on ragged ones"""
    K, N = 512, 256
    Fm = rnd(sum(n + m for n, m in NM) + 2, K, seed=489)
    aoff, boff, o = [], [], 1
    for n, m in NM:
        aoff.append(o)
        boff.append(o + n)
        o += n + m
    pair = lambda dev, tl: dict(row0=torch.tensor(tl.h_g_row0).to(dev), M=torch.tensor([m for _, m in NM], dtype=torch.int32).to(dev),
                                aoff=torch.tensor(aoff, dtype=torch.int32).to(dev),
                                boff=torch.tensor(boff, dtype=torch.int32).to(dev), uniform32=False)
    Fg = Fm.to(DEV)
    _declined(hip, knobs, 'pair_uniform32 = 0', N, K, [n * m for n, m in NM], dict(FA=Fm, FB=Fm, amode=2, pairop=1),
              dict(FA=Fg, FB=Fg, amode=2, pairop=1), pair=pair)


def test_refused_strides_and_knob_values(hip, knobs):
    """ldf % 4 and ldy % 4 with Y never reach the choice: mmmot_gemm_rows and mmmot_gemm_rows_choice refuse them alike;
    the grid limit refuses negative values and leaves the choice of kernel alone"""
    c = Case('minus', 256, 256, [(2, 32)], seed=490)
    Y = torch.zeros(c.R, c.N + 2, device=DEV)[:, :c.N]                # ldy = N + 2
    for fn in (hip.gemm, hip.gemm_choice):
        einval(fn, c.W16g, c.g, c.N, c.K, **c.kwargs(Y, None))
    kw = c.kwargs(None, torch.zeros(c.T, 2, c.N, device=DEV))
    kw['FA'] = torch.zeros(c.FA.shape[0], c.K + 2, device=DEV)[:, :c.K]      # ldf = K + 2
    for fn in (hip.gemm, hip.gemm_choice):
        einval(fn, c.W16g, c.g, c.N, c.K, **kw)
    assert knobs[1](-1) == -1 and knobs[1](0) == 0
    assert hip.lib.mmmot_gemm_rows_choice(None, None, None, None, None) == -1
    a = hip._gemm_args(c.W16g, c.g, c.N, c.K, *[None] * 5, torch.zeros(c.T, 2, c.N, device=DEV), None, None, c.FAg, c.FBg, c.pt_g,
                       2, 2, 0, True, c.osc, None, None, None)
    assert knobs[0](3) == 0
    assert hip.lib.mmmot_gemm_rows_choice(ctypes.byref(a), None, None, None, None) == 0        # every pointer may be NULL
    for limit in (0, 1, 8, 1000):
        assert knobs[1](limit) == 0
        assert hip.gemm_choice(c.W16g, c.g, c.N, c.K, **c.kwargs(None, torch.zeros(c.T, 2, c.N, device=DEV))) == (1, 1, 8, 8)
