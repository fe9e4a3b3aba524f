"""Every launch branch of the image trunk's kernels (csrc/conv3x3_hl16_patch.hip with its patch_*.inc parts, csrc/conv3x3.hip)
against the float64 specification in tests/fake_ops.py: TorchOps(torch.float64).conv3x3 on the decoded hl16 operands,
.conv3x3_raw for the raw (training) launch, ._conv_hq8 - the statement of the hq8 arithmetic - for the hq8 launch, the
float64 two-layer computation for the fused first launches.

Conventions:
* every case first asks mmmot_patch_choice which instantiation the launch it is about to make would run, and asserts the
  branch it names (tile width forced with mmmot_set_patch_tile_width; the block edge follows from the map);
* the output is a 16-byte-aligned slice of a larger NaN buffer (not 32-byte aligned): the guards before and behind it
  keep their bytes, and every element between them is written;
* the input lies between guards of NaN bit patterns of its format (fp16 NaNs, e4m3 NaNs, fp32 NaNs, bytes of 255); the
  second launch of every case has other guards (the largest finite values) and must give the same bytes;
* a counter block is bound around the launches of a case and reads (0, 0, 0, 0) afterwards (raw launches: it keeps the
  sentinel it held); activations and weights are sized so that no output comes near 1792;
* knobs are set through `knobs` and restored in its `finally`.

Shapes, Cout = 256 (two 128-channel or four 64-channel tiles), Cin = 32 (one slab: every slab is a transition slab) and
96 (odd slab count: the patch buffers swap roles):
  block edge 16  L = 2, 20 x 12 (pooled: 21 x 13 -> 10 x 6)   partial blocks on both axes; the pool drops a row and a column
  block edge 8   L = 5, 7 x 8 (pooled -> 3 x 4)                four blocks per tile: tiles straddle crops, ragged last tile
  block edge 4   L = 19, 3 x 4 (pooled -> 1 x 2)               16 maps per tile, ragged second tile, unused pixel slots
  chained        L = 12 / 47 / 179 of the same maps: 48 / 24 / 24 tiles of 128 channels on 8 workgroups

Case -> branch (the choice is one function, mmmot_patch_choose of csrc/patch_choice.h; tests/test_patch_choice_cpu.py pins
it without a GPU).  conv3x3_hl16_patch_kernel<BN, BS, POOL, FUSE1, Q8, RAW>:
  <64 | 128, 16 | 8 | 4, 0 | 1>                  test_patch_matrix[hl16-bn*-bs*-pool*-cin*]    12 instantiations x 2 Cin
  <64 | 128, 16 | 8 | 4, 0, 0, 0, RAW>           test_patch_matrix[raw-bn*-bs*-pool0-cin*]      6 instantiations x 2 Cin
  <64 | 128, 16 | 8 | 4, 0 | 1, 0, Q8>           test_patch_matrix[hq8-bn*-bs*-pool*-cin*]     12 instantiations x 2 Cin
  the same 30 with >= 3 tiles per workgroup      test_patch_chained[kind-bs*-pool*] (128-channel tiles, and 64 for bit-equality)
  per-channel scales on <128, 8> and <128, 4>    test_patch_per_channel_scales[bs8], [bs4]
  raw output above 1e6, negative values          test_raw_is_unclamped[bn*-bs*]
  range guard, exact counts                      test_range_guard_counts[kind-bs*-pool*], test_range_guard_unbound
  <64, 16, 1, FUSE1> from fp32 crops             test_conv1_fused[hl16-HxW], from bytes: [u8-HxW]
  <64, 16, 1, FUSE1, Q8> from fp32 crops         test_conv1_fused[hq8-HxW], from bytes: [u8q8-HxW]
  conv1_1 range counter of the fused launches    test_conv1_fused_range_counter[hl16 | hq8 | u8 | u8q8]
conv3x3_kernel<BN, FIRST, POOL, OUT16, RAW> (no dispatcher but Cout % 128, first, pool):
  <64 | 128, 0 | 1, 0 | 1>                       test_tile_kernel[bn_relu-bn*-first*-pool*]     8 instantiations
  <64 | 128, 0 | 1, 0, 0, RAW>                   test_tile_kernel[raw-bn*-first*-pool0]         4 instantiations
  <64 | 128, 1, 0, OUT16>                        test_tile_kernel[first_hl16-bn*-first1-pool0]  2 instantiations
Refused calls (MMMOT_EINVAL, nothing launched):  test_launchers_refuse, test_knobs_refuse

Bounds, as a fraction of the reference's maximum (test_kernels_gpu.close), are the project's for the same arithmetic at
K <= 9 x 512 (no case here is longer): hl16 2e-6 (tests/test_conv_patch_gpu.py), raw 3e-6 (tests/test_train_vgg_gpu.py), hq8
ENC_TOL = 1.3e-4 against the statement (tests/test_hq8_gpu.py), fp32 tile kernel 3e-6 (tests/test_kernels_gpu.py), fused first
launch 3e-6 / 2.5e-4 for hq8 (tests/test_conv_patch_gpu.py, tests/test_hq8_gpu.py), per-channel scales 4e-6 of the channel's
maximum + 2^-24.  Measured on an MI355X (worst case of each arithmetic, printed by the tests):
  hl16 9.98e-7   raw 7.42e-7   hq8 1.11e-5   fp32 9.09e-7   fused hl16 7.31e-7   fused hq8 2.37e-5
  per-channel scales: 7.4e-5 of the smallest channel's maximum (4e-4: the 2^-24 quantum of the hl16 output format)
  raw lifted above 1e6: 6.96e-7 of the channel's maximum; conv1_1 range counter: 687 (tile, lane) pairs, both forms
"""
import contextlib
import ctypes
import functools

import pytest
import torch

from common import normalise_u8, u8_image
from fake_ops import TorchOps
from mmmot_amd import _lib
from mmmot_amd.crops import MEAN, STD
from mmmot_amd.pack import (conv1_weight_shift, from_hl16, from_hq8_act, hl16_channel_shifts, hl16_weight_shift, hq8_parts,
                            to_hl16, to_hq8_act, to_hq8_w)
from test_hq8_gpu import ENC_TOL
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu

EINVAL = -1
COUT = 256
GUARD = 4096                      # words on either side of a guarded operand (16 KB)
NAN32 = 0x7fc00000                # what torch.full(float('nan')) holds
IN_GUARDS = {                     # format: (NaN pattern, largest finite pattern) as int32 words
    'hl16': (0x7e007e00, 0x7bff7bff),                    # fp16 NaN / 65504 in both halves
    'hq8': (0x7e7f7e7f, 0x7b7e7b7e),                     # fp16 NaN = e4m3 bytes 0x7e (448), 0x7f (NaN) / finite in both readings
    'f32': (NAN32, 0x7f7fffff),
    'u8': (-1, 0x7f7f7f7f),
}
SHAPES = {  # block edge: (L, H, W) unpooled, (L, H, W) pooled, L of the chained shape
    16: ((2, 20, 12), (2, 21, 13), 12),
    8: ((5, 7, 8), (5, 7, 8), 47),
    4: ((19, 3, 4), (19, 3, 4), 179),
}
WORST = {}


def note(what, got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    e = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
    WORST[what] = max(WORST.get(what, 0.0), e)
    print('%s: error / max|ref| %.2e (worst so far %.2e)' % (what, e, WORST[what]))


@contextlib.contextmanager
def knobs(width=0, limit=0, min_block=0):
    lib = _lib.load()
    try:
        assert lib.mmmot_set_patch_tile_width(width) == 0
        assert lib.mmmot_set_patch_grid_limit(limit) == 0
        assert lib.mmmot_set_patch_min_block(min_block) == 0
        yield
    finally:
        lib.mmmot_set_patch_tile_width(0)
        lib.mmmot_set_patch_grid_limit(0)
        lib.mmmot_set_patch_min_block(0)


@contextlib.contextmanager
def bound(hip, fill=0):
    c = torch.full((4,), fill, dtype=torch.int32).cuda()
    hip.trunk_range_bind(c)
    try:
        yield c
    finally:
        hip.trunk_range_bind(None)


def bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.int32)


def guarded_in(t, pattern):
    """device copy of `t` (4-byte or 1-byte elements) between GUARD words of `pattern`, 16 bytes past a 32-byte boundary"""
    raw = t.contiguous().view(-1).view(torch.uint8)
    lead, n = (GUARD + 4) * 4, raw.numel()
    buf = torch.full((2 * GUARD + 4 + (n + 15) // 16 * 4,), pattern, dtype=torch.int32).view(torch.uint8)
    buf[lead:lead + n] = raw
    dev = buf.cuda()
    view = dev[lead:lead + n].view(t.dtype).view(t.shape)
    assert view.data_ptr() % 32 == 16
    return view, dev


class Out:
    """[rows][cols] fp32-typed output between NaN guards: a 16-byte-aligned (not 32) slice of a larger buffer"""

    def __init__(self, rows, cols):
        self.n = rows * cols
        self.buf = torch.full((2 * GUARD + 4 + self.n,), float('nan')).cuda()
        self.view = self.buf[GUARD + 4:GUARD + 4 + self.n].view(rows, cols)
        assert self.view.data_ptr() % 32 == 16

    def check(self, what):
        b = bits(self.buf)
        assert bool((b[:GUARD + 4] == NAN32).all()) and bool((b[GUARD + 4 + self.n:] == NAN32).all()), \
            '%s: the guards around the output changed' % what
        return b[GUARD + 4:GUARD + 4 + self.n].clone()

    def untouched(self):
        return bool((bits(self.buf) == NAN32).all())


def choice(hip, L, H, W, bn, bs, grid=None, min_items=0):
    got = hip.patch_choice(L, H, W, COUT)
    assert got[:2] == (bn, bs), 'the launch would run <%d, %d>, the case names <%d, %d>' % (got[0], got[1], bn, bs)
    assert grid is None or got[3] == grid, got
    assert got[2] >= min_items, got
    return got


# ---- operands and float64 references, shared between the cases of a shape ---------------------------------------------
@functools.lru_cache(maxsize=None)
def patch_case(kind, L, H, W, Cin, pool, seed=800):
    """-> (x records, w records, bias, oscale scalar, float64 reference [rows][COUT]) on the host"""
    x = rnd(L * H * W, Cin, seed=seed) * 3.0
    if kind != 'raw':
        x = torch.relu(x)
    w = rnd(9, COUT, Cin, seed=seed + 1, scale=(2.0 / (9 * Cin)) ** 0.5)
    bias = rnd(COUT, seed=seed + 2, scale=0.1)
    shift = hl16_weight_shift(w)
    emu = TorchOps(torch.float64)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    if kind == 'hq8':
        xr, wr = to_hq8_act(x), to_hq8_w(w.double() * 2.0 ** shift)
        ref = emu._conv_hq8(hq8_parts(xr), wr, bias, L, H, W, Cin, COUT, bool(pool), 2.0 ** -shift)
    else:
        xr, wr = to_hl16(x), to_hl16(w.double() * 2.0 ** shift)
        ref = torch.zeros(L * Ho * Wo, COUT, dtype=torch.float64)
        xd, wd = from_hl16(xr).view(L, H, W, Cin), from_hl16(wr).double() * 2.0 ** -shift
        if kind == 'raw':
            emu.conv3x3_raw(xd, wd, bias, ref, L, H, W, Cin, COUT, False)
        else:
            emu.conv3x3(xd, wd, bias, ref, L, H, W, Cin, COUT, False, bool(pool))
    assert float(ref.abs().max()) < 100.0  # far from 1792 and 65000: the range guard has nothing to count
    return xr, wr, bias, 2.0 ** -shift, ref


def launch(hip, kind, x, w, bias, out, L, H, W, Cin, pool, osc):
    if kind == 'hl16':
        hip.conv3x3_hl16_patch(x, w, bias, out, L, H, W, Cin, COUT, bool(pool), osc)
    elif kind == 'hq8':
        hip.conv3x3_hq8(x, w, bias, out, L, H, W, Cin, COUT, bool(pool), osc)
    else:
        hip.conv3x3_raw_hl16(x, w, bias, out, L, H, W, Cin, COUT, osc)


def decode(hip, kind, view):
    if kind == 'raw':
        return view.clone()
    dec = torch.zeros_like(view)
    (hip.hq8_unpack if kind == 'hq8' else hip.hl16_unpack)(view.contiguous(), dec)
    return dec


BOUND = {'hl16': 2e-6, 'raw': 3e-6, 'hq8': ENC_TOL}


def run_patch(hip, kind, L, H, W, Cin, pool, bn, bs, limit=0, min_block=0, pattern=0, min_items=0, what=''):
    """one guarded launch under the knobs -> (output bytes, decoded output)"""
    xr, wr, bias, osc, _ = patch_case(kind, L, H, W, Cin, pool)
    x, xbuf = guarded_in(xr, IN_GUARDS['hq8' if kind == 'hq8' else 'hl16'][pattern])
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = Out(L * Ho * Wo, COUT)
    oscv = torch.full((COUT,), osc).cuda()
    sentinel = 77 if kind == 'raw' else 0
    with knobs(width=bn, limit=limit, min_block=min_block), bound(hip, sentinel) as counters:
        choice(hip, L, H, W, bn, bs, grid=8 if limit else None, min_items=min_items)
        launch(hip, kind, x, wr.cuda(), bias.cuda(), out.view, L, H, W, Cin, pool, oscv)
        torch.cuda.synchronize()
        assert counters.tolist() == [sentinel] * 4, '%s: range counters %s' % (what, counters.tolist())
    return out.check(what), decode(hip, kind, out.view)


MATRIX = [(kind, bn, bs, pool, cin) for kind in ('hl16', 'raw', 'hq8') for bn in (64, 128) for bs in (16, 8, 4)
          for pool in ((0,) if kind == 'raw' else (0, 1)) for cin in (32, 96)]


@pytest.mark.parametrize('kind,bn,bs,pool,cin', MATRIX, ids=['%s-bn%d-bs%d-pool%d-cin%d' % c for c in MATRIX])
def test_patch_matrix(hip, kind, bn, bs, pool, cin):
    L, H, W = SHAPES[bs][1 if pool else 0][:3]
    what = '%s <%d, %d, %d> Cin %d' % (kind, bn, bs, pool, cin)
    ref = patch_case(kind, L, H, W, cin, pool)[4]
    got, dec = run_patch(hip, kind, L, H, W, cin, pool, bn, bs, what=what)
    note(kind, dec, ref)
    close(dec, ref, BOUND[kind], what + ' vs float64')
    if kind == 'raw':
        assert bool((dec < 0).any()), 'raw output: no ReLU'
    # again, between other input guards: the same bytes
    again, _ = run_patch(hip, kind, L, H, W, cin, pool, bn, bs, pattern=1, what=what)
    assert torch.equal(got, again), what + ': a second launch (other input guards) gives other bytes'
    other, _ = run_patch(hip, kind, L, H, W, cin, pool, 192 - bn, bs, what=what)
    assert torch.equal(got, other), what + ': %d- and %d-channel tiles differ' % (bn, 192 - bn)
    capped, _ = run_patch(hip, kind, L, H, W, cin, pool, bn, bs, limit=8, what=what)
    assert torch.equal(got, capped), what + ': grid limit 8 and 0 differ'
    if bs == 4:
        haloed, _ = run_patch(hip, kind, L, H, W, cin, pool, bn, 8, min_block=8, what=what)
        assert torch.equal(got, haloed), what + ': whole-map and haloed 8 x 8 geometry differ'


CHAINED = [(kind, bs, pool) for kind in ('hl16', 'raw', 'hq8') for bs in (16, 8, 4) for pool in ((0,) if kind == 'raw' else (0, 1))]


@pytest.mark.parametrize('kind,bs,pool', CHAINED, ids=['%s-bs%d-pool%d' % c for c in CHAINED])
def test_patch_chained(hip, kind, bs, pool):
    """at least three 128-channel tiles per workgroup (grid capped at 8): the successor's first slab and weight stages
    stream in during the last slab; Cin = 96, so the two patch buffers swap roles from tile to tile"""
    (_, H, W), L = SHAPES[bs][1 if pool else 0], SHAPES[bs][2]
    what = '%s chained <128, %d, %d>' % (kind, bs, pool)
    ref = patch_case(kind, L, H, W, 96, pool)[4]
    got, dec = run_patch(hip, kind, L, H, W, 96, pool, 128, bs, limit=8, min_items=24, what=what)
    note(kind, dec, ref)
    close(dec, ref, BOUND[kind], what + ' vs float64')
    again, _ = run_patch(hip, kind, L, H, W, 96, pool, 128, bs, limit=8, pattern=1, min_items=24, what=what)
    assert torch.equal(got, again), what + ': a second launch gives other bytes'
    free, _ = run_patch(hip, kind, L, H, W, 96, pool, 128, bs, what=what)
    assert torch.equal(got, free), what + ': grid limit 8 and 0 differ'
    narrow, _ = run_patch(hip, kind, L, H, W, 96, pool, 64, bs, limit=8, min_items=48, what=what)
    assert torch.equal(got, narrow), what + ': 64- and 128-channel tiles differ'
    if bs == 4:
        haloed, _ = run_patch(hip, kind, L, H, W, 96, pool, 128, 8, limit=8, min_block=8, what=what)
        assert torch.equal(got, haloed), what + ': whole-map and haloed 8 x 8 geometry differ'


@pytest.mark.parametrize('bs', [8, 4])
def test_patch_per_channel_scales(hip, bs):
    """gains spread over 1e6 with one power-of-two weight scale per output channel (pack.hl16_channel_shifts), on the
    128-channel tiles of the small-map geometries; the bound of test_conv3x3_hl16_patch_per_channel_scales"""
    (L, H, W), Cin = SHAPES[bs][0], 96
    g = torch.Generator().manual_seed(79)
    gain = torch.pow(10.0, torch.rand(COUT, generator=g) * 6.0 - 4.0).double()
    x = torch.relu(rnd(L * H * W, Cin, seed=820)) * 3.0
    w = rnd(9, COUT, Cin, seed=821, scale=(2.0 / (9 * Cin)) ** 0.5).double() * gain.view(1, -1, 1)
    bias = (rnd(COUT, seed=822, scale=0.1).double() * gain).float()
    shifts = hl16_channel_shifts(w)
    assert int(shifts.max() - shifts.min()) >= 15
    w16, x16 = to_hl16(w * torch.pow(2.0, shifts.double()).view(1, -1, 1)), to_hl16(x)
    osc = torch.pow(2.0, -shifts.double()).float()
    ref = torch.zeros(L * H * W, COUT, dtype=torch.float64)
    TorchOps(torch.float64).conv3x3(from_hl16(x16).view(L, H, W, Cin), from_hl16(w16).double() * osc.double().view(1, -1, 1),
                                    bias, ref, L, H, W, Cin, COUT, False, False)
    xin, xbuf = guarded_in(x16, IN_GUARDS['hl16'][0])
    out = Out(L * H * W, COUT)
    with knobs(width=128), bound(hip) as counters:
        choice(hip, L, H, W, 128, bs)
        hip.conv3x3_hl16_patch(xin, w16.cuda(), bias.cuda(), out.view, L, H, W, Cin, COUT, False, osc.cuda())
        torch.cuda.synchronize()
        assert counters.tolist() == [0, 0, 0, 0]
    out.check('per-channel scales')
    dec = decode(hip, 'hl16', out.view).cpu().double()
    assert torch.isfinite(dec).all()
    err, chmax = (dec - ref).abs().amax(dim=0), ref.abs().amax(dim=0)
    print('per-channel scales <128, %d>: worst per-channel relative error %.2e (output maxima %.1e .. %.1e)' % (
        bs, (err / chmax.clamp_min(1e-30)).max().item(), chmax.min().item(), chmax.max().item()))
    assert (err <= 4e-6 * chmax + 2.0 ** -24).all()


@pytest.mark.parametrize('bs', [16, 8, 4])
@pytest.mark.parametrize('bn', [64, 128])
def test_raw_is_unclamped(hip, bn, bs):
    """the raw launch has no ReLU, no clamp at 65000 and no range guard: a per-channel oscale lifts every third channel
    by 2^22 (outputs above 1e6), each channel within 3e-6 of its own maximum, the bound counter block untouched"""
    (L, H, W), Cin = SHAPES[bs][0], 32
    xr, wr, bias, osc, _ = patch_case('raw', L, H, W, Cin, 0)
    lift = torch.ones(COUT, dtype=torch.float64)
    lift[::3] = 2.0 ** 22
    ref = torch.zeros(L * H * W, COUT, dtype=torch.float64)
    TorchOps(torch.float64).conv3x3_raw(from_hl16(xr).view(L, H, W, Cin), from_hl16(wr).double() * (osc * lift).view(1, -1, 1),
                                        bias, ref, L, H, W, Cin, COUT, False)
    chmax = ref.abs().amax(dim=0)
    assert bool((chmax[::3] > 1e6).all()) and bool((ref < -65000.0).any()) and bool((ref > 65000.0).any())
    x, xbuf = guarded_in(xr, IN_GUARDS['hl16'][0])
    out = Out(L * H * W, COUT)
    with knobs(width=bn), bound(hip, 77) as counters:
        choice(hip, L, H, W, bn, bs)
        hip.conv3x3_raw_hl16(x, wr.cuda(), bias.cuda(), out.view, L, H, W, Cin, COUT, (osc * lift).float().cuda())
        torch.cuda.synchronize()
        assert counters.tolist() == [77] * 4, 'a raw launch touched the range counters'
    out.check('raw, lifted channels')
    got = out.view.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().amax(dim=0)
    print('raw <%d, %d> lifted: worst per-channel error / channel maximum %.2e' % (bn, bs, (err / chmax).max().item()))
    assert (err <= 3e-6 * chmax).all()
    assert bool((got < 0).any())


# ---- range guard: exact counts ------------------------------------------------------------------------------------------
HOT, WARM = (3, 64, 127, 130, 255), (7, 65, 200)    # output channels planted at 70000 / (hq8) at 2000


@functools.lru_cache(maxsize=None)
def guard_case(kind, L, H, W, pool):
    Cin = 32
    x = torch.relu(rnd(L * H * W, Cin, seed=840)) * 3.0
    w = rnd(9, COUT, Cin, seed=841, scale=(2.0 / (9 * Cin)) ** 0.5)
    bias = rnd(COUT, seed=842, scale=0.1)
    w[:, list(HOT), :] = 0.0
    bias[list(HOT)] = 70000.0
    if kind == 'hq8':
        w[:, list(WARM), :] = 0.0
        bias[list(WARM)] = 2000.0
    shift = hl16_weight_shift(w)
    emu = TorchOps(torch.float64)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    if kind == 'hq8':
        xr, wr = to_hq8_act(x), to_hq8_w(w.double() * 2.0 ** shift)
        ref = emu._conv_hq8(hq8_parts(xr), wr, bias, L, H, W, Cin, COUT, bool(pool), 2.0 ** -shift)
    else:
        xr, wr = to_hl16(x), to_hl16(w.double() * 2.0 ** shift)
        ref = torch.zeros(L * Ho * Wo, COUT, dtype=torch.float64)
        emu.conv3x3(from_hl16(xr).view(L, H, W, Cin), from_hl16(wr).double() * 2.0 ** -shift, bias, ref, L, H, W, Cin, COUT, False,
                    bool(pool))
    # no computed output within 10 % of a limit: float32 and float64 count the same elements.  The planted channels are
    # no computed outputs - zero weights, so 70000 (7.7 % above 65000) and 2000 are exact in every arithmetic
    cold = [n for n in range(COUT) if n not in HOT + (WARM if kind == 'hq8' else ())]
    for lim in (1792.0, 65000.0):
        assert not bool(((ref[:, cold] > 0.9 * lim) & (ref[:, cold] < 1.1 * lim)).any())
    assert float(ref[:, cold].max()) < 100.0
    assert bool((ref[:, list(HOT)] == 70000.0).all()) and (kind != 'hq8' or bool((ref[:, list(WARM)] == 2000.0).all()))
    emu._guard(ref, kind == 'hq8')
    want = tuple(emu.range)
    rows = L * Ho * Wo
    assert want == ((len(HOT) + len(WARM)) * rows if kind == 'hq8' else 0, len(HOT) * rows, 0, 0)
    return xr, wr, bias, 2.0 ** -shift, ref, want, cold


def check_planted(kind, out_bits, rows):
    """the clamped (70000 -> 65000) and, hq8, the e4m3-saturated (2000) outputs carry the host encoder's bytes"""
    raw = out_bits.view(torch.uint8)
    if kind == 'hq8':
        rec = raw.view(rows, COUT // 32, 128)
        for chans, value in ((HOT, 70000.0), (WARM, 2000.0)):
            want = to_hq8_act(torch.full((1, 32), value)).view(torch.uint8).view(128)
            for n in chans:
                c = n % 32
                for sl in (slice(2 * c, 2 * c + 2), slice(64 + c, 65 + c), slice(96 + c, 97 + c)):
                    assert bool((rec[:, n // 32, sl] == want[sl]).all()), 'hq8 bytes of planted channel %d' % n
    else:
        unit = raw.view(torch.int16).view(rows, COUT // 8, 2, 8)
        want = to_hl16(torch.full((1, 8), 65000.0)).view(torch.int16).view(2, 8)
        for n in HOT:
            assert bool((unit[:, n // 8, :, n % 8] == want[:, 0]).all()), 'hl16 bytes of clamped channel %d' % n


GUARDED = [(kind, bs, pool) for kind in ('hl16', 'hq8') for bs in (16, 8, 4) for pool in (0, 1)]


@pytest.mark.parametrize('kind,bs,pool', GUARDED, ids=['%s-bs%d-pool%d' % c for c in GUARDED])
def test_range_guard_counts(hip, kind, bs, pool):
    """counters [0] (hq8: elements above 1792) and [1] (elements above 65000) equal TorchOps._guard's counts of output
    elements - of POOLED elements on a pooled layer, no padding pixel of a partial block or ragged tile among them -
    whatever the tile width and the chaining: the chained shapes, one workgroup per tile (limit 0) and at least three
    tiles per workgroup (limit 8)"""
    (_, H, W), L = SHAPES[bs][1 if pool else 0], SHAPES[bs][2]
    xr, wr, bias, osc, ref, want, cold = guard_case(kind, L, H, W, pool)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    rows = L * Ho * Wo
    x, xbuf = guarded_in(xr, IN_GUARDS[kind][0])
    first = None
    for bn in (64, 128):
        for limit in (0, 8):
            out = Out(rows, COUT)
            with knobs(width=bn, limit=limit), bound(hip) as counters:
                items, grid = choice(hip, L, H, W, bn, bs, grid=8 if limit else None, min_items=24)[2:]
                whole = hip.patch_choice(1 << 16, 16, 16, 64)[3]   # the device's full grid: 256 workgroups on an MI355X
                assert limit or grid == min((items + 7) // 8 * 8, whole)   # unchained there: a workgroup per tile
                launch(hip, kind, x, wr.cuda(), bias.cuda(), out.view, L, H, W, 32, pool, osc)
                torch.cuda.synchronize()
                got = tuple(counters.tolist())
            what = '%s <%d, %d, %d> limit %d' % (kind, bn, bs, pool, limit)
            assert got == want, '%s: counters %s, TorchOps._guard counts %s' % (what, got, want)
            b = out.check(what)
            check_planted(kind, b, rows)
            dec = decode(hip, kind, out.view)
            close(dec[:, cold], ref[:, cold], BOUND[kind], what + ' (channels in range) vs float64')
            first = b if first is None else first
            assert torch.equal(first, b), what + ': bytes differ from the first launch'


def test_range_guard_unbound(hip):
    """without a bound block the launches report to the library's per-device block (trunk_range_read)"""
    kind, bs, pool = 'hq8', 8, 1
    L, H, W = SHAPES[bs][1]
    xr, wr, bias, osc, ref, want, cold = guard_case(kind, L, H, W, pool)
    out = Out(L * (H // 2) * (W // 2), COUT)
    hip.trunk_range_bind(None)
    hip.trunk_range_read('cuda', reset=True)
    assert hip.trunk_range_read('cuda', reset=False) == (0, 0, 0, 0)
    launch(hip, kind, xr.cuda(), wr.cuda(), bias.cuda(), out.view, L, H, W, 32, pool, osc)
    assert hip.trunk_range_read('cuda', reset=True) == want
    assert hip.trunk_range_read('cuda', reset=True) == (0, 0, 0, 0)
    out.check('unbound')


# ---- fused first launch: conv1_1 + conv1_2 + pool ----------------------------------------------------------------------
FUSED = ['hl16', 'hq8', 'u8', 'u8q8']
MAPS = [(2, 2), (2, 36), (36, 2), (18, 18)]   # one pixel row / column; one pixel past a block plus halo (16 + 1 + 1)


@functools.lru_cache(maxsize=None)
def fused_case(entry, H, W, plant=0.0):
    """-> (crops as launched, fp32 crops, launch arguments on the host, reference rows (decoded), q8)"""
    L, q8, from_u8 = 3, entry in ('hq8', 'u8q8'), entry.startswith('u8')
    if from_u8:
        u8 = u8_image(L, H, W, seed=860 + H * W)
        crops = normalise_u8(u8)
    else:
        crops = rnd(L, 3, H, W, seed=860 + H * W) * 1.5
    w1 = rnd(64, 3, 3, 3, seed=861, scale=(2.0 / 27) ** 0.5)
    b1 = rnd(64, seed=862, scale=0.1)
    if plant:
        b1[5] = plant
    w2 = rnd(9, 64, 64, seed=863, scale=(2.0 / 576) ** 0.5)
    b2 = rnd(64, seed=864, scale=0.1)
    w1p = torch.zeros(64, 32)
    w1p[:, :27] = w1.permute(0, 2, 3, 1).reshape(64, 27)
    s1, s2 = conv1_weight_shift(w1p, b1), hl16_weight_shift(w2)
    w1h = to_hl16(w1p.double() * 2.0 ** s1)
    w2d = to_hq8_w(w2.double() * 2.0 ** s2) if q8 else to_hl16(w2.double() * 2.0 ** s2)
    rows = L * (H // 2) * (W // 2)
    ref = None
    if not plant and q8:
        want = torch.zeros(rows, 64)
        TorchOps(torch.float64).conv1_fused_hq8(crops, w1h, b1, 2.0 ** -s1, w2d, b2, 2.0 ** -s2, want, L, H, W)
        ref = from_hq8_act(want)
    elif not plant:  # the float64 two-layer computation from the same (hl16-rounded) weights
        w1r = (from_hl16(w1h) * 2.0 ** -s1)[:, :27].view(64, 3, 3, 3).permute(0, 3, 1, 2).double()
        w2r = (from_hl16(w2d.reshape(9 * 64, 64)) * 2.0 ** -s2).view(3, 3, 64, 64).permute(2, 3, 0, 1).double()
        y = torch.relu(torch.nn.functional.conv2d(crops.double(), w1r, b1.double(), padding=1))
        y = torch.relu(torch.nn.functional.conv2d(y, w2r, b2.double(), padding=1))
        ref = torch.nn.functional.max_pool2d(y, 2, 2).permute(0, 2, 3, 1).reshape(-1, 64)
    return (u8 if from_u8 else crops), (w1h, b1, 2.0 ** -s1, w2d, b2, 2.0 ** -s2), ref, q8


def launch_fused(hip, entry, crops, args, out, H, W):
    w1h, b1, o1, w2d, b2, o2 = args
    dev = (w1h.cuda(), b1.cuda(), o1, w2d.cuda(), b2.cuda(), o2)
    if entry.startswith('u8'):
        hip.conv1_fused_u8(crops, MEAN, STD, *dev, out, 3, H, W, q8=entry == 'u8q8')
    else:
        (hip.conv1_fused_hq8 if entry == 'hq8' else hip.conv1_fused_hl16)(crops, *dev, out, 3, H, W)


@pytest.mark.parametrize('H,W', MAPS, ids=['%dx%d' % m for m in MAPS])
@pytest.mark.parametrize('entry', FUSED)
def test_conv1_fused(hip, entry, H, W):
    crops, args, ref, q8 = fused_case(entry, H, W)
    rows = 3 * (H // 2) * (W // 2)
    fmt = 'u8' if entry.startswith('u8') else 'f32'
    res = []
    for limit, pattern in ((0, 0), (8, 1)):
        x, xbuf = guarded_in(crops, IN_GUARDS[fmt][pattern])
        out = Out(rows, 64)
        with knobs(width=128, limit=limit), bound(hip) as counters:   # the width knob does not reach the fused launches
            launch_fused(hip, entry, x, args, out.view, H, W)
            torch.cuda.synchronize()
            assert counters.tolist() == [0, 0, 0, 0], counters.tolist()
        res.append(out.check('fused %s %d x %d' % (entry, H, W)))
        if limit == 0:
            dec = decode(hip, 'hq8' if q8 else 'hl16', out.view)
            note('fused hq8' if q8 else 'fused hl16', dec, ref)
            close(dec, ref, 2.5e-4 if q8 else 3e-6, 'fused first launch (%s) %d x %d vs float64' % (entry, H, W))
    assert torch.equal(res[0], res[1]), 'fused %s: grid limit 8 (and other input guards) changed the bytes' % entry


def c11_lanes(H, W, extra_round):
    """lanes that own channel 5 and at least one in-image pixel of a tile's 18 x 18 haloed patch, summed over the tiles of
    one crop (see test_conv1_fused_range_counter)"""
    total = 0
    for by in range((H + 15) // 16):
        for bx in range((W + 15) // 16):
            for wave in range(8):
                for l15 in range(16):
                    hit = False
                    for rr in range(3):
                        g = wave + 8 * rr
                        if g >= 21:
                            if not extra_round:
                                continue
                            g = 20
                        n = min(g * 16 + l15, 323)
                        gy, gx = by * 16 - 1 + n // 18, bx * 16 - 1 + n % 18
                        hit = hit or (0 <= gy < H and 0 <= gx < W)
                    total += hit
    return total


@pytest.mark.parametrize('entry', FUSED)
def test_conv1_fused_range_counter(hip, entry):
    """Counter [2] of the fused launches, as patch_prologue.inc / patch_kloop.inc count it: conv1_1 is computed per tile for
    the 18 x 18 haloed patch in rounds of 16 pixels - wave w takes rounds w, w + 8 and w + 16 (< 21), lane l of a round
    the pixel 16 round + (l & 15) (past 323: pixel 323 again) and the channels 16 mb + 4 (l >> 4) .. + 3, mb = 0 .. 3.
    Every lane keeps the running maximum of the values it produced for a tile - after scale, ReLU and the clamp at 65504,
    patch pixels outside the image being 0 - and adds ONE to [2] when that maximum exceeds 65000 (hq8: 1792), then
    starts over: [2] counts (tile, lane) pairs, not elements.  The hl16 launch computes the patch of a workgroup's second
    and later tiles under the K loop of the tile before, where waves 5 - 7 repeat round 20 as their third; the tests'
    maps make no difference between the two forms unless a lane's only in-image pixel is one of that round.
    A conv1_1 bias of 70000 (2000) on channel 5 - lanes 16 .. 31 of every wave - puts every in-image patch pixel above the
    limit: the count lies between the two forms' and is the same for every launch of a grid; in range it is 0."""
    q8 = entry in ('hq8', 'u8q8')
    H = W = 18
    for plant in (0.0, 2000.0 if q8 else 70000.0):
        crops, args, _, _ = fused_case(entry, H, W, plant)
        x, xbuf = guarded_in(crops, IN_GUARDS['u8' if entry.startswith('u8') else 'f32'][0])
        for limit in (0, 8):
            seen = []
            for _ in range(3):
                out = Out(3 * 81, 64)
                with knobs(limit=limit), bound(hip) as counters:
                    launch_fused(hip, entry, x, args, out.view, H, W)
                    torch.cuda.synchronize()
                    seen.append(counters.tolist())
                out.check('fused %s, conv1_1 bias %g' % (entry, plant))
            assert seen[0] == seen[1] == seen[2], 'counters differ between launches: %s' % seen
            if not plant:
                assert seen[0] == [0, 0, 0, 0]
            else:
                lo, hi = 3 * c11_lanes(H, W, False), 3 * c11_lanes(H, W, True)
                print('fused %s limit %d: counters %s, (tile, lane) pairs by the rule %d .. %d' % (entry, limit, seen[0], lo, hi))
                assert seen[0][2] > 0 and lo <= seen[0][2] <= hi and seen[0][3] == 0


# ---- fp32 tile kernel (csrc/conv3x3.hip) --------------------------------------------------------------------------------
TILE = [('bn_relu', bn, first, pool) for bn in (64, 128) for first in (0, 1) for pool in (0, 1)] + \
       [('raw', bn, first, 0) for bn in (64, 128) for first in (0, 1)] + [('first_hl16', bn, 1, 0) for bn in (64, 128)]


@pytest.mark.parametrize('entry,bn,first,pool', TILE, ids=['%s-bn%d-first%d-pool%d' % c for c in TILE])
def test_tile_kernel(hip, entry, bn, first, pool):
    """Cout = 64 -> conv3x3_kernel<64, ...>, Cout = 128 -> <128, ...> (Cout % 128 == 0 is the launcher's whole condition).
    L = 3 maps of 5 x 7: 3 x 4 x 3 x 4 = 144 quad-ordered rows, so the second 128-row tile is ragged and straddles crops,
    and the odd sides leave half-empty quads; first_hl16 needs even sides: 6 x 10 = 180 rows."""
    L, H, W = (3, 6, 10) if entry == 'first_hl16' else (3, 5, 7)
    Cin, Cout = (3 if first else 64), bn
    emu = TorchOps(torch.float64)
    x = rnd(L, 3, H, W, seed=880) if first else torch.relu(rnd(L, H, W, Cin, seed=880))
    if entry == 'raw' and not first:
        x = rnd(L, H, W, Cin, seed=880)
    wp = rnd(Cout, 32, seed=881, scale=0.2) if first else rnd(9, Cout, Cin, seed=881, scale=(2.0 / (9 * Cin)) ** 0.5)
    if first:
        wp[:, 27:] = 0
    bias = rnd(Cout, seed=882, scale=0.1)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    ref = torch.zeros(L * Ho * Wo, Cout, dtype=torch.float64)
    if entry == 'raw':
        emu.conv3x3_raw(x, wp, bias, ref, L, H, W, Cin, Cout, bool(first))
    else:
        emu.conv3x3(x, wp, bias, ref, L, H, W, Cin, Cout, bool(first), bool(pool))
    what = 'conv3x3_kernel<%d, %d, %d> (%s)' % (bn, first, pool, entry)
    res = []
    for pattern in (0, 1):
        xin, xbuf = guarded_in(x, IN_GUARDS['f32'][pattern])
        out = Out(L * Ho * Wo, Cout)
        if entry == 'bn_relu':
            hip.conv3x3(xin, wp.cuda(), bias.cuda(), out.view, L, H, W, Cin, Cout, bool(first), bool(pool))
        elif entry == 'raw':
            hip.conv3x3_raw(xin, wp.cuda(), bias.cuda(), out.view, L, H, W, Cin, Cout, bool(first))
        else:
            hip.conv3x3_first_hl16(xin, wp.cuda(), bias.cuda(), out.view, L, H, W, Cout)
        torch.cuda.synchronize()
        res.append(out.check(what))
        if pattern == 0:
            dec = decode(hip, 'hl16', out.view) if entry == 'first_hl16' else out.view.clone()
            note('fp32', dec, ref)
            close(dec, ref, 3e-6, what + ' vs float64')
            if entry == 'raw':
                assert bool((dec < 0).any())
    assert torch.equal(res[0], res[1]), what + ': a second launch (other input guards) gives other bytes'


# ---- what the launchers refuse ------------------------------------------------------------------------------------------
def test_launchers_refuse(hip):
    """MMMOT_EINVAL and no launch: the output keeps its NaNs, the bound counters their zeros"""
    with bound(hip) as counters:
        calls, out = refused_calls()
        torch.cuda.synchronize()
        assert counters.tolist() == [0, 0, 0, 0]
    bad = [what for what, status in calls if status != EINVAL]
    assert not bad, 'not refused: ' + ', '.join(bad)
    assert len(calls) == 3 * 7 + 4 * 5 + 3 + 6 + 3 * 7
    assert out.untouched(), 'a refused call wrote to the output'


def refused_calls():
    lib = _lib.load()
    L, H, W, Cin, Cout = 2, 6, 8, 32, 64
    f = lambda *shape: torch.zeros(*shape).cuda()  # noqa: E731
    x, w, b, osc = f(L * H * W, 64), f(9 * 128 * 64), f(128), torch.ones(128).cuda()
    crops, crops8 = f(L, 3, H, W), torch.zeros(L, H, W, 3, dtype=torch.uint8).cuda()
    out = Out(L * H * W, 128)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = p(out.view)
    big = (1 << 16, 64, 64, 32)   # L * H * W * (Cin / 4) = 2^31: past the 32-bit piece offsets
    assert big[0] * big[1] * big[2] * (big[3] // 4) >= (1 << 31) - 64
    calls = []
    for name, extra in (('mmmot_conv3x3_bn_relu_hl16_patch', (0, p(osc), s)), ('mmmot_conv3x3_bn_relu_hq8', (0, p(osc), s)),
                        ('mmmot_conv3x3_raw_hl16', (p(osc), s))):
        fn = getattr(lib, name)
        for what, a in (('Cin % 32', (p(x), p(w), p(b), o, L, H, W, 48, Cout)), ('Cout % 64', (p(x), p(w), p(b), o, L, H, W, Cin, 96)),
                        ('Cout = 32', (p(x), p(w), p(b), o, L, H, W, Cin, 32)),
                        ('misaligned in', (p(x, 4), p(w), p(b), o, L, H, W, Cin, Cout)),
                        ('misaligned wp', (p(x), p(w, 8), p(b), o, L, H, W, Cin, Cout)),
                        ('misaligned out', (p(x), p(w), p(b), p(out.view, 4), L, H, W, Cin, Cout)),
                        ('piece limit', (p(x), p(w), p(b), o) + big + (Cout,))):
            calls.append((name + ': ' + what, fn(*a, *extra)))
    w1 = f(64 * 32)
    for name, head, tail in (
            ('mmmot_conv1_fused_hl16', (p(crops),), (s,)), ('mmmot_conv1_fused_hq8', (p(crops),), (s,)),
            ('mmmot_conv1_fused_u8', (p(crops8), 0.5, 0.5, 0.5, 0.2, 0.2, 0.2), (0, s)),
            ('mmmot_conv1_fused_u8', (p(crops8), 0.5, 0.5, 0.5, 0.2, 0.2, 0.2), (1, s))):
        fn = getattr(lib, name)
        for what, a in (('odd H', (p(w1), p(b), 1.0, p(w), p(b), p(osc), o, L, 5, W)), ('odd W', (p(w1), p(b), 1.0, p(w), p(b), p(osc), o, L, H, 7)),
                        ('misaligned w1', (p(w1, 4), p(b), 1.0, p(w), p(b), p(osc), o, L, H, W)),
                        ('misaligned w2', (p(w1), p(b), 1.0, p(w, 4), p(b), p(osc), o, L, H, W)),
                        ('misaligned out', (p(w1), p(b), 1.0, p(w), p(b), p(osc), p(out.view, 8), L, H, W))):
            calls.append((name + ': ' + what, fn(*head, *a, *tail)))
    for k in range(3):
        std = [0.2, 0.2, 0.2]
        std[k] = 0.0
        calls.append(('mmmot_conv1_fused_u8: std[%d] == 0' % k, lib.mmmot_conv1_fused_u8(
            p(crops8), 0.5, 0.5, 0.5, *std, p(w1), p(b), 1.0, p(w), p(b), p(osc), o, L, H, W, 0, s)))
    for what, a in (('odd H', (p(crops), p(w), p(b), o, L, 5, W, Cout)), ('odd W', (p(crops), p(w), p(b), o, L, H, 7, Cout)),
                    ('Cout % 64', (p(crops), p(w), p(b), o, L, H, W, 96)), ('misaligned in', (p(crops, 4), p(w), p(b), o, L, H, W, Cout)),
                    ('misaligned wp', (p(crops), p(w, 4), p(b), o, L, H, W, Cout)),
                    ('misaligned out', (p(crops), p(w), p(b), p(out.view, 4), L, H, W, Cout))):
        calls.append(('mmmot_conv3x3_first_hl16: ' + what, lib.mmmot_conv3x3_first_hl16(*a, s)))
    for name, tail in (('mmmot_conv3x3_bn_relu', (0, s)), ('mmmot_conv3x3_bn_relu', (1, s)), ('mmmot_conv3x3_raw', (s,))):
        fn = getattr(lib, name)
        for what, a in (('first with Cin != 3', (p(crops), p(w), p(b), o, L, H, W, 32, Cout, 1)),
                        ('Cin % 32', (p(x), p(w), p(b), o, L, H, W, 48, Cout, 0)), ('Cout % 64', (p(x), p(w), p(b), o, L, H, W, Cin, 96, 0)),
                        ('first, Cout % 64', (p(crops), p(w), p(b), o, L, H, W, 3, 32, 1)),
                        ('misaligned in', (p(x, 4), p(w), p(b), o, L, H, W, Cin, Cout, 0)),
                        ('misaligned wp', (p(x), p(w, 4), p(b), o, L, H, W, Cin, Cout, 0)),
                        ('misaligned out', (p(x), p(w), p(b), p(out.view, 4), L, H, W, Cin, Cout, 0))):
            calls.append((name + ': ' + what, fn(*a, *tail)))
    return calls, out


def test_knobs_refuse(hip):
    lib = _lib.load()
    with knobs():
        for v in (-1, 1, 32, 96, 127, 192, 256):
            assert lib.mmmot_set_patch_tile_width(v) == EINVAL, v
        for v in (-1, 2, 5, 16):
            assert lib.mmmot_set_patch_min_block(v) == EINVAL, v
        for v in (-8, 4, 12):
            assert lib.mmmot_set_patch_grid_limit(v) == EINVAL, v
        n_cu = ctypes.c_int(0)
        assert lib.mmmot_device_info(torch.cuda.current_device(), ctypes.byref(n_cu), ctypes.create_string_buffer(32), 32) == 0
        if n_cu.value == 256:
            # the refused values changed nothing: the automatic choice of tests/test_patch_choice_cpu.py
            assert hip.patch_choice(70, 4, 4, 512) == (64, 4, 40, 40)
        for bad in ((0, 4, 4, 64), (1, 0, 4, 64), (1, 4, -1, 64), (1, 4, 4, 96), (1, 4, 4, 0)):
            assert lib.mmmot_patch_choice(*bad, None, None, None, None) == EINVAL, bad
        assert lib.mmmot_patch_choice(1, 4, 4, 64, None, None, None, None) == 0
    c = torch.zeros(8, dtype=torch.int32).cuda()
    try:
        for off in (1, 2, 3):
            assert lib.mmmot_trunk_range_bind(ctypes.c_void_p(c.data_ptr() + off)) == EINVAL
        assert lib.mmmot_trunk_range_bind(ctypes.c_void_p(c.data_ptr() + 4)) == 0
    finally:
        hip.trunk_range_bind(None)
