"""The M16 instantiations of the trunk's patch kernel (v_mfma_f32_16x16x32_f16 on fragment pairs exchanged in registers:
csrc/patch_fragments.inc, patch_kloop.inc, patch_epilogue.inc), reached through the real dispatchers.

Which layers run in that form is mmmot_patch_m16 (csrc/patch_choice.h, pinned by tests/test_m16_layout_cpu.py): the
plain f16x3 layers with Cin = 128 .. 256, Cin % 64 == 0, except 128 -> 128 - so Cin = 128 here, where
tests/test_trunk_kernels_gpu.py (Cin = 32 and 96) covers the 32x32x16 form.  conv3x3_hl16_patch_kernel<BN, BS, POOL, 0, 0, RAW, M16 = 1>: 64 | 128 x 16 | 8 | 4 x
(unpooled, pooled, raw) = 18 instantiations; every case asks mmmot_patch_choice for the <BN, BS> its launch would run and
asserts it (tile width forced with mmmot_set_patch_tile_width, the block edge follows from the map).

Shapes - the smallest at which the form can go wrong.  Cin = 128 is four 32-channel slabs: interior slabs of both
parities of the alternating K loop, the transition slab, the last slab.  Three crops of
  16 x 16     block edge 16, one block per tile
  8 x 8       block edge 8, four blocks per tile (a ragged tile: 3 of 4)
  4 x 4       block edge 4 (whole maps, 3 of 16), and the haloed 8 x 8 geometry under mmmot_set_patch_min_block(8)
  21 x 21     pooled only: an odd map (floor pooling -> 10 x 10) with partial blocks on both axes
with Cout = 64 (one 64-channel tile), 192 (three of 64: with the grid capped at 8 the 16 x 16 and 21 x 21 maps chain two
tiles on a workgroup) and 256 (two 128-channel tiles or four of 64: the 128-channel instantiations).  Cout = 128 is the one
layer shape the rule leaves in the 32x32x16 form: its cases hold that form to the same checks on the same four-slab shapes.
test_m16_chained (Cout = 256) runs more tiles than workgroups on every geometry and both tile widths.

Every case: float64 on the decoded hl16 operands (tests/fake_ops.py) between NaN guards, the bounds of
tests/test_trunk_kernels_gpu.py (hl16 2e-6, raw 3e-6 of the reference's maximum); the same bytes from a second launch
(other input guards), the other tile width, grid limit 8 against 0 and, for whole maps, the haloed geometry; range
counters exact (test_m16_range_guard plants channels above 65000).  Knobs are restored by `knobs`."""
import functools

import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd.pack import from_hl16, hl16_weight_shift, to_hl16
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)
from test_trunk_kernels_gpu import BOUND, IN_GUARDS, Out, bound, guarded_in, knobs, note

pytestmark = pytest.mark.gpu

CIN = 128
MAPS = {16: (16, 16), 8: (8, 8), 4: (4, 4)}   # block edge -> map
ODD = (21, 21)                                # pooled -> 10 x 10, block edge 16
L3 = 3


def out_hw(H, W, pool):
    return (H // 2, W // 2) if pool else (H, W)


@functools.lru_cache(maxsize=None)
def case(kind, L, H, W, cout, pool, hot=()):
    """-> (x units, w units, bias, oscale, float64 reference [rows][cout]); `hot`: output channels planted at 70000"""
    x = rnd(L * H * W, CIN, seed=1600) * 3.0
    if kind != 'raw':
        x = torch.relu(x)
    w = rnd(9, cout, CIN, seed=1601, scale=(2.0 / (9 * CIN)) ** 0.5)
    bias = rnd(cout, seed=1602, scale=0.1)
    if hot:
        w[:, list(hot), :] = 0.0
        bias[list(hot)] = 70000.0
    shift = hl16_weight_shift(w)
    xr, wr = to_hl16(x), to_hl16(w.double() * 2.0 ** shift)
    Ho, Wo = out_hw(H, W, pool)
    ref = torch.zeros(L * Ho * Wo, cout, dtype=torch.float64)
    xd, wd = from_hl16(xr).view(L, H, W, CIN), from_hl16(wr).double() * 2.0 ** -shift
    emu = TorchOps(torch.float64)
    if kind == 'raw':
        emu.conv3x3_raw(xd, wd, bias, ref, L, H, W, CIN, cout, False)
    else:
        emu.conv3x3(xd, wd, bias, ref, L, H, W, CIN, cout, False, bool(pool))
    cold = [n for n in range(cout) if n not in hot]
    assert float(ref[:, cold].abs().max()) < 100.0   # far from 65000: the range guard counts the planted channels only
    return xr, wr, bias, 2.0 ** -shift, ref


def run(hip, kind, L, H, W, cout, pool, bn, bs, limit=0, min_block=0, pattern=0, min_items=0, hot=(), want=(0, 0, 0, 0)):
    """one guarded launch under the knobs, branch asserted -> (output bytes, decoded output)"""
    xr, wr, bias, osc, _ = case(kind, L, H, W, cout, pool, hot)
    x, xbuf = guarded_in(xr, IN_GUARDS['hl16'][pattern])
    Ho, Wo = out_hw(H, W, pool)
    out = Out(L * Ho * Wo, cout)
    oscv = torch.full((cout,), osc).cuda()
    sentinel = 77 if kind == 'raw' else 0
    what = 'M16 %s <%d, %d, %d> Cout %d %dx%d limit %d' % (kind, bn, bs, pool, cout, H, W, limit)
    with knobs(width=bn, limit=limit, min_block=min_block), bound(hip, sentinel) as counters:
        got = hip.patch_choice(L, H, W, cout)
        assert got[:2] == (bn, bs), '%s: the launch would run <%d, %d>' % (what, got[0], got[1])
        assert not limit or got[3] == 8, got
        assert got[2] >= min_items, got
        if kind == 'raw':
            hip.conv3x3_raw_hl16(x, wr.cuda(), bias.cuda(), out.view, L, H, W, CIN, cout, oscv)
        else:
            hip.conv3x3_hl16_patch(x, wr.cuda(), bias.cuda(), out.view, L, H, W, CIN, cout, bool(pool), oscv)
        torch.cuda.synchronize()
        counts = tuple(counters.tolist())
    assert counts == ((sentinel,) * 4 if kind == 'raw' else tuple(want)), '%s: range counters %s' % (what, counts)
    b = out.check(what)
    if kind == 'raw':
        return b, out.view.clone()
    dec = torch.zeros_like(out.view)
    hip.hl16_unpack(out.view.contiguous(), dec)
    return b, dec


def widths(cout):
    return (128, 64) if cout % 128 == 0 else (64,)


KINDS = [('hl16', 0), ('hl16', 1), ('raw', 0)]
MATRIX = [(kind, pool, bs, cout) for kind, pool in KINDS for bs in (16, 8, 4) for cout in (64, 128, 192, 256)] + \
         [('hl16', 1, 21, cout) for cout in (64, 128, 192, 256)]


@pytest.mark.parametrize('kind,pool,bs,cout', MATRIX, ids=['%s-pool%d-bs%d-cout%d' % c for c in MATRIX])
def test_m16_matrix(hip, kind, pool, bs, cout):
    (H, W), bs = (ODD, 16) if bs == 21 else (MAPS[bs], bs)
    ref = case(kind, L3, H, W, cout, pool)[4]
    bn = widths(cout)[0]
    what = 'M16 %s <%d, %d, %d> Cout %d %dx%d' % (kind, bn, bs, pool, cout, H, W)
    got, dec = run(hip, kind, L3, H, W, cout, pool, bn, bs)
    note('m16 ' + kind, dec, ref)
    close(dec, ref, BOUND[kind], what + ' vs float64')
    if kind == 'raw':
        assert bool((dec < 0).any()), 'raw output: no ReLU'
    again, _ = run(hip, kind, L3, H, W, cout, pool, bn, bs, pattern=1)
    assert torch.equal(got, again), what + ': a second launch (other input guards) gives other bytes'
    for other in widths(cout)[1:]:
        narrow, _ = run(hip, kind, L3, H, W, cout, pool, other, bs)
        assert torch.equal(got, narrow), what + ': %d- and %d-channel tiles differ' % (bn, other)
    capped, _ = run(hip, kind, L3, H, W, cout, pool, bn, bs, limit=8)
    assert torch.equal(got, capped), what + ': grid limit 8 and 0 differ'
    if bs == 4:
        haloed, _ = run(hip, kind, L3, H, W, cout, pool, bn, 8, min_block=8)
        assert torch.equal(got, haloed), what + ': whole-map and haloed 8 x 8 geometry differ'


CHAIN_L = {16: 5, 8: 17, 4: 65}   # five pixel tiles: ten 128-channel or twenty 64-channel tiles of Cout = 256
CHAINED = [(kind, pool, bs) for kind, pool in KINDS for bs in (16, 8, 4)]


@pytest.mark.parametrize('kind,pool,bs', CHAINED, ids=['%s-pool%d-bs%d' % c for c in CHAINED])
def test_m16_chained(hip, kind, pool, bs):
    """more tiles than the eight workgroups of a capped grid: tiles follow each other on a workgroup (the successor's
    first slab and weight stages stream in during the last slab; every tile restarts the alternation of the K loop)"""
    (H, W), L, cout = MAPS[bs], CHAIN_L[bs], 256
    ref = case(kind, L, H, W, cout, pool)[4]
    what = 'M16 %s chained <128, %d, %d>' % (kind, bs, pool)
    got, dec = run(hip, kind, L, H, W, cout, pool, 128, bs, limit=8, min_items=10)
    note('m16 ' + kind, dec, ref)
    close(dec, ref, BOUND[kind], what + ' vs float64')
    again, _ = run(hip, kind, L, H, W, cout, pool, 128, bs, limit=8, pattern=1, min_items=10)
    assert torch.equal(got, again), what + ': a second launch gives other bytes'
    free, _ = run(hip, kind, L, H, W, cout, pool, 128, bs)
    assert torch.equal(got, free), what + ': grid limit 8 and 0 differ'
    narrow, _ = run(hip, kind, L, H, W, cout, pool, 64, bs, limit=8, min_items=20)
    assert torch.equal(got, narrow), what + ': 64- and 128-channel tiles differ'
    if bs == 4:
        haloed, _ = run(hip, kind, L, H, W, cout, pool, 128, 8, limit=8, min_block=8)
        assert torch.equal(got, haloed), what + ': whole-map and haloed 8 x 8 geometry differ'


HOT = (3, 64, 127, 130, 255)   # output channels planted at 70000: clamped to 65000 and counted
GUARDED = [(bs, pool) for bs in (16, 8, 4) for pool in (0, 1)]


@pytest.mark.parametrize('bs,pool', GUARDED, ids=['bs%d-pool%d' % c for c in GUARDED])
def test_m16_range_guard(hip, bs, pool):
    """counter [1] = the output elements above 65000 - pooled elements on a pooled layer, no padding pixel of a ragged
    tile among them - on both tile widths; the clamped channels carry the host encoder's bytes"""
    (H, W), cout = MAPS[bs], 256
    ref = case('hl16', L3, H, W, cout, pool, HOT)[4]
    Ho, Wo = out_hw(H, W, pool)
    rows = L3 * Ho * Wo
    emu = TorchOps(torch.float64)
    emu._guard(ref.clone(), False)
    want = tuple(emu.range)
    assert want == (0, len(HOT) * rows, 0, 0)
    cold = [n for n in range(cout) if n not in HOT]
    first = None
    for bn in (128, 64):
        b, dec = run(hip, 'hl16', L3, H, W, cout, pool, bn, bs, hot=HOT, want=want)
        close(dec[:, cold], ref[:, cold], BOUND['hl16'], 'M16 range guard <%d, %d, %d> (channels in range) vs float64' % (bn, bs, pool))
        unit = b.view(torch.uint8).view(torch.int16).view(rows, cout // 8, 2, 8)
        clamped = to_hl16(torch.full((1, 8), 65000.0)).view(torch.int16).view(2, 8)
        for n in HOT:
            assert bool((unit[:, n // 8, :, n % 8] == clamped[:, 0]).all()), 'hl16 bytes of clamped channel %d' % n
        first = b if first is None else first
        assert torch.equal(first, b), 'range guard: 64- and 128-channel tiles differ'
