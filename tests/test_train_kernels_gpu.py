"""Every launch branch of the training step's second and third slice (csrc/train.hip, csrc/train_vgg.hip, and the forward
convolution kernels run as the input gradient) against a float64 statement of the same operation, with the conventions
of tests/test_backward_kernels_gpu.py:

* outputs are slices of NaN buffers with guard rows - a column slice wherever the entry point takes a leading dimension,
  flat guards elsewhere - and everything around the output must still be NaN after the launch;
* inputs with a leading dimension are column slices of NaN buffers, the others lie between NaN guards;
* every case is launched twice on fresh buffers and the two results must be equal bit for bit;
* the reference is ``TorchOps(torch.float64)`` (tests/fake_ops.py), except: the input gradient (float64 autograd of
  ``F.conv2d`` w.r.t. its input - independent of the weight flip), the GHM bin decisions (the float32 statement of
  ``TorchOps.ghm_loss``, like the reference's tensor-vs-scalar comparisons) and the layer composite (float64 autograd
  through conv2d -> training-mode batch_norm -> relu -> max_pool2d, tests/test_train_kernels_cpu.py);
* inputs on a decision boundary (ReLU sign, pool argmax, GHM bin edge, smooth-L1 |d| = 1) are either constructed from
  exactly representable values, so that fp32 and float64 provably agree, or kept off the boundary; the distance is
  asserted on the CPU before anything is launched, and no element is excluded from a comparison.

Tolerances are those the existing tests of the same kernel assert (tests/test_train_gpu.py, tests/test_train_vgg_gpu.py),
as a fraction of the reference's maximum.

Which case reaches which branch is said at the case lists below.  What four one-line mutations would break (by reasoning and
by the CPU twin; no broken kernel was run on a device):
* the grid-stride increment `idx += (long)gridDim.x * 256` of bn_relu_pool_kernel / maxpool_bwd_kernel /
  rows_gather_scale_kernel taken out (one pass only): the units behind the cap stay NaN in test_bn_relu_pool_beyond_the_grid_cap,
  test_maxpool_bwd_beyond_the_grid_cap and test_rows_gather_scale[1048583-8];
* `a[k][e] > best[e]` -> `>=` in maxpool_bwd_kernel: windows 4 .. 9 of WINDOWS send their gradient to the last maximum in
  test_maxpool_ties_go_to_the_first_maximum (and the integer ties of test_maxpool_bwd_beyond_the_grid_cap);
* dgrad_weights without `flip(0)`, or without `permute(0, 2, 1)`: every case of test_input_gradient_through_the_flipped_weights
  and dX of test_one_trunk_layer_forward_and_backward are off by O(1) of their maximum, as
  test_train_kernels_cpu.py::test_a_wrong_input_gradient_weight_layout_is_noticed shows on the emulation."""
import functools

import pytest
import torch
import torch.nn.functional as F

from fake_ops import TorchOps
from mmmot_amd.plan import RowTiles
from mmmot_amd.train_vgg import dgrad_weights
from test_backward_kernels_gpu import ARITH, DEV, EINVAL, NAN, arithmetic, both, flat, put, slab, twice, untouched  # noqa: F401
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)
from test_train_kernels_cpu import LAYER_CASES, MARGIN, fake_engine, layer_case, layer_errors, run_layer

pytestmark = pytest.mark.gpu
emu = TorchOps(torch.float64)


def fput(t):
    """a contiguous input (an entry point without a leading dimension) between NaN guards"""
    buf, v = flat(*t.shape)
    v.copy_(t)
    return v


def sput(t, extra=4):
    """a 2-D input as a column slice with row stride C + 4 + extra of a NaN buffer"""
    buf, v = slab(t.shape[0], t.shape[1], extra=extra)
    v.copy_(t)
    return v


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- rows_stats -------------------------------------------------------------------------------------------------------
# narrow branch (C / 4 <= 128 lanes per row, 256 / (C / 4) row phases through LDS): C = 4 (256 phases of one lane), 64 (16),
# 128 (8), 256 (4), 512 (2) and 192 (48 lanes, 5 phases: threads 240 .. 255 idle); wide branch: 516 (one pass, lane 129 the
# last live one), 1024 (a full pass), 2048 (gridDim.y = 2)
RS_C = [4, 64, 128, 192, 256, 512, 516, 1024, 2048]
# one tile of one row; tiles of 3 / 1 / 2 rows - shorter than the phase count of every narrow C but 512, whose 2 phases the
# 1-row tiles undercut; eleven 1-row tiles; full, partial and 1-row tiles of one group
RS_TILINGS = [[1], [3, 1, 2], [1] * 11, [5, 300, 128, 1]]


def check_rows_stats(hip, what, Z, C, counts):
    tc, tg = both(counts)
    Zg = sput(Z)
    assert Zg.stride(0) == C + 8
    pr = torch.zeros(tc.T, 2, C, dtype=torch.float64)
    emu.rows_stats(Z, C, tc, pr)
    (pg,) = twice(what, lambda: [flat(tc.T, 2, C)], lambda part: hip.rows_stats(Zg, C, tg, part))
    close(pg[:, 0], pr[:, 0], 2e-6, what + ' sums')
    close(pg[:, 1], pr[:, 1], 2e-6, what + ' squares around the tile mean')  # judged on their own maximum, not the sums'


@pytest.mark.parametrize('C', RS_C)
def test_rows_stats(hip, C):
    for counts in RS_TILINGS:
        Z = rnd(sum(counts), C, seed=6) * 2 + 0.3
        check_rows_stats(hip, 'rows_stats C %d %s' % (C, counts), Z, C, counts)


@pytest.mark.parametrize('C', [64, 516])
def test_rows_stats_of_columns_far_from_zero(hip, C):
    """every column at a mean of 1000 sigma: part[t][1] is the sum of squares around the TILE MEAN (d = y - mean is exact in
    fp32 up to the mean's own error, which enters squared), not E[y^2] - mean^2 (which would lose all six digits), so it
    keeps the 2e-6 of the well-centred cases"""
    counts = [5, 300, 128, 1]
    Z = 100.0 + 0.1 * rnd(sum(counts), C, seed=7)
    check_rows_stats(hip, 'rows_stats mean 1000 sigma C %d' % C, Z, C, counts)


# ---- bn_relu_pool / maxpool_bwd ---------------------------------------------------------------------------------------
# the smallest map, one odd side (the last row / column belongs to no window), both odd with several windows, even
POOL_MAPS = [(2, 2), (2, 3), (3, 2), (9, 7), (8, 8)]
POOL_MARGIN = 1e-5  # of max |y|; fp32 has y = fmaf(z, sc, sh) to 6e-8 |y|


def mixed_sign(C, seed):
    sc = rnd(C, seed=seed).abs() + 0.5
    sc[1::2] *= -1.0  # a negative gamma is legal
    return sc


def pool_inputs(L, H, W, C, seed=0):
    """Z, sc (both signs), sh with every y = z sc + sh at least POOL_MARGIN max|y| from the ReLU kink and the two largest
    post-ReLU values of every window with a positive maximum that far apart, in float64 (elements / windows that miss it
    are moved by a fixed amount until it holds; then it is asserted: the argmax and the sign are the same in fp32)"""
    Z = rnd(L * H * W, C, seed=seed + 1) * 2 + 0.3
    sc, sh = mixed_sign(C, seed + 2), rnd(C, seed=seed + 3)
    Ho, Wo = H // 2, W // 2
    slot = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).view(1, 1, 2, 1, 2, 1)

    def bad():
        y = (Z.double() * sc.double() + sh.double()).view(L, H, W, C)
        m = POOL_MARGIN * y.abs().max().item()
        win = torch.relu(y)[:, :2 * Ho, :2 * Wo].reshape(L, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(L, Ho, Wo, C, 4)
        two = win.topk(2, dim=-1)[0]
        return y.abs() < m, (two[..., 0] > 0) & (two[..., 0] - two[..., 1] < m)
    for _ in range(8):
        kink, tie = bad()
        Z.view(L, H, W, C)[kink] += 0.25
        Z.view(L, H, W, C)[:, :2 * Ho, :2 * Wo] += (tie.view(L, Ho, 1, Wo, 1, C) * slot * 0.25).reshape(L, 2 * Ho, 2 * Wo, C)
    kink, tie = bad()
    assert not kink.any() and not tie.any(), (int(kink.sum()), int(tie.sum()))
    return Z, sc, sh


def check_pool_kernels(hip, what, Z, sc, sh, L, H, W, C, dP=None):
    Zg, scg, shg = fput(Z), fput(sc), fput(sh)
    for pool in (0, 1):
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        ar = torch.zeros(L * Ho * Wo, C, dtype=torch.float64)
        emu.bn_relu_pool(Z, C, sc, sh, L, H, W, pool, ar)
        (ag,) = twice('%s bn_relu_pool pool=%d' % (what, pool), lambda: [flat(L * Ho * Wo, C)],
                      lambda A: hip.bn_relu_pool(Zg, C, scg, shg, L, H, W, pool, A))
        close(ag, ar, 2e-6, '%s bn_relu_pool pool=%d' % (what, pool))
    dP = rnd(L * (H // 2) * (W // 2), C, seed=9) if dP is None else dP
    dr = torch.zeros(L * H * W, C, dtype=torch.float64)
    emu.maxpool_bwd(Z, C, sc, sh, dP, L, H, W, dr)
    dPg = fput(dP)
    (dg,) = twice(what + ' maxpool_bwd', lambda: [flat(L * H * W, C)],
                  lambda dA: hip.maxpool_bwd(Zg, C, scg, shg, dPg, L, H, W, dA))
    close(dg, dr, 1e-6, what + ' maxpool_bwd')
    return dg, dr


@pytest.mark.parametrize('L', [1, 3])
@pytest.mark.parametrize('C', [4, 64, 512])
def test_bn_relu_pool_and_maxpool_bwd(hip, C, L):
    """C = 4: one lane per pixel; sc of both signs; odd maps: the pooled output ignores the last row / column and
    maxpool_bwd writes exact zeros there"""
    for H, W in POOL_MAPS:
        Z, sc, sh = pool_inputs(L, H, W, C, seed=10 * H + W)
        dg, _ = check_pool_kernels(hip, 'C %d L %d map %dx%d' % (C, L, H, W), Z, sc, sh, L, H, W, C)
        d4 = dg.view(L, H, W, C)
        assert (d4[:, 2 * (H // 2):] == 0).all() and (d4[:, :, 2 * (W // 2):] == 0).all()


# windows of post-ReLU values in (0,0), (0,1), (1,0), (1,1) order: a unique maximum in each slot; two equal positive
# maxima (slots 0/1, 1/2, 2/3, 0/3, 1/3); four equal; all <= 0 (zeros; negatives and a zero)
WINDOWS = [(3, 1, 2, -1), (1, 3, 0, 2), (0, -2, 3, 1), (2, 1, -1, 3),
           (2, 2, 1, 0), (1, 3, 3, -1), (0, 1, 2, 2), (2, -1, 0, 2), (-1, 3, 1, 3),
           (2, 2, 2, 2), (0, 0, 0, 0), (-1, -2, 0, -3)]
FIRST_MAX = [0, 1, 2, 3, 0, 1, 2, 0, 1, 0, 0, 0]


@pytest.mark.parametrize('L,C', [(3, 4), (1, 64)])
@pytest.mark.parametrize('H,W', [(2, 2), (9, 7), (8, 8), (3, 2)])
def test_maxpool_ties_go_to_the_first_maximum(hip, H, W, L, C):
    """Z from small integers, sc = +-1, sh = 0: fp32 and float64 compute the same values, ties are ties on both sides.  Every
    window type of WINDOWS occurs in every window position of a crop (the L * C >= 12 (crop, channel) pairs of a position
    walk through all twelve), the last full window of an odd map included.  The gradient goes to the first maximum in
    row-major order (a '>=' in the kernel's argmax would send windows 4 .. 9 to their last), the last row / column of an
    odd map is exact zeros, and the comparison is EXACT - against the routing written out here and against the float64
    specification."""
    assert L * C >= len(WINDOWS)
    assert all(max(max(w), 0) == max(w[k], 0) and all(max(w[j], 0) < max(w[k], 0) for j in range(k)) for w, k in zip(WINDOWS, FIRST_MAX))
    Ho, Wo = H // 2, W // 2
    sc = torch.ones(C)
    sc[1::2] = -1.0
    sh = torch.zeros(C)
    l_, y_, x_, c_ = torch.meshgrid(torch.arange(L), torch.arange(Ho), torch.arange(Wo), torch.arange(C), indexing='ij')
    kind = (c_ + C * l_ + y_ * Wo + x_) % len(WINDOWS)
    for pos in [(0, 0), (Ho - 1, Wo - 1)]:
        assert sorted(set(kind[:, pos[0], pos[1], :].reshape(-1).tolist())) == list(range(len(WINDOWS)))
    vals = torch.tensor(WINDOWS, dtype=torch.float32)[kind]                                   # [L][Ho][Wo][C][4]
    post = torch.full((L, H, W, C), 3.0)                                                      # leftover row / column: 3
    post[:, :2 * Ho, :2 * Wo] = vals.view(L, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(L, 2 * Ho, 2 * Wo, C)
    Z = (post * sc).reshape(L * H * W, C)                                                     # z sc = post exactly
    dP = rnd(L * Ho * Wo, C, seed=9)
    dP = dP + torch.where(dP < 0, -0.5, 0.5)                                                  # no zero gradient
    arg = torch.tensor(FIRST_MAX)[kind]
    hot = torch.nn.functional.one_hot(arg, 4).float() * dP.view(L, Ho, Wo, C, 1)
    want = torch.zeros(L, H, W, C)
    want[:, :2 * Ho, :2 * Wo] = hot.view(L, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(L, 2 * Ho, 2 * Wo, C)
    dg, dr = check_pool_kernels(hip, 'constructed %dx%d' % (H, W), Z, sc, sh, L, H, W, C, dP=dP)
    assert torch.equal(dr.float().view(L, H, W, C), want)                                     # the specification agrees
    assert torch.equal(dg.cpu().view(L, H, W, C), want)
    Zg, scg, shg = fput(Z), fput(sc), fput(sh)
    (pg,) = twice('constructed pool', lambda: [flat(L * Ho * Wo, C)], lambda A: hip.bn_relu_pool(Zg, C, scg, shg, L, H, W, 1, A))
    assert torch.equal(pg.cpu().view(L, Ho, Wo, C), torch.relu(vals).max(-1)[0])


CAP = 16384 * 256  # (4 channels x 1 output) units one pass of the capped grids of bn_relu_pool / maxpool_bwd covers


@pytest.mark.parametrize('pool,H,W,C', [(0, 512, 513, 64), (1, 1025, 1026, 64)])
def test_bn_relu_pool_beyond_the_grid_cap(hip, pool, H, W, C):
    """more units than 16384 workgroups x 256 threads: the grid-stride loop's second pass (the production path at
    128 x 224 x 224 x 64); without the loop's increment everything behind unit CAP would stay NaN"""
    L = 1
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    assert CAP < L * Ho * Wo * (C // 4) < CAP + CAP // 100
    Z = rnd(L * H * W, C, seed=20) * 2 + 0.3
    sc, sh = mixed_sign(C, 21), rnd(C, seed=22)
    ar = torch.zeros(L * Ho * Wo, C, dtype=torch.float64)
    emu.bn_relu_pool(Z, C, sc, sh, L, H, W, pool, ar)
    Zg, scg, shg = Z.to(DEV), sc.to(DEV), sh.to(DEV)
    (ag,) = twice('bn_relu_pool over the cap', lambda: [flat(L * Ho * Wo, C)],
                  lambda A: hip.bn_relu_pool(Zg, C, scg, shg, L, H, W, pool, A))
    close(ag, ar, 2e-6, 'bn_relu_pool over the cap, pool=%d' % pool)


def test_maxpool_bwd_beyond_the_grid_cap(hip):
    """ceil(H / 2) * ceil(W / 2) * C / 4 just above the cap (C = 4: the smallest tensor, 67 M elements): second pass of the
    loop.  Integer Z with sc = +-1, sh = 0 keeps 17 M windows free of fp32-vs-float64 decisions; ties go to the first."""
    L, H, W, C = 1, 4097, 4097, 4
    assert CAP < L * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4) < CAP + CAP // 100
    g = torch.Generator().manual_seed(23)
    Z = torch.randint(-2, 4, (L * H * W, C), generator=g).float()
    sc, sh = torch.tensor([1.0, -1.0, 1.0, -1.0]), torch.zeros(C)
    dP = rnd(L * (H // 2) * (W // 2), C, seed=24)
    dr = torch.zeros(L * H * W, C, dtype=torch.float64)
    emu.maxpool_bwd(Z, C, sc, sh, dP, L, H, W, dr)
    Zg, scg, shg, dPg = Z.to(DEV), sc.to(DEV), sh.to(DEV), dP.to(DEV)
    (dg,) = twice('maxpool_bwd over the cap', lambda: [flat(L * H * W, C)],
                  lambda dA: hip.maxpool_bwd(Zg, C, scg, shg, dPg, L, H, W, dA))
    close(dg, dr, 1e-6, 'maxpool_bwd over the cap')
    assert torch.equal(dg.cpu(), dr.float())  # routing only: nothing is rounded


# ---- conv3x3_wgrad ----------------------------------------------------------------------------------------------------
# (L, H, W, Cin, Cout, ns, scales).  The shapes of tests/test_train_vgg_gpu.py (all four tile instantiations <64,64>,
# <64,128>, <128,64>, <128,128> of the f16 kernel) at their scale, then:
#   H = 1: the dy = -1 / +1 tap rows are masked everywhere; W = 1: the dx = -1 / +1 taps are; W = 2: each dx tap is masked in
#   every other pixel; all three clamp the six-slot loads at both ends of the tensor;  1 x 1 x 1: one pixel, eight taps zero;
#   64 pixels: exactly one chunk; ns = 5 on one chunk: four shares of the f16 kernel are empty (exact zeros; the fp32
#   kernel splits pixels, none empty);  192 channels: three 64-wide tiles on either axis, <64,64> with grid 3 x 3.
WG_CASES = [(2, 6, 5, 64, 64, 1, (1.0,)), (3, 8, 8, 128, 64, 3, (1.0,)), (1, 4, 4, 64, 256, 2, (1.0,)),
            (5, 14, 14, 128, 128, 4, (1e-6,)), (2, 28, 20, 256, 128, 7, (3e-5,)), (3, 7, 9, 64, 128, 2, (1.0,)),
            (2, 31, 17, 128, 128, 5, (1.0,)), (4, 3, 3, 64, 64, 2, (1.0,)), (1, 70, 66, 64, 64, 9, (1e-4,)),
            (3, 1, 7, 64, 64, 2, (1.0, 1e-6)), (3, 7, 1, 64, 64, 2, (1.0, 1e-6)), (2, 5, 2, 64, 128, 1, (1.0, 1e-6)),
            (1, 1, 1, 64, 64, 1, (1.0, 1e-6)), (1, 8, 8, 64, 64, 1, (1.0, 1e-6)), (1, 8, 8, 64, 64, 5, (1.0, 1e-6)),
            (2, 6, 5, 192, 192, 2, (1.0, 1e-6)), (2, 6, 5, 64, 192, 3, (1.0, 1e-6))]


@functools.lru_cache(None)
def wgrad_case(L, H, W, Cin, Cout):
    """dZ at scale 1 and A, drawn like tests/test_train_vgg_gpu.py draws them, shared by the tests of a shape (a scale is
    applied to dZ in fp32 by the caller, and the float64 reference is taken from the scaled values)"""
    dZ, A = rnd(L * H * W, Cout, seed=10), torch.relu(rnd(L * H * W, Cin, seed=11)) * 2.0
    return dZ, A


def wgrad_reference(dZ, A, L, H, W, Cin, Cout):
    ref = torch.zeros(1, 9 * Cout * Cin, dtype=torch.float64)
    emu.conv3x3_wgrad(dZ, A, L, H, W, Cin, Cout, 1, ref)
    return ref[0]


def check_wgrad(hip, what, f16, dZ, A, ref, L, H, W, Cin, Cout, ns, scale, launch=None):
    """the sum over the shares against the float64 gradient (after dividing by the gradient's scale), no share with a NaN
    (the caller adds them all), empty shares exact zeros"""
    dZg, Ag = fput(dZ), fput(A)
    launch = launch or (lambda dW, dZg, Ag: hip.conv3x3_wgrad(dZg, Ag, L, H, W, Cin, Cout, ns, dW))
    with arithmetic(hip, f16):
        (got,) = twice(what, lambda: [flat(ns, 9 * Cout * Cin)], lambda dW: launch(dW, dZg, Ag))
    assert torch.isfinite(got).all(), what + ': a share holds a non-finite value'
    got = got.cpu().double()
    units = -(-L * H * W // 64) if f16 else L * H * W  # the f16 kernel splits 64-pixel chunks, the fp32 kernel pixels
    for s in range(ns):
        if units * s // ns == units * (s + 1) // ns:
            assert (got[s] == 0).all(), '%s: empty share %d of %d is not zero' % (what, s, ns)
    if scale == 0.0:
        assert (got == 0).all(), what + ': zero dZ, non-zero dW'
    else:
        close(got.sum(0) / scale, ref / scale, 3e-6, what)
    return got


@ARITH
@pytest.mark.parametrize('L,H,W,Cin,Cout,ns,scales', WG_CASES)
def test_conv3x3_wgrad(hip, f16, L, H, W, Cin, Cout, ns, scales):
    dZ1, A = wgrad_case(L, H, W, Cin, Cout)
    for scale in scales:
        dZ = dZ1 * scale
        ref = wgrad_reference(dZ, A, L, H, W, Cin, Cout)
        got = check_wgrad(hip, 'conv3x3_wgrad %s scale %g' % ('f16x3' if f16 else 'f32', scale), f16, dZ, A, ref, L, H, W,
                          Cin, Cout, ns, scale)
        if f16 and (L, H, W, ns) == (1, 8, 8, 5):
            assert sum(int((got[s] == 0).all()) for s in range(ns)) == 4


@ARITH
@pytest.mark.parametrize('L,H,W,Cin,Cout,ns', [(2, 6, 5, 64, 64, 1), (3, 8, 8, 128, 64, 3), (1, 8, 8, 64, 64, 5)])
def test_conv3x3_wgrad_of_a_zero_gradient(hip, f16, L, H, W, Cin, Cout, ns):
    """an all-zero dZ: a zero maximum means 'unscaled' (mm_pow2_shift), dW is exactly zero and finite"""
    dZ1, A = wgrad_case(L, H, W, Cin, Cout)
    check_wgrad(hip, 'conv3x3_wgrad zero dZ', f16, dZ1 * 0.0, A, None, L, H, W, Cin, Cout, ns, 0.0)


@pytest.mark.parametrize('L,H,W,Cin,Cout,ns', [(2, 6, 5, 64, 64, 1), (3, 8, 8, 128, 64, 3), (2, 5, 2, 64, 128, 1),
                                               (2, 31, 17, 128, 128, 5)])
def test_conv3x3_wgrad_f16_without_a_maximum(hip, L, H, W, Cin, Cout, ns):
    """the f16 entry point with dzamax = NULL (no scaling) on O(1) gradients: the same tolerance"""
    dZ, A = wgrad_case(L, H, W, Cin, Cout)
    ref = wgrad_reference(dZ, A, L, H, W, Cin, Cout)

    def launch(dW, dZg, Ag):
        st = hip.lib.mmmot_conv3x3_wgrad_f16(dZg.data_ptr(), Ag.data_ptr(), L, H, W, Cin, Cout, ns, dW.data_ptr(), None, stream())
        assert st == 0
    check_wgrad(hip, 'conv3x3_wgrad_f16 dzamax NULL', True, dZ, A, ref, L, H, W, Cin, Cout, ns, 1.0, launch=launch)


# ---- conv3x3_first_wgrad ----------------------------------------------------------------------------------------------
# (3, 9, 6): the existing shape; W = 1: the x += 4 walk wraps four rows per step; W = 2: two; W = 3: once or twice;
# 1 x 1 x 1: one pixel, three of the four pixel phases idle; (2, 7, 13): W > 4, odd.  Blocks: 1, 5 and P + 3 (more blocks
# than pixels: at least three are empty and write exact zeros)
FW_MAPS = [(3, 9, 6), (2, 5, 1), (2, 4, 2), (3, 3, 3), (1, 1, 1), (2, 7, 13)]


def check_first_wgrad(hip, what, dZ, X, L, H, W, nb, per_block=False):
    P = L * H * W
    ref = torch.zeros(nb, 64 * 28, dtype=torch.float64)
    emu.conv3x3_first_wgrad(dZ, X, L, H, W, ref)
    dZg, Xg = fput(dZ), fput(X)
    (got,) = twice(what, lambda: [flat(nb, 64 * 28)], lambda PW: hip.conv3x3_first_wgrad(dZg, Xg, L, H, W, PW))
    got = got.cpu().double()
    for b in range(nb):
        if P * b // nb == P * (b + 1) // nb:
            assert (got[b] == 0).all(), '%s: empty block %d of %d is not zero' % (what, b, nb)
        elif per_block:
            close(got[b], ref[b], 2e-6, '%s block %d of %d' % (what, b, nb))
    close(got, ref, 2e-6, what + ' per block')
    close(got.sum(0), ref.sum(0), 2e-6, what + ' summed')


@pytest.mark.parametrize('L,H,W', FW_MAPS)
def test_conv3x3_first_wgrad(hip, L, H, W):
    P = L * H * W
    dZ, X = rnd(P, 64, seed=12), rnd(L, 3, H, W, seed=13)
    for nb in (1, 5, P + 3):
        check_first_wgrad(hip, 'first_wgrad %dx%dx%d nb %d' % (L, H, W, nb), dZ, X, L, H, W, nb)


def test_conv3x3_first_wgrad_of_a_cancelling_gradient(hip):
    """what the kernel's float64 accumulators are for: after BatchNorm backward every column of dZ sums to zero (removed here
    in float64, before rounding to fp32) while the input has a mean ten times its spread (X = 1 + 0.1 noise): each tap's sum
    is sum dZ (X - 1) + sum dZ, and a block's sum dZ - no longer zero for a part of the pixels - is what fp32 accumulation
    would have to carry exactly.  Each block's partial against the per-block float64 specification, to 2e-6 of THAT
    block's maximum (adding the blocks is colsum's business)."""
    L, H, W = 2, 7, 13
    P = L * H * W
    d = rnd(P, 64, seed=14).double()
    dZ = (d - d.mean(0, keepdim=True)).float()
    assert dZ.double().sum(0).abs().max().item() < 1e-5
    X = 1.0 + 0.1 * rnd(L, 3, H, W, seed=15)
    for nb in (1, 5):
        check_first_wgrad(hip, 'first_wgrad cancelling nb %d' % nb, dZ, X, L, H, W, nb, per_block=True)


# ---- the input gradient: the forward kernels on dgrad_weights(wp) -----------------------------------------------------
# Cin != Cout in both orders (a transposition that is wrong only then), 192 (three 64-wide tiles), 256 x 128; maps with odd
# sides, a 4 x 4 one (the 4-pixel block edge of the hl16 kernel) and a single row; a gradient of training magnitude
DG_CHANNELS = [(64, 128), (128, 64), (192, 64), (256, 128)]  # (Cout, Cin) of the FORWARD layer
DG_MAPS = [(2, 7, 9), (1, 4, 4), (3, 1, 5)]


@functools.lru_cache(None)
def dgrad_case(L, H, W, Cout, Cin, scale):
    """dZ [P][Cout], the forward weights wp [tap][Cout][Cin], and float64 autograd's d conv2d / d input: no flip in sight"""
    dZ = rnd(L * H * W, Cout, seed=20) * scale
    wp = rnd(9, Cout, Cin, seed=21, scale=(2.0 / (9 * Cin)) ** 0.5)
    x = torch.zeros(L, Cin, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wp.double().view(3, 3, Cout, Cin).permute(2, 3, 0, 1), None, padding=1)
    (gx,) = torch.autograd.grad(y, x, dZ.double().view(L, H, W, Cout).permute(0, 3, 1, 2))
    return dZ, wp, gx.permute(0, 2, 3, 1).reshape(L * H * W, Cin)


@pytest.mark.parametrize('hl16', [False, True], ids=['raw', 'raw_hl16'])
@pytest.mark.parametrize('Cout,Cin', DG_CHANNELS)
def test_input_gradient_through_the_flipped_weights(hip, Cout, Cin, hl16):
    """conv3x3_raw / conv3x3_raw_hl16 exactly as layer_backward_train launches them: on the product's dgrad_weights(wp)
    (not a copy of the expression), Cin and Cout exchanged, a zero bias; the hl16 kernel with the device-side power-of-two
    scales of dZ and of the weights.  Without the flip(0), or without the permute, the result is off by O(1) of its
    maximum (tests/test_train_kernels_cpu.py shows both)."""
    new = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=DEV)
    for L, H, W in DG_MAPS:
        for scale in (1.0, 3e-6):
            dZ, wp, ref = dgrad_case(L, H, W, Cout, Cin, scale)
            P = L * H * W
            dZg, wpg = fput(dZ), wp.to(DEV)
            wflip = dgrad_weights(wpg)
            assert tuple(wflip.shape) == (9, Cin, Cout) and wflip.is_contiguous()
            zero = torch.zeros(Cin, device=DEV)
            what = 'input gradient %s Cout %d Cin %d %dx%dx%d scale %g' % ('hl16' if hl16 else 'f32', Cout, Cin, L, H, W, scale)
            if hl16:
                amz, amw, dz16, wf16, osc = new(1), new(1), new(P, Cout), torch.empty_like(wflip), new(Cin)
                hip.absmax(dZg, amz)
                hip.absmax(wpg, amw)
                hip.hl16_pack_pow2(dZg, dz16, amz, 11)
                hip.hl16_pack_pow2(wflip, wf16, amw, 14)
                hip.pow2_oscale(osc, amz, 11, amw, 14)
                (dX,) = twice(what, lambda: [flat(P, Cin)],
                              lambda out: hip.conv3x3_raw_hl16(dz16, wf16, zero, out, L, H, W, Cout, Cin, osc))
                close(dX.cpu().double() / scale, ref / scale, 3e-6, what)
            else:
                (dX,) = twice(what, lambda: [flat(P, Cin)],
                              lambda out: hip.conv3x3_raw(dZg, wflip, zero, out, L, H, W, Cout, Cin, False))
                close(dX.cpu().double() / scale, ref / scale, 1e-5, what)


# ---- rows_gather_scale ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R,C', [(1, 4), (5000, 512), (1048583, 8)])
def test_rows_gather_scale(hip, R, C):
    """S and X column slices with lds, ldx > C, scale present and absent, equality exact (one fp32 product per element,
    correctly rounded on both sides).  1048583 x 8: R C / 4 = 2097166 units, more than the 8192 x 256 the grid is capped
    at - the grid-stride loop's second pass."""
    if R > 1 << 20:
        assert 8192 * 256 < R * (C // 4) < 8192 * 256 + 64
    S = rnd(37, C, seed=1)
    idx = torch.randint(0, 37, (R,), generator=torch.Generator().manual_seed(2)).int()
    scale = rnd(37, seed=3).abs() + 0.1
    Sg, idxg, scg = sput(S), idx.to(DEV), fput(scale)
    assert Sg.stride(0) > C
    for sc, scd in ((scale, scg), (None, None)):
        ref = torch.zeros(R, C, dtype=torch.float64)
        emu.rows_gather_scale(S, idx, sc, ref, C)
        (got,) = twice('rows_gather_scale', lambda: [slab(R, C, extra=4)], lambda X: hip.rows_gather_scale(Sg, idxg, scd, X, C))
        assert got.stride(0) == C + 8
        assert torch.equal(got.cpu(), ref.float())


# ---- pointnet_layer1_bwd ----------------------------------------------------------------------------------------------
# one row (three row quarters idle), 127 / 128 (a full tile) / 129 rows (a second tile of one row), tiles of one group
PN_TILINGS = [[1], [127], [128], [129], [5, 300, 128, 1]]


def check_pointnet_l1(hip, what, dY, X, counts):
    tc, tg = both(counts)
    K = X.shape[1]
    ref = torch.zeros(tc.T, 64 * (K + 1), dtype=torch.float64)
    emu.pointnet_layer1_bwd(dY, X, tc, ref)
    dYg, Xg = fput(dY), fput(X)
    (got,) = twice(what, lambda: [flat(tc.T, 64 * (K + 1))], lambda PW: hip.pointnet_layer1_bwd(dYg, Xg, tg, PW))
    for t in range(tc.T):
        close(got[t], ref[t], 2e-6, '%s tile %d' % (what, t))


@pytest.mark.parametrize('K', [3, 4])
def test_pointnet_layer1_bwd(hip, K):
    for counts in PN_TILINGS:
        R = sum(counts)
        check_pointnet_l1(hip, 'pointnet_layer1_bwd K %d %s' % (K, counts), rnd(R, 64, seed=4), rnd(R, K, seed=5) * 10, counts)


@pytest.mark.parametrize('K', [3, 4])
def test_pointnet_layer1_bwd_of_a_cancelling_gradient(hip, K):
    """what its float64 accumulators are for: the columns of dY sum to zero over every tile (removed in float64 before
    rounding) against coordinates tens of metres from the origin with decimetres of spread - each tile to 2e-6 of its own
    maximum, which is 0.2 / 40 of what the uncancelled terms reach"""
    counts = [5, 300, 128, 1]
    tc = RowTiles(counts, 'cpu')
    R = sum(counts)
    d = rnd(R, 64, seed=4).double()
    for t in range(tc.T):
        r0, n = int(tc.h_row0[t]), int(tc.h_nrows[t])
        d[r0:r0 + n] -= d[r0:r0 + n].mean(0, keepdim=True)
    dY = d.float()
    centre = torch.tensor([40.0, -15.0, 2.0, 0.3])[:K]
    X = centre + 0.2 * rnd(R, K, seed=5)
    check_pointnet_l1(hip, 'pointnet_layer1_bwd cancelling K %d' % K, dY, X, counts)


# ---- score_loss -------------------------------------------------------------------------------------------------------
SL_N, SL_M = 13, 9  # R C = 3 x 117 = 351 elements: with 64 blocks only blocks 0 (256 elements) and 1 (95) receive any


def score_inputs(kind):
    g = torch.Generator().manual_seed(kind)
    C = SL_N * SL_M
    x = torch.randn(3, C, generator=g) * 2
    y = (torch.rand(C, generator=g) > 0.7).float()
    mrow, mcol = (torch.rand(SL_N, generator=g) > 0.3).float(), (torch.rand(SL_M, generator=g) > 0.3).float()
    ign = y.clone()
    ign[::5] = -1.0
    masks = [dict(), dict(mrow=mrow, mcol=mcol, M=SL_M, mask_mode=1), dict(mcol=ign, M=C, mask_mode=2)]
    return x, y, masks


def mask_of(mask, C):
    m = torch.ones(C, dtype=torch.float64)
    if mask:
        ind = (lambda v: (v == 1.0)) if mask['mask_mode'] == 1 else (lambda v: (v != -1.0))
        c = torch.arange(C)
        if mask.get('mrow') is not None:
            m = m * ind(mask['mrow'][c // mask['M']]).double()
        if mask.get('mcol') is not None:
            m = m * ind(mask['mcol'][c % mask['M']]).double()
    return m


def off_the_smooth_l1_switch(x, y, mask, special=()):
    """moves x where | |x m - y| - 1 | < 1e-4 (fp32 has x m - y to 6e-8 |.|), then asserts it.  Not judged: masked columns
    (m = 0: d = -y is exact on both sides, on the switch or not) and `special`, the columns holding constructed values."""
    C = x.shape[1]
    m = mask_of(mask, C)
    dist = lambda: ((x.double() * m - y.double()).abs() - 1.0).abs()
    keep = m != 0
    keep[list(special)] = False
    for _ in range(4):
        x[:, keep] += torch.where(dist() < 1e-4, 0.01, 0.0).float()[:, keep]
    assert dist()[:, keep].min().item() >= 1e-4


def check_score_loss(hip, what, x, y, kind, mask, nblocks, accumulate, tol_g=2e-6):
    R_, C = x.shape
    gr, pr = torch.zeros(R_, C, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    emu.score_loss(x, y, kind, 0.37, gr, pr, **mask)
    xg, yg = sput(x), fput(y)
    assert xg.stride(0) > C
    dmask = {k: (fput(v) if torch.is_tensor(v) else v) for k, v in mask.items()}
    start = torch.arange(nblocks).float() * 0.5 + 5.0

    def make():
        buf, v = flat(nblocks)
        if accumulate:
            v.copy_(start)
        return [slab(R_, C), (buf, v)]
    gg, pg = twice(what, make, lambda g, PL: hip.score_loss(xg, yg, kind, 0.37, g, PL, accumulate=accumulate, **dmask))
    assert gg.stride(0) > C
    close(gg, gr, tol_g, what + ' gradient')
    pg = pg.cpu().double() - (start.double() if accumulate else 0.0)
    assert torch.isfinite(pg).all()
    assert abs(pg.sum().item() - pr.item()) < 1e-5 * (1 + abs(pr.item())), (what, pg.sum().item(), pr.item())
    for b in range(nblocks):  # block b takes the elements 256 b .. 256 b + 255, then strides by 256 nblocks
        if 256 * b >= R_ * C:
            assert pg[b].item() == 0.0, '%s: block %d received no element and %s' % (
                what, b, 'changed its value' if accumulate else 'did not write 0')


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('nblocks', [1, 3, 64])
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_score_loss(hip, kind, nblocks, accumulate):
    """1 block: two trips of its grid-stride loop, every element in one sum; 3 blocks: 351 elements over 3 x 256 threads,
    block 2 receives none; 64: 62 such blocks - without `accumulate` they write exact 0, with it they leave their value.
    x and g column slices (ldx, ldg > C), the three mask forms."""
    x, y, masks = score_inputs(kind)
    for mask in masks:
        x1 = x.clone()
        if kind == 2:
            off_the_smooth_l1_switch(x1, y, mask)
        check_score_loss(hip, 'score_loss kind %d nb %d acc %d' % (kind, nblocks, accumulate), x1, y, kind, mask, nblocks, accumulate)


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_score_loss_of_huge_logits(hip, kind):
    """x = +-100 and +-1e4 against both targets: expf(-x) overflows to inf for x = -100 already (1 / (1 + inf) = 0) and
    expf(-|x|) underflows; loss and gradient stay finite and meet the tolerances (judged on their own tensor: its maximum
    is 2e4 for the L2 gradient)"""
    x, y, _ = score_inputs(kind)
    big = torch.tensor([100.0, -100.0, 1e4, -1e4])
    x[:, 1:5], x[:, 11:15] = big, big
    y[1:5], y[11:15] = 0.0, 1.0
    if kind == 2:
        off_the_smooth_l1_switch(x, y, {})
    check_score_loss(hip, 'score_loss huge kind %d' % kind, x, y, kind, {}, 3, False)


@pytest.mark.parametrize('kind', [1, 2])
def test_smooth_l1_at_its_switch(hip, kind):
    """d = x - y = +-(1 - 2^-20) and +-(1 + 2^-20), built from exactly representable x and y in {0, 1} so that fp32 computes
    d exactly and both sides take the same branch (asserted); kind 1: L2 on the same inputs"""
    e = 2.0 ** -20
    x, y, _ = score_inputs(kind)
    d = torch.tensor([1 - e, -(1 - e), 1 + e, -(1 + e)], dtype=torch.float64)
    cols = list(range(1, 5)) + list(range(11, 15))
    y[1:5], y[11:15] = 0.0, 1.0
    x[:, 1:5], x[:, 11:15] = d.float(), (d + 1.0).float()
    got = x[:, cols].double() - y[cols].double()
    assert torch.equal(got, torch.cat([d, d]).expand(3, 8))                         # exactly representable
    assert torch.equal((x[:, cols] - y[cols]).double(), got)                        # and fp32 subtracts them exactly
    assert torch.equal((got.abs() - 1.0).abs(), torch.full((3, 8), e, dtype=torch.float64))
    off_the_smooth_l1_switch(x, y, {}, special=cols)
    check_score_loss(hip, 'score_loss at |d| = 1, kind %d' % kind, x, y, kind, {}, 3, False)


# ---- ghm_loss ---------------------------------------------------------------------------------------------------------
def ghm_inputs(R_, C, bins, all_ignored=False):
    """x, y with (columns 1 .. 6) x in {0, 40, -200} against y in {0, 1}: gradient lengths exactly 0.5, 1, 0, 0.5, 0, 1;
    every other valid element at least 1e-5 from every bin edge in float64 (fp32 has sigmoid(x) to a few 1e-7); asserted"""
    x = rnd(R_, C, seed=70) * 3
    y = (rnd(C, seed=71) > 0).float()
    y[::7] = -1.0
    x[:, 1:7] = torch.tensor([0.0, 40.0, -200.0, 0.0, 40.0, -200.0])
    y[1:7] = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    edges = torch.tensor([i / bins for i in range(bins)] + [1.0, 1.0 + 1e-6], dtype=torch.float64)
    valid = (y != -1.0).expand(R_, C).clone()
    valid[:, 1:7] = False

    def near():
        gl = (torch.sigmoid(x.double()) - y.double()).abs()
        return ((gl.unsqueeze(-1) - edges).abs().min(-1)[0] < 1e-5) & valid
    for _ in range(4):
        x[near()] += 0.01
    assert not near().any()
    # the constructed elements, in the float32 arithmetic of the bin decisions
    gl = (torch.sigmoid(x[0, 1:7]) - y[1:7]).abs()
    assert gl.tolist() == [0.5, 1.0, 0.0, 0.5, 0.0, 1.0]
    e32 = torch.tensor([i / bins for i in range(bins)] + [1.0 + 1e-6], dtype=torch.float64).float()
    bin_of = lambda v: [b for b in range(bins) if e32[b] <= v < e32[b + 1]]
    assert bin_of(0.5) == [bins // 2] and bin_of(1.0) == [bins - 1] and bin_of(0.0) == [0]  # 0.5: edge 15 of 30
    if all_ignored:
        y[:] = -1.0
    return x, y


def check_ghm(hip, what, x, y, bins, mom, accumulate):
    R_, C = x.shape
    acc0 = rnd(bins, seed=72).abs().double() * 5 + 0.5
    gr, pr, ar = torch.zeros(R_, C, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), acc0.clone()
    emu.ghm_loss(x, y, 1.5, gr, pr, ar, bins=bins, momentum=mom)
    xg, yg = sput(x), fput(y)
    accs = []

    def launch(g, PL):
        buf = torch.full((bins + 16,), NAN, dtype=torch.float64, device=DEV)
        buf[8:8 + bins] = acc0.to(DEV)
        hip.ghm_loss(xg, yg, 1.5, g, PL, buf[8:8 + bins], bins=bins, momentum=mom, accumulate=accumulate)
        accs.append(buf.cpu())

    def make():
        buf, v = flat(1)
        v.fill_(2.0)
        return [slab(R_, C), (buf, v)]
    gg, pg = twice(what, make, launch)
    assert gg.stride(0) > C and xg.stride(0) > C
    close(gg, gr, 2e-6, what + ' gradient')
    loss = pg.item() - (2.0 if accumulate else 0.0)
    assert abs(loss - pr.item()) < 1e-5 * (1 + abs(pr.item())), (what, loss, pr.item())
    assert torch.equal(accs[0][8:8 + bins], accs[1][8:8 + bins])
    for a in accs:
        assert torch.isnan(a[:8]).all() and torch.isnan(a[8 + bins:]).all(), what + ': acc_sum written out of bounds'
    ag = accs[0][8:8 + bins]
    assert (ag - ar).abs().max().item() < 1e-9 * (1 + ar.abs().max().item())
    assert (gg.cpu()[:, y == -1.0] == 0).all()  # ignored targets carry no gradient
    return gg, loss, ag, acc0


@pytest.mark.parametrize('mom', [0.0, 0.75])
@pytest.mark.parametrize('bins', [1, 30, 64])
@pytest.mark.parametrize('R_,C', [(3, 700), (1, 11)])
def test_ghm_loss(hip, R_, C, bins, mom):
    """3 x 700: nine trips of the 256-thread loops; bins = 1 (everything in one bin) and 64 (the most the kernel holds);
    gradient lengths exactly on the edges 0, 0.5 and 1.0 - the last must land in the last bin through its + 1e-6 edge;
    x and g column slices; with momentum 0 acc_sum is not written"""
    x, y = ghm_inputs(R_, C, bins)
    for accumulate in (False, True):
        _, _, ag, acc0 = check_ghm(hip, 'ghm %dx%d bins %d mom %g' % (R_, C, bins, mom), x, y, bins, mom, accumulate)
        if mom == 0.0:
            assert torch.equal(ag, acc0)
        else:
            assert not torch.equal(ag, acc0)


@pytest.mark.parametrize('mom', [0.0, 0.75])
def test_ghm_loss_with_every_target_ignored(hip, mom):
    x, y = ghm_inputs(3, 700, 30, all_ignored=True)
    gg, loss, ag, acc0 = check_ghm(hip, 'ghm all ignored', x, y, 30, mom, False)
    assert (gg == 0).all() and loss == 0.0 and torch.equal(ag, acc0)


# ---- launcher rejections ----------------------------------------------------------------------------------------------
def test_launchers_reject_what_the_kernels_cannot_take(hip):
    """through the status code: nothing is launched by a rejected call.  Each entry point first takes a tiny valid call
    (status 0), then the same call with ONE argument changed."""
    lib, s = hip.lib, stream()
    z, out = torch.zeros(1 << 16, device=DEV), torch.zeros(1 << 16, device=DEV)
    acc = torch.ones(64, dtype=torch.float64, device=DEV)
    zi = torch.zeros(16, dtype=torch.int32, device=DEV)
    t = RowTiles([1], DEV)
    p, o, r0, nr = z.data_ptr(), out.data_ptr(), t.row0.data_ptr(), t.nrows.data_ptr()

    def sweep(fn, base, changes):
        assert fn(*base) == 0, fn.__name__
        for pos, val in changes:
            args = list(base)
            args[pos] = val
            assert fn(*args) == EINVAL, (fn.__name__, pos, val)
    sweep(lib.mmmot_rows_stats, (p, 8, 8, r0, nr, 1, o, s), [(2, 6), (0, p + 4), (6, o + 4)])
    sweep(lib.mmmot_bn_relu_pool, (p, 8, p, p, 1, 2, 2, 1, o, s),
          [(1, 6), (0, p + 4), (2, p + 4), (3, p + 4), (8, o + 4), (5, 1), (6, 1)])        # pool with H < 2, W < 2
    sweep(lib.mmmot_maxpool_bwd, (p, 8, p, p, p, 1, 2, 2, o, s),
          [(1, 6), (0, p + 4), (2, p + 4), (3, p + 4), (4, p + 4), (8, o + 4), (6, 1), (7, 1)])
    sweep(lib.mmmot_rows_gather_scale, (p, 8, zi.data_ptr(), None, o, 8, 1, 8, s), [(7, 6), (0, p + 4), (4, o + 4)])
    sweep(lib.mmmot_conv3x3_wgrad, (p, p, 1, 1, 1, 64, 64, 1, o, s), [(7, 0), (7, 257)])
    sweep(lib.mmmot_conv3x3_wgrad_f16, (p, p, 1, 1, 1, 64, 64, 1, o, None, s), [(7, 0), (7, 257), (0, p + 4), (1, p + 4)])
    sweep(lib.mmmot_conv3x3_first_wgrad, (p, p, 1, 1, 1, o, 1, s), [(6, 0), (6, 65536)])
    sweep(lib.mmmot_pointnet_layer1_bwd, (p, p, 3, r0, nr, 1, o, s), [(2, 5)])
    sweep(lib.mmmot_score_loss, (p, 8, p, None, None, 0, 0, -1.0, 0, 1.0, 1, 8, o, 8, o + 4096, 1, 0, s), [(15, 4097), (15, 0)])
    sweep(lib.mmmot_ghm_loss, (p, 8, p, -1.0, 1.0, 1, 8, 30, 0.75, acc.data_ptr(), o, 8, o + 4096, 0, s),
          [(7, 0), (7, 65), (8, 1.0), (1, 7), (11, 7)])                                     # bins, momentum, ldx < C, ldg < C
    torch.cuda.synchronize()


# ---- one trunk layer, forward and backward ----------------------------------------------------------------------------
# worst error of each output over the six cases and both arithmetics, as a fraction of the reference's maximum (db: of
# max |dZ| x rows), measured on an MI355X; the test asserts four times that (the arithmetic is deterministic: the factor
# covers another seed or shape, not noise)
LAYER_MEASURED = dict(A=6.5e-7, dX=1.3e-6, dW=4.0e-7, db=1.8e-8, dgamma=5.0e-7, dbeta=1.3e-7)


@ARITH
@pytest.mark.parametrize('case', list(LAYER_CASES), ids=lambda c: 'x'.join(map(str, c)))
def test_one_trunk_layer_forward_and_backward(hip, case, f16):
    """layer_forward_train / layer_backward_train of mmmot_amd/train_vgg.py - the bodies of the trunk's layer loops - on
    ONE layer against float64 autograd through conv2d -> batch_norm(training) -> relu (-> max_pool2d).  The inputs keep
    every BatchNorm output MARGIN = 3e-5 max|y| from zero and the two largest values of every pool window that far apart
    (asserted on the CPU), and the device's normalised output is within a quarter of that of the reference everywhere
    (asserted after the forward): every ReLU and argmax decision is the same on both sides, nothing is excluded, and the
    gradients are held to a kernel-level tolerance instead of the 3e-2 .. 5e-2 of the end-to-end tests.
    Measured (MI355X, worst over the cases, f16x3 / f32): the normalised output 7.5e-7 of max |y| (the limit is 7.5e-6),
    A 6.4e-7 / 5.7e-7, dX 7.1e-7 / 1.2e-6, dW 3.9e-7 / 2.9e-7, dgamma 4.7e-7 / 5.0e-7, dbeta 1.3e-7 / 1.3e-7, db 1.8e-8 / 1.3e-8
    of max |dZ| x rows; the first-layer cases (no dX) stay below 1.6e-7 everywhere.  LAYER_MEASURED rounds these up."""
    inputs, ref = layer_case(case)
    with arithmetic(hip, f16):
        ly, got = run_layer(hip, case, inputs, torch.float32, DEV)
    torch.cuda.synchronize()
    Lyr = ly['L']
    y = (Lyr.Y.double() * Lyr.sc.double() + Lyr.sh.double()).cpu()  # the kernels' fmaf(z, sc, sh) to 1e-7 of |y|
    top = ref['y'].abs().max().item()
    assert (y - ref['y']).abs().max().item() <= MARGIN / 4 * top
    err = layer_errors(case, got, ref)
    print('layer %s %s: %s' % (case, 'f16x3' if f16 else 'f32', ' '.join('%s=%.2e' % kv for kv in sorted(err.items()))))
    for k, e in err.items():
        assert e <= 4 * LAYER_MEASURED[k], (k, e, LAYER_MEASURED[k])
