"""Every launch branch of the head's backward kernels (csrc/backward.hip, csrc/gemm_tn_f16.hip, mmmot_absmax) against
the float64 specification in tests/fake_ops.py, which tests/test_backward_cpu.py pins against torch.autograd.

Conventions of every case:
* outputs with a leading dimension are column slices (offset 4, row stride > row length) of a NaN buffer with 8 guard
  rows above and below; outputs without one (dW, db, P, M, dlogits, DN) lie between 8 guard rows of NaN in a flat
  buffer.  After the launch the slice is compared with the specification and everything around it must still be NaN: an
  out-of-bounds write shows without leaving allocated memory.  pair_bwd's dF accumulates, so its slice starts from
  known non-zero values;
* inputs are column slices of NaN buffers too wherever the entry point takes a leading dimension: a read beside the
  operand poisons the result;
* every case is launched twice on fresh buffers and the two results must be equal bit for bit;
* inputs that sit on a decision boundary (the ReLU mask of gn_bwd, p == q of dual_max) would make fp32 and float64
  take different branches: the distance from the boundary is asserted on the CPU before anything is launched, and no
  element is excluded from a comparison.

Tolerances are those of tests/test_backward_gpu.py, as a fraction of the reference's maximum."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

from fake_ops import TorchOps
from mmmot_amd.plan import BatchPlan, RowTiles
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
GUARD = 8
EINVAL = -1
emu = TorchOps()


# ---- guarded buffers --------------------------------------------------------------------------------------------------
def slab(rows, cols, off=4, extra=8):
    """(buffer, view): a [rows][cols] column slice at column `off` of a NaN buffer, GUARD rows above and below"""
    buf = torch.full((rows + 2 * GUARD, off + cols + extra), NAN, device=DEV)
    return buf, buf[GUARD:GUARD + rows, off:off + cols]


def flat(*shape):
    """(buffer, view): a contiguous tensor between GUARD rows of NaN on either side (entry points without an ld)"""
    n, g = int(np.prod(shape)), GUARD * int(shape[-1])
    g += -g % 4  # keeps the view 16-byte aligned
    buf = torch.full((n + 2 * g,), NAN, device=DEV)
    return buf, buf[g:g + n].view(*shape)


def put(t):
    """a 2-D input on the device as a strided column slice of a NaN buffer (1-D inputs: between NaN guards)"""
    buf, v = slab(*t.shape) if t.dim() == 2 else flat(*t.shape)
    v.copy_(t)
    return v


def untouched(buf, view, what):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    outside = buf[~inside]
    assert torch.isnan(outside).all(), '%s: %d elements written outside the output' % (what, int((~torch.isnan(outside)).sum()))


def twice(what, make, launch):
    """launch(*views) on two fresh sets of guarded outputs: bit-equal results, nothing written around them; -> views"""
    runs = []
    for _ in range(2):
        outs = make()
        launch(*[v for _, v in outs])
        runs.append(outs)
    for k, ((b0, v0), (b1, v1)) in enumerate(zip(*runs)):
        assert torch.equal(v0, v1), '%s: output %d differs between two launches' % (what, k)
        untouched(b0, v0, '%s output %d' % (what, k))
        untouched(b1, v1, '%s output %d' % (what, k))
    return [v for _, v in runs[0]]


def both(counts):
    return RowTiles(counts, 'cpu'), RowTiles(counts, DEV)


def row_groups(tiles):
    return torch.repeat_interleave(torch.arange(tiles.G), torch.as_tensor(tiles.h_g_count).long())


@contextlib.contextmanager
def arithmetic(hip, f16):
    """the weight-gradient GEMM on the fp16 matrix cores (mmmot_gemm_tn_f16) or exact fp32 (mmmot_gemm_tn)"""
    prev, hip.tn_f16 = hip.tn_f16, f16
    try:
        yield
    finally:
        hip.tn_f16 = prev


ARITH = pytest.mark.parametrize('f16', [True, False], ids=['f16x3', 'f32'])


# ---- gemm_tn ----------------------------------------------------------------------------------------------------------
# one (N, K) per instantiation of gemm_tn_f16_kernel (<128,128>, <128,64>, <64,128>, <64,64>) and a 3 x 5 grid of <64,64>
TN_NK = [(128, 128), (128, 192), (64, 128), (64, 64), (192, 320)]
# row quads and 16-row MFMA steps that are partly valid, full tiles, a last tile of one row
TN_COUNTS = [[1], [3], [127], [128], [129], [5, 300, 128, 1]]


def check_gemm_tn(hip, what, tc, tg, N, K, dY, kw_c, kw_g, scale=1.0, nsplits=None):
    """all of nsplit in (1, T, T + 3), with and without db: per-share partials against the specification's shares, empty
    shares exact zeros, the sum of the shares against the nsplit = 1 specification"""
    T = tc.T
    dYg = put(dY)
    whole = None
    for ns in nsplits or (1, T, T + 3):
        dWc, dbc = torch.zeros(ns, N, K, dtype=torch.float64), torch.zeros(ns, N, dtype=torch.float64)
        emu.gemm_tn(dY, tc, N, K, dWc, dbc, nsplit=ns, **kw_c)
        if ns == 1:
            whole = (dWc[0], dbc[0])
        dWg, dbg = twice('%s nsplit %d' % (what, ns), lambda: [flat(ns, N, K), flat(ns, N)],
                         lambda dW, db: hip.gemm_tn(dYg, tg, N, K, dW, db, nsplit=ns, **kw_g))
        (dW0,) = twice('%s nsplit %d, no db' % (what, ns), lambda: [flat(ns, N, K)],
                       lambda dW: hip.gemm_tn(dYg, tg, N, K, dW, None, nsplit=ns, **kw_g))
        assert torch.equal(dW0, dWg), '%s nsplit %d: dW depends on db' % (what, ns)
        dWg, dbg = dWg.cpu().double() / scale, dbg.cpu().double() / scale
        close(dWg, dWc / scale, 2e-6, '%s dW (nsplit %d)' % (what, ns))
        close(dbg, dbc / scale, 2e-6, '%s db (nsplit %d)' % (what, ns))
        for s in range(ns):
            if T * s // ns == T * (s + 1) // ns:
                assert (dWg[s] == 0).all() and (dbg[s] == 0).all(), '%s: empty share %d of %d is not zero' % (what, s, ns)
        close(dWg.sum(0), whole[0] / scale, 2e-6, '%s dW summed over %d shares' % (what, ns))
        close(dbg.sum(0), whole[1] / scale, 2e-6, '%s db summed over %d shares' % (what, ns))


@ARITH
@pytest.mark.parametrize('N,K', TN_NK)
@pytest.mark.parametrize('amode', [0, 1])
def test_gemm_tn_rows(hip, amode, N, K, f16):
    """plain and normalise + ReLU A operands over every tile-length class; amode 1 also over two groups of [129, 3] rows
    (per-group sc / sh), X / sc / sh / dY as strided slices"""
    for counts in TN_COUNTS + ([[129, 3]] if amode else []):
        tc, tg = both(counts)
        X, dY = rnd(tc.R, K, seed=40), rnd(tc.R, N, seed=41)
        kw_c = dict(X=X)
        if amode:
            kw_c.update(sc=rnd(tc.G, K, seed=42) + 1.0, sh=rnd(tc.G, K, seed=43) * 0.5)
        kw_g = {k: put(v) for k, v in kw_c.items()}
        with arithmetic(hip, f16):
            check_gemm_tn(hip, 'gemm_tn amode %d %s' % (amode, counts), tc, tg, N, K, dY, dict(kw_c, amode=amode),
                          dict(kw_g, amode=amode))


@ARITH
@pytest.mark.parametrize('N,K', TN_NK)
@pytest.mark.parametrize('pairop', [0, 1, 2])
def test_gemm_tn_pair(hip, pairop, N, K, f16):
    """the pairwise A operand over a 3-frame sample, a 1 x 1 pair and a 12 x 11 pair (a full tile and a 4-row one), F a
    column slice with ldf > K"""
    samples = [([3, 2, 4], None), ([1, 1], None), ([12, 11], None)]
    pc, pg = BatchPlan(samples, 32, 'cpu', use_points=False), BatchPlan(samples, 32, DEV, use_points=False)
    tc, tg = pc.pair_tiles, pg.pair_tiles
    assert sorted(set(tc.h_nrows.tolist())) == [1, 4, 6, 8, 128]
    F, dY = rnd(3 * pc.Lt, K, seed=44), rnd(tc.R, N, seed=45)
    Fg = put(F)
    assert Fg.stride(0) > K
    pair_c = dict(row0=tc.g_row0, M=pc.pg_M, aoff=pc.pg_aoff, boff=pc.pg_boff)
    pair_g = dict(row0=tg.g_row0, M=pg.pg_M, aoff=pg.pg_aoff, boff=pg.pg_boff)
    with arithmetic(hip, f16):
        check_gemm_tn(hip, 'gemm_tn pair op %d' % pairop, tc, tg, N, K, dY,
                      dict(FA=F, FB=F, pair=pair_c, amode=2, pairop=pairop), dict(FA=Fg, FB=Fg, pair=pair_g, amode=2, pairop=pairop))


@ARITH
@pytest.mark.parametrize('mag', ['1', '1e-6', '1e-20', 'outlier', 'zero'])
def test_gemm_tn_gradient_magnitude(hip, mag, f16):
    """gradients of training size and far below: the fp16 kernel scales dY by a power of two taken from its maximum on
    the device, so the result relative to the gradient's scale does not depend on that scale.  'outlier': one element
    1e4 times the rest (the scale follows it; judged on the tensor maximum like every case).  An all-zero dY gives
    exact zeros, nothing non-finite (a zero maximum means 'unscaled')."""
    N, K = 128, 192
    tc, tg = both([5, 300, 128, 1])
    X, sc, sh = rnd(tc.R, K, seed=46), rnd(tc.G, K, seed=47) + 1.0, rnd(tc.G, K, seed=48) * 0.5
    scale = 1e-6 if mag == 'outlier' else 0.0 if mag == 'zero' else float(mag)
    dY = rnd(tc.R, N, seed=49) * scale
    if mag == 'outlier':
        dY[200, 77] = 1e4 * scale
    kw_c = dict(X=X, sc=sc, sh=sh, amode=1)
    kw_g = dict(X=put(X), sc=put(sc), sh=put(sh), amode=1)
    with arithmetic(hip, f16):
        if mag == 'zero':
            dW, db = twice('gemm_tn zero dY', lambda: [flat(3, N, K), flat(3, N)],
                           lambda dW, db: hip.gemm_tn(put(dY), tg, N, K, dW, db, nsplit=3, **kw_g))
            assert (dW == 0).all() and (db == 0).all()
        else:
            check_gemm_tn(hip, 'gemm_tn dY %s' % mag, tc, tg, N, K, dY, kw_c, kw_g, scale=scale, nsplits=(1, 3))


# ---- absmax -----------------------------------------------------------------------------------------------------------
def run_absmax(hip, X, ld, R, C):
    def launch(out):
        st = hip.lib.mmmot_absmax(X.data_ptr(), ld, R, C, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == 0
    (out,) = twice('absmax', lambda: [flat(1)], launch)
    return out.item()


@pytest.mark.parametrize('R,C', [(1, 4), (7, 132), (300, 64), (4097, 2048)])
def test_absmax(hip, R, C):
    """contiguous (through HipOps) and strided (ld > C), the maximum a negative element, all zeros; 4097 x 2048 (34 MB) asks
    for 1025 workgroups, more than the 1024 the launch is capped at: the grid-stride loop runs"""
    X = rnd(R, C, seed=50)
    X[R - 1, C - 3] = -9.5  # the maximum is a negative element, in the last row
    want = X.abs().max().item()
    assert want == 9.5
    Xg = X.to(DEV)
    out = torch.full((1,), NAN, device=DEV)
    hip.absmax(Xg, out)
    assert out.item() == want
    assert run_absmax(hip, Xg, C, R, C) == want
    if R * C > 1 << 22:
        assert (R * (C // 4) + 2047) // 2048 > 1024
        wide = torch.full((R, C + 8), NAN, device=DEV)  # a full slab would double the 34 MB
        Xs = wide[:, 4:4 + C]
        Xs.copy_(Xg)
    else:
        Xs = put(X)
    assert Xs.stride(0) > C
    assert run_absmax(hip, Xs, Xs.stride(0), R, C) == want
    X[R - 1, C - 3] = 0.5  # without the outlier: an ordinary element, wherever it lies
    Xs[R - 1, C - 3] = 0.5
    assert run_absmax(hip, Xs, Xs.stride(0), R, C) == X.abs().max().item()
    Xs.zero_()
    assert run_absmax(hip, Xs, Xs.stride(0), R, C) == 0.0


# ---- GroupNorm backward -------------------------------------------------------------------------------------------------
# narrow path (C <= 512): 64 (4 row phases per 16 .. 256 threads), 192 and 320 (256 / (C/4) is no integer: idle threads),
# 512 (one phase); wide path: 516 (smallest, a partly idle workgroup), 1024 (production), 2048 (gridDim.y = 2);
# (1024, 1): C / NG > 256, the strided loop of finalize
GN_CASES = [(64, 64), (64, 4), (192, 1), (320, 320), (512, 16), (516, 1), (1024, 1024), (1024, 1), (2048, 8)]


def gn_inputs(R, G, C, grp, seed=0):
    """Y, dA, sc1, sh1, gamma, beta with every z = yhat * gamma + beta at least 1e-5 from the ReLU kink in float64 (Y is
    moved by 0.25 where it is not; asserted, so another seed cannot put an element on the boundary unnoticed)"""
    Y, dA = rnd(R, C, seed=seed + 1), rnd(R, C, seed=seed + 2)
    sc1, sh1 = rnd(G, C, seed=seed + 3).abs() + 0.3, rnd(G, C, seed=seed + 4) * 0.2
    gamma, beta = rnd(C, seed=seed + 5), rnd(C, seed=seed + 6) * 0.3
    gamma = gamma + torch.where(gamma < 0, -0.5, 0.5)  # both signs, |gamma| >= 0.5
    z = lambda: (Y.double() * sc1[grp].double() + sh1[grp].double()) * gamma.double() + beta.double()
    Y[z().abs() < 1e-4] += 0.25
    assert z().abs().min().item() >= 1e-5
    return Y, dA, sc1, sh1, gamma, beta


def check_gn(hip, what, tc, tg, C, NG, relu, cpu, gpu):
    """the three kernels on (dA, Y, sc1, sh1, gamma, beta) given as CPU tensors and as device views"""
    R, G = tc.R, tc.G
    dA, Y, sc1, sh1, gamma, beta = cpu
    dAg, Yg, sc1g, sh1g, gammag, betag = gpu
    Pc = torch.zeros(tc.T, 2, C)
    emu.gn_bwd_partial(dA, Y, C, sc1, sh1, gamma, beta, relu, tc, Pc)
    (Pg,) = twice(what + ' partial', lambda: [flat(tc.T, 2, C)],
                  lambda P: hip.gn_bwd_partial(dAg, Yg, C, sc1g, sh1g, gammag, betag, relu, tg, P))
    close(Pg, Pc, 2e-5, what + ' gn_bwd_partial')
    S = torch.stack([Pc[int(tc.h_g_tile0[g]):int(tc.h_g_tile0[g]) + int(tc.h_g_ntiles[g])].sum(0) for g in range(G)])
    S = S.reshape(G * 2, C).contiguous()
    Mc = torch.zeros(G, 2, C)
    emu.gn_bwd_finalize(S, tc, C, NG, gamma, Mc)
    Sg = put(S.reshape(-1)).view(G * 2, C)
    (Mg,) = twice(what + ' finalize', lambda: [flat(G, 2, C)], lambda M: hip.gn_bwd_finalize(Sg, tg, C, NG, gammag, M))
    close(Mg, Mc, 2e-6, what + ' gn_bwd_finalize')
    dYc = torch.zeros(R, C)
    emu.gn_bwd_apply(dA, Y, C, sc1, sh1, gamma, beta, relu, Mc, tc, dYc)
    Mcg = put(Mc.reshape(-1)).view(G, 2, C)
    (dYg,) = twice(what + ' apply', lambda: [slab(R, C)],
                   lambda dY: hip.gn_bwd_apply(dAg, Yg, C, sc1g, sh1g, gammag, betag, relu, Mcg, tg, dY))
    close(dYg, dYc, 2e-6, what + ' gn_bwd_apply')


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('C,NG', GN_CASES)
def test_gn_backward(hip, C, NG, relu):
    tc, tg = both([5, 300, 128, 1])
    assert tc.G == 4
    cpu = gn_inputs(tc.R, tc.G, C, row_groups(tc))
    Y, dA, sc1, sh1, gamma, beta = cpu
    gpu = (put(dA), put(Y), put(sc1), put(sh1), put(gamma), put(beta))
    assert gpu[0].stride(0) > C and gpu[2].stride(0) > C
    check_gn(hip, 'C %d NG %d relu %d' % (C, NG, relu), tc, tg, C, NG, relu, (dA, Y, sc1, sh1, gamma, beta), gpu)


@pytest.mark.parametrize('relu', [False, True])
def test_gn_backward_on_layer_columns(hip, relu):
    """fusion C in production: a 1024-channel layer, per-channel normalisation, the three kernels on the views that
    Layer.columns(512) hands out (Y[:, 512:], gamma[512:], sc1[:, 512:]), relu=False like backward.py"""
    from mmmot_amd.tape import Layer
    tc, tg = both([5, 300, 128, 1])
    Y, dA, sc1, sh1, gamma, beta = gn_inputs(tc.R, tc.G, 1024, row_groups(tc), seed=10)
    mk = lambda f, tiles: Layer(f(Y), 1024, 1024, f(gamma), f(beta), f(sc1), f(sh1), f(sc1), f(sh1), tiles, 1e-5).columns(512)
    Lc, Lg = mk(lambda t: t, tc), mk(put, tg)
    assert Lg.C == 512 and Lg.NG == 512 and Lg.Y.stride(0) > 1024 and Lg.Y.storage_offset() % 4 == 0
    dA = dA[:, :512].contiguous()
    check_gn(hip, 'columns(512) relu %d' % relu, tc, tg, 512, 512, relu, (dA, Lc.Y, Lc.sc1, Lc.sh1, Lc.gamma, Lc.beta),
             (put(dA), Lg.Y, Lg.sc1, Lg.sh1, Lg.gamma, Lg.beta))


# ---- rowdot_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act,use_idx', [(0, False), (0, True), (2, False), (2, True)])
@pytest.mark.parametrize('K', [4, 64, 100, 128, 512, 2048])
def test_rowdot_backward(hip, K, act, use_idx):
    """K below, at and above a wave's 64 lanes, no multiple of it, and the largest the entry point takes (its dynamic LDS
    is 4 x (K + 4) floats); tiles of 1, 3, 128 and 2 rows (shorter than the four waves); PW with ldpw = K + 1 (packed) and
    K + 4.  w ~ 2 / sqrt(K), so that the pre-activation is O(1) at every K and the sigmoid's derivative is not all tail."""
    tc, tg = both([1, 3, 130])
    R = tc.R
    X, w = rnd(R, K, seed=60), rnd(K, seed=61) * (2.0 / math.sqrt(K))
    sc, sh = rnd(tc.G, K, seed=62) + 1.0, rnd(tc.G, K, seed=63) * 0.5
    gidx = torch.randperm(2 * R, generator=torch.Generator().manual_seed(1))[:R].to(torch.int32) if use_idx else None
    gout = rnd(2 * R if use_idx else R, seed=64)
    dAc, PWc = torch.zeros(R, K), torch.zeros(tc.T, K + 1)
    emu.rowdot_bwd(X, K, w, 0.3, sc, sh, tc, act, gout, gidx, dAc, PWc)
    Xg, wg, scg, shg, goutg = put(X), put(w), put(sc), put(sh), put(gout)
    gidxg = None if gidx is None else gidx.to(DEV)
    for extra in (0, 3):
        dAg, PWg = twice('rowdot_bwd ldpw K+%d' % (1 + extra), lambda: [slab(R, K), slab(tc.T, K + 1, off=0, extra=extra)],
                         lambda dA, PW: hip.rowdot_bwd(Xg, K, wg, 0.3, scg, shg, tg, act, goutg, gidxg, dA, PW))
        assert PWg.stride(0) == K + 1 + extra
        close(dAg, dAc, 2e-6, 'rowdot_bwd dA')
        close(PWg, PWc, 2e-5, 'rowdot_bwd partial dw / db')


def test_rowdot_backward_refusals(hip):
    """K = 2049 (more LDS than the kernel is sized for) and ldpw = K (no room for the db column): MMMOT_EINVAL"""
    tg = RowTiles([3], DEV)
    z = torch.zeros(16, 2052, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def status(K, ldpw):
        return hip.lib.mmmot_rowdot_bwd(z.data_ptr(), 2052, K, z.data_ptr(), 0.0, z.data_ptr(), z.data_ptr(), 2052,
                                        tg.row0.data_ptr(), tg.nrows.data_ptr(), tg.group.data_ptr(), tg.T, 0, z.data_ptr(),
                                        None, z.data_ptr(), 2052, z.data_ptr(), ldpw, s)
    assert status(2049, 2052) == EINVAL
    assert status(128, 128) == EINVAL


# ---- softmax_pairs_bwd ------------------------------------------------------------------------------------------------
# single-element blocks, one row / one column longer than a wave and close to a workgroup, more columns than the 256
# threads of the column loop (3 x 300), the forward test's 130 x 70; the last block has logits x 40 (max subtraction)
SM_BLOCKS = [(5, 7), (1, 1), (1, 200), (200, 1), (130, 70), (3, 300), (9, 6)]


@functools.lru_cache(None)
def softmax_inputs():
    sizes = [n * m for n, m in SM_BLOCKS]
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    R = int(row0[-1])
    logits, dout = rnd(R, seed=74) * 4.0, rnd(R, seed=71)
    logits[row0[-2]:] *= 10.0
    # dual_max sends the gradient to p or to q, whichever is larger, so p and q must be apart in float64 by more than fp32
    # can blur them (1 x 1 blocks have p = q = 1 and a zero gradient either way).  An ABSOLUTE distance of 1e-5 cannot
    # hold in these blocks: p and q each sum to 1 over the 70 / 130 entries of a row / column of the 130 x 70 block, and
    # with logits of spread 4 both are below 1e-5 in 3590 of its 9100 elements (39 of 54 in the x 40 block).  What decides
    # the branch in fp32 is the RELATIVE distance - fp32 has p and q to ~4e-6 relative each (rounding of x - max up to
    # 2^-18, expf) - so the condition is: |p - q| >= 1e-5 * max(p, q) everywhere, and >= 1e-5 absolute wherever
    # max(p, q) >= 1e-3.  Logits that miss it are lowered by a fixed 0.37 (3.7 in the x 40 block, where an element that
    # is the maximum of its row and of its column has p = q = 1 to the last bit) until it holds; then it is asserted.
    def apart(k):
        n, m = SM_BLOCKS[k]
        x = logits[row0[k]:row0[k + 1]].double().view(n, m)
        p, q = torch.softmax(x, 1), torch.softmax(x, 0)
        big, d = torch.max(p, q), (p - q).abs()
        return (d >= 1e-5 * big) & ((d >= 1e-5) | (big < 1e-3))
    for k, (n, m) in enumerate(SM_BLOCKS):
        if n * m == 1:
            continue
        for _ in range(8):
            logits[row0[k]:row0[k + 1]].view(n, m)[~apart(k)] -= 3.7 if k == len(SM_BLOCKS) - 1 else 0.37
        assert apart(k).all(), 'block %d: %d elements with p and q too close for dual_max' % (k, int((~apart(k)).sum()))
    gN = torch.tensor([n for n, _ in SM_BLOCKS], dtype=torch.int32)
    gM = torch.tensor([m for _, m in SM_BLOCKS], dtype=torch.int32)
    return logits, dout, torch.tensor(row0[:-1]), gN, gM, R, max(n + m for n, m in SM_BLOCKS)


@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_softmax_backward(hip, mode):
    logits, dout, r0, gN, gM, R, max_nm = softmax_inputs()
    G = len(SM_BLOCKS)
    dc = torch.zeros(R)
    emu.softmax_pairs_bwd(logits, dout, dc, r0, gN, gM, G, max_nm, mode)
    lg, dg, r0g, gNg, gMg = put(logits), put(dout), r0.to(DEV), gN.to(DEV), gM.to(DEV)
    (got,) = twice('softmax_pairs_bwd', lambda: [flat(R)],
                   lambda dl: hip.softmax_pairs_bwd(lg, dg, dl, r0g, gNg, gMg, G, max_nm, mode))
    close(got, dc, 3e-6, 'softmax_pairs_bwd mode %d' % mode)


def test_softmax_backward_refusal(hip):
    """3 x max_nm floats of LDS: 5461 fits 64 KB, 5462 does not and is refused"""
    z = torch.zeros(4, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = hip.lib.mmmot_softmax_pairs_bwd(z.data_ptr(), z.data_ptr(), z.data_ptr(), zero.data_ptr(), one.data_ptr(),
                                         one.data_ptr(), 1, 5462, 1, torch.cuda.current_stream().cuda_stream)
    assert st == EINVAL
    assert 3 * 5462 * 4 > 64 * 1024 >= 3 * 5461 * 4


# ---- pair_bwd / pair_expand_bwd ---------------------------------------------------------------------------------------
PAIR_SAMPLES = [([5, 7], None), ([1, 1], None), ([1, 130], None), ([130, 1], None), ([3, 2, 4], None)]


@pytest.mark.parametrize('pairop', [0, 1, 2])
@pytest.mark.parametrize('C', [4, 256, 516, 1024])
def test_pair_backward(hip, C, pairop):
    """C = 4 (one thread), 516 and 1024 (a second trip of the c += 512 loop, partly and fully); rows and columns longer
    than the 128 threads; the middle frame of the 3-frame sample receives the b side of one pair and the a side of the
    next on top of a non-zero dF; columns where a == b exactly (|a - b| has the sub-gradient 0 there)"""
    from mmmot_amd.backward import _aux
    pc = BatchPlan(PAIR_SAMPLES, 32, 'cpu', rows=(0,), use_points=False)
    pg = BatchPlan(PAIR_SAMPLES, 32, DEV, rows=(0,), use_points=False)
    ac, ag, tc, tg = _aux(pc), _aux(pg), pc.pair_tiles, pg.pair_tiles
    assert list(zip(pc.h_pg_N.tolist(), pc.h_pg_M.tolist())) == [(5, 7), (1, 1), (1, 130), (130, 1), (3, 2), (2, 4)]
    F, dX, dF0 = rnd(pc.Lt, C, seed=80), rnd(tc.R, C, seed=81), rnd(pc.Lt, C, seed=82)
    ties = 0
    for g, (i, j) in ((0, (1, 2)), (1, (0, 0)), (2, (0, 129)), (3, (77, 0)), (4, (2, 1)), (5, (1, 3))):
        F[int(pc.h_pg_boff[g]) + j, 0:3] = F[int(pc.h_pg_aoff[g]) + i, 0:3]
        ties += 3
    assert ties == 18
    dFc = dF0.clone()
    sides = [(ac.a_grp, ac.a_idx, ag.a_grp, ag.a_idx), (ac.b_grp, ac.b_idx, ag.b_grp, ag.b_idx)]
    for side, (bg_c, bi_c, _, _) in enumerate(sides):
        emu.pair_bwd(dX, F, dFc, C, tc.g_row0, pc.pg_N, pc.pg_M, pc.pg_aoff, pc.pg_boff, bg_c, bi_c, pairop, side)
    Fg, dXg = put(F), put(dX)

    def make():
        buf, v = slab(pc.Lt, C)
        v.copy_(dF0)
        return [(buf, v)]

    def launch(dF):
        for side, (_, _, bg_g, bi_g) in enumerate(sides):
            hip.pair_bwd(dXg, Fg, dF, C, tg.g_row0, pg.pg_N, pg.pg_M, pg.pg_aoff, pg.pg_boff, bg_g, bi_g, pairop, side)
    (dFg,) = twice('pair_bwd', make, launch)
    close(dFg, dFc, 2e-6, 'pair_bwd op %d' % pairop)
    if pairop == 1:  # the 1 x 1 pair ties in columns 0..2: both of its rows keep their start values there
        r = int(pc.h_pg_aoff[1])
        assert torch.equal(dFg[r:r + 2, 0:3].cpu(), dF0[r:r + 2, 0:3])
    if pairop == 0:  # pair_expand_bwd does not depend on the pairwise op
        dV = rnd(pc.v_tiles.R, C, seed=83)
        dAc = torch.zeros(tc.R, C)
        emu.pair_expand_bwd(dV, dAc, C, tc, tc.g_row0, pc.pg_N, pc.pg_M, ac.vrow0)
        dVg = put(dV)
        (dAg,) = twice('pair_expand_bwd', lambda: [slab(tc.R, C)],
                       lambda dA: hip.pair_expand_bwd(dVg, dA, C, tg, tg.g_row0, pg.pg_N, pg.pg_M, ag.vrow0))
        close(dAg, dAc, 1e-6, 'pair_expand_bwd')


# ---- fusion_c_bwd / add_rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [64, 512])
def test_fusion_c_bwd_and_add_rows(hip, C):
    tc, tg = both([1, 129, 7])
    R = tc.R
    Y0, Y1, dFu = rnd(R, 2 * C, seed=90), rnd(R, 2 * C, seed=91), rnd(R, C, seed=92)
    sc0, sh0, sc1, sh1 = rnd(tc.G, C, seed=93) + 1.0, rnd(tc.G, C, seed=94), rnd(tc.G, C, seed=95) + 1.0, rnd(tc.G, C, seed=96)
    outs_c = [torch.zeros(R, C) for _ in range(4)]
    emu.fusion_c_bwd(dFu, Y0, Y1, sc0, sh0, sc1, sh1, tc, *outs_c, C)
    args = (dFu.to(DEV), put(Y0), put(Y1), put(sc0), put(sh0), put(sc1), put(sh1), tg)
    # DY: the gate columns [:, :C] of [R][2C] buffers (the GroupNorm backward fills the other half); DN: no ld
    outs_g = twice('fusion_c_bwd', lambda: [slab(R, C, off=0, extra=C + 8), slab(R, C, off=0, extra=C + 8), flat(R, C), flat(R, C)],
                   lambda DY0, DY1, DN0, DN1: hip.fusion_c_bwd(*args, DY0, DY1, DN0, DN1, C))
    for a, b, what in zip(outs_g, outs_c, ('dgate0', 'dgate1', 'dn0', 'dn1')):
        close(a, b, 3e-6, 'fusion_c_bwd ' + what)
    A, B = rnd(R, C, seed=97), rnd(R, C, seed=98)
    Ag, Bg = put(A), slab(R, C, off=8, extra=4)[1]
    Bg.copy_(B)
    assert Ag.stride(0) != Bg.stride(0) or Ag.storage_offset() != Bg.storage_offset()
    (Yg,) = twice('add_rows', lambda: [slab(R, C, off=12, extra=4)], lambda Y: hip.add_rows(Ag, Bg, Y, C))
    assert torch.equal(Yg.cpu(), A + B)
