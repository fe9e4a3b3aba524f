"""Taped-layer primitives of the training step: what backward.py (the head), train.py (PointNet) and train_vgg.py (the
image encoder) share.

A training forward keeps, per 'GEMM -> GroupNorm (-> ReLU)' layer, a ``Layer``: the pre-norm output, its statistics, its
parameters and its row tiling.  ``Layer.backward`` is the backward of such a layer - GroupNorm backward, weight gradient
``dW = dY^T A``, input gradient ``dA = dY W`` - and ``taped`` attaches a (forward, backward) pair of launch schedules to
autograd.  Everything numeric happens in libmmmot_hip.so; this file allocates, orders launches and caches small tables.
"""
import collections

import numpy as np
import torch

from .plan import PoolLevels

SEGSUM_CHUNK = 128  # rows per first-level segment of a long strided sum


def chunked_segments(start, count, stride, device):
    """sum (divisor 1) of `count[i]` rows from `start[i]` with `stride` as PoolLevels: two levels - SEGSUM_CHUNK-row chunks of
    every segment, then a segment's chunk sums - when any segment is longer than 4 * SEGSUM_CHUNK rows"""
    return PoolLevels.chunked(start, count, stride, device, chunk=SEGSUM_CHUNK, longer_than=4 * SEGSUM_CHUNK, div=1)


def segsum(eng, X, C, segs, out):
    """segment sums through mmmot_segment_mean (divisor 1); `segs`: the PoolLevels of chunked_segments"""
    segs.pool(eng.ops, X, C, out)


def tile_sums(plan, tiles, device):
    """(per-group, total) segment tables that sum the [T][2][C] partials of a tiling, viewed as [2T][C] rows; built once
    per (plan, tiling).  Each is a PoolLevels for segsum - long segments in two levels (chunks, chunk sums): one
    segment is one workgroup, and the 8 624 tiles of a full-resolution trunk layer walked by two workgroups were the 0.9 ms
    launches of the training step's kernel table (profiles/r05/rocprofv3_kernel_stats_train.txt)."""
    cache = plan.__dict__.setdefault('_tile_sums', {})
    key = id(tiles)
    if key not in cache:
        start = np.stack([2 * tiles.h_g_tile0, 2 * tiles.h_g_tile0 + 1], 1).reshape(-1)
        count = np.repeat(tiles.h_g_ntiles, 2)
        grp = chunked_segments(start, count, 2, device)
        tot = chunked_segments(np.array([0, 1]), np.array([tiles.T, tiles.T]), 2, device)
        cache[key] = (grp, tot)
    return cache[key]


COLSUM_CHUNK = 128  # rows per segment of one level of colsum


def colsum(eng, X):
    """column sums of a [rows][C] tensor (C % 4 == 0) through the strided-mean kernel with divisor 1.  One segment = one
    workgroup per 256 channels, and a workgroup walks its rows sixteen at a time: the 2 048-row chunks this used to cut
    took 180 us each however few there were (the bias gradients of the trunk: 2.6 ms of a training step -
    profiles/HISTORY.md round 6; tools/train_segment_calls.py lists the call sites), a single segment over a trunk layer's 1.1 M rows 0.9 ms.  So: COLSUM_CHUNK-row
    chunks, level after level, until at most 2 * COLSUM_CHUNK rows are left (1.1 M rows of 64 channels: viewed as 276 k rows
    of 256, 2 156 -> 17 -> 1)."""
    rows, C = int(X.shape[0]), int(X.shape[1])
    cache = eng.__dict__.setdefault('_colsum_segs', {})  # the PoolLevels per row count: small uploads saved per call
    # narrow rows: a lane of the kernel owns 4 channels, so a 64-channel tensor would keep 16 lanes of a wave busy - k
    # consecutive rows are viewed as one row of k * C channels (the sums of the rows = r mod k classes), folded at the end
    fold, C0 = 1, C
    if X.is_contiguous():
        while C * 2 <= 256 and rows % 2 == 0 and rows > 2 * COLSUM_CHUNK:
            fold, C, rows = fold * 2, C * 2, rows // 2
        X = X.view(rows, C)
    key = (rows, str(X.device))
    levels = cache.get(key)
    if levels is None:
        if len(cache) > 256:
            cache.clear()
        levels = cache[key] = PoolLevels.chunked([0], [rows], 1, X.device, chunk=COLSUM_CHUNK, longer_than=2 * COLSUM_CHUNK,
                                                 div=1, repeat=True)
    out = torch.empty(1, C, dtype=X.dtype, device=X.device)
    levels.pool(eng.ops, X, C, out)
    return out[0] if fold == 1 else out.view(fold, C0).sum(0)


def unit(eng, C, dev, dtype=torch.float32):
    key = ('unit', C, str(dev)) if dtype == torch.float32 else ('unit', C, str(dev), dtype)
    if key not in eng.ws:
        eng.ws[key] = (torch.ones(C, dtype=dtype, device=dev), torch.zeros(C, dtype=dtype, device=dev))
    return eng.ws[key]


def dgrad_gemm(eng, W, tiles, X, Y):
    """Y = X W for a forward weight W [N_f][K_f] (the input gradient dA_in = dY W of a 1x1 layer): the row GEMM with the
    transposed weight, exact fp32 matrix cores.  (Not the f16x3 row GEMM: its A operand - here the GRADIENT dY, 1e-4 ..
    1e-7 - is split into fp16 halves unscaled, i.e. into fp16's subnormals; measured: the SGD-step parity went from 2e-6
    to > 1e-5.  The weight-gradient GEMM scales dY by its maximum first, mmmot_gemm_tn_f16.)  The transposed copy is cached
    on the engine per (storage, version) of W, so a backward does not re-transpose an unchanged weight.  An entry keeps
    a reference to W itself: the key contains W's ADDRESS, and a weight that is freed (the folded PointNet weights are
    fresh tensors every step) would hand its address - at version 0 - to the next step's fold, which would then hit the
    previous step's transpose (tests/test_train_cpu.py runs three steps against the oracle)."""
    Nf, Kf = int(W.shape[0]), int(W.shape[1])
    cache = eng.__dict__.get('_wt_cache')
    if cache is None:
        cache = eng.__dict__['_wt_cache'] = collections.OrderedDict()
    key = (W.data_ptr(), W._version, Nf, Kf)
    ent = cache.get(key)
    if ent is not None:
        cache.move_to_end(key)  # least-recently-USED eviction: a persistent weight that is hit every step stays
    else:
        # ~30 weights pass through per step (the folded PointNet weights are fresh tensors every step, the head weights
        # change version with every optimizer step): room for two steps, evict the entry unused for longest
        while len(cache) >= 64:
            cache.popitem(last=False)
        ent = cache[key] = (W, W.detach().t().contiguous())  # data movement; W pinned while the entry lives
    wt = ent[1]
    eng.ops.gemm(wt, tiles, Kf, Nf, X=X, Y=Y)


def weight_grad(eng, dY, tiles, N, K, shares=None, **operand):
    """(dW [N][K], db [N]) = (dY^T A, column sums of dY) of a row GEMM whose A operand `operand` describes (X / sc / sh /
    amode, or FA / FB / pair / pairop).  The reduction over the rows is split into `shares` contiguous shares of the
    tiles (one workgroup walks one share for one 64 x 64 tile of dW; default: one per 8 tiles, at most 16) whose partial
    sums are added by the strided-sum kernel: deterministic."""
    ns = max(1, min(16, tiles.T // 8)) if shares is None else shares
    dWp = torch.empty(ns, N * K, dtype=dY.dtype, device=dY.device)  # dY's dtype, like gn_backward's buffers
    dbp = torch.empty(ns, N, dtype=dY.dtype, device=dY.device)
    eng.ops.gemm_tn(dY, tiles, N, K, dWp, dbp, nsplit=ns, **operand)
    if ns > 1:
        return colsum(eng, dWp).view(N, K), colsum(eng, dbp)
    return dWp.view(N, K), dbp.view(N)


def gn_backward(eng, plan, L, dA, out=None, relu=True):
    """dA = gradient w.r.t. relu(GroupNorm(Y)) (or GroupNorm(Y) when ``relu`` is False) -> (dY, dgamma [C],
    dbeta [C]).  ``out``: view to write dY into.  Buffers take dA's dtype (fp32 on the device; the float64 emulation of the
    tests keeps float64 between the operators that way)."""
    ops, tiles, C, dev = eng.ops, L.tiles, L.C, dA.device
    P = torch.empty(tiles.T, 2, C, dtype=dA.dtype, device=dev)
    ops.gn_bwd_partial(dA, L.Y, C, L.sc1, L.sh1, L.gamma, L.beta, relu, tiles, P)
    seg_g, seg_t = tile_sums(plan, tiles, dev)
    S = torch.empty(tiles.G * 2, C, dtype=dA.dtype, device=dev)
    tot = torch.empty(2, C, dtype=dA.dtype, device=dev)
    P2 = P.view(2 * tiles.T, C)
    segsum(eng, P2, C, seg_g, S)
    segsum(eng, P2, C, seg_t, tot)
    M = torch.empty(tiles.G, 2, C, dtype=dA.dtype, device=dev)
    ops.gn_bwd_finalize(S, tiles, C, L.NG, L.gamma, M)
    dY = out if out is not None else torch.empty(tiles.R, C, dtype=dA.dtype, device=dev)
    ops.gn_bwd_apply(dA, L.Y, C, L.sc1, L.sh1, L.gamma, L.beta, relu, M, tiles, dY)
    return dY, tot[1], tot[0]


class Layer:
    """One 'GEMM -> GroupNorm -> ReLU' layer on the tape: pre-norm output Y [tiles.R][C], its statistics (sc / sh with the
    layer's affine for the consumer's prologue, sc1 = rstd and sh1 = -mean * rstd), its parameters, its row tiling."""

    def __init__(self, Y, C, NG, gamma, beta, sc, sh, sc1, sh1, tiles, eps):
        self.Y, self.C, self.NG, self.gamma, self.beta = Y, C, NG, gamma, beta
        self.sc, self.sh, self.sc1, self.sh1, self.tiles, self.eps = sc, sh, sc1, sh1, tiles, eps

    def columns(self, c0):
        """the layer of the channels c0.. of a per-channel normalisation (NG == C: every channel's statistics are its own)"""
        assert self.NG == self.C
        C = self.C - c0
        return Layer(self.Y[:, c0:], C, C, self.gamma[c0:], self.beta[c0:], self.sc[:, c0:], self.sh[:, c0:],
                     self.sc1[:, c0:], self.sh1[:, c0:], self.tiles, self.eps)

    def backward(self, eng, plan, dA, W, shares=None, out=None, relu=True, **operand):
        """Backward of 'Y = A W^T + b, relu(GroupNorm(Y))' from dA, the gradient w.r.t. the normalised output (``out`` /
        ``relu``: see gn_backward): W [C][K] is the forward weight, `operand` the A operand of the weight-gradient GEMM
        (see weight_grad, which also takes ``shares``).  Returns (dA_in [tiles.R][K], dW, db, dgamma, dbeta)."""
        K = int(W.shape[1])
        dY, dgamma, dbeta = gn_backward(eng, plan, self, dA, out=out, relu=relu)
        dW, db = weight_grad(eng, dY, self.tiles, self.C, K, shares, **operand)
        dX = torch.empty(self.tiles.R, K, dtype=dA.dtype, device=dA.device)
        dgrad_gemm(eng, W, self.tiles, dY, dX)
        return dX, dW, db, dgamma, dbeta


def norm_layer(eng, part, tiles, Y, C, NG, gamma, beta, sc=None, sh=None):
    """The Layer of a pre-norm output Y with per-tile statistics `part`: finalize twice, (gamma, beta) -> sc / sh for the
    consumer's prologue (unless the caller has them already), (1, 0) -> sc1 = rstd, sh1 = -mean * rstd."""
    new = lambda: torch.empty(tiles.G, C, dtype=Y.dtype, device=Y.device)
    if sc is None:
        sc, sh = new(), new()
        eng.ops.gn_finalize(part, tiles, C, NG, gamma, beta, eng.eps, sc, sh)
    sc1, sh1 = new(), new()
    one, zero = unit(eng, C, Y.device, Y.dtype)
    eng.ops.gn_finalize(part, tiles, C, NG, one, zero, eng.eps, sc1, sh1)
    return Layer(Y, C, NG, gamma, beta, sc, sh, sc1, sh1, tiles, eng.eps)


def det_batch_stats(layer, n):
    """(mean, unbiased variance) of a training-mode BatchNorm layer from its unit statistics - what
    ``running_mean`` / ``running_var`` are updated with."""
    rstd = layer.sc1[0]
    mean = -layer.sh1[0] / rstd
    var = (1.0 / (rstd * rstd) - layer.eps) * (n / max(n - 1, 1))
    return mean, var


def update_running_stats(bn, layer, n):
    """the momentum update of nn.BatchNorm in training mode, from the statistics of `layer` over its n positions"""
    mean, var = det_batch_stats(layer, n)
    m = bn.momentum if bn.momentum is not None else 0.1
    with torch.no_grad():
        bn.running_mean.mul_(1 - m).add_(m * mean)
        bn.running_var.mul_(1 - m).add_(m * var)
        bn.num_batches_tracked += 1


class _Taped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd, keys, *params):
        outs, ctx.tape = fwd(x.detach().contiguous(), [p.detach() for p in params])
        ctx.bwd, ctx.keys = bwd, keys
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.outs = [(tuple(o.shape), o.device) for o in outs]
        ctx.save_for_backward(x)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *d_outs):
        (x,) = ctx.saved_tensors
        d_outs = [torch.zeros(s, dtype=torch.float32, device=dev) if d is None else d.contiguous()
                  for d, (s, dev) in zip(d_outs, ctx.outs)]
        dx, grads = ctx.bwd(x.detach().contiguous(), ctx.tape, *d_outs)
        return (dx, None, None, None) + tuple(grads[k].reshape(s) if k in grads else None
                                              for k, s in zip(ctx.keys, ctx.shapes))


def taped(x, keys, params, fwd, bwd):
    """Attach a taped launch schedule to autograd.  ``fwd(x, params) -> (outputs, tape)`` and ``bwd(x, tape, *d_outputs) ->
    (dx or None, {key: gradient})`` see detached, contiguous tensors, a zero tensor for an output nobody differentiated,
    and return gradients in any shape with the parameter's element count; `keys` name `params` in the gradient dict (a key
    it lacks: no gradient).  Returns the tuple of outputs on the autograd graph of x and params."""
    return _Taped.apply(x, fwd, bwd, tuple(keys), *params)
