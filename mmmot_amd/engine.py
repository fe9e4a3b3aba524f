"""Launch schedule of the mmMOT forward over the device operator layer.

One ``Engine`` owns the packed weights of a ``TrackingNet`` and a workspace
arena; ``forward(plan, crops, points)`` issues the kernel sequence for a whole
batch of samples on the current HIP stream and returns device tensors.  The
schedule follows the data flow of reference modules/tracking_net.py:128-193
(feature -> determine_det -> associate) but not its module structure: every
normalisation on the path is a whole-sample reduction, so the schedule is a
chain of  GEMM(+stats epilogue) -> finalize -> next GEMM(normalise prologue).

``ops`` is the operator backend: ``mmmot_amd.ops.HipOps`` in the product.  The
engine itself only allocates memory and orders launches.
"""
import contextlib
import itertools
import os
import threading

import numpy as np
import torch

from .ops import (ACT_NONE, ACT_RELU, ACT_SIGMOID, A_NORM_RELU, A_PAIR, A_PLAIN, FUSION_MODES, PAIR_OPS,
                  SOFTMAX_MODES)
from .range_guard import RangeGuard
from .tape import norm_layer

POOL_INPUT = {'f32': 0, 'hl16': 1, 'hq8': 2}  # the segment mean's `hl16` argument: the format its input rows are stored in
EPS = 1e-5  # nn.GroupNorm / nn.BatchNorm default used everywhere in the reference
_SERIALS = itertools.count(1)


def check_crop_side(S):
    if S < 32 or S % 2 != 0:
        # five 2x2 poolings: a 32-pixel crop ends in a 1 x 1 map.  Sides that are not a multiple of 32 give odd maps
        # on the way down, floored by every pooling like nn.MaxPool2d(2, 2) (reference modules/vgg.py:72) - e.g.
        # 100 -> 50 -> 25 -> 12 -> 6 -> 3.  The first layer (NCHW crops, fused conv1_1 + conv1_2 + pool) wants an
        # even side; the reference's dataset resizes every crop to 224 (dataset/test_seq_dataset.py:218).
        raise ValueError('crop side %d is not supported: the HIP VGG trunk needs an even side >= 32; resize the crops '
                         '(mmmot_amd.crops.crop_resize_normalize)' % S)


def check_crop_layout(dets):
    """Host check of the crops of a reference-shaped call, before anything is queued: the normalised fp32 [L,3,S,S]
    tensor or the uint8 [L,S,S,3] crops of the resize (mmmot_amd.crops.crop_resize_u8) with an even side >= 32.
    Returns the side S."""
    if dets.dtype == torch.uint8:
        if dets.dim() != 4 or dets.shape[3] != 3 or dets.shape[1] != dets.shape[2]:
            raise ValueError('uint8 crops must be [L,S,S,3] (HWC, the output of mmmot_amd.crops.crop_resize_u8), got %s'
                             % (tuple(dets.shape),))
        S = int(dets.shape[1])
    else:
        S = int(dets.shape[-1])
    check_crop_side(S)
    return S


class Engine:
    eps = EPS

    def __init__(self, packed, ops, fusion='A', affinity_op='multiply', softmax_mode='none',
                 neg_threshold=0.0, score_arch='branch_cls', end_mode='avg', trunk=None):
        trunk = trunk or os.environ.get('MMMOT_TRUNK', 'f16x3')
        if trunk not in ('f16x3', 'f16q8', 'f32'):
            raise ValueError("trunk must be 'f16x3' (fp16 matrix cores, 3-term split), 'f16q8' (fp16 main term + "
                             "fp8 correction terms, include/mmmot_hip.h hq8) or 'f32' (exact fp32 MFMA)")
        self.trunk = trunk            # arithmetic the trunk currently runs in
        self.serial = next(_SERIALS)  # identifies this engine in the stamps of appearance rows (TrackingNet.encode_appearance)
        self.trunk_requested = trunk
        # the range guard (mmmot_amd/range_guard.py) lowers `trunk` for good when activations leave the range of the
        # reduced formats, and records here what it found
        self.guard = RangeGuard(self)
        self.range_events = []
        self.last_out_of_range_forward = None  # index of the latest forward whose out-of-range results were already returned
        self.out_of_range_window = None  # (first, last) forward indices of the latest asynchronous detection
        self._busy = threading.Lock()  # see forward()
        self._last_stream = None
        # image_first(): (key of the image branch that is already in the workspace for the next forward, the event recorded
        # in front of it - where the LiDAR branch may start from - or None)
        self._head_start = None
        # f16q8 only: trunk layers (indices into P['vgg'], 1..12) that run the hq8 arithmetic; None = all of them
        # (MMMOT_Q8_LAYERS=all).  The others run f16x3; at a boundary the activation tensor is re-encoded (hq8 <-> hl16,
        # two small kernels).  Default: conv3_1 .. conv5_3 (layers 4..12).  Measured on trained-like statistics
        # (tools/study_robustness.py, calibrated BatchNorm, per-channel gains over 1e4, heavy-tailed weights): the
        # full-resolution layers 1..3 carry two thirds of the e4m3 error (all layers 5.8e-4 .. 9.5e-4 of the 1e-3
        # budget; layers 4..12 3.8e-4 .. 4.0e-4) for a fifth of the trunk's time.
        ql = os.environ.get('MMMOT_Q8_LAYERS', '4,5,6,7,8,9,10,11,12')
        self.q8_layers = None if ql == 'all' else set(int(v) for v in ql.split(',') if v)
        # PointNet conv5 / conv1: statistics pass + fused normalise-ReLU-segment-sum pass instead of
        # materialising the [P][1024] / [P][512] tensors (MMMOT_PN_FUSED=0 keeps the materialising path)
        self.pn_fused = os.environ.get('MMMOT_PN_FUSED', '1') != '0'
        # conv5 statistics from the Gram matrix of its input instead of a statistics pass of the GEMM
        self.pn_gram = os.environ.get('MMMOT_PN_GRAM', '1') != '0'
        # conv2..conv4 (K = 64) from the persistent weight-resident kernel (pn_mlp64.hip) instead of the generic row GEMM
        self.pn_mlp64 = os.environ.get('MMMOT_PN_MLP64', '1') != '0'
        # LiDAR branch on a side stream next to the trunk: opt-in (MMMOT_TWO_STREAMS=1).  Measured (profiles/README.md
        # r02): cfg3 x 8 pairs 275.3 -> 276.0 pairs/s (noise) while every trunk launch's own duration grows by the time
        # it waits for CUs; B = 1 hipGraph replay 2.85 -> 2.71 ms, eager latency unchanged.
        self.two_streams = os.environ.get('MMMOT_TWO_STREAMS', '0') == '1'
        # forward() after image_first(): PointNet on a side stream beside the already running trunk (MMMOT_PN_BESIDE_TRUNK=0: behind it)
        self.pn_beside_trunk = os.environ.get('MMMOT_PN_BESIDE_TRUNK', '1') != '0'
        self._side = {}
        # SkipPool heads: one launch per stage (MMMOT_SP_FUSED=0: LayerNorm / GEMM / LayerNorm / GEMM / LayerNorm launches)
        self.sp_fused = os.environ.get('MMMOT_SP_FUSED', '1') != '0'
        # conv1_1 evaluated inside conv1_2's patch prologue (MMMOT_FUSE_CONV1=0: two launches)
        self.fuse_conv1 = os.environ.get('MMMOT_FUSE_CONV1', '1') != '0'
        # f16q8 applies to crops of at least this side; smaller crops run the f16x3 trunk.  The e4m3 correction
        # terms cost ~3e-4 of score error at the 64..224-pixel crops of the reference's configurations and more
        # where less spatial averaging follows the trunk (6e-4 measured at 32-pixel crops, tests/test_hq8_gpu.py),
        # while the trunk is a negligible part of the step there.
        self.q8_min_crop = int(os.environ.get('MMMOT_Q8_MIN_CROP', '64'))
        self.mlp = 'f32' if trunk == 'f32' else 'f16x3'  # the 1x1-conv / linear GEMMs: exact fp32 only with the f32 trunk
        if affinity_op not in PAIR_OPS:
            raise ValueError('unknown affinity_op %r' % (affinity_op,))
        if softmax_mode not in SOFTMAX_MODES and softmax_mode != 'none':
            softmax_mode = 'none'  # reference falls through to the raw logits (tracking_net.py:123-124)
        self.end_mode = end_mode  # 'avg': mean over the prev / curr axis, anything else: maximum (new_end.py:69-74)
        self.P = packed
        self.ops = ops
        self.fusion = fusion
        self.affinity_op = affinity_op
        self.softmax_mode = softmax_mode
        self.neg_threshold = float(neg_threshold)
        self.score_arch = score_arch
        self.ws = {}
        self.dev = None
        self.keep = None         # optional dict collecting per-stage tensors (tests)
        self._tape = None        # recording(): the dict the running schedule records its layers in
        self.conv_events = None  # optional list collecting per-launch HIP events (bench.py)

    # ---- workspace arena ---------------------------------------------------
    def buf(self, name, *shape, device=None, dtype=torch.float32):
        if self._tape is not None:  # recording(): owned storage, a tape must survive the next forward
            return torch.empty(*shape, dtype=dtype, device=device if device is not None else self.dev)
        return self._arena(name, *shape, device=device, dtype=dtype)

    def _arena(self, name, *shape, device=None, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= int(s)
        t = self.ws.get(name)
        if t is None or t.numel() < n or t.dtype != dtype or (device is not None and t.device != torch.device(device)):
            t = torch.empty(max(n, 4), dtype=dtype, device=device if device is not None else self.dev)
            self.ws[name] = t
        return t[:n].view(*shape)

    def buf64(self, name, *shape):
        return self.buf(name, *shape, dtype=torch.float64)

    def _finalize(self, name, part, tiles, C, NG, gamma, beta, Y=None):
        """GroupNorm (NG groups) scale / shift of the layer `name` from its per-tile statistics `part`.  `Y`: the layer's
        pre-norm output, for the tape.Layer that recording() keeps under `name`."""
        sc = self.buf(name + '_sc', tiles.G, C)
        sh = self.buf(name + '_sh', tiles.G, C)
        self.ops.gn_finalize(part, tiles, C, NG, gamma, beta, EPS, sc, sh)
        if self._tape is not None:
            self._tape[name] = norm_layer(self, part, tiles, Y, C, NG, gamma, beta, sc, sh)
        return sc, sh

    def _gemm(self, d, name, tiles, N, K, **kw):
        """Row GEMM with weight d[name]: on the fp16 matrix cores (3-term hi/lo split, hl16 weight copy
        made by pack._add_hl16_copies) when mlp == 'f16x3', else on the exact fp32 MFMA."""
        if self.mlp == 'f16x3' and (name + '_h16') in d:
            self.ops.gemm(d[name + '_h16'], tiles, N, K, w_hl16=True, oscale=d[name + '_os'], **kw)
        else:
            self.ops.gemm(d[name], tiles, N, K, **kw)

    def _gemm_gn(self, d, name, tiles, N, K, y, gn, NG, gamma, beta, **kw):
        """_gemm into the workspace buffer `y` [tiles.R][N] with the statistics epilogue, then the GroupNorm (NG groups)
        scale / shift of that output (workspace `gn`_sc / _sh): (Y, scale, shift) for the consumer's prologue."""
        Y = self.buf(y, tiles.R, N)
        part = self._part(tiles, N)
        self._gemm(d, name, tiles, N, K, Y=Y, part=part, **kw)
        return (Y,) + self._finalize(gn, part, tiles, N, NG, gamma, beta, Y=Y)

    @contextlib.contextmanager
    def recording(self):
        """The training forward is the forward, recorded.  Inside the block buf() hands out owned tensors instead of arena
        views (the statistics scratch `part` stays in the arena: the finalize right behind the GEMM consumes it), every
        _finalize also computes the unit statistics and keeps a tape.Layer under its name, and _stash keeps its tensor
        under its key.  Yields that dict: {'aff_1': Layer, ..., 'aff_v': tensor, ...}."""
        prev, self._tape = self._tape, {}
        try:
            yield self._tape
        finally:
            self._tape = prev

    @contextlib.contextmanager
    def fp32_mlp(self):
        """row GEMMs on the fp32 weights inside the block (the training forward: the fp16-split copies of the head are not
        rebuilt after an optimizer step - TrackingNet.refresh_head_device)"""
        prev, self.mlp = self.mlp, 'f32'
        try:
            yield
        finally:
            self.mlp = prev

    def _side_stream(self, dev):
        key = str(dev)
        st = self._side.get(key)
        if st is None:
            st = self._side[key] = torch.cuda.Stream(device=dev)
        return st

    def _part(self, tiles, N):
        return self._arena('part', tiles.T, 2, N)

    def _stash(self, key, t):
        if self.keep is not None:
            self.keep[key] = t.detach().clone()
        if self._tape is not None:
            self._tape[key] = t

    # ---- image branch: VGG16-BN trunk + SkipPool heads ---------------------
    def appearance(self, plan, crops, cat):
        """crops [Lt,3,S,S] NCHW (reference contract) -> cat[:, 0:512]."""
        ops, Lt, S = self.ops, plan.Lt, plan.S
        check_crop_side(S)
        if Lt * S * S * 16 >= 2 ** 31 - 64:
            # the trunk kernels address activations with 32-bit offsets in 16-byte pieces (largest tensor: L x S x S x 64)
            raise ValueError('%d crops of %dx%d in one launch sequence exceed the 32-bit piece offsets of the trunk kernels '
                             '(L*S*S*16 < 2^31): split the batch' % (Lt, S, S))
        x, H, W = crops, S, S
        u8 = crops.dtype == torch.uint8  # the 8-bit crops of the resize [Lt][S][S][3]: ToTensor + Normalize on the device
        q8 = self.q8_in_force(S)  # activations travel as hq8 records (fp16 hi + two e4m3 copies, same bytes)
        f16 = self.trunk in ('f16x3', 'f16q8')  # activations travel in the hl16 split-half / hq8 format (same bytes)
        vgg = self.P['vgg']
        # conv1_1 + conv1_2 + pool as one launch when the trunk has the VGG16 head (3 -> 64 -> 64, pool)
        fuse1 = (f16 and self.fuse_conv1 and len(vgg) > 1 and vgg[0]['cout'] == 64 and
                 vgg[1]['cin'] == 64 and vgg[1]['cout'] == 64 and vgg[1]['pool'] and not vgg[0]['last'] and
                 not vgg[0]['pool'])
        if u8 and not fuse1:
            # exact-fp32 trunk / unfused first layer: they read the fp32 model input - made here from the bytes with the
            # same IEEE arithmetic as the host pipeline (one small kernel; the fused first launch takes the bytes itself)
            x = self.buf('vgg_crops32', Lt, 3, S, S)
            ops.u8_normalize(crops, self._mean_std(crops.device), x, Lt, S)
            u8 = False
        fmt = 'raw'  # format of x: 'raw' NCHW crops, 'f32' NHWC fp32, 'hl16', 'hq8' (same bytes per value)
        for li, cv in enumerate(vgg):
            if fuse1 and li == 0:
                continue
            lq8 = q8 and (self.q8_layers is None or li in self.q8_layers)  # this layer's arithmetic
            want = 'hq8' if lq8 else 'hl16'
            if f16 and fmt in ('hl16', 'hq8') and fmt != want:
                # arithmetic boundary inside an f16q8 trunk: re-encode the activation tensor (exact up to the target
                # format's own rounding)
                n = Lt * H * W * cv['cin']
                tmp = self.buf('vgg_recode32', n)
                (ops.hq8_unpack if fmt == 'hq8' else ops.hl16_unpack)(x, tmp)
                x = self.buf('vgg_recode', n)
                (ops.hq8_pack if want == 'hq8' else ops.hl16_pack)(tmp, x)
                fmt = want
            Ho, Wo = (H // 2, W // 2) if cv['pool'] else (H, W)
            out = self.buf('vgg%d' % (li & 1), Lt * Ho * Wo, cv['cout'])
            if self.conv_events is not None:  # bench.py: HIP events around every trunk launch
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if fuse1 and li == 1:
                c0 = vgg[0]
                if u8:
                    from .crops import MEAN, STD
                    ops.conv1_fused_u8(x, MEAN, STD, c0['wp16'], c0['bias'], c0['oscale'], cv['wpq8'] if lq8 else cv['wp16'],
                                       cv['bias'], cv['oscale'], out, Lt, H, W, q8=lq8)
                elif lq8:
                    ops.conv1_fused_hq8(x, c0['wp16'], c0['bias'], c0['oscale'], cv['wpq8'], cv['bias'], cv['oscale'],
                                        out, Lt, H, W)
                else:
                    ops.conv1_fused_hl16(x, c0['wp16'], c0['bias'], c0['oscale'], cv['wp16'], cv['bias'],
                                         cv['oscale'], out, Lt, H, W)
                fmt = want
            elif f16 and li == 0:  # unfused first layer: exact fp32 MFMA on the crops, output encoded for layer 1
                nq8 = q8 and (self.q8_layers is None or 1 in self.q8_layers)
                if nq8:
                    tmp = self.buf('vgg_first32', Lt * H * W, cv['cout'])
                    ops.conv3x3(x, cv['wp'], cv['bias'], tmp, Lt, H, W, cv['cin'], cv['cout'], True, cv['pool'])
                    ops.hq8_pack(tmp, out)
                else:
                    ops.conv3x3_first_hl16(x, cv['wp'], cv['bias'], out, Lt, H, W, cv['cout'])
                fmt = 'hq8' if nq8 else 'hl16'
            elif lq8:
                ops.conv3x3_hq8(x, cv['wpq8'], cv['bias'], out, Lt, H, W, cv['cin'], cv['cout'], cv['pool'], cv['oscale'])
                fmt = 'hq8'
            elif not f16:
                ops.conv3x3(x, cv['wp'], cv['bias'], out, Lt, H, W, cv['cin'], cv['cout'], li == 0, cv['pool'])
                fmt = 'f32'
            else:
                ops.conv3x3_hl16_patch(x, cv['wp16'], cv['bias'], out, Lt, H, W, cv['cin'], cv['cout'], cv['pool'],
                                       cv['oscale'])
                fmt = 'hl16'
            if self.conv_events is not None:
                e1.record()
                self.conv_events.append((li, Lt * H * W, cv['cin'], cv['cout'], e0, e1))
            x, H, W = out, Ho, Wo
            if cv['last']:
                self._stash('vgg_stage%d' % cv['stage'], x)
                self._skippool(plan, cv['stage'], x, H * W, cv['cout'], cat, fmt)

    def _mean_std(self, dev):
        key = ('mean_std', str(dev))
        if key not in self.ws:
            from .crops import MEAN, STD
            self.ws[key] = torch.tensor(list(MEAN) + list(STD), dtype=torch.float32, device=dev)
        return self.ws[key]

    def q8_in_force(self, S):
        """crops of side S run the hq8 arithmetic: an f16q8 trunk, and crops of at least q8_min_crop pixels"""
        return self.trunk == 'f16q8' and S >= self.q8_min_crop

    def trunk_elements(self, plan):
        """activation elements the trunk writes per forward (the denominator of the range guard's fractions)"""
        n, H = 0, plan.S
        for cv in self.P['vgg']:
            if cv['pool']:
                H //= 2
            n += plan.Lt * H * H * cv['cout']
        return n

    def _skippool(self, plan, s, x, hw, C, cat, fmt='f32'):
        """reference modules/appear_net.py:9-32 for stage s -> cat[:, 128 s : 128 (s+1)]; `fmt`: the format x is stored in"""
        hl16 = POOL_INPUT[fmt]
        ops, Lt, hd, T = self.ops, plan.Lt, self.P['skippool'][s], plan.det_tiles
        pooled = self.buf('sp_pool', Lt, C)
        # large maps in two levels: row chunks of a crop -> partial sums -> mean (few crops: see plan._crop_segments)
        plan.crop_segments(hw).pool(ops, x, C, pooled, partial=lambda n: self.buf('sp_partial', n, C), hl16=hl16)
        if self.sp_fused and hasattr(ops, 'skippool_head'):
            ops.skippool_head(pooled, C, hd, EPS, cat[:, 128 * s:128 * (s + 1)], Lt)  # the whole head in one launch
            return
        ln0 = self.buf('sp_ln0', Lt, C)
        ops.row_layernorm(pooled, C, hd['g0'], hd['b0'], EPS, False, ln0, Lt)
        C4 = hd['w1'].shape[0]
        h1 = self.buf('sp_h1', Lt, C4)
        self._gemm(hd, 'w1', T, C4, C, X=ln0, bias=hd['c1'], Y=h1)
        ln1 = self.buf('sp_ln1', Lt, C4)
        ops.row_layernorm(h1, C4, hd['g2'], hd['b2'], EPS, True, ln1, Lt)
        h2 = self.buf('sp_h2', Lt, 128)
        self._gemm(hd, 'w4', T, 128, C4, X=ln1, bias=hd['c4'], Y=h2)
        ops.row_layernorm(h2, 128, hd['g5'], hd['b5'], EPS, True, cat[:, 128 * s:128 * (s + 1)], Lt)

    # ---- LiDAR branch: PointNet with folded transforms ----------------------
    def pointnet(self, plan, points, cat):
        """points [P,3] -> cat[:, 512:1024]; reference modules/point_net.py:25-44,115-153."""
        ops, pn, T, D, Pn, Lt = self.ops, self.P['pointnet'], plan.pt_tiles, plan.det_tiles, plan.P, plan.Lt
        y1 = self.buf('pn_y1', Pn, 64)
        part = self._part(T, 64)
        ops.pointnet_layer1(points, pn['w1'], pn['b1'], y1, part, T)
        sc1, sh1 = self._finalize('pn1', part, T, 64, 64, pn['g1'], pn['be1'])
        # conv2..conv5: each consumes relu(gn(previous)) through the GEMM prologue
        x, sc, sh = y1, sc1, sh1
        for i, (N, K) in zip((2, 3, 4), ((64, 64), (64, 64), (128, 64))):
            y = self.buf('pn_y%d' % i, Pn, N)
            part = self._part(T, N)
            if self.pn_mlp64 and self.mlp == 'f16x3' and ('w%d_h16' % i) in pn:
                ops.pn_mlp64(pn['w%d_h16' % i], pn['w%d_os' % i], T, N, x, sc, sh, pn['b%d' % i], y, part)
            else:
                self._gemm(pn, 'w%d' % i, T, N, K, X=x, bias=pn['b%d' % i], Y=y, part=part, sc=sc, sh=sh,
                           amode=A_NORM_RELU)
            sc, sh = self._finalize('pn%d' % i, part, T, N, N, pn['g%d' % i], pn['be%d' % i])
            x = y
        # conv5 128->1024 + GN + ReLU + per-detection average (named max_feats in the reference,
        # point_net.py:138-148)
        seg1024 = self._norm_relu_pool(plan, 'w5', '5', 128, 1024, x, sc, sh)
        self._stash('pn_seg1024', seg1024)
        # PointNet_v1.conv1 split: per-detection 1024-channel part becomes a gathered bias
        dbias = self.buf('pn_dbias', Lt, 512)
        self._gemm(pn, 'wc1b', D, 512, 1024, X=seg1024, bias=pn['bc1'], Y=dbias)
        seg512 = self._norm_relu_pool(plan, 'wc1a', 'c1', 64, 512, y1, sc1, sh1, dbias=dbias)
        yc2, sc2, sh2 = self._gemm_gn(pn, 'wc2', D, 512, 512, 'pn_yc2', 'pnc2', 16, pn['gc2'], pn['bec2'], X=seg512,
                                      bias=pn['bc2'])
        ops.affine_act(yc2, 512, sc2, sh2, D, ACT_RELU, cat[:, 512:1024])

    def _norm_relu_pool(self, plan, w, s, K, N, x, sc, sh, dbias=None):
        """One "normalise and pool" layer of PointNet over the points: v = pn[w] relu(gn(x)) + bias (conv5, s = '5') or
        + dbias[detection of the row] (PointNet_v1.conv1, s = 'c1'), the GroupNorm statistics of v, then the per-detection
        mean of relu(gn(v)) -> workspace 'pn_seg<N>' [Lt][N].  Fused (pn_fused): the [P][N] tensor (1 GiB per cfg3 pair for
        conv5) is never stored - one pass for the statistics, one that normalises in the epilogue and emits per-tile column
        sums; on the A-resident kernel (hl16 weights only) the statistics may come from the second moments of the
        K-channel input instead (pn_gram: no GEMM pass).  Otherwise the tensor is materialised and pooled."""
        ops, pn, T, Lt = self.ops, self.P['pointnet'], plan.pt_tiles, plan.Lt
        name, g, be = 'pn' + s, pn['g' + s], pn['be' + s]
        if dbias is None:
            ares_kw = row_kw = dict(bias=pn['b' + s])
        else:
            ares_kw, row_kw = dict(dbias=dbias, tile_dbrow=plan.tile_det), dict(dbias=dbias, rowidx=plan.row_det)
        seg = self.buf('pn_seg%d' % N, Lt, N)
        if self.pn_fused and self.mlp == 'f16x3' and (w + '_h16') in pn:  # A-resident kernel
            TD, TH = plan.ptd_tiles, plan.ptd_half  # detection-aligned tiles and their 64-row halves
            if self.pn_gram and (dbias is None or hasattr(ops, 'gn_finalize_gram_dbias')):
                # over (detection-aligned, for the gathered bias) super-tiles: a pass over 4 K bytes per point
                GT, gram = (plan.gram_tiles, 'gram') if dbias is None else (plan.gram64_tiles, 'gram64')
                Gp, Sp = self.buf64(gram + '_G', GT.T, K * K), self.buf64(gram + '_S', GT.T, K)
                ops.gram_rows(x, K, sc, sh, GT, Gp, Sp)
                osc, osh = self.buf(name + '_sc', GT.G, N), self.buf(name + '_sh', GT.G, N)
                work = self.buf64(gram + '_work', GT.G, K * K + K)
                if dbias is None:
                    ops.gn_finalize_gram(Gp, Sp, GT, K, pn[w], pn['b' + s], N, g, be, EPS, work, osc, osh)
                else:
                    ops.gn_finalize_gram_dbias(Gp, Sp, GT, plan.gram64_tile_det, K, pn[w], dbias, N, g, be, EPS, work,
                                               osc, osh)
            else:
                part = self._part(TH, N)
                ops.gemm_ares(pn[w + '_h16'], pn[w + '_os'], TD, N, K, x, sc, sh, part=part, **ares_kw)
                osc, osh = self._finalize(name, part, TH, N, N, g, be)
            cs = self.buf('pn_colsum', TH.T, N)
            timed = self.conv_events is not None and dbias is None  # bench.py: HIP events around PointNet's dominant launch
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            ops.gemm_ares(pn[w + '_h16'], pn[w + '_os'], TD, N, K, x, sc, sh, osc=osc, osh=osh, colsum=cs, **ares_kw)
            if timed:
                e1.record()
                self.conv_events.append((name, plan.P, K, N, e0, e1))
            ops.segment_mean(cs, N, plan.det_half_segs, seg)
        elif self.pn_fused:
            TD = plan.ptd_tiles
            part = self._part(TD, N)
            self._gemm(pn, w, TD, N, K, X=x, part=part, sc=sc, sh=sh, amode=A_NORM_RELU, **row_kw)
            osc, osh = self._finalize(name, part, TD, N, N, g, be)
            cs = self.buf('pn_colsum', TD.T, N)
            self._gemm(pn, w, TD, N, K, X=x, sc=sc, sh=sh, amode=A_NORM_RELU, osc=osc, osh=osh, colsum=cs, **row_kw)
            ops.segment_mean(cs, N, plan.det_tile_segs, seg)
        else:
            y, osc, osh = self._gemm_gn(pn, w, T, N, K, 'pn_y' + s, name, N, g, be, X=x, sc=sc, sh=sh, amode=A_NORM_RELU,
                                        **row_kw)
            ops.segment_mean(y, N, plan.det_segs, seg, sc=osc, sh=osh, relu=True)
        return seg

    # ---- fusion module A / B / C --------------------------------------------
    def fuse(self, plan, cat, F):
        """cat [Lt,1024] -> F [3,Lt,512]; reference modules/fusion_net.py."""
        ops, fu, D, Lt = self.ops, self.P['fusion'], plan.det_tiles, plan.Lt
        mode = FUSION_MODES[self.fusion]
        img, pts = cat[:, 0:512], cat[:, 512:1024]
        if self.fusion == 'A':
            y0, sc0, sh0 = self._gemm_gn(fu, 'w0', D, 512, 1024, 'fu_y0', 'fu0', 512, fu['g0'], fu['be0'], X=cat,
                                         bias=fu['b0'])
            ops.fusion_combine(mode, cat, y0, None, sc0, sh0, None, None, D, F, Lt, 512)
            return
        N = 512 if self.fusion == 'B' else 1024
        ys, scs, shs = [], [], []
        for j, x in enumerate((img, pts)):  # NB: *_p weights consume the IMAGE features
            y, sc, sh = self._gemm_gn(fu, 'w%d' % j, D, N, 512, 'fu_y%d' % j, 'fu%d' % j, N, fu['g%d' % j],
                                      fu['be%d' % j], X=x, bias=fu['b%d' % j])
            ys.append(y)
            scs.append(sc[:, N - 512:])
            shs.append(sh[:, N - 512:])
        ops.fusion_combine(mode, cat, ys[0], ys[1], scs[0], shs[0], scs[1], shs[1], D, F, Lt, 512)

    # ---- negative-rejection head --------------------------------------------
    def det_scores(self, plan, F):
        """F [nR,Lt,512] -> [nR,Lt]; reference modules/tracking_net.py:91-100,149-163 (eval)."""
        ops, wd, T = self.ops, self.P['w_det'], plan.F_tiles
        R = plan.nR * plan.Lt
        X = F.view(R, 512)
        h0 = self.buf('det_h0', R, 512)
        self._gemm(wd, 'w0', T, 512, 512, X=X, bias=wd['b0'], Y=h0, act=ACT_RELU)
        h1 = self.buf('det_h1', R, 256)
        self._gemm(wd, 'w3', T, 256, 512, X=h0, bias=wd['b3'], Y=h1, act=ACT_RELU)
        out = torch.empty(plan.nR, plan.Lt, dtype=torch.float32, device=F.device)
        act = ACT_SIGMOID if 'cls' in self.score_arch else ACT_NONE
        ops.rowdot(h1, 256, wd['w6'], wd['b6'], T, out.view(-1), act=act, use_thr=True, thr=self.neg_threshold)
        return out

    # ---- pairwise affinity + new/end + softmax ------------------------------
    def affinity(self, plan, F):
        """reference modules/gcn.py:68-82, new_end.py:62-82, tracking_net.py:106-126."""
        ops, lk, PT, VT = self.ops, self.P['w_link'], plan.pair_tiles, plan.v_tiles
        nR, Lt, R = plan.nR, plan.Lt, plan.pair_tiles.R
        Ff = F.view(nR * Lt, 512)
        # uniform32 (include/mmmot_hip.h: pair_uniform32): every 32-row block of a pair tile lies inside one i - needs
        # M % 32 == 0 in every group AND tiles that start a multiple of 32 rows into their group
        pair = dict(row0=PT.g_row0, M=plan.pg_M, aoff=plan.pg_aoff, boff=plan.pg_boff, uniform32=plan.pair_uniform32)
        # stacked [new_end.conv0 ; conv1.0] over the on-the-fly pairwise tensor
        ya = self.buf('aff_ya', R, 1024)
        part = self._part(PT, 1024)
        self._gemm(lk, 'wa', PT, 1024, 512, FA=Ff, FB=Ff, pair=pair, amode=A_PAIR,
                 pairop=PAIR_OPS[self.affinity_op], bias=lk['ba'], Y=ya, part=part)
        sc_ne, sh_ne = self._finalize('aff_ne0', part[:, :, 0:512], PT, 512, 1, lk['g_ne0'], lk['be_ne0'], Y=ya[:, 0:512])
        sc1, sh1 = self._finalize('aff_1', part[:, :, 512:1024], PT, 512, 512, lk['g1'], lk['be1'], Y=ya[:, 512:1024])
        # new / end vectors: strided means of relu(gn(conv0)) over the prev / curr axis
        V = self.buf('aff_v', VT.R, 512)
        ops.segment_mean(ya[:, 0:512], 512, plan.v_segs, V, sc=sc_ne, sh=sh_ne, relu=True,
                         take_max=(self.end_mode != 'avg'))
        self._stash('aff_v', V)
        vh0, scv, shv = self._gemm_gn(lk, 'nw0', VT, 512, 512, 'aff_vh0', 'aff_v1', 1, lk['ng1'], lk['nbe1'], X=V,
                                      bias=lk['nb0'])
        vh1, scv2, shv2 = self._gemm_gn(lk, 'nw3', VT, 128, 512, 'aff_vh1', 'aff_v4', 1, lk['ng4'], lk['nbe4'], X=vh0,
                                        bias=lk['nb3'], sc=scv, sh=shv, amode=A_NORM_RELU)
        ne = torch.zeros(2, nR, Lt, dtype=torch.float32, device=F.device)  # eval-mode zero padding (tracking_net.py:183-189)
        ops.rowdot(vh1, 128, lk['nw6'], lk['nb6'], VT, ne.view(-1), sc=scv2, sh=shv2, act=ACT_SIGMOID,
                   omap=plan.v_omap)
        # link branch
        y3, sc4, sh4 = self._gemm_gn(lk, 'w3', PT, 512, 512, 'aff_y3', 'aff_4', 512, lk['g4'], lk['be4'],
                                     X=ya[:, 512:1024], bias=lk['b3'], sc=sc1, sh=sh1, amode=A_NORM_RELU)
        y6, sc7, sh7 = self._gemm_gn(lk, 'w6', PT, 128, 512, 'aff_y6', 'aff_7', 128, lk['g7'], lk['be7'], X=y3,
                                     bias=lk['b6'], sc=sc4, sh=sh4, amode=A_NORM_RELU)
        logits = torch.empty(R, dtype=torch.float32, device=F.device)
        ops.rowdot(y6, 128, lk['w9'], lk['b9'], PT, logits, sc=sc7, sh=sh7)
        self._stash('aff_logits', logits)
        link = logits
        if self.softmax_mode != 'none':
            link = torch.empty_like(logits)
            ops.softmax_pairs(logits, link, PT.g_row0, plan.pg_N, plan.pg_M, PT.G, plan.max_nm,
                              SOFTMAX_MODES[self.softmax_mode])
        return link, ne[0], ne[1]

    # ---- whole forward -------------------------------------------------------
    def forward(self, plan, crops=None, points=None, appearance=None):
        """Returns dict(det [nR,Lt], link flat, new [nR,Lt], end [nR,Lt], feats F, cat).

        ``appearance``: precomputed appearance rows (fp32 [.., 512], contiguous, on the weights' device: the output of
        TrackingNet.encode_appearance) in place of the image branch for some frames - (a) every row, [Lt, 512] with
        crops=None: neither the trunk nor the SkipPool heads run; (b) the first frame's N rows of a B = 1 pair plan with
        the crops of the second frame only: the trunk runs on those M crops into cat[N:].  The rows are copied into the
        appearance half of `cat`; everything after it is the same launch sequence."""
        # One forward at a time per engine: the workspace arena (self.ws), the packed weights and the range-guard
        # block are mutable state behind the integer handle of the registered operators (mmmot_amd/torch_ops.py), which
        # an operator schema cannot express.  A second thread entering while a forward is being issued is refused; a
        # forward issued on ANOTHER stream than the previous one first waits for that stream (the previous forward's
        # kernels still read and write the same workspace), so consecutive forwards are ordered whatever stream they
        # are launched on.  Outputs: det / link / new / end are freshly allocated per call; 'F' and 'cat' are views
        # of the workspace, valid until the next forward of this engine.
        with self._exclusive():
            cur = self._follow_stream(next((t for t in (crops, points, appearance) if t is not None), None))
            with self._pinned(cur):
                return self._forward(plan, crops, points, appearance)

    @contextlib.contextmanager
    def _exclusive(self):
        """one launch sequence at a time on this engine (see forward)"""
        if not self._busy.acquire(blocking=False):
            raise RuntimeError('mmmot_amd: concurrent forwards on one engine (its workspace arena is shared mutable state); '
                               'use one TrackingNet per thread, or serialise the calls')
        try:
            yield
        finally:
            self._busy.release()

    def _follow_stream(self, ref):
        """torch's current stream on `ref`'s device, ordered behind the stream of this engine's previous launch sequence
        (whose kernels still use the same workspace); None for host tensors"""
        if ref is None or not ref.is_cuda:
            return None
        cur = torch.cuda.current_stream(ref.device)
        last = self._last_stream
        if last is not None and last != cur and not torch.cuda.is_current_stream_capturing():
            cur.wait_stream(last)
        self._last_stream = cur
        return cur

    def _pinned(self, cur):
        """the operator backend's stream pinning for a launch sequence on `cur` (nothing for backends without it)"""
        pin = getattr(self.ops, 'on_current_stream', None)
        return contextlib.nullcontext() if pin is None else pin(cur)

    def _check_crops(self, plan, crops, Lt=None):
        Lt = plan.Lt if Lt is None else Lt
        ok_f32 = crops is not None and crops.dtype == torch.float32 and tuple(crops.shape) == (Lt, 3, plan.S, plan.S)
        ok_u8 = crops is not None and crops.dtype == torch.uint8 and tuple(crops.shape) == (Lt, plan.S, plan.S, 3)
        if not (ok_f32 or ok_u8) or not crops.is_contiguous():
            raise ValueError('crops must be a contiguous fp32 [%d,3,%d,%d] tensor (the reference\'s normalised `dets`) or '
                             'the uint8 [%d,%d,%d,3] crops of the resize' % (Lt, plan.S, plan.S, Lt, plan.S, plan.S))
        check_crop_side(plan.S)  # here, before any launch (appearance() repeats it for its direct callers)

    def _check_appearance(self, plan, crops, appearance):
        """Host checks of supplied appearance rows and the crops beside them, before anything is queued (see forward).
        Returns the number of leading rows supplied: Lt (shape a) or the first frame's N (shape b)."""
        if not ((0 in plan.rows) or (2 in plan.rows)):
            raise ValueError('appearance rows given for a plan whose rows %r do not use the image branch' % (plan.rows,))
        dev = next(t for t in self.P['vgg'][0].values() if torch.is_tensor(t)).device
        if (not torch.is_tensor(appearance) or appearance.dtype != torch.float32 or appearance.dim() != 2
                or appearance.shape[1] != 512 or not appearance.is_contiguous() or appearance.device != dev):
            raise ValueError('appearance rows must be a contiguous fp32 [L,512] tensor on %s (TrackingNet.encode_appearance), '
                             'got %s' % (dev, 'a %s %s tensor on %s' % (appearance.dtype, tuple(appearance.shape),
                                                                       appearance.device)
                                         if torch.is_tensor(appearance) else type(appearance).__name__))
        n = int(appearance.shape[0])
        if crops is None:
            if n != plan.Lt:
                raise ValueError('appearance rows without crops must cover every detection of the plan: [%d,512], got '
                                 '[%d,512]' % (plan.Lt, n))
            return n
        if plan.B != 1 or len(plan.frame_counts[0]) != 2:
            raise ValueError('appearance rows beside crops need a plan of one frame pair (B = 1, two frames)')
        N, M = plan.frame_counts[0]
        L = int(crops.shape[0]) if crops.dim() > 0 else -1
        if n + L > plan.Lt:
            raise ValueError('appearance rows (%d) and crops (%d) are given for the same frame: rows for the first frame '
                             '(%d detections), crops for the second (%d)' % (n, L, N, M))
        if n != N:
            raise ValueError('appearance rows beside crops belong to the first frame: [%d,512], got [%d,512]' % (N, n))
        self._check_crops(plan, crops, Lt=M)
        if crops.device != dev:
            raise ValueError('crops on %s, weights on %s' % (crops.device, dev))
        return n

    def _image_key(self, plan, crops, appearance):
        """what image_first() leaves in `cat`: the next forward with the same inputs skips its image branch"""
        key = (crops.data_ptr(), plan.Lt, plan.S, crops.dtype)
        if appearance is not None:
            key += (appearance.data_ptr(), int(appearance.shape[0]))
        return key

    def _image_branch(self, plan, crops, appearance, cat):
        """the appearance half of `cat`: supplied rows copied in, the trunk (under the range guard) for the rest"""
        if appearance is None:
            self.guard.run(self.appearance, plan, crops, cat)
            return
        n = int(appearance.shape[0])
        cat[:n, 0:512].copy_(appearance)  # a device copy, no arithmetic
        if n < plan.Lt:
            self.guard.run(self.appearance, plan.tail_crops(), crops, cat[n:])

    def encode(self, plan, crops):
        """The image branch of `plan`'s crops alone, under the range guard: owned fp32 rows [Lt, 512] (the appearance half
        of `cat`) and the index of the forward they were computed in."""
        with self._exclusive():
            self._check_crops(plan, crops)
            self.drop_head_start()  # `cat` is overwritten: an image branch issued before is gone
            cur = self._follow_stream(crops)
            self.dev = crops.device
            cat = self.buf('cat', plan.Lt, 1024)
            with self._pinned(cur):
                self.guard.run(self.appearance, plan, crops, cat)
            return cat[:, 0:512].clone(), self.guard.n_forward - 1

    def image_first(self, plan, crops, appearance=None):
        """Issue the image branch (trunk + SkipPool heads -> the appearance half of `cat`) of the NEXT ``forward`` now.
        The trunk needs the detections' counts only, not the point split: the reference-shaped call (TrackingNet.forward)
        launches it before it reads ``points_split`` back and builds the full plan, so that ~0.3 ms of host work hide
        behind ~2 ms of device work.  `plan` may be any plan with the same frame counts and crop side (its image tables are
        the ones used); the next ``forward`` with the same crops tensor skips its own image branch.  ``appearance``: the
        first frame's rows of shape (b) of ``forward`` - copied in, the trunk runs on the second frame's crops."""
        with self._exclusive():
            if appearance is None:
                self._check_crops(plan, crops)
            else:
                self._check_appearance(plan, crops, appearance)
            cur = self._follow_stream(crops)
            self.dev = crops.device
            cat = self.buf('cat', plan.Lt, 1024)
            self._head_start = None
            # what was queued before the trunk: the point the LiDAR branch of the coming forward may start from (side stream)
            pre = None
            if cur is not None and self.pn_beside_trunk and not torch.cuda.is_current_stream_capturing():
                pre = torch.cuda.Event()
                pre.record(cur)
            with self._pinned(cur):
                self._image_branch(plan, crops, appearance, cat)
            self._head_start = (self._image_key(plan, crops, appearance), pre)

    def drop_head_start(self):
        """forget the image branch image_first() issued: the forward it was meant for does not come, or `cat` is reused"""
        self._head_start = None

    def _forward(self, plan, crops=None, points=None, appearance=None):
        rows = plan.rows
        need_img = (0 in rows) or (2 in rows)
        need_pts = (1 in rows) or (2 in rows)
        (token, pre), self._head_start = self._head_start or (None, None), None  # taken by this forward, whatever follows
        if appearance is not None:
            self._check_appearance(plan, crops, appearance)
        elif need_img:
            self._check_crops(plan, crops)
        dev = next(t for t in (crops, appearance, points) if t is not None).device
        self.dev = dev
        Lt = plan.Lt
        cat = self.buf('cat', Lt, 1024)
        # image_first() ran the image branch of exactly these inputs into `cat` already
        img_done = (need_img and crops is not None and token is not None
                    and token == self._image_key(plan, crops, appearance))
        if need_pts:
            kin = int(self.P['pointnet']['w1'].shape[1])  # 3 (xyz) or 4 (xyz + reflectivity)
            if points is None or tuple(points.shape) != (plan.P, kin) or not points.is_contiguous():
                raise ValueError('points must be a contiguous [%d,%d] tensor' % (plan.P, kin))
        # The two branches meet only in `cat` (disjoint column halves, disjoint workspace buffers), so the LiDAR branch
        # can run on a side stream (two_streams, opt-in): the trunk's persistent workgroups fill every CU (one per CU,
        # all its LDS and registers) - the branches never share a CU, only PointNet's small-grid launches and the
        # uneven tail of a trunk layer leave CUs to the other stream.  Fork / join are events: capturable in a hipGraph.
        side = None
        if (img_done and need_pts and pre is not None and dev.type == 'cuda' and hasattr(self.ops, 'on_stream')
                and not torch.cuda.is_current_stream_capturing()):
            # the trunk of this forward is already running (image_first): the LiDAR branch goes beside it - it starts from
            # the point the trunk was launched at, not behind it.  At the reference's call shape (one frame pair) the last
            # trunk layers leave CUs idle (conv5 of 22 crops: 176 tiles on 256 CUs) and PointNet's ~15 small launches
            # hide there
            main = torch.cuda.current_stream(dev)
            sd = self._side_stream(dev)
            sd.wait_event(pre)
            with self.ops.on_stream(sd):
                self.pointnet(plan, points, cat)
            main.wait_stream(sd)
            need_pts = False  # done
        elif need_img and need_pts and self.two_streams and dev.type == 'cuda' and hasattr(self.ops, 'on_stream'):
            side = self._side_stream(dev)
        if side is not None:
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)  # inputs (and the previous forward's readers of the workspace) are ordered before
            with self.ops.on_stream(side):
                self.pointnet(plan, points, cat)
            if not img_done:
                self._image_branch(plan, crops, appearance, cat)
            main.wait_stream(side)
        else:
            if need_img and not img_done:
                self._image_branch(plan, crops, appearance, cat)
            if need_pts:
                self.pointnet(plan, points, cat)
        F = self.buf('F', plan.nR, Lt, 512)
        if rows == (0, 1, 2):
            self.fuse(plan, cat, F)
        else:
            for ri, r in enumerate(rows):  # single-modality rows: a device copy, no arithmetic
                if r == 2:
                    raise ValueError('the fused row needs rows=(0,1,2)')
                F[ri].copy_(cat[:, 512 * r:512 * (r + 1)])
        det = self.det_scores(plan, F)
        link, new, end = self.affinity(plan, F)
        return dict(det=det, link=link, new=new, end=end, F=F, cat=cat)
