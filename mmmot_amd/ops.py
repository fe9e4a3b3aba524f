"""Python-side operator layer over the C-ABI (include/mmmot_hip.h).

``HipOps`` takes torch CUDA tensors (possibly 2-D row-strided views), extracts
raw device pointers / leading dimensions and calls libmmmot_hip.so on torch's
current HIP stream.  torch is used for device memory and streams only - no
torch operator computes anything on this path.  CPU tensors are rejected:
there is no fallback.
"""
import contextlib
import ctypes
import os
import threading

import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
A_PLAIN, A_NORM_RELU, A_PAIR = 0, 1, 2
PAIR_OPS = {'multiply': 0, 'minus_abs': 1, 'minus': 2}
SOFTMAX_MODES = {'single': 1, 'dual': 2, 'dual_add': 3, 'dual_max': 4}
FUSION_MODES = {'A': 0, 'B': 1, 'C': 2}
LOSS_KINDS = {'bce': 0, 'l2': 1, 'l1': 2}


def _pointer(dtype):
    """The converter of a pointer argument to ``dtype`` data: a device tensor of that dtype -> its address; None -> NULL;
    anything that is no tensor passes as it is (an address the caller has checked itself, a ctypes byref / array)."""
    def ptr(t):
        if t is None:
            return None
        try:
            cuda = t.is_cuda
        except AttributeError:
            return t
        if not cuda:
            raise RuntimeError('mmmot_amd HIP ops need device tensors (got %s); there is no CPU fallback' % t.device)
        if t.dtype != dtype:
            raise TypeError('expected %s, got %s' % (dtype, t.dtype))
        return t.data_ptr()
    return ptr


# element type of a pointer parameter by the header's pointee; the packed Adam rows travel as a uint8 block
_POINTERS = {c: _pointer(d) for c, d in (
    ('float', torch.float32), ('int', torch.int32), ('unsigned int', torch.int32), ('long long', torch.int64),
    ('double', torch.float64), ('unsigned char', torch.uint8), ('mmmot_adam_row', torch.uint8))}
# `void*` buffers (hl16 / hq8 records, workspaces) have no element type in the header: their call sites say it
_ptr, _iptr = _POINTERS['float'], _POINTERS['int']


def _converter(p):
    if p.pointee is None:
        return float if p.ctype in (ctypes.c_float, ctypes.c_double) else int
    return _POINTERS.get(p.pointee)  # None (passed as it is): void*, char*, the args structs - the caller's to check


def _call(name, params):
    """``f(fn, ops, *args)`` of one entry point: calls ``fn`` with every argument through the converter of its parameter
    in the header and, where the entry takes one, ``ops._stream()`` behind them (resolved last, as a wrapper that spells
    the call out would).  One generated lambda per entry, built once at import: the same conversions as a loop over a
    converter tuple cost about 1 us more per launch, which the host-bound B = 1 forward (~80 launches in 2.5 ms) shows."""
    stream = name in _lib.TAKES_STREAM
    conv = {'c%d' % i: _converter(p) for i, p in enumerate(params[:-1] if stream else params)}
    args = ['a%d' % i for i in range(len(conv))]
    passed = ['a%d' % i if conv['c%d' % i] is None else 'c%d(a%d)' % (i, i) for i in range(len(conv))]
    passed += ['ops._stream()'] * stream
    return eval('lambda fn, ops, %s: fn(%s)' % (', '.join(args), ', '.join(passed)), conv)


_CALLS = {name: _call(name, params) for name, params in _lib.PARAMS.items()}


def _ld(t):
    """Leading dimension of a 2-D row-strided view (unit inner stride)."""
    if t is None:
        return 0
    if t.dim() == 1:
        return t.shape[0]
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError('expected a 2-D view with unit inner stride, got shape %s stride %s' % (
            tuple(t.shape), tuple(t.stride())))
    return t.stride(0)


class HipOps:
    """The product backend: every method is one C-ABI call."""
    name = 'hip'

    def __init__(self):
        self.lib = _lib.load()
        self._osvecs = {}
        self._scr = {}
        # weight-gradient GEMMs: fp16 matrix cores with the 3-term split (default) or MMMOT_GEMM_TN=f32: exact fp32 MFMA
        self.tn_f16 = os.environ.get('MMMOT_GEMM_TN', 'f16x3') != 'f32'
        # the stream a launch sequence was pinned to is per THREAD: two threads sharing one model, each under its own
        # torch.cuda.stream(), must not see each other's pin
        self._tls = threading.local()

    @property
    def _pinned_stream(self):
        return getattr(self._tls, 'stream', None)

    @_pinned_stream.setter
    def _pinned_stream(self, v):
        self._tls.stream = v

    def _scratch(self, name, n, device):
        key = (name, n, str(device))
        t = self._scr.get(key)
        if t is None:
            t = self._scr[key] = torch.empty(n, dtype=torch.float32, device=device)
        return t

    def _osv(self, oscale, Cout, like):
        """The [Cout] per-output-channel scale vector of the trunk entry points; a python float (the kernel tests'
        one-scale-per-layer case) is expanded to a cached constant vector."""
        if torch.is_tensor(oscale):
            if oscale.numel() != Cout:
                raise ValueError('oscale must hold one scale per output channel')
            return oscale
        key = (float(oscale), Cout, like.device)
        v = self._osvecs.get(key)
        if v is None:
            v = self._osvecs[key] = torch.full((Cout,), float(oscale), dtype=torch.float32, device=like.device)
        return v

    def _stream(self):
        s = getattr(self._tls, 'stream', None)
        return torch.cuda.current_stream().cuda_stream if s is None else s

    @contextlib.contextmanager
    def on_current_stream(self, stream=None):
        """Resolve torch's current HIP stream once for a whole launch sequence (``torch.cuda.current_stream()`` costs
        ~8 us per call - 0.6 ms over the ~80 launches of a forward); the stream must not change inside the block.
        ``stream``: the already resolved current stream (a torch.cuda.Stream), if the caller has it."""
        prev = self._pinned_stream
        self._pinned_stream = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
        try:
            yield
        finally:
            self._pinned_stream = prev

    @contextlib.contextmanager
    def on_stream(self, stream):
        """Launch on ``stream`` (a torch.cuda.Stream) inside the block - the LiDAR branch of a two-stream forward -
        whatever stream the surrounding ``on_current_stream`` block pinned."""
        prev = self._pinned_stream
        self._pinned_stream = stream.cuda_stream
        try:
            with torch.cuda.stream(stream):
                yield
        finally:
            self._pinned_stream = prev

    def _status(self, name, *args):
        """One C-ABI call: ``args`` are the header's parameters in order, without the stream (appended where the entry
        takes one); pointers and scalars are converted as the header types them.  Returns the entry's status."""
        return _CALLS[name](getattr(self.lib, name), self, *args)

    def _launch(self, name, *args):
        """``_status`` that raises unless the entry returned 0 (spelled out: one python call less per launch)."""
        st = _CALLS[name](getattr(self.lib, name), self, *args)
        if st != 0:
            _lib.check(st, name)

    def conv3x3(self, inp, wp, bias, out, L, H, W, Cin, Cout, first, pool):
        self._launch('mmmot_conv3x3_bn_relu', inp, wp, bias, out, L, H, W, Cin, Cout, first, pool)

    def conv3x3_hl16_patch(self, inp, wp, bias, out, L, H, W, Cin, Cout, pool, oscale):
        """fp16-split trunk layer (LDS-resident haloed patch kernel): inp/out/wp are fp32-typed buffers holding hl16
        data (same bytes), oscale the [Cout] vector of per-output-channel 2^-shift."""
        self._launch('mmmot_conv3x3_bn_relu_hl16_patch', _ptr(inp), _ptr(wp), bias, _ptr(out), L, H, W, Cin, Cout, pool,
                     self._osv(oscale, Cout, out))

    def conv1_fused_hl16(self, crops, w1, bias1, oscale1, w2, bias2, oscale2, out, L, H, W):
        """conv1_1 + conv1_2 + max-pool in one launch (the conv1_1 tensor never reaches HBM)."""
        self._launch('mmmot_conv1_fused_hl16', crops, _ptr(w1), bias1, oscale1, _ptr(w2), bias2,
                     self._osv(oscale2, 64, out), _ptr(out), L, H, W)

    def conv3x3_hq8(self, inp, wp, bias, out, L, H, W, Cin, Cout, pool, oscale):
        """conv3x3_hl16_patch in hq8 arithmetic: activations / weights are hq8 records (pack.to_hq8_act / to_hq8_w)."""
        self._launch('mmmot_conv3x3_bn_relu_hq8', _ptr(inp), _ptr(wp), bias, _ptr(out), L, H, W, Cin, Cout, pool,
                     self._osv(oscale, Cout, out))

    def conv1_fused_hq8(self, crops, w1, bias1, oscale1, w2, bias2, oscale2, out, L, H, W):
        """conv1_fused_hl16 with conv1_2 in hq8 arithmetic (w1 hl16, w2 hq8, out hq8)."""
        self._launch('mmmot_conv1_fused_hq8', crops, _ptr(w1), bias1, oscale1, _ptr(w2), bias2,
                     self._osv(oscale2, 64, out), _ptr(out), L, H, W)

    def conv1_fused_u8(self, crops_u8, mean, std, w1, bias1, oscale1, w2, bias2, oscale2, out, L, H, W, q8=False):
        """conv1_fused_hl16 / _hq8 fed by the 8-bit crops [L][H][W][3]: ToTensor + Normalize in the loader"""
        self._launch('mmmot_conv1_fused_u8', crops_u8, mean[0], mean[1], mean[2], std[0], std[1], std[2], _ptr(w1), bias1,
                     oscale1, _ptr(w2), bias2, self._osv(oscale2, 64, out), _ptr(out), L, H, W, bool(q8))

    def u8_normalize(self, crops_u8, mean_std, out, N, S):
        self._launch('mmmot_u8_normalize', crops_u8, N, S, mean_std, out)

    def crop_augment(self, crops_u8, params, mean_std, out, out_u8, L, S):
        """random-resized-crop + flip + ToTensor / Normalize of the 8-bit crops [L][S][S][3]: params the device int32
        [L][5] table (top, left, h, w, flip); out fp32 [L][3][S][S] and / or out_u8 [L][S][S][3]"""
        self._launch('mmmot_crop_augment', crops_u8, params, L, S, mean_std, out, out_u8)

    def trunk_range_read(self, device, reset=True):
        """(e4m3-saturated, fp16-clamped, conv1_1 hits, 0) activation-element counters of the trunk epilogues on
        ``device`` since the last reset; synchronises the current stream (see mmmot_trunk_range_read)."""
        if torch.device(device).type != 'cuda':
            raise RuntimeError('mmmot_amd HIP ops need device tensors (got %s); there is no CPU fallback' % device)
        buf = (ctypes.c_uint * 4)()
        with torch.cuda.device(device):
            torch.cuda.current_stream().synchronize()
            self._launch('mmmot_trunk_range_read', buf, reset)
        return tuple(int(v) for v in buf)

    def trunk_range_bind(self, counters):
        """Counter block (int32 [4] device tensor, or None = the library's per-device block) the trunk launches issued
        by this thread report to from now on (mmmot_trunk_range_bind)."""
        self._launch('mmmot_trunk_range_bind', counters)

    def set_patch_tile_width(self, bn):
        """Test knob: output channels per tile of the patch kernels (0 = automatic, 64, 128; mmmot_set_patch_tile_width)."""
        self._launch('mmmot_set_patch_tile_width', bn)

    def patch_choice(self, L, H, W, Cout):
        """(channels per tile, block edge, tiles, workgroups) of the next patch-kernel launch of this shape under the
        current knobs (mmmot_patch_choice); no launch."""
        v = [ctypes.c_int(0) for _ in range(4)]
        self._launch('mmmot_patch_choice', L, H, W, Cout, *[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    def hq8_pack(self, x, y):
        self._launch('mmmot_hq8_pack', x, _ptr(y), x.numel())

    def hq8_unpack(self, x, y):
        self._launch('mmmot_hq8_unpack', _ptr(x), y, y.numel())

    def conv3x3_first_hl16(self, inp, wp, bias, out, L, H, W, Cout):
        self._launch('mmmot_conv3x3_first_hl16', inp, wp, bias, _ptr(out), L, H, W, Cout)

    def hl16_pack(self, x, y):
        self._launch('mmmot_hl16_pack', x, _ptr(y), x.numel())

    def hl16_unpack(self, x, y):
        self._launch('mmmot_hl16_unpack', _ptr(x), y, y.numel())

    # ---- training step on the fp16 matrix cores: device-side power-of-two scales, raw-output trunk convolution ----
    def absmax(self, X, out):
        """out[0] = max |X| over a contiguous [R][C] tensor (device scalar, no host round trip)"""
        R, C = X.numel() // X.shape[-1], X.shape[-1]
        self._launch('mmmot_absmax', X, C, R, C, out)

    def hl16_pack_pow2(self, x, y, amax, target):
        self._launch('mmmot_hl16_pack_pow2', x, _ptr(y), x.numel(), amax, target)

    def pow2_oscale(self, out, amax_a, target_a, amax_b=None, target_b=0):
        self._launch('mmmot_pow2_oscale', out, out.numel(), amax_a, target_a, amax_b, target_b)

    def conv3x3_raw_hl16(self, x16, w16, bias, out, L, H, W, Cin, Cout, oscale):
        self._launch('mmmot_conv3x3_raw_hl16', _ptr(x16), _ptr(w16), bias, out, L, H, W, Cin, Cout, oscale)

    def gemm(self, W, tiles, N, K, X=None, bias=None, dbias=None, rowidx=None, Y=None, part=None,
             sc=None, sh=None, FA=None, FB=None, pair=None, amode=A_PLAIN, pairop=0, act=ACT_NONE,
             w_hl16=False, oscale=1.0, osc=None, osh=None, colsum=None):
        """W: [N][K] fp32 weights, or (w_hl16=True) the hl16 split-half copy scaled by 1/oscale.
        colsum [T][N] (+ osc/osh [G][N]): per-tile column sums of relu(v * osc + osh) (fused next-norm consumer)."""
        a = self._gemm_args(W, tiles, N, K, X, bias, dbias, rowidx, Y, part, sc, sh, FA, FB, pair, amode, pairop, act,
                            w_hl16, oscale, osc, osh, colsum)
        self._launch('mmmot_gemm_rows', ctypes.byref(a))

    def gemm_choice(self, W, tiles, N, K, **kw):
        """(wide, nh, items, grid) of the gemm launch of the same arguments under the current variant and grid limit
        (mmmot_gemm_rows_choice); no launch."""
        d = dict(X=None, bias=None, dbias=None, rowidx=None, Y=None, part=None, sc=None, sh=None, FA=None, FB=None,
                 pair=None, amode=A_PLAIN, pairop=0, act=ACT_NONE, w_hl16=False, oscale=1.0, osc=None, osh=None, colsum=None)
        d.update(kw)
        a = self._gemm_args(W, tiles, N, K, *[d[k] for k in ('X', 'bias', 'dbias', 'rowidx', 'Y', 'part', 'sc', 'sh', 'FA',
                                                             'FB', 'pair', 'amode', 'pairop', 'act', 'w_hl16', 'oscale',
                                                             'osc', 'osh', 'colsum')])
        v = [ctypes.c_int(0) for _ in range(4)]
        self._launch('mmmot_gemm_rows_choice', ctypes.byref(a), *[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    def set_gemm_wide_grid_limit(self, n):
        """Test knob: cap of the wide kernel's persistent grid (0 = automatic; mmmot_set_gemm_wide_grid_limit)."""
        self._launch('mmmot_set_gemm_wide_grid_limit', n)

    @staticmethod
    def _gemm_args(W, tiles, N, K, X, bias, dbias, rowidx, Y, part, sc, sh, FA, FB, pair, amode, pairop, act, w_hl16,
                   oscale, osc, osh, colsum):
        a = _lib.GemmArgs()
        a.X, a.ldx = _ptr(X), _ld(X)
        a.W = _ptr(W)
        a.bias = _ptr(bias)
        a.dbias, a.rowidx, a.lddb = _ptr(dbias), _iptr(rowidx), _ld(dbias)
        a.Y, a.ldy = _ptr(Y), _ld(Y)
        a.part = _ptr(part)
        a.sc, a.sh, a.ldsc = _ptr(sc), _ptr(sh), _ld(sc)
        a.FA, a.FB, a.ldf = _ptr(FA), _ptr(FB), _ld(FA)
        a.tile_row0, a.tile_nrows, a.tile_group = _iptr(tiles.row0), _iptr(tiles.nrows), _iptr(tiles.group)
        if pair is not None:
            a.grp_row0, a.grp_M = _iptr(pair['row0']), _iptr(pair['M'])
            a.grp_aoff, a.grp_boff = _iptr(pair['aoff']), _iptr(pair['boff'])
            a.pair_uniform32 = int(bool(pair.get('uniform32', False)))  # every M a multiple of 32 (the caller's plan knows)
        a.T, a.N, a.K = tiles.T, N, K
        a.amode, a.pairop, a.act = amode, pairop, act
        a.w_hl16, a.oscale = int(w_hl16), float(oscale)
        a.osc, a.osh, a.ldosc = _ptr(osc), _ptr(osh), _ld(osc)
        a.colsum = _ptr(colsum)
        return a

    def gemm_ares(self, W16, oscale, tiles, N, K, X, sc, sh, bias=None, dbias=None, tile_dbrow=None, part=None,
                  osc=None, osh=None, colsum=None):
        """A-resident GEMM (hl16 weights): statistics `part` [2T][2][N] and/or `colsum` [2T][N] per 64-row
        half tile; the product itself is never stored (see include/mmmot_hip.h: mmmot_gemm_ares)."""
        a = _lib.GemmAresArgs()
        a.X, a.ldx = _ptr(X), _ld(X)
        a.sc, a.sh, a.ldsc = _ptr(sc), _ptr(sh), _ld(sc)
        a.W, a.bias = _ptr(W16), _ptr(bias)
        a.dbias, a.tile_dbrow, a.lddb = _ptr(dbias), _iptr(tile_dbrow), _ld(dbias)
        a.tile_row0, a.tile_nrows, a.tile_group = _iptr(tiles.row0), _iptr(tiles.nrows), _iptr(tiles.group)
        a.part = _ptr(part)
        a.osc, a.osh, a.ldosc = _ptr(osc), _ptr(osh), _ld(osc)
        a.colsum = _ptr(colsum)
        a.T, a.N, a.K, a.oscale = tiles.T, N, K, float(oscale)
        self._launch('mmmot_gemm_ares', ctypes.byref(a))

    def pn_mlp64(self, W16, oscale, tiles, N, X, sc, sh, bias, Y, part):
        """PointNet K = 64 layer: Y / part of relu(X*sc+sh) W^T + b from the persistent weight-resident kernel (same
        results contract as gemm(amode=A_NORM_RELU, w_hl16=True, K=64); see mmmot_pn_mlp64)."""
        self._launch('mmmot_pn_mlp64', X, _ld(X), sc, sh, _ld(sc), _ptr(W16), oscale, bias, Y, _ld(Y), part, tiles.row0,
                     tiles.nrows, tiles.group, tiles.T, N)

    def gram_rows(self, X, K, sc, sh, tiles, Gout, Sout):
        """Per super-tile Gram matrix / column sums (float64) of relu(X*sc+sh); see mmmot_gram_rows.  K = 128: only the
        32 x 32 blocks on and above the block diagonal of Gout are written (the lower ones keep what the buffer held);
        gn_finalize_gram(_dbias) reads those blocks only."""
        self._launch('mmmot_gram_rows', X, _ld(X), K, sc, sh, _ld(sc), tiles.row0, tiles.nrows, tiles.group, tiles.T,
                     Gout, Sout)

    def gn_finalize_gram(self, Gp, Sp, tiles, K, W, bias, N, gamma, beta, eps, work, sc, sh):
        """GroupNorm(N, N) scale/shift of v = W a + b from the Gram partials of a; see mmmot_gn_finalize_gram."""
        self._launch('mmmot_gn_finalize_gram', Gp, Sp, tiles.g_tile0, tiles.g_ntiles, tiles.g_count, tiles.G, K, W, bias,
                     N, gamma, beta, eps, work, sc, sh)

    def gn_finalize_gram_dbias(self, Gp, Sp, tiles, tile_det, K, W, dbias, N, gamma, beta, eps, work, sc, sh):
        """GroupNorm(N, N) scale/shift of v = W a + dbias[det] from the Gram partials of a over detection-aligned
        super-tiles (tile_det: int32 [T], the dbias row of every super-tile); see mmmot_gn_finalize_gram_dbias."""
        self._launch('mmmot_gn_finalize_gram_dbias', Gp, Sp, tiles.g_tile0, tiles.g_ntiles, tiles.g_count, tiles.G,
                     tiles.nrows, tile_det, K, W, dbias, _ld(dbias), N, gamma, beta, eps, work, sc, sh)

    def gn_finalize(self, part, tiles, C, NG, gamma, beta, eps, sc, sh):
        """part: [T][2][>=C] view (unit inner stride); statistics of its first C channels."""
        if part.dim() != 3 or part.stride(2) != 1 or part.stride(0) != 2 * part.stride(1):
            raise ValueError('part must be a [T][2][C] view of a [T][2][ldp] buffer')
        self._launch('mmmot_gn_finalize', part, tiles.g_tile0, tiles.g_ntiles, tiles.g_count,
                     tiles.nrows if tiles.ragged else None, tiles.G, part.stride(1), C, NG, gamma, beta, eps, sc, sh)

    def segment_mean(self, X, C, segs, out, sc=None, sh=None, relu=False, use_group=True, hl16=False, take_max=False):
        """segs.div (optional int32 tensor): divisor per segment instead of its row count; take_max: maximum over the
        segment instead of the mean."""
        self._launch('mmmot_segment_mean', X, _ld(X), C, segs.start, segs.count, segs.stride,
                     segs.group if use_group else None, getattr(segs, 'div', None), segs.n, sc, sh, _ld(sc),
                     bool(relu) | (2 if take_max else 0), out, _ld(out), hl16)

    def rowdot(self, X, K, w, b, tiles, out, sc=None, sh=None, act=ACT_NONE, use_thr=False, thr=0.0, omap=None):
        self._launch('mmmot_rowdot', X, _ld(X), K, w, b, sc, sh, _ld(sc), tiles.row0, tiles.nrows, tiles.group, tiles.T,
                     act, use_thr, thr, out, omap)

    def row_layernorm(self, X, C, gamma, beta, eps, relu, Y, R):
        self._launch('mmmot_row_layernorm', X, _ld(X), C, gamma, beta, eps, relu, Y, _ld(Y), R)

    def skippool_head(self, P, C, hd, eps, out, R):
        """one SkipPool head (appear_net.py:19-32) on the pooled rows P [R][C] -> out [R][128]; hd: packed head dict"""
        self._launch('mmmot_skippool_head', P, _ld(P), C, hd['w1'].shape[0], hd['g0'], hd['b0'], hd['w1'], hd['c1'],
                     hd['g2'], hd['b2'], hd['w4'], hd['c4'], hd['g5'], hd['b5'], eps, out, _ld(out), R)

    def pointnet_layer1(self, X, W, bias, Y, part, tiles):
        """X [P][K] with K = W.shape[1] in (3, 4)."""
        self._launch('mmmot_pointnet_layer1', X, W.shape[1], W, bias, Y, part, tiles.row0, tiles.nrows, tiles.T)

    def affine_act(self, X, C, sc, sh, tiles, act, Y):
        self._launch('mmmot_affine_act', X, _ld(X), C, sc, sh, _ld(sc), tiles.row0, tiles.nrows, tiles.group, tiles.T, act,
                     Y, _ld(Y))

    def fusion_combine(self, mode, cat, Y0, Y1, sc0, sh0, sc1, sh1, tiles, F, Lt, C):
        self._launch('mmmot_fusion_combine', mode, cat, Y0, _ld(Y0), Y1, _ld(Y1), sc0, sh0, sc1, sh1, _ld(sc0),
                     tiles.row0, tiles.nrows, tiles.group, tiles.T, F, Lt, C)

    def softmax_pairs(self, logits, out, row0, gN, gM, G, max_nm, mode):
        self._launch('mmmot_softmax_pairs', logits, out, row0, gN, gM, G, max_nm, mode)

    # ---- frame-pair association (include/mmmot_hip.h, csrc/assign.hip) ------------------------------------------
    def associate_pairs(self, det, new, end, link, pairs, B, max_nm, out, out_off, objective):
        """B frame pairs solved exactly in one launch; see mmmot_associate_pairs.  pairs / out_off: int32 device tensors."""
        self._launch('mmmot_associate_pairs', det, new, end, link, pairs, B, max_nm, out, out_off, objective)

    def associate_chains(self, det, new, end, link, chains, B, max_n, max_L, out, out_off, objective):
        """B chains of 2 .. 8 frames solved exactly in one launch; see mmmot_associate_chains.  chains / out_off: int32
        device tensors."""
        self._launch('mmmot_associate_chains', det, new, end, link, chains, B, max_n, max_L, out, out_off, objective)

    def associate_sequences(self, det, new, end, link, seqs, nts, B, max_T, max_n, max_L, out, ids, objective, info, ws):
        """B whole sequences solved exactly in one launch; see mmmot_associate_sequences.  seqs / nts / ids / info: int32
        device tensors; ws: the fp64 workspace."""
        self._associate_sequences('mmmot_associate_sequences', (), det, new, end, link, seqs, nts, B, max_T, max_n, max_L,
                                  out, ids, objective, info, ws)

    def associate_sequences_gap(self, det, new, end, link, seqs, nts, B, max_T, max_n, max_L, max_gap, out, ids, objective,
                                info, ws):
        """B whole sequences with skip links of up to ``max_gap`` frames solved exactly in one launch; see
        mmmot_associate_sequences_gap.  seqs / nts / ids / info: int32 device tensors; ws: the fp64 workspace."""
        self._associate_sequences('mmmot_associate_sequences_gap', (max_gap,), det, new, end, link, seqs, nts, B,
                                  max_T, max_n, max_L, out, ids, objective, info, ws)

    def _associate_sequences(self, name, gap, det, new, end, link, seqs, nts, B, max_T, max_n, max_L, out, ids, objective,
                             info, ws):
        """the two entries' one argument list; ``gap``: () or (max_gap,), which the gap entry takes after max_L"""
        self._launch(name, det, new, end, link, seqs, nts, B, nts.numel(), max_T, max_n, max_L, *gap,
                     min(det.numel(), new.numel(), end.numel()), link.numel(), out, out.numel(), ids, objective, info, ws,
                     ws.numel())

    def track_ids(self, blocks, pairs, out_off, frame_idx, B, max_nm, state, ids_out):
        """Track IDs of B consecutive pairs of one sequence from their solver blocks; see mmmot_track_ids.  pairs /
        out_off / frame_idx / state / ids_out: int32 device tensors; state is updated in place."""
        self._launch('mmmot_track_ids', blocks, pairs, out_off, frame_idx, B, max_nm, state, ids_out)

    def track_chain_ids(self, blocks, chains, out_off, frame_idx, B, max_n, state, ids_out):
        """Track IDs of B consecutive windows (2 .. 8 frames) of one sequence from their solver blocks; see
        mmmot_track_chain_ids.  chains / out_off / frame_idx / state / ids_out: int32 device tensors; state is updated in
        place."""
        self._launch('mmmot_track_chain_ids', blocks, chains, out_off, frame_idx, B, max_n, state, ids_out)

    def track_ids_multi(self, blocks, table, out_off, frame_idx, seq_start, S, B, max_n, states, ids_out, chains=False):
        """The ID step of S sequences in one launch; see mmmot_track_ids_multi / mmmot_track_chain_ids_multi
        (``chains``).  seq_start [S + 1] and the state table [S, TRACK_STATE_INTS] are int32 device tensors."""
        self._launch('mmmot_track_chain_ids_multi' if chains else 'mmmot_track_ids_multi', blocks, table, out_off,
                     frame_idx, seq_start, S, B, max_n, states, ids_out)

    def clear_mot(self, boxes, nG, nT, nD, frames, NF, g_attr, t_attr, traj_off, traj_obj, NTr, seq_off, S, params,
                  frame_d, frame_i, gt_out, traj_i, seq_d, seq_i):
        """CLEAR-MOT evaluation of S sequences in four launches; see mmmot_clear_mot.  boxes / frame_d / seq_d: fp64
        device tensors, the rest int32; params: (min_overlap, min_height, max_truncation, max_occlusion)."""
        self._launch('mmmot_clear_mot', boxes, nG, nT, nD, frames, NF, g_attr, t_attr, traj_off, traj_obj, NTr, seq_off, S,
                     params[0], params[1], params[2], params[3], frame_d, frame_i, gt_out, traj_i, seq_d, seq_i)

    def hota(self, boxes, nG, nT, nD, frames, NF, frame_seq, g_attr, t_id, seq_tab, S, cells, sumG, sumT, max_boxes,
             max_dontcare, params, prepare, work, frame_d, frame_i, seq_d, seq_i):
        """HOTA / IDF1 evaluation of S sequences in a fixed number of launches; see mmmot_hota.  boxes / frame_d /
        seq_d: fp64 device tensors, work: an int32 device tensor (8-byte aligned), the rest int32; params: (min_height,
        max_truncation, max_occlusion)."""
        self._launch('mmmot_hota', boxes, nG, nT, nD, frames, NF, frame_seq, g_attr, t_id, seq_tab, S, cells, sumG, sumT,
                     max_boxes, max_dontcare, params[0], params[1], params[2], prepare, _iptr(work), 4 * work.numel(),
                     frame_d, frame_i, seq_d, seq_i)

    def mot3d(self, boxes, box3d, sigma, nG, nT, nD, frames, cell_off, NF, g_attr, t_attr, traj_off, traj_obj, NTr,
              seq_off, S, mode, levels, phase, params, table, cells, msig, frame_d, frame_i, gt_out, traj_i, seq_d, seq_i,
              thr, reach):
        """One phase of the 3D MOT evaluation of S sequences; see mmmot_mot3d.  boxes / box3d / sigma / table / msig /
        frame_d / seq_d / thr: fp64 device tensors, the rest int32; params: (gate, min_height, max_truncation,
        max_occlusion)."""
        self._launch('mmmot_mot3d', boxes, box3d, sigma, nG, nT, nD, frames, cell_off, NF, g_attr, t_attr, traj_off,
                     traj_obj, NTr, seq_off, S, mode, levels, phase, params[0], params[1], params[2], params[3], table,
                     cells, msig, frame_d, frame_i, gt_out, traj_i, seq_d, seq_i, thr, reach)

    def generate_gt(self, ids, cls, chains, B, max_n, max_L, out, out_off):
        """Training targets of B chains in one launch; see mmmot_generate_gt.  ids / cls / chains / out_off: int32 device
        tensors; out: fp32."""
        self._launch('mmmot_generate_gt', ids, cls, chains, B, max_n, max_L, out, out_off)

    def match_dets(self, det_xywh, gt_xywh, gt_id, gt_name, frames, NF, car_code, dontcare_code, max_iou, max_n, det_id,
                   det_cls):
        """Ground-truth id and class of the detections of NF frames in one launch; see mmmot_match_dets.  det_xywh /
        gt_xywh: fp64 device tensors, the rest int32."""
        self._launch('mmmot_match_dets', det_xywh, gt_xywh, gt_id, gt_name, frames, NF, car_code, dontcare_code, max_iou,
                     max_n, det_id, det_cls)

    def fill_tracks(self, det, ids, frame_start, frame_no, seq_start, xf, wtab, L, F, S, max_fill, capacity, work,
                    fill_start, out, out_id, out_src, info):
        """Gap filling of S tracked sequences in five launches; see mmmot_fill_tracks.  det / out: fp32 device tensors,
        xf (or None: a standing camera) / wtab: fp64, the rest int32.  Returns the entry's status instead of raising, so
        that a caller can tell a refused call (MMMOT_EINVAL) from its results."""
        return self._status('mmmot_fill_tracks', det, ids, frame_start, frame_no, seq_start, xf, wtab, L, F, S, max_fill,
                            capacity, work, fill_start, out, out_id, out_src, info)

    def smooth_tracks(self, det, ids, frame_start, frame_no, seq_start, observed, xf0, L, F, S, params, yaw_flip, work,
                      out, out_vel, info):
        """Kalman / RTS smoothing of S tracked sequences in five launches; see mmmot_smooth_tracks.  det / out / out_vel
        (or None): fp32 device tensors, xf0 (or None: a standing camera): fp64, observed (or None) and the rest int32;
        ``params`` = (q_loc, r_loc, v0_loc, q_yaw, r_yaw, v0_yaw, q_dim, r_dim).  Returns the entry's status instead of
        raising, like ``fill_tracks``; the stream is passed as for ``gate_links``."""
        return self._status('mmmot_smooth_tracks', det, ids, frame_start, frame_no, seq_start, observed, xf0, L, F, S,
                            *params, yaw_flip, work, out, out_vel, info, self._stream())

    def stitch_tracks(self, det, ids, frame_start, frame_no, seq_start, vel, xf0, k_start, pairs, r2, inv_r2, L, F, S,
                      n_tracks, n_link, max_k, min_dt, max_dt, min_rows, mode, max_size_ratio, gap_penalty, work, out_ids,
                      nxt, links, objective, info):
        """Tracklet stitching of S tracked sequences in seven launches and the pair solver's; see mmmot_stitch_tracks.
        det / vel (or None) / links: fp32 device tensors, xf0 (or None: a standing camera) / r2 / inv_r2 / objective:
        fp64, the rest int32.  Returns the entry's status instead of raising, like ``fill_tracks``; the stream is passed
        as for ``gate_links``."""
        return self._status('mmmot_stitch_tracks', det, ids, frame_start, frame_no, seq_start, vel, xf0, k_start, pairs,
                            r2, inv_r2, L, F, S, n_tracks, n_link, max_k, min_dt, max_dt, min_rows, mode, max_size_ratio,
                            gap_penalty, work, out_ids, nxt, links, objective, info, self._stream())

    def gate_links(self, det, frame_start, frame_no, blocks, xf, r2, inv_r2, link, out_link, kept, L, F, NB, rec_gaps,
                   n_link, mode, max_dt, max_size_ratio, weight):
        """The motion gate over NB link blocks in one launch; see mmmot_gate_links.  det / link / out_link: fp32 device
        tensors (link = out_link = None: count only; out_link may be link), xf (or None) / r2 / inv_r2: fp64, the rest
        int32.  Returns the entry's status instead of raising, like ``fill_tracks``.  The entry takes its stream as an
        ordinary argument (``hip_stream``), so it is passed here."""
        return self._status('mmmot_gate_links', det, frame_start, frame_no, blocks, xf, r2, inv_r2, link, out_link, kept,
                            L, F, NB, rec_gaps, n_link, mode, max_dt, max_size_ratio, weight, self._stream())

    def adam_step(self, chunks, ptrs, scal, beta1, beta2, eps):
        """One Adam step of T tensors in one launch; see mmmot_adam_step and mmmot::adam_step (torch_ops.py).  chunks: the
        device int32 [n, 2] chunk table; ptrs / scal: the step's HOST tables, int64 [T, 6] (p, g, m, v, numel, flags) and
        float64 [T, 4] (step_size, bc2_sqrt, decay, l2), packed into mmmot_adam_row rows and uploaded here."""
        from . import torch_ops
        T = torch_ops.adam_tables(chunks, ptrs, scal, beta1, beta2, eps)
        self.adam_step_table(torch_ops.adam_pack(ptrs, scal, chunks.device), T, chunks, int(chunks.shape[0]), beta1, beta2,
                             eps)

    def adam_step_table(self, table, T, chunks, n_chunks, beta1, beta2, eps):
        """The launch alone, on a packed table: the device uint8 block of T 64-byte mmmot_adam_row rows."""
        self._launch('mmmot_adam_step', table, T, chunks, n_chunks, beta1, beta2, eps)

    # ---- training backward of the pairwise block (include/mmmot_hip.h, csrc/backward.hip) -------------------
    def gn_bwd_partial(self, dA, Y, C, sc1, sh1, gamma, beta, relu, tiles, P):
        self._launch('mmmot_gn_bwd_partial', dA, _ld(dA), Y, _ld(Y), C, sc1, sh1, _ld(sc1), gamma, beta, relu, tiles.row0,
                     tiles.nrows, tiles.group, tiles.T, P)

    def gn_bwd_finalize(self, S, tiles, C, NG, gamma, M):
        self._launch('mmmot_gn_bwd_finalize', S, tiles.g_count, tiles.G, C, NG, gamma, M)

    def gn_bwd_apply(self, dA, Y, C, sc1, sh1, gamma, beta, relu, M, tiles, dY):
        self._launch('mmmot_gn_bwd_apply', dA, _ld(dA), Y, _ld(Y), C, sc1, sh1, _ld(sc1), gamma, beta, relu, M, tiles.row0,
                     tiles.nrows, tiles.group, tiles.T, dY, _ld(dY))

    def gemm_tn(self, dY, tiles, N, K, dW, db=None, X=None, sc=None, sh=None, FA=None, FB=None, pair=None,
                amode=A_PLAIN, pairop=0, nsplit=1):
        """dW [nsplit][N][K] / db [nsplit][N]: per-share partial sums when nsplit > 1 (see mmmot_gemm_tn).  `tiles` of at
        most 128 rows: mmmot_gemm_tn_f16 stages 128 rows of a tile and would drop the rest (the fp32 kernel would not, but
        one contract for both arithmetics)."""
        if tiles.T and int(tiles.h_nrows.max()) > 128:
            raise ValueError('gemm_tn needs tiles of at most 128 rows, got %d' % int(tiles.h_nrows.max()))
        a = _lib.GemmTnArgs()
        a.nsplit = int(nsplit)
        a.dY, a.lddy = _ptr(dY), _ld(dY)
        a.X, a.ldx = _ptr(X), _ld(X)
        a.sc, a.sh, a.ldsc = _ptr(sc), _ptr(sh), _ld(sc)
        a.FA, a.FB, a.ldf = _ptr(FA), _ptr(FB), _ld(FA)
        a.tile_row0, a.tile_nrows, a.tile_group = _iptr(tiles.row0), _iptr(tiles.nrows), _iptr(tiles.group)
        if pair is not None:
            a.grp_row0, a.grp_M = _iptr(pair['row0']), _iptr(pair['M'])
            a.grp_aoff, a.grp_boff = _iptr(pair['aoff']), _iptr(pair['boff'])
        a.T, a.N, a.K, a.amode, a.pairop = tiles.T, N, K, amode, pairop
        a.dW, a.db = _ptr(dW), _ptr(db)
        if self.tn_f16:
            # fp16 matrix cores (3-term split), dY scaled by a power of two taken from its maximum on the device
            # one scalar per (device, stream): two backward passes issued on different streams through one HipOps
            # must not land their maxima in each other's scale
            amax = self._scratch(('tn_amax', int(self._stream() or 0)), 1, dY.device)
            self._launch('mmmot_absmax', dY, _ld(dY), tiles.R, N, amax)
            self._launch('mmmot_gemm_tn_f16', ctypes.byref(a), amax)
            return
        self._launch('mmmot_gemm_tn', ctypes.byref(a))

    def pair_bwd(self, dX, F, dF, C, row0, gN, gM, aoff, boff, blk_group, blk_idx, pairop, side):
        self._launch('mmmot_pair_bwd', dX, _ld(dX), F, _ld(F), dF, _ld(dF), C, row0, gN, gM, aoff, boff, blk_group,
                     blk_idx, blk_group.numel(), pairop, side)

    def pair_expand_bwd(self, dV, dA, C, tiles, row0, gN, gM, vrow0):
        self._launch('mmmot_pair_expand_bwd', dV, _ld(dV), dA, _ld(dA), C, tiles.row0, tiles.nrows, tiles.group, tiles.T,
                     row0, gN, gM, vrow0)

    def segment_argmax(self, X, C, segs, idx, sc=None, sh=None, relu=False, use_group=True):
        """idx int32 [segs.n][>= C] <- the first row (0 .. count - 1) of every segment that attains the maximum
        segment_mean(take_max=True) writes for the same arguments"""
        self._launch('mmmot_segment_argmax', X, _ld(X), C, segs.start, segs.count, segs.stride,
                     segs.group if use_group else None, segs.n, sc, sh, _ld(sc), bool(relu), idx, _ld(idx))

    def pair_expand_max_bwd(self, dV, idx, dA, C, tiles, row0, gN, gM, vrow0):
        self._launch('mmmot_pair_expand_max_bwd', dV, _ld(dV), idx, _ld(idx), dA, _ld(dA), C, tiles.row0, tiles.nrows,
                     tiles.group, tiles.T, row0, gN, gM, vrow0)

    def rowdot_bwd(self, X, K, w, b, sc, sh, tiles, act, gout, gidx, dA, PW):
        self._launch('mmmot_rowdot_bwd', X, _ld(X), K, w, b, sc, sh, _ld(sc), tiles.row0, tiles.nrows, tiles.group,
                     tiles.T, act, gout, gidx, dA, _ld(dA), PW, _ld(PW))

    def softmax_pairs_bwd(self, logits, dout, dlogits, row0, gN, gM, G, max_nm, mode):
        self._launch('mmmot_softmax_pairs_bwd', logits, dout, dlogits, row0, gN, gM, G, max_nm, mode)

    def fusion_c_bwd(self, dFu, Y0, Y1, sc0, sh0, sc1, sh1, tiles, DY0, DY1, DN0, DN1, C):
        self._launch('mmmot_fusion_c_bwd', dFu, Y0, _ld(Y0), Y1, _ld(Y1), sc0, sh0, sc1, sh1, _ld(sc0), tiles.row0,
                     tiles.nrows, tiles.group, tiles.T, DY0, DY1, _ld(DY0), DN0, DN1, C)

    def add_rows(self, A, B, Y, C):
        self._launch('mmmot_add_rows', A, _ld(A), B, _ld(B), Y, _ld(Y), A.shape[0], C)

    # ---- training step, second slice (csrc/train.hip) ----------------------------------------------------------
    def rows_gather_scale(self, S, rowidx, scale, X, C):
        """X[r][:C] = S[rowidx[r]][:C] * scale[rowidx[r]] (scale None: 1): backward of the per-detection average pools"""
        self._launch('mmmot_rows_gather_scale', S, _ld(S), rowidx, scale, X, _ld(X), X.shape[0], C)

    # ---- dropout of the LiDAR encoder (csrc/dropout.hip): keep(r, c) = philox(seed; r, c >> 2)[c & 3] >= threshold ----
    def segment_mean_dropout(self, X, C, segs, out, sc, sh, seed, threshold, scale, use_group=True):
        """segment_mean(relu=True) over the dropped rows: mean_t keep(r, c) * scale * relu(X[r][c] * sc + sh)"""
        self._launch('mmmot_segment_mean_dropout', X, _ld(X), C, segs.start, segs.count,
                     segs.group if use_group else None, segs.n, sc, sh, _ld(sc), seed, threshold, scale, out, _ld(out))

    def rows_gather_scale_dropout(self, S, rowidx, scale, X, C, seed, threshold, dscale):
        """rows_gather_scale times the mask: X[r][:C] = keep(r, c) * dscale * (S[rowidx[r]][:C] * scale[rowidx[r]])"""
        self._launch('mmmot_rows_gather_scale_dropout', S, _ld(S), rowidx, scale, X, _ld(X), X.shape[0], C, seed,
                     threshold, dscale)

    def dropout_mask(self, seed, threshold, out):
        """out uint8 [R][C] contiguous <- keep(r, c): the mask exactly as the two kernels above see it"""
        if out.dim() != 2 or not out.is_contiguous():
            raise ValueError('dropout_mask writes a contiguous [R][C] uint8 tensor')
        self._launch('mmmot_dropout_mask', seed, threshold, out.shape[0], out.shape[1], out)

    def pointnet_layer1_bwd(self, dY, X, tiles, PW):
        """PW [T][64 * (K + 1)] per-tile partials of (dW1 [64][K] | db1 [64]) interleaved per channel; K = X.shape[1]"""
        self._launch('mmmot_pointnet_layer1_bwd', dY, X, X.shape[1], tiles.row0, tiles.nrows, tiles.T, PW)

    def score_loss(self, x, y, kind, scale, g, PL, mrow=None, mcol=None, M=0, mask_mode=0, ignore=-1.0, accumulate=False):
        """one TrackingLoss term over x [R][C] (see mmmot_score_loss); PL [nblocks] partial sums of the scaled loss
        (accumulate: added to PL's contents)"""
        R, C = x.shape
        self._launch('mmmot_score_loss', x, _ld(x), y, mrow, mcol, M, mask_mode, ignore, kind, scale, R, C, g, _ld(g), PL,
                     PL.numel(), bool(accumulate))

    # ---- training step, third slice: training-mode VGG trunk (csrc/train_vgg.hip, conv3x3.hip RAW) ----
    def ghm_loss(self, x, y, scale, g, PL, acc_sum, bins=30, momentum=0.75, ignore=-1.0, accumulate=False):
        """the 'ghm' DetLoss term (mmmot_ghm_loss): x, g [R][C]; y [C]; acc_sum float64 [bins] = the module's running state"""
        R, C = x.shape
        self._launch('mmmot_ghm_loss', x, _ld(x), y, ignore, scale, R, C, bins, momentum, acc_sum, g, _ld(g), PL,
                     accumulate)

    def conv3x3_raw(self, inp, wp, bias, out, L, H, W, Cin, Cout, first):
        self._launch('mmmot_conv3x3_raw', inp, wp, bias, out, L, H, W, Cin, Cout, first)

    def rows_stats(self, Y, C, tiles, part):
        self._launch('mmmot_rows_stats', Y, _ld(Y), C, tiles.row0, tiles.nrows, tiles.T, part)

    def bn_relu_pool(self, Z, C, sc, sh, L, H, W, pool, A):
        self._launch('mmmot_bn_relu_pool', Z, C, sc, sh, L, H, W, bool(pool), A)

    def maxpool_bwd(self, Z, C, sc, sh, dP, L, H, W, dA):
        self._launch('mmmot_maxpool_bwd', Z, C, sc, sh, dP, L, H, W, dA)

    def conv3x3_wgrad(self, dZ, A, L, H, W, Cin, Cout, nsplit, dW, amax=None):
        if self.tn_f16:
            # fp16 matrix cores (3-term split), dZ scaled by a power of two taken from its maximum on the device
            # (`amax`: that maximum when the caller has it already - the input-gradient convolution uses the same one)
            if amax is None:
                amax = self._scratch(('tn_amax', int(self._stream() or 0)), 1, dZ.device)
                self._launch('mmmot_absmax', dZ, Cout, L * H * W, Cout, amax)
            self._launch('mmmot_conv3x3_wgrad_f16', dZ, A, L, H, W, Cin, Cout, nsplit, dW, amax)
            return
        self._launch('mmmot_conv3x3_wgrad', dZ, A, L, H, W, Cin, Cout, nsplit, dW)

    def conv3x3_first_wgrad(self, dZ, X, L, H, W, PW):
        self._launch('mmmot_conv3x3_first_wgrad', dZ, X, L, H, W, PW, PW.shape[0])

    def selftest_mfma(self, A, B, C, K):
        self._launch('mmmot_selftest_mfma', A, B, C, K)
