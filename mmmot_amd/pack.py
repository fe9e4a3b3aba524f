"""Host-side weight packing for the HIP path (done once per load_state_dict).

Everything here is exact algebra on the reference's parameters, carried out in
fp64 and rounded once to fp32:

* eval-mode BatchNorm folded into the preceding conv
  (reference modules/vgg.py:74-76, modules/tracking_net.py:92-100);
* conv weights re-laid out for the implicit-GEMM kernel
  ([9][Cout][Cin] tap-major; first layer [Cout][32] with k = tap*3 + c);
* the two PointNet spatial transforms evaluated in closed form and folded into
  the adjacent 1x1 convs.  STN3d (modules/point_net.py:72-86) ends in
  GroupNorm(C, C) over a 1 x C tensor: every group holds ONE value, so the
  normalised value is 0 and the output is the affine bias; hence
  ``trans = output(relu(fc_bn2.bias)) + I`` independent of the points
  (torch >= 1.6 refuses that GroupNorm call outright);
* PointNet_v1.conv1 (1088 -> 512, point_net.py:26-28) split into its per-point
  64-channel part and its per-detection 1024-channel part;
* weight matrices that consume the same input stacked along N
  (fusion C gates + inputs, new_end.conv0 + w_link.conv1.0).
"""
import torch


def _d(t):
    return t.detach().to('cpu', torch.float64)


def fold_bn(w, b, bn_w, bn_b, mean, var, eps=1e-5):
    s = _d(bn_w) / torch.sqrt(_d(var) + eps)
    wf = _d(w) * s.reshape(-1, *([1] * (w.dim() - 1)))
    bf = (_d(b) - _d(mean)) * s + _d(bn_b)
    return wf, bf


def to_hl16(x):
    """[..., C] real tensor -> fp32-typed tensor of the same shape whose BYTES are the hl16 split-half
    format of include/mmmot_hip.h: per 8 channels [8 x fp16 hi | 8 x fp16 lo], hi = fp16(x),
    lo = fp16(x - hi) (computed in fp64, so hi + lo carries 22 significand bits of x)."""
    x = x.detach().to('cpu', torch.float64)
    C = x.shape[-1]
    assert C % 8 == 0
    hi = x.to(torch.float16)
    lo = (x - hi.to(torch.float64)).to(torch.float16)
    lead = x.shape[:-1]
    u = torch.stack([hi.reshape(*lead, C // 8, 8), lo.reshape(*lead, C // 8, 8)], dim=-2).contiguous()
    return u.view(torch.float32).reshape(*lead, C)


def from_hl16(y):
    """Inverse of to_hl16 (fp32-typed hl16 buffer [..., C] -> fp32 values)."""
    C = y.shape[-1]
    u = y.contiguous().view(torch.float16).reshape(*y.shape[:-1], C // 8, 2, 8).to(torch.float32)
    return (u[..., 0, :] + u[..., 1, :]).reshape(*y.shape[:-1], C)


def _e4m3(x):
    """fp64 -> OCP FP8 E4M3 (saturating at +-448), returned as uint8 codes"""
    return x.clamp(-448.0, 448.0).to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)


def _hq8_records(hi, p4, p6):
    """hi fp16 [..., C], p4 / p6 uint8 e4m3 codes [..., C] -> fp32-typed [..., C] whose bytes are the hq8 records
    of include/mmmot_hip.h: per 32 channels [32 x fp16 | 32 x e4m3 (p4) | 32 x e4m3 (p6)]"""
    lead, C = hi.shape[:-1], hi.shape[-1]
    assert C % 32 == 0
    rec = torch.cat([hi.contiguous().view(torch.uint8).reshape(*lead, C // 32, 64), p4.reshape(*lead, C // 32, 32),
                     p6.reshape(*lead, C // 32, 32)], dim=-1).contiguous()
    return rec.view(torch.float32).reshape(*lead, C)


def to_hq8_act(x):
    """[..., C] activations -> hq8 records [fp16 hi | e4m3(x / 4) | e4m3((x - hi) * 512)] (C % 32 == 0)."""
    x = x.detach().to('cpu', torch.float64).clamp(-65000.0, 65000.0)
    hi = x.to(torch.float16)
    return _hq8_records(hi, _e4m3(x * 0.25), _e4m3((x - hi.to(torch.float64)) * 512.0))


def to_hq8_w(w):
    """[..., Cin] weights ALREADY scaled by 2^shift (hl16_weight_shift) -> hq8 weight records
    [fp16 hi | e4m3((w - hi) * 32) | e4m3(hi / 64)]."""
    w = w.detach().to('cpu', torch.float64)
    hi = w.to(torch.float16)
    return _hq8_records(hi, _e4m3((w - hi.to(torch.float64)) * 32.0), _e4m3(hi.to(torch.float64) / 64.0))


def hq8_parts(y):
    """hq8 records (fp32-typed [..., C]) -> (hi, p4, p6) decoded to fp64 [..., C] (no scaling applied)"""
    C = y.shape[-1]
    rec = y.detach().cpu().contiguous().view(torch.uint8).reshape(*y.shape[:-1], C // 32, 128)
    hi = rec[..., :64].contiguous().view(torch.float16).to(torch.float64).reshape(*y.shape[:-1], C)
    p4 = rec[..., 64:96].contiguous().view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64)
    p6 = rec[..., 96:128].contiguous().view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64)
    return hi, p4.reshape(*y.shape[:-1], C), p6.reshape(*y.shape[:-1], C)


def from_hq8_act(y):
    """value a consumer of an hq8 activation tensor sees outside the convolutions: hi + e4m3 lo * 2^-9 (fp32)"""
    hi, _, p6 = hq8_parts(y)
    return (hi + p6 / 512.0).to(torch.float32)


def hl16_weight_shift(w):
    """Power-of-two pre-scale that puts max|w| near 2^14 so the lo halves stay in fp16's normal range."""
    import math
    m = float(w.abs().max())
    return 0 if m == 0.0 else max(-14, min(24, int(math.floor(math.log2(16384.0 / m)))))


def conv1_weight_shift(wp, bias):
    """Pre-scale of the fused first layer's [Cout][32] weights: the folded bias rides in the k = 27 slot of the same fp16
    hi/lo records (csrc/conv3x3_hl16_patch.hip, FUSE1), so |bias| * 2^shift has to stay inside fp16 as well."""
    import math
    shift = hl16_weight_shift(wp)
    mb = float(bias.abs().max())
    if mb > 0.0:
        shift = min(shift, int(math.floor(math.log2(32768.0 / mb))))
    return max(-14, shift)


def hl16_channel_shifts(wp):
    """Per-OUTPUT-channel power-of-two pre-scales of a trunk weight [9][Cout][Cin] (fp64): channel n is scaled so that
    max|w[:, n, :]| lands in (2^13, 2^14].  A trained, BatchNorm-folded VGG layer has per-channel gains
    gamma / sqrt(var + eps) spread over orders of magnitude; with ONE scale per layer the e4m3 copies of a low-gain
    channel (hq8: e4m3(32 w_lo) underflows below 2^-9, e4m3(w_hi / 64) loses its 3 mantissa bits below 2^-6) would
    silently drop that channel's correction terms.  Returns an int64 tensor [Cout]."""
    import math
    m = wp.abs().amax(dim=(0, 2))
    return torch.tensor([0 if float(v) == 0.0 else max(-14, min(40, int(math.floor(math.log2(16384.0 / float(v))))))
                         for v in m], dtype=torch.int64)


def _add_hl16_copies(P, device):
    """For every row-GEMM weight ([N][K] fp32, K % 64 == 0) add ``<name>_h16`` (hl16 split-half copy
    scaled by 2^shift) and ``<name>_os`` (= 2^-shift) so the engine can run the GEMM on the fp16
    matrix cores (mmmot_gemm_args.w_hl16)."""
    def visit(d):
        for k in list(d.keys()):
            v = d[k]
            if torch.is_tensor(v) and v.dim() == 2 and v.dtype == torch.float32 and v.shape[1] % 64 == 0 \
                    and v.shape[0] % 64 == 0 and not k.startswith('trans'):
                shift = hl16_weight_shift(v)
                d[k + '_h16'] = to_hl16(v.detach().cpu().double() * (2.0 ** shift)).contiguous().to(device)
                d[k + '_os'] = 2.0 ** (-shift)
    for key in ('pointnet', 'fusion', 'w_det', 'w_link'):
        if key in P:
            visit(P[key])
    for hd in P.get('skippool', []):
        visit(hd)


def stn_transform(sd, prefix, k):
    """Closed-form STN3d output (k x k), fp64."""
    beta2 = _d(sd[prefix + 'fc_bn2.bias'])
    out = _d(sd[prefix + 'output.weight']) @ torch.relu(beta2) + _d(sd[prefix + 'output.bias'])
    return out.reshape(k, k) + _d(sd[prefix + 'idt'])


# (sequential index of each conv inside its stage, pool-after flag), per stage;
# mirrors how appear_net.py:130-157 regroups vgg16_bn.features (the first
# max-pool does not close a stage).
VGG_STAGES = [
    [(0, 3, 64, False), (3, 64, 64, True), (7, 64, 128, False), (10, 128, 128, True)],
    [(0, 128, 256, False), (3, 256, 256, False), (6, 256, 256, True)],
    [(0, 256, 512, False), (3, 512, 512, False), (6, 512, 512, True)],
    [(0, 512, 512, False), (3, 512, 512, False), (6, 512, 512, True)],
]


# ---- the head's packed layout: P['fusion'] (modes A / B / C) and P['w_link'] ----
# packed key -> (how, reference-keyed sources ...):
#   'mat'   every source flattened to [N][K], concatenated along 0 (weights that consume the same input, stacked along N);
#   'vec'   every source reshaped to a vector, concatenated along 0; a number stands for a constant vector as long as the
#           source behind it (fusion C: the gate rows pass the GroupNorm of the input rows with gain one, shift zero);
#   'float' the python float of a one-element tensor (the rowdot kernels take their output bias by value).
def _conv_norm(w, b, g, be, conv, norm):
    return {w: ('mat', conv + '.weight'), b: ('vec', conv + '.bias'),
            g: ('vec', norm + '.weight'), be: ('vec', norm + '.bias')}


def _gated(j, gate, inp):
    gate, inp = 'fusion_module.%s.' % gate, 'fusion_module.%s.' % inp
    return {'w%d' % j: ('mat', gate + '0.weight', inp + '0.weight'), 'b%d' % j: ('vec', gate + '0.bias', inp + '0.bias'),
            'g%d' % j: ('vec', 1.0, inp + '1.weight'), 'be%d' % j: ('vec', 0.0, inp + '1.bias')}


_FM, _WL, _NE = 'fusion_module.', 'w_link.conv1.', 'w_link.w_new_end.'
FUSION_LAYOUT = {
    'A': _conv_norm('w0', 'b0', 'g0', 'be0', _FM + 'input_w.0', _FM + 'input_w.1'),           # w0 [512][1024]
    # NB reference naming trap: *_p is applied to feats[:1] = IMAGE
    'B': {**_conv_norm('w0', 'b0', 'g0', 'be0', _FM + 'input_p.0', _FM + 'input_p.1'),
          **_conv_norm('w1', 'b1', 'g1', 'be1', _FM + 'input_i.0', _FM + 'input_i.1')},
    'C': {**_gated(0, 'gate_p', 'input_p'), **_gated(1, 'gate_i', 'input_i')},                # w0, w1 [1024][512]
}
LINK_LAYOUT = {
    'wa': ('mat', _NE + 'conv0.0.weight', _WL + '0.weight'),                                   # [1024][512]
    'ba': ('vec', _NE + 'conv0.0.bias', _WL + '0.bias'),
    'g_ne0': ('vec', _NE + 'conv0.1.weight'), 'be_ne0': ('vec', _NE + 'conv0.1.bias'),
    'g1': ('vec', _WL + '1.weight'), 'be1': ('vec', _WL + '1.bias'),
    **_conv_norm('w3', 'b3', 'g4', 'be4', _WL + '3', _WL + '4'),
    **_conv_norm('w6', 'b6', 'g7', 'be7', _WL + '6', _WL + '7'),
    'w9': ('vec', _WL + '9.weight'), 'b9': ('float', _WL + '9.bias'),
    **_conv_norm('nw0', 'nb0', 'ng1', 'nbe1', _NE + 'conv1.0', _NE + 'conv1.1'),
    **_conv_norm('nw3', 'nb3', 'ng4', 'nbe4', _NE + 'conv1.3', _NE + 'conv1.4'),
    'nw6': ('vec', _NE + 'conv1.6.weight'), 'nb6': ('float', _NE + 'conv1.6.bias'),
}


def build_head(layout, get):
    """The entries of a head layout from ``get(reference key) -> tensor``, in the tensors' own dtype and on their own
    device: pack_weights hands in fp64 host copies, TrackingNet.refresh_head_device the live fp32 parameters."""
    out = {}
    for k, (how, *src) in layout.items():
        if how == 'float':
            out[k] = float(get(src[0]).item())
            continue
        ts = [s if isinstance(s, float) else get(s).flatten(1) if how == 'mat' else get(s).reshape(-1) for s in src]
        ts = [torch.full_like(ts[i + 1], t) if isinstance(t, float) else t for i, t in enumerate(ts)]
        out[k] = ts[0] if len(ts) == 1 else torch.cat(ts, 0)
    return out


def pack_weights(sd, fusion, device, eps=1e-5):
    """sd: reference-keyed state_dict (TrackingNet).  Returns dict of fp32 device tensors."""
    f32 = lambda t: t.to(torch.float32).contiguous().to(device)
    P = {}

    # ---- VGG trunk ---------------------------------------------------------
    if 'appearance.layers.0.0.weight' in sd:
        convs = []
        for s, stage in enumerate(VGG_STAGES):
            for (idx, cin, cout, pool) in stage:
                p = 'appearance.layers.%d.' % s
                w, b = fold_bn(sd[p + '%d.weight' % idx], sd[p + '%d.bias' % idx],
                               sd[p + '%d.weight' % (idx + 1)], sd[p + '%d.bias' % (idx + 1)],
                               sd[p + '%d.running_mean' % (idx + 1)], sd[p + '%d.running_var' % (idx + 1)], eps)
                if cin == 3:
                    # [Cout][3][3][3] (n,c,ky,kx) -> [Cout][k = (ky*3+kx)*3 + c], padded to 32
                    wk = w.permute(0, 2, 3, 1).reshape(cout, 27)
                    wp = torch.zeros(cout, 32, dtype=torch.float64)
                    wp[:, :27] = wk
                else:
                    # -> [tap = ky*3+kx][Cout][Cin]
                    wp = w.permute(2, 3, 0, 1).reshape(9, cout, cin)
                cv = dict(wp=f32(wp), bias=f32(b), cin=cin, cout=cout, pool=pool, stage=s,
                          last=(idx == stage[-1][0]))
                if cin == 3:
                    # fp16-split (hl16) copy of the first layer's [Cout][32] weights for the fused conv1_1+conv1_2
                    # kernel: one power-of-two scale for the layer (hl16 keeps 22 bits down to 2^-17 of the maximum)
                    # (the bias travels in the k = 27 slot of these records: conv1_weight_shift)
                    shift = conv1_weight_shift(wp, b)
                    cv['wp16'] = to_hl16(wp * (2.0 ** shift)).contiguous().to(device)
                    cv['oscale'] = 2.0 ** (-shift)
                else:
                    # hl16 ('f16x3') and hq8 ('f16q8') copies for the matrix-core trunk: every OUTPUT channel scaled
                    # by its own power of two (exact), undone by the [Cout] vector `oscale` in the epilogue
                    shifts = hl16_channel_shifts(wp)
                    ws = wp * torch.pow(2.0, shifts.to(torch.float64)).reshape(1, -1, 1)
                    cv['wp16'] = to_hl16(ws).contiguous().to(device)
                    cv['wpq8'] = to_hq8_w(ws).contiguous().to(device)
                    cv['oscale'] = f32(torch.pow(2.0, -shifts.to(torch.float64)))
                    cv['wshift'] = shifts
                convs.append(cv)
        P['vgg'] = convs
        heads = []
        for s in range(4):
            p = 'appearance.global_pool.%d.fc.' % s
            heads.append(dict(
                g0=f32(_d(sd[p + '0.weight'])), b0=f32(_d(sd[p + '0.bias'])),
                w1=f32(_d(sd[p + '1.weight']).flatten(1)), c1=f32(_d(sd[p + '1.bias'])),
                g2=f32(_d(sd[p + '2.weight'])), b2=f32(_d(sd[p + '2.bias'])),
                w4=f32(_d(sd[p + '4.weight']).flatten(1)), c4=f32(_d(sd[p + '4.bias'])),
                g5=f32(_d(sd[p + '5.weight'])), b5=f32(_d(sd[p + '5.bias'])),
            ))
        P['skippool'] = heads

    # ---- PointNet ----------------------------------------------------------
    if 'point_net.feat.conv1.weight' in sd:
        q = 'point_net.feat.'
        kin = int(sd[q + 'conv1.weight'].shape[1])  # 3 (xyz) or 4 (xyz + reflectivity, tracking_net.py:41)
        T1 = stn_transform(sd, q + 'stn1.', kin)
        T2 = stn_transform(sd, q + 'stn2.', 64)
        cw = lambda name: _d(sd[name]).flatten(1)
        pn = dict(trans1=f32(T1), trans2=f32(T2))
        pn['w1'] = f32(cw(q + 'conv1.weight') @ T1.t())          # [64][3 | 4]
        pn['b1'] = f32(_d(sd[q + 'conv1.bias']))
        pn['w2'] = f32(cw(q + 'conv2.weight') @ T2.t())          # [64][64] acts on relu(gn1(.))
        pn['b2'] = f32(_d(sd[q + 'conv2.bias']))
        for i in (3, 4, 5):
            pn['w%d' % i] = f32(cw(q + 'conv%d.weight' % i))
            pn['b%d' % i] = f32(_d(sd[q + 'conv%d.bias' % i]))
        for i in (1, 2, 3, 4, 5):
            pn['g%d' % i] = f32(_d(sd[q + 'bn%d.weight' % i]))
            pn['be%d' % i] = f32(_d(sd[q + 'bn%d.bias' % i]))
        wc1 = cw('point_net.conv1.weight')                        # [512][1088]
        pn['wc1a'] = f32(wc1[:, :64] @ T2.t())                    # per-point part (on relu(gn1(.)))
        pn['wc1b'] = f32(wc1[:, 64:])                             # per-detection part [512][1024]
        pn['bc1'] = f32(_d(sd['point_net.conv1.bias']))
        pn['gc1'] = f32(_d(sd['point_net.bn1.weight']))
        pn['bec1'] = f32(_d(sd['point_net.bn1.bias']))
        pn['wc2'] = f32(cw('point_net.conv2.weight'))
        pn['bc2'] = f32(_d(sd['point_net.conv2.bias']))
        pn['gc2'] = f32(_d(sd['point_net.bn2.weight']))
        pn['bec2'] = f32(_d(sd['point_net.bn2.bias']))
        P['pointnet'] = pn

    # ---- fusion, w_link: pure data movement, written down once (FUSION_LAYOUT / LINK_LAYOUT) ----
    def head(layout):
        """the entries of a head layout from `sd` in fp64, rounded once to fp32; none when sd lacks the module"""
        if not all(s in sd for _, *src in layout.values() for s in src if isinstance(s, str)):
            return {}
        return {k: f32(v) if torch.is_tensor(v) else v for k, v in build_head(layout, lambda key: _d(sd[key])).items()}

    P['fusion'] = dict(mode=fusion, **head(FUSION_LAYOUT.get(fusion, {})))
    lk = head(LINK_LAYOUT)
    if lk:
        P['w_link'] = lk

    # ---- w_det (BatchNorm1d folded) ---------------------------------------
    if 'w_det.0.weight' in sd:
        w0, b0 = fold_bn(sd['w_det.0.weight'], sd['w_det.0.bias'], sd['w_det.1.weight'], sd['w_det.1.bias'],
                         sd['w_det.1.running_mean'], sd['w_det.1.running_var'], eps)
        w3, b3 = fold_bn(sd['w_det.3.weight'], sd['w_det.3.bias'], sd['w_det.4.weight'], sd['w_det.4.bias'],
                         sd['w_det.4.running_mean'], sd['w_det.4.running_var'], eps)
        P['w_det'] = dict(w0=f32(w0.flatten(1)), b0=f32(b0), w3=f32(w3.flatten(1)), b3=f32(b3),
                          w6=f32(_d(sd['w_det.6.weight']).reshape(-1)), b6=float(sd['w_det.6.bias'].item()))

    _add_hl16_copies(P, device)
    return P
