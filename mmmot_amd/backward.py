"""Training step of the head: fusion module A / B / C, the negative-rejection head w_det in training mode and the
pairwise block, forward with a tape and backward.

The pairwise block is ``affinity_module.forward`` + ``NewEndIndicator_v2.forward`` + the softmax modes of
``TrackingNet.associate`` (reference modules/gcn.py:68-82, new_end.py:62-82, tracking_net.py:106-126); its gradients go
to the fused features F (3 x L x 512 in the reference, [nR*Lt][512] here) and to every ``w_link.*`` parameter - the part
of the training step ``tracking_model.py:50-66`` (forward -> loss -> backward) that runs over the N x M pair space.  In
training mode this block and the fusion module are identical to eval mode (GroupNorm only: no BatchNorm, and the network's
one dropout sits in the LiDAR encoder - ``use_dropout``, mmmot_amd/train.py - not here), so
their training forward IS ``Engine.affinity`` / ``Engine.fuse``, run under ``Engine.recording()``: the engine's own
schedule, with the pre-norm tensors kept on a tape under the engine's layer names.  w_det normalises with the batch
statistics in training mode, which is not the eval arithmetic: ``det_forward_train`` is a schedule of its own.

    link, new, end = affinity_autograd(model, plan, F)        # F requires grad / w_link parameters require grad
    det, link, new, end = head_autograd(model, plan, cat)     # cat [Lt][1024]: the encoders' features
    loss(...).backward()                                      # fills the inputs' .grad and the parameters' .grad

Everything numeric happens in libmmmot_hip.so (csrc/backward.hip + the forward kernels); torch does memory, views,
transposes of weights (data movement) and the autograd bookkeeping.  The encoders' training step is in train.py (PointNet,
the loss, the whole-network forward) and train_vgg.py (the image encoder); the layer primitives all three share in tape.py.
"""
import numpy as np
import torch

from .ops import ACT_NONE, ACT_SIGMOID, A_NORM_RELU, A_PAIR, A_PLAIN, PAIR_OPS, SOFTMAX_MODES
from .tape import colsum, dgrad_gemm, gn_backward, norm_layer, taped, weight_grad
from .tape import update_running_stats as momentum_update  # head_autograd has a flag of that name

# packed name -> reference state_dict key (w_link.*); 'wa' / 'ba' are the stacked [new_end.conv0 ; conv1.0] layer
PARAM_KEYS = {
    'g_ne0': 'w_link.w_new_end.conv0.1.weight', 'be_ne0': 'w_link.w_new_end.conv0.1.bias',
    'g1': 'w_link.conv1.1.weight', 'be1': 'w_link.conv1.1.bias',
    'w3': 'w_link.conv1.3.weight', 'b3': 'w_link.conv1.3.bias',
    'g4': 'w_link.conv1.4.weight', 'be4': 'w_link.conv1.4.bias',
    'w6': 'w_link.conv1.6.weight', 'b6': 'w_link.conv1.6.bias',
    'g7': 'w_link.conv1.7.weight', 'be7': 'w_link.conv1.7.bias',
    'w9': 'w_link.conv1.9.weight', 'b9': 'w_link.conv1.9.bias',
    'nw0': 'w_link.w_new_end.conv1.0.weight', 'nb0': 'w_link.w_new_end.conv1.0.bias',
    'ng1': 'w_link.w_new_end.conv1.1.weight', 'nbe1': 'w_link.w_new_end.conv1.1.bias',
    'nw3': 'w_link.w_new_end.conv1.3.weight', 'nb3': 'w_link.w_new_end.conv1.3.bias',
    'ng4': 'w_link.w_new_end.conv1.4.weight', 'nbe4': 'w_link.w_new_end.conv1.4.bias',
    'nw6': 'w_link.w_new_end.conv1.6.weight', 'nb6': 'w_link.w_new_end.conv1.6.bias',
}


class _PairAux:
    """Integer tables of the pairwise block's backward that the forward plan does not carry (built once per plan)."""

    def __init__(self, plan):
        dev = plan.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        gN, gM = plan.h_pg_N, plan.h_pg_M
        # V rows of group g: M "new" rows then N "end" rows (plan.v_tiles has two groups per pair group)
        self.vrow0 = up(np.concatenate([[0], np.cumsum(gN + gM)])[:-1])
        a_g, a_i, b_g, b_j = [], [], [], []
        for g, (n, m) in enumerate(zip(gN, gM)):
            a_g += [g] * int(n); a_i += list(range(int(n)))
            b_g += [g] * int(m); b_j += list(range(int(m)))
        self.a_grp, self.a_idx, self.b_grp, self.b_idx = up(a_g), up(a_i), up(b_g), up(b_j)


def _aux(plan):
    if not hasattr(plan, '_bwd_aux'):
        plan._bwd_aux = _PairAux(plan)
    return plan._bwd_aux


def affinity_forward_train(eng, plan, F):
    """Engine.affinity, recorded: the tape the backward needs.  F: [nR, Lt, 512] (contiguous).  Returns
    (link flat [R], new [nR, Lt], end [nR, Lt], tape)."""
    eng.dev = F.device
    with eng.recording() as tape:
        link, new, end = eng.affinity(plan, F)
    return link, new, end, tape


def affinity_backward(eng, plan, F, t, d_link, d_new, d_end):
    """Returns (dF [nR, Lt, 512], {reference state_dict key: gradient tensor in the parameter's shape})."""
    ops, lk, PT, VT = eng.ops, eng.P['w_link'], plan.pair_tiles, plan.v_tiles
    nR, Lt, R = plan.nR, plan.Lt, plan.pair_tiles.R
    dev = F.device
    aux = _aux(plan)
    Ff = F.reshape(nR * Lt, 512)
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    pairop = PAIR_OPS[eng.affinity_op]
    g = {}
    # ---- link branch, from the scores back to dYa[:, 512:] ----
    d_link = d_link.reshape(-1).contiguous()
    if eng.softmax_mode != 'none':
        dlogits = new(R)
        ops.softmax_pairs_bwd(t['aff_logits'], d_link, dlogits, PT.g_row0, plan.pg_N, plan.pg_M, PT.G, plan.max_nm,
                              SOFTMAX_MODES[eng.softmax_mode])
    else:
        dlogits = d_link
    L7, L4, L1, NE0, V1, V4 = t['aff_7'], t['aff_4'], t['aff_1'], t['aff_ne0'], t['aff_v1'], t['aff_v4']
    dA6, PW = new(R, 128), new(PT.T, 132)
    ops.rowdot_bwd(L7.Y, 128, lk['w9'], lk['b9'], L7.sc, L7.sh, PT, ACT_NONE, dlogits, None, dA6, PW)
    pw = colsum(eng, PW)
    g['w9'], g['b9'] = pw[:128], pw[128:129]
    dA3, g['w6'], g['b6'], g['g7'], g['be7'] = L7.backward(eng, plan, dA6, lk['w6'], X=L4.Y, sc=L4.sc, sh=L4.sh,
                                                           amode=A_NORM_RELU)
    dA1, g['w3'], g['b3'], g['g4'], g['be4'] = L4.backward(eng, plan, dA3, lk['w3'], X=L1.Y, sc=L1.sc, sh=L1.sh,
                                                           amode=A_NORM_RELU)
    dYa = new(R, 1024)
    _, g['g1'], g['be1'] = gn_backward(eng, plan, L1, dA1, out=dYa[:, 512:1024])
    # ---- new / end branch, from the scores back to dYa[:, :512] ----
    d_ne = torch.stack([d_new, d_end]).reshape(-1).contiguous()
    dAv1, PW = new(VT.R, 128), new(VT.T, 132)
    ops.rowdot_bwd(V4.Y, 128, lk['nw6'], lk['nb6'], V4.sc, V4.sh, VT, ACT_SIGMOID, d_ne, plan.v_omap, dAv1, PW)
    pw = colsum(eng, PW)
    g['nw6'], g['nb6'] = pw[:128], pw[128:129]
    dAv0, g['nw3'], g['nb3'], g['ng4'], g['nbe4'] = V4.backward(eng, plan, dAv1, lk['nw3'], X=V1.Y, sc=V1.sc, sh=V1.sh,
                                                                amode=A_NORM_RELU)
    dV, g['nw0'], g['nb0'], g['ng1'], g['nbe1'] = V1.backward(eng, plan, dAv0, lk['nw0'], X=t['aff_v'], amode=A_PLAIN)
    dAne = new(R, 512)
    if eng.end_mode == 'avg':
        ops.pair_expand_bwd(dV, dAne, 512, PT, PT.g_row0, plan.pg_N, plan.pg_M, aux.vrow0)
    else:
        # maxima (new_end.py:72-74): the forward keeps no indices - the first-maximum row of every (vector, channel) is
        # recomputed from the tape with Engine.affinity's own segment_mean arguments, then dV goes to that row alone
        idx = torch.empty(VT.R, 512, dtype=torch.int32, device=dev)
        ops.segment_argmax(NE0.Y, 512, plan.v_segs, idx, sc=NE0.sc, sh=NE0.sh, relu=True)
        ops.pair_expand_max_bwd(dV, idx, dAne, 512, PT, PT.g_row0, plan.pg_N, plan.pg_M, aux.vrow0)
    _, g['g_ne0'], g['be_ne0'] = gn_backward(eng, plan, NE0, dAne, out=dYa[:, 0:512])
    # ---- the stacked first layer over the pairwise tensor, and the pairwise operand generation ----
    pair = dict(row0=PT.g_row0, M=plan.pg_M, aoff=plan.pg_aoff, boff=plan.pg_boff)
    dWa, dba = weight_grad(eng, dYa, PT, 1024, 512, FA=Ff, FB=Ff, pair=pair, amode=A_PAIR, pairop=pairop)
    dX = new(R, 512)
    dgrad_gemm(eng, lk['wa'], PT, dYa, dX)
    dF = torch.zeros(nR * Lt, 512, dtype=torch.float32, device=dev)
    common = (PT.g_row0, plan.pg_N, plan.pg_M, plan.pg_aoff, plan.pg_boff)
    ops.pair_bwd(dX, Ff, dF, 512, *common, aux.a_grp, aux.a_idx, pairop, 0)
    ops.pair_bwd(dX, Ff, dF, 512, *common, aux.b_grp, aux.b_idx, pairop, 1)
    # ---- reference-keyed parameter gradients (flat / 2-D; the caller reshapes to the parameter's shape) ----
    out = {'w_link.w_new_end.conv0.0.weight': dWa[0:512], 'w_link.w_new_end.conv0.0.bias': dba[0:512],
           'w_link.conv1.0.weight': dWa[512:1024], 'w_link.conv1.0.bias': dba[512:1024]}
    for name, key in PARAM_KEYS.items():
        out[key] = g[name]
    return dF.view(nR, Lt, 512), out


# ======================================================================================================================
# The rest of the head - fusion module A / B / C and the negative-rejection head w_det in TRAINING mode
# (reference modules/fusion_net.py:31-42,62-70,85-92; tracking_net.py:91-100,149-163 with self.training: BatchNorm1d on
# batch statistics over the 3 modality rows x L detections, no sigmoid, no neg_threshold mask).  Together with the
# pairwise block this is everything between the encoder features `cat` [Lt][1024] and the four score tensors.
# ======================================================================================================================
def _t2(p):
    """conv weight [N, K, 1(, 1)] -> [N][K] fp32 view on the parameter's device"""
    return p.detach().reshape(p.shape[0], -1).contiguous()


def fusion_forward_train(eng, plan, cat):
    """Engine.fuse, recorded: cat [Lt][1024] -> (F [3][Lt][512], tape) (GroupNorm only: identical to eval)."""
    eng.dev = cat.device
    F = torch.empty(3, plan.Lt, 512, dtype=torch.float32, device=cat.device)
    with eng.recording() as tape:
        eng.fuse(plan, cat, F)
    return F, tape


def fusion_backward(eng, plan, cat, t, dF):
    """dF [3][Lt][512] -> (dcat [Lt][1024], {fusion_module.* key: grad}).  The weight gradients run as one share: the
    detections of a sample are a few tiles."""
    ops, fu, D, Lt = eng.ops, eng.P['fusion'], plan.det_tiles, plan.Lt
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=cat.device)
    fm = 'fusion_module.'
    out = {}
    dcat = new(Lt, 1024)
    if eng.fusion == 'A':
        (dconv, out[fm + 'input_w.0.weight'], out[fm + 'input_w.0.bias'], out[fm + 'input_w.1.weight'],
         out[fm + 'input_w.1.bias']) = t['fu0'].backward(eng, plan, dF[2], fu['w0'], shares=1, relu=False, X=cat,
                                                         amode=A_PLAIN)
        ops.add_rows(dconv[:, 0:512], dF[0], dcat[:, 0:512], 512)
        ops.add_rows(dconv[:, 512:1024], dF[1], dcat[:, 512:1024], 512)
        return dcat, out
    names = (('gate_p', 'input_p'), ('gate_i', 'input_i'))  # *_p acts on the IMAGE half (naming trap)
    Ls = (t['fu0'], t['fu1'])
    if eng.fusion == 'C':
        # the recorded layers span the stacked [gate ; input] GEMM; the GroupNorm acts on the `input` half, columns 512..
        # (per-channel normalisation: the statistics of those columns are those of a finalize over them alone)
        y0, y1 = Ls[0].Y, Ls[1].Y
        Ls = (Ls[0].columns(512), Ls[1].columns(512))
        DY = [new(Lt, 1024), new(Lt, 1024)]
        DN = [new(Lt, 512), new(Lt, 512)]
        ops.fusion_c_bwd(dF[2], y0, y1, Ls[0].sc, Ls[0].sh, Ls[1].sc, Ls[1].sh, D, DY[0], DY[1], DN[0], DN[1], 512)
    for j in range(2):
        x, inp = cat[:, 512 * j:512 * (j + 1)], fm + names[j][1]
        if eng.fusion == 'B':
            dconv, out[inp + '.0.weight'], out[inp + '.0.bias'], out[inp + '.1.weight'], out[inp + '.1.bias'] = \
                Ls[j].backward(eng, plan, dF[2], fu['w%d' % j], shares=1, relu=False, X=x, amode=A_PLAIN)
        else:  # C: the gates' gradient is in DY[j][:, :512] already, the GEMMs run over the stacked layer
            _, out[inp + '.1.weight'], out[inp + '.1.bias'] = gn_backward(eng, plan, Ls[j], DN[j], out=DY[j][:, 512:1024],
                                                                          relu=False)
            dW, db = weight_grad(eng, DY[j], D, 1024, 512, shares=1, X=x, amode=A_PLAIN)
            out[fm + names[j][0] + '.0.weight'], out[fm + names[j][0] + '.0.bias'] = dW[0:512], db[0:512]
            out[inp + '.0.weight'], out[inp + '.0.bias'] = dW[512:1024], db[512:1024]
            dconv = new(Lt, 512)
            dgrad_gemm(eng, fu['w%d' % j], D, DY[j], dconv)
        ops.add_rows(dconv, dF[j], dcat[:, 512 * j:512 * (j + 1)], 512)
    return dcat, out


def det_forward_train(eng, model, plan, F):
    """w_det in TRAINING mode (tracking_net.py:149-151 with self.training): conv -> BatchNorm1d on the batch statistics of
    the 3 x L positions -> ReLU, twice, then the 1-channel conv; raw scores (no sigmoid, no threshold mask).
    F [nR][Lt][512] -> det [nR][Lt].  One sample per call, like the reference (its batch is 1: the BatchNorm statistics
    are those of one sample)."""
    if plan.B != 1:
        raise NotImplementedError('training-mode w_det: one sample per call (BatchNorm statistics are per forward)')
    ops, T = eng.ops, plan.F_tiles
    R = plan.nR * plan.Lt
    dev = F.device
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    wd = model.w_det
    X = F.reshape(R, 512)
    t = {}
    h0, part = new(R, 512), new(T.T, 2, 512)
    ops.gemm(_t2(wd[0].weight), T, 512, 512, X=X, bias=wd[0].bias.detach(), Y=h0, part=part)
    t['d0'] = norm_layer(eng, part, T, h0, 512, 512, wd[1].weight.detach(), wd[1].bias.detach())
    h1, part = new(R, 256), new(T.T, 2, 256)
    ops.gemm(_t2(wd[3].weight), T, 256, 512, X=h0, bias=wd[3].bias.detach(), Y=h1, part=part, sc=t['d0'].sc,
             sh=t['d0'].sh, amode=A_NORM_RELU)
    t['d1'] = norm_layer(eng, part, T, h1, 256, 256, wd[4].weight.detach(), wd[4].bias.detach())
    det = new(plan.nR, plan.Lt)
    t['w6'], t['b6'] = wd[6].weight.detach().reshape(-1).contiguous(), float(wd[6].bias.item())
    ops.rowdot(h1, 256, t['w6'], t['b6'], T, det.view(-1), sc=t['d1'].sc, sh=t['d1'].sh, act=ACT_NONE)
    return det, t


def det_backward(eng, model, plan, F, t, d_det):
    """d_det [nR][Lt] -> (dF [nR][Lt][512], {w_det.* key: grad}); one-share weight gradients, like the fusion module's."""
    ops, T = eng.ops, plan.F_tiles
    R = plan.nR * plan.Lt
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=F.device)
    wd = model.w_det
    out = {}
    D0, D1 = t['d0'], t['d1']
    dA1, PW = new(R, 256), new(T.T, 260)
    ops.rowdot_bwd(D1.Y, 256, t['w6'], t['b6'], D1.sc, D1.sh, T, ACT_NONE, d_det.reshape(-1).contiguous(), None, dA1, PW)
    pw = colsum(eng, PW)
    out['w_det.6.weight'], out['w_det.6.bias'] = pw[:256], pw[256:257]
    dA0, out['w_det.3.weight'], out['w_det.3.bias'], out['w_det.4.weight'], out['w_det.4.bias'] = D1.backward(
        eng, plan, dA1, _t2(wd[3].weight), shares=1, X=D0.Y, sc=D0.sc, sh=D0.sh, amode=A_NORM_RELU)
    dF, out['w_det.0.weight'], out['w_det.0.bias'], out['w_det.1.weight'], out['w_det.1.bias'] = D0.backward(
        eng, plan, dA0, _t2(wd[0].weight), shares=1, X=F.reshape(R, 512), amode=A_PLAIN)
    return dF.view(plan.nR, plan.Lt, 512), out


def head_forward_train(eng, model, plan, cat):
    """cat [Lt][1024] (encoder features) -> (det, link, new, end, tape): fusion -> w_det (training mode) + pairwise block"""
    F, tf = fusion_forward_train(eng, plan, cat)
    det, td = det_forward_train(eng, model, plan, F)
    link, new, end, ta = affinity_forward_train(eng, plan, F)
    return det, link, new, end, dict(F=F, fusion=tf, det=td, aff=ta)


def head_backward(eng, model, plan, cat, tape, d_det, d_link, d_new, d_end):
    """-> (dcat [Lt][1024], {state_dict key: grad} for fusion_module.*, w_det.*, w_link.*)"""
    F = tape['F']
    dF_a, grads = affinity_backward(eng, plan, F, tape['aff'], d_link, d_new, d_end)
    dF_d, g_d = det_backward(eng, model, plan, F, tape['det'], d_det)
    dF = torch.empty_like(dF_a)
    eng.ops.add_rows(dF_a.view(-1, 512), dF_d.view(-1, 512), dF.view(-1, 512), 512)
    dcat, g_f = fusion_backward(eng, plan, cat, tape['fusion'], dF)
    grads.update(g_d)
    grads.update(g_f)
    return dcat, grads


def current_engine(model):
    """The model's engine with the head packed from the parameters as they are NOW: fusion and w_link run from the
    packed copies, w_det's training forward from the live parameters - after an ``optimizer.step()`` (or any in-place
    edit: the parameters' version counters moved) the head is re-packed first, so forward and gradients never mix two
    generations of weights."""
    eng = model.engine()
    if hasattr(model, 'head_is_current') and not model.head_is_current():
        # on the device (no host packing; the fp16-split copies go stale and the training forward uses fp32 weights)
        eng = model.refresh_head_device() if hasattr(model, 'refresh_head_device') else model.refresh_head()
    return eng


def _named(model, *prefixes):
    named = [(k, p) for k, p in model.named_parameters() if k.split('.')[0] in prefixes]
    return [k for k, _ in named], [p for _, p in named]


def head_autograd(model, plan, cat, update_running_stats=True):
    """Differentiable head of ``model`` in training mode: encoder features cat [Lt][1024] (image | LiDAR) ->
    (det [nR, Lt] raw scores, link flat, new [nR, Lt], end [nR, Lt]); ``backward()`` fills ``cat.grad`` and the ``.grad``
    of every fusion_module / w_det / w_link parameter.  With ``update_running_stats`` the BatchNorm buffers of w_det take
    the momentum update PyTorch's training mode does."""
    eng = current_engine(model)
    tapes = []

    def fwd(c, _):
        with eng.fp32_mlp():  # the fp16-split copies of the head are not rebuilt after an optimizer step
            det, link, new, end, tape = head_forward_train(eng, model, plan, c)
        tapes.append(tape)
        return (det, link, new, end), tape

    out = taped(cat, *_named(model, 'fusion_module', 'w_det', 'w_link'), fwd,
                lambda c, tape, *d: head_backward(eng, model, plan, c, tape, *d))
    if update_running_stats:
        # like nn.BatchNorm1d in training mode, the buffers take the momentum update whether or not autograd records
        for idx, name in ((1, 'd0'), (4, 'd1')):
            momentum_update(model.w_det[idx], tapes[0]['det'][name], plan.nR * plan.Lt)
    return out


def affinity_autograd(model, plan, F):
    """Differentiable pairwise block of ``model`` (a TrackingNet on the device): F [nR, Lt, 512] ->
    (link flat [sum nR*N*M], new [nR, Lt], end [nR, Lt]) attached to the autograd graph; ``backward()`` fills
    ``F.grad`` and the ``.grad`` of every ``model.w_link`` parameter.  The packed weights are those of
    ``model.engine()``, re-packed here when a head parameter changed since (``model.head_is_current()``)."""
    eng = current_engine(model)

    def fwd(f, _):
        with eng.fp32_mlp():
            link, new, end, tape = affinity_forward_train(eng, plan, f)
        return (link, new, end), tape

    return taped(F, *_named(model, 'w_link'), fwd, lambda f, tape, *d: affinity_backward(eng, plan, f, tape, *d))
