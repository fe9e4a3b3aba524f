#!/usr/bin/env python
"""Generate tests/golden/endmax_train_s10_C.npz: one training step of the REFERENCE with ``end_mode='max'``.

    python tools/gen_golden_endmax_train.py

The counterpart of oracle/gen_golden_train.py for the one model configuration its cases leave out:
``NewEndIndicator_v2`` taking the maximum over the prev / curr axis (reference modules/new_end.py:72-74), whose backward
sends a new / end vector's gradient to the first row that attains the maximum.  The imported
``modules.TrackingNet(end_mode='max').train()`` and the imported ``cost.TrackingLoss`` run the step of
``tracking_model.py:50-66`` on one small sample (fusion C, minus_abs, dual_add, N = 6, M = 5, S = 64, 40 points per
detection); nothing of the reference is copied, only data is written.  The import shims, the sample, the ground truth
draw, the loss settings, the gradient slices and the keys of the file are those of oracle/gen_golden_train.py (imported
from there), so tests/common.py::load_train_case / compare_train_step read the file like a ``train_*.npz`` one; the
``case`` entry carries ``end_mode='max'`` for tests/common.py::case_kwargs.

The file is NOT named ``train_*.npz``: the tests parametrised over that pattern run the operator emulation of
tests/fake_ops.py, which does not know the two operators of the 'max' backward (tests/end_max_ref.py adds them).

Before it writes, the script asserts the float64-capable restatement (oracle/restatement.py::tracking_forward_train with
``cfg['end_mode'] = 'max'`` + tracking_loss, differentiated by torch.autograd) against the reference's step, with the
bounds of oracle/gen_golden_train.py.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
from gen_golden import BASE, GOLD, import_reference  # noqa: E402
from gen_golden_loss import uint8_eq  # noqa: E402
from gen_golden_train import LOSS_KW, case_inputs, grad_slices, make_gts  # noqa: E402
from mmmot_amd.weights import generate_state_dict  # noqa: E402
from oracle import restatement as R  # noqa: E402

CASE = dict(name='endmax_train_s10_C', fusion='C', aff='minus_abs', sm='dual_add', N=6, M=5, S=64, pts=40, seed=1041,
            gt_seed=45, end_mode='max')


def main():
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    c = CASE
    ref_modules = import_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        import cost as ref_cost
    counts = [c['N'], c['M']]
    kw = dict(BASE, score_fusion_arch=c['fusion'], affinity_op=c['aff'], softmax_mode=c['sm'], seq_len=2, dropblock=0,
              end_mode=c['end_mode'])
    with contextlib.redirect_stdout(io.StringIO()):
        model = ref_modules.TrackingNet(**kw)
        crit = ref_cost.TrackingLoss(**LOSS_KW)
    sd0 = generate_state_dict(model.state_dict(), seed=0)
    model.load_state_dict(sd0, strict=True)
    model.train()
    dets, info, dsplit = case_inputs(c)
    gts = make_gts(counts, c['gt_seed'])
    det, links, new, end, trans = model(dets, info, dsplit)
    with uint8_eq():
        loss = crit(dsplit, gts[0], gts[1], gts[2], gts[3], det, links, new, end, trans)
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    after = {k: v.detach().clone() for k, v in model.state_dict().items()}

    # ---- the restatement on the same sample (float32 like the reference), through autograd ----
    sd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and k in grads and k.split('.')[-1] != 'idt'
              else v.clone()) for k, v in sd0.items()}
    cfg = dict(fusion=c['fusion'], affinity_op=c['aff'], softmax_mode=c['sm'], end_mode=c['end_mode'])
    stats = {}
    o_det, o_links, o_new, o_end, o_trans = R.tracking_forward_train(
        sd, cfg, None, info['points'], info['points_split'], [int(d) for d in dsplit], crops=dets, bn_stats=stats)
    o_loss = R.tracking_loss(counts, gts[0], gts[1], gts[2], gts[3], o_det, o_links, o_new, o_end, o_trans, **LOSS_KW)
    o_loss.backward()
    e = dict(det=(det - o_det).abs().max().item(), new=(new - o_new).abs().max().item(),
             end=(end - o_end).abs().max().item(), loss=abs(loss.item() - o_loss.item()),
             link=max((a - b).abs().max().item() for a, b in zip(links, o_links)))
    rel, resid = 0.0, 0.0
    for k, g in grads.items():
        og = sd[k].grad if (sd[k].requires_grad and sd[k].grad is not None) else torch.zeros_like(g)
        d = (g - og).abs().max().item()
        if g.abs().max().item() > 1e-5:
            rel = max(rel, d / g.abs().max().item())
        else:
            resid = max(resid, d)
    e['grad_rel'], e['grad_residue_abs'] = rel, resid
    e['bn'] = max((after[k] - v).abs().max().item() for k, v in stats.items())
    print('%-22s loss %.6f  |reference - restatement|: %s' % (c['name'], loss.item(),
          ' '.join('%s=%.1e' % kv for kv in e.items())), flush=True)
    assert max(e['det'], e['new'], e['end'], e['link'], e['loss']) < 5e-5 and e['bn'] < 1e-5, e
    assert e['grad_rel'] < 2e-3 and e['grad_residue_abs'] < 1e-5, e
    # the step is not the 'avg' one: the same sample through the mean pool gives other new / end scores
    a_det, a_links, a_new, a_end, _ = R.tracking_forward_train(
        {k: v.detach() for k, v in sd0.items()}, dict(cfg, end_mode='avg'), None, info['points'], info['points_split'],
        [int(d) for d in dsplit], crops=dets)
    assert (a_new - new).abs().max().item() > 1e-3 and (a_end - end).abs().max().item() > 1e-3

    # ---- the fixture: the keys of oracle/gen_golden_train.py ----
    out = dict(counts=np.asarray(counts), loss=np.float32(loss.item()), det=det.detach().numpy(),
               new=new.detach().numpy(), end=end.detach().numpy(), trans1=trans[0].detach().numpy(),
               trans2=trans[1].detach().numpy(), gt_det=gts[0].numpy(), gt_new=gts[2].numpy(), gt_end=gts[3].numpy())
    for i, l in enumerate(links):
        out['link%d' % i], out['gt_link%d' % i] = l.detach().numpy(), gts[1][i].numpy()
    keys = sorted(grads)
    out['grad_keys'] = np.asarray(keys)
    out['grad_norms'] = np.asarray([[grads[k].double().sum().item(), (grads[k].double() ** 2).sum().item(),
                                     grads[k].abs().max().item()] for k in keys], np.float64)
    for k, n in grad_slices(c).items():
        g = grads[k]
        out['g:' + k] = (g if n is None else g[:n]).contiguous().numpy()
    for k, v in after.items():
        if 'running_' in k or 'num_batches_tracked' in k:
            out['bn:' + k] = v.numpy()
    out['case'] = np.asarray(repr(sorted(c.items())))
    out['loss_kwargs'] = np.asarray(repr(sorted(LOSS_KW.items())))
    path = os.path.join(GOLD, c['name'] + '.npz')
    np.savez_compressed(path, **out)
    print('fixture written: %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
