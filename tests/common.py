"""Shared helpers for the test-suite (golden fixtures, model construction)."""
import json
import os

import numpy as np
import torch

from mmmot_amd import TrackingNet
from mmmot_amd.synth import make_pair
from mmmot_amd.weights import init_module, state_dict_for_profile

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = 1e-3  # BASELINE.json north_star: outputs within 1e-3 (fp32) of the reference CPU path


def manifest():
    with open(os.path.join(GOLD, 'manifest.json')) as f:
        return json.load(f)


def case_names(light_only=False):
    """Small fixtures (outputs + stage checkpoints).  The full-size ones are in full_case_names()."""
    names = [c['name'] for c in manifest()['cases'] if not c.get('full')]
    if light_only:
        names = [n for n in names if not n.startswith('s3_')]
    return names


def full_case_names():
    """BASELINE.json-size fixtures (cfg3 / cfg4 shapes, outputs of the imported reference only)."""
    return [c['name'] for c in manifest()['cases'] if c.get('full')]


def get_case(name):
    m = manifest()
    c = [x for x in m['cases'] if x['name'] == name][0]
    return c, m['base_kwargs']


def case_inputs(c):
    if 'counts' in c:
        dets, info, _ = make_pair(c['counts'][0], sum(c['counts'][1:]), c['S'], c['pts'], c['seed'], ragged=True)
        return dets, info, [torch.tensor([x]) for x in c['counts']]
    return make_pair(c['N'], c['M'], c['S'], c['pts'], c['seed'], c['ragged'], reflectivity=bool(c.get('refl')))


def case_kwargs(c, base):
    kw = dict(base, score_fusion_arch=c['fusion'], affinity_op=c['aff'], softmax_mode=c['sm'],
              end_mode=c.get('end_mode', base.get('end_mode', 'avg')))
    if c.get('refl'):
        kw['without_reflectivity'] = False
    if 'dropblock' in c:
        kw['dropblock'] = c['dropblock']
    if 'counts' in c:
        kw['seq_len'] = len(c['counts'])
    return kw


def build_model(c, base, device='cpu', ops=None):
    m = TrackingNet(**case_kwargs(c, base))
    if 'weights' in c:  # fixtures generated on other weight statistics than the seed-0 default (oracle/gen_golden.py)
        m.load_state_dict(state_dict_for_profile(m.state_dict(), c['weights'], c['S']), strict=True)
    else:
        init_module(m, 0)
    m.eval()
    if device != 'cpu':
        m = m.to(device)
    if ops is not None:
        m.set_ops(ops)
    return m


def golden(name):
    return np.load(os.path.join(GOLD, name + '.npz'))


def compare_outputs(out, g, tol=TOL, rows=(0, 1, 2)):
    """out = (det, links, new, end, trans) from a model/oracle; g = golden npz."""
    det, links, new, end, trans = out
    r = list(rows)
    errs = {
        'det': np.abs(det.detach().cpu().numpy() - g['det'][r]).max(),
        'new': np.abs(new.detach().cpu().numpy() - g['new'][r]).max(),
        'end': np.abs(end.detach().cpu().numpy() - g['end'][r]).max(),
        'link': max(np.abs(l.detach().cpu().numpy() - g['link%d' % i][r]).max() for i, l in enumerate(links)),
    }
    if trans is not None:
        errs['trans'] = max(np.abs(trans[0].detach().cpu().numpy() - g['trans1']).max(),
                            np.abs(trans[1].detach().cpu().numpy() - g['trans2']).max())
    bad = {k: float(v) for k, v in errs.items() if not (v <= tol)}
    assert not bad, 'outputs differ from the reference golden by more than %.0e: %r (all: %r)' % (tol, bad, errs)
    return errs


# ---- training-step fixtures of the IMPORTED reference (oracle/gen_golden_train.py) ----
def train_case_names():
    import glob
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, 'train_*.npz')))


def load_train_case(name):
    """-> (case dict, loss kwargs, fixture npz, inputs (dets, info, dets_split), gts (det, [link], new, end))"""
    import ast
    g = np.load(os.path.join(GOLD, name + '.npz'))
    c = dict(ast.literal_eval(str(g['case'])))
    kw = dict(ast.literal_eval(str(g['loss_kwargs'])))
    if 'counts' in c:
        dets, info, _ = make_pair(c['counts'][0], sum(c['counts'][1:]), c['S'], c['pts'], c['seed'], ragged=True)
        ds = [torch.tensor([x]) for x in c['counts']]
    else:
        dets, info, ds = make_pair(c['N'], c['M'], c['S'], c['pts'], c['seed'], True)
    n = len(ds) - 1
    t = lambda k: torch.from_numpy(g[k])
    gts = (t('gt_det'), [t('gt_link%d' % i) for i in range(n)], t('gt_new'), t('gt_end'))
    return c, kw, g, (dets, info, ds), gts


def compare_train_step(g, outs, loss, grad_of, buffers, out_tol, loss_tol, grad_tol, norm_tol, bn_tol, what):
    """One training step against a reference fixture.  outs = (det, [links], new, end, trans); grad_of(key) -> gradient
    tensor (or None = zero); buffers: key -> tensor for the 'bn:' entries.  Gradients are compared relative to the
    largest entry of the REFERENCE's gradient tensor (grad_norms[:, 2]); tensors whose reference gradient is rounding
    residue (< 1e-5: biases in front of a normalisation, the STN layers behind the one-value-per-group GroupNorm) must
    stay below 1e-4 absolutely.  Returns a dict of the worst differences."""
    det, links, new, end, trans = outs
    f = lambda x: x.detach().cpu().double().numpy()
    worst = dict(det=np.abs(f(det) - g['det']).max(), new=np.abs(f(new) - g['new']).max(), end=np.abs(f(end) - g['end']).max(),
                 link=max(np.abs(f(l) - g['link%d' % i]).max() for i, l in enumerate(links)),
                 trans=max(np.abs(f(trans[0]) - g['trans1']).max(), np.abs(f(trans[1]) - g['trans2']).max()),
                 loss=abs(float(loss) - float(g['loss'])))
    assert max(worst[k] for k in ('det', 'new', 'end', 'link', 'trans')) < out_tol, (what, worst)
    assert worst['loss'] < loss_tol * max(1.0, abs(float(g['loss']))), (what, worst)
    keys = [str(k) for k in g['grad_keys']]
    norms = {k: g['grad_norms'][i] for i, k in enumerate(keys)}
    sl, nm, res = 0.0, 0.0, 0.0
    for name in g.files:
        if not name.startswith('g:'):
            continue
        k = name[2:]
        want = g[name]
        got = grad_of(k)
        got = np.zeros_like(want) if got is None else f(got)[:want.shape[0]]
        sl = max(sl, np.abs(got - want).max() / norms[k][2])
    for k in keys:
        got = grad_of(k)
        got = None if got is None else f(got)
        s1, s2, amax = norms[k]
        if amax < 1e-5:
            if got is not None:
                res = max(res, np.abs(got).max())
            continue
        assert got is not None, (what, k, 'no gradient')
        nm = max(nm, abs(np.sqrt((got ** 2).sum()) - np.sqrt(s2)) / np.sqrt(s2), abs(np.abs(got).max() - amax) / amax)
    worst.update(grad_slices=sl, grad_norms=nm, grad_residue=res)
    assert sl < grad_tol and nm < norm_tol and res < 1e-4, (what, worst)
    bn = 0.0
    for name in g.files:
        if name.startswith('bn:'):
            got = buffers[name[3:]].detach().cpu().double().numpy()
            bn = max(bn, np.abs(got - g[name]).max())
    worst['bn_buffers'] = bn
    assert bn < bn_tol, (what, worst)
    return worst


# ---- 8-bit crops and poisoned workspaces (tests/test_u8_crops_*.py, tests/test_workspace_poison_*.py) ----
U8_LO = (0, 96, 192)  # R in [0, 64), G in [96, 160), B in [192, 256): a swapped channel or a wrong mean cannot pass


def u8_crops(dets):
    """uint8 [L,S,S,3] crops (HWC, what mmmot_amd.crops.crop_resize_u8 returns) made from the fp32 [L,3,S,S] crops of
    make_pair (every detection keeps its own appearance): each colour channel in its own 64-value byte range, bytes 0
    and 255 both present."""
    q = ((dets.float() + 2.2) * (64.0 / 4.9)).floor().clamp(0, 63)
    q = q + torch.tensor(U8_LO, dtype=torch.float32).view(1, 3, 1, 1)
    u8 = q.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    u8[0, 0, 0, 0] = 0
    u8[-1, -1, -1, 2] = 255
    return u8


def u8_image(L, H, W, seed):
    """i.i.d. uint8 [L,H,W,3] pixels with the channel ranges of u8_crops, bytes 0 and 255 present"""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 64, (L, H, W, 3), generator=g, dtype=torch.int32) + torch.tensor(U8_LO, dtype=torch.int32)
    u8 = u8.to(torch.uint8)
    u8[0, 0, 0, 0] = 0
    u8[-1, -1, -1, 2] = 255
    return u8


def normalise_u8(u8):
    """host ToTensor + Normalize of uint8 [L,H,W,3] crops -> fp32 [L,3,H,W]: oracle.crops_ref.to_tensor_normalize per crop"""
    from oracle.crops_ref import to_tensor_normalize
    return torch.from_numpy(np.ascontiguousarray(np.stack([to_tensor_normalize(c) for c in u8.cpu().numpy()])))


class CallLog:
    """Operator backend proxy that records every operator an engine calls (stream pinning is not a launch)."""
    _quiet = ('name', 'on_current_stream', 'on_stream')

    def __init__(self, ops):
        self.ops = ops
        self.calls = []

    def __getattr__(self, k):
        v = getattr(self.ops, k)
        if k in self._quiet or k.startswith('_') or not callable(v):
            return v

        def call(*a, **kw):
            self.calls.append(k)
            return v(*a, **kw)
        return call


POISON = (0xFF, 0x7B)  # NaN as f64 / f32 / f16 / e4m3;  finite but huge: 1.3e36 (f32), 61280 (f16), 352 (e4m3)


def poison_workspace(eng, byte):
    """Fill every scratch entry of the engine's workspace arena (string keys) byte-wise.  Tuple keys hold constants
    (('mean_std', dev), the backward's ('unit', C, dev)) and are left alone."""
    n = 0
    for k, t in eng.ws.items():
        if isinstance(k, str):
            t.view(torch.uint8).fill_(byte)
            n += 1
    assert n > 0, 'empty workspace: nothing was poisoned'


def scores(out):
    """(det, [links], new, end) of a forward, detached copies on the host"""
    det, links, new, end = out[:4]
    c = lambda t: t.detach().cpu().clone()
    return c(det), [c(l) for l in links], c(new), c(end)


def assert_same_scores(got, want, what):
    names = ('det', 'link', 'new', 'end')
    for name, a, b in zip(names, got, want):
        for i, (x, y) in enumerate(zip(a, b) if name == 'link' else [(a, b)]):
            assert x.shape == y.shape, (what, name, i, x.shape, y.shape)
            if not torch.equal(x, y):
                d = (x.double() - y.double()).abs()
                raise AssertionError('%s: %s%s differs: max |diff| %.3e, %d of %d elements differ, %d non-finite' % (
                    what, name, '[%d]' % i if name == 'link' else '', d.nan_to_num(float('inf')).max().item(),
                    int((x != y).sum()), x.numel(), int((~torch.isfinite(x)).sum())))
    assert len(got[1]) == len(want[1]), what


def check_over_poison(m, call, what):
    """warm-up forward, then for each poison pattern: fill the workspace, repeat the forward, compare bit for bit"""
    with torch.no_grad():
        want = scores(call())
        for byte in POISON:
            poison_workspace(m.engine(), byte)
            assert_same_scores(scores(call()), want, '%s, workspace filled with 0x%02X' % (what, byte))
    return want


# ---- in-place head edits a captured forward can follow (tests/test_graph_gpu.py, tests/test_batch_sizes_gpu.py) ----
def edit_below_half_max(w, factor, gain=None):
    """Scale, in place, the entries of the weight `w` ([N][K] after flattening) whose magnitude - times the per-row
    `gain` the packing folds in, if any - is below HALF the largest one.  The largest folded magnitude stays what it
    was, and with it the power-of-two scale of the weight's fp16-split copy (pack.hl16_weight_shift reads max |w| only):
    the one python scalar a packed matrix carries."""
    f = w.detach().flatten(1).double()
    if gain is not None:
        f = f * gain.double().view(-1, 1)
    mask = (f.abs() < 0.5 * f.abs().max()).view_as(w)
    assert 0 < int(mask.sum()) < mask.numel()
    with torch.no_grad():
        w.mul_(torch.where(mask, torch.full_like(w, factor), torch.ones_like(w)))


def packed_scalars(P):
    return {(s, k): v for s in ('fusion', 'w_det', 'w_link') for k, v in P[s].items() if not torch.is_tensor(v)}
