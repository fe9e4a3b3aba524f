#!/usr/bin/env python
"""Generate tests/golden/pointnet_dropout_<name>.npz by running the REFERENCE's PointNet_v1 with use_dropout=True.

    python tools/gen_golden_pointnet_dropout.py --reference <checkout of the reference project>

``modules/point_net.py`` is loaded from the checkout on its own (it imports torch only) and ``PointNet_v1`` is used as it
is; nothing of it is copied, only data is written.  The module gets this project's seeded weights
(``weights.init_module(mirror, 0)`` on ``mmmot_amd.modules.PointNet_v1``, handed over through ``state_dict``), is
converted to float64 and stays in training mode.  Its ``dropout`` attribute - ``nn.Dropout(0.5)``, whose own bit stream
differs between devices and versions - is replaced by a module that multiplies by a GIVEN factor tensor [1][512][P]:
the device mask of DESIGN.md section 17 (tests/dropout_ref.mask, threshold 0x80000000) times 2.  What the fixture pins
against the reference is therefore WHERE the factor acts (between relu(bn1(conv1)) and the per-detection average pool,
elementwise over points x channels) and everything the gradient passes through behind and in front of it.

Per case (3 and 4 input channels; N = 3, M = 2, about 30 points per detection, one detection of a single point):
the case dict, the mask seed, ``out`` [L][512], for every parameter with a gradient (sum, sum of squares, max |.|) of
it, and the full gradient of the tensors of at most 1024 elements.  Loss: sum(out * w) + sum(trans2 * wt) with the fixed
weights of tests/test_train_gpu.py::test_pointnet_backward_on_the_device (randn seeds 3 and 4).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True
import dropout_ref  # noqa: E402
from mmmot_amd.modules import PointNet_v1  # noqa: E402
from mmmot_amd.synth import make_pair  # noqa: E402
from mmmot_amd.weights import init_module  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = [dict(name='xyz', N=3, M=2, S=8, pts=30, seed=41, ragged=True, refl=0, mask_seed=0x5EED0D120B0A7001),
         dict(name='refl', N=3, M=2, S=8, pts=30, seed=42, ragged=True, refl=1, mask_seed=20191027)]
SMALL = 1024


class Factor(torch.nn.Module):
    def __init__(self, factor):
        super().__init__()
        self.factor = factor

    def forward(self, x):
        return x * self.factor


def load_point_net(reference):
    # the STN's GroupNorm(C, C) over a 1 x C tensor: the torch of the reference's day had no batch-size check for
    # group_norm in training mode (oracle/gen_golden.py does the same)
    torch.nn.functional._verify_batch_size = lambda size: None
    spec = importlib.util.spec_from_file_location('ref_point_net', os.path.join(reference, 'modules', 'point_net.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    a = ap.parse_args()
    ref = load_point_net(a.reference)
    for c in CASES:
        kin = 3 + c['refl']
        mirror = PointNet_v1(kin, use_dropout=True)
        init_module(mirror, 0)
        m = ref.PointNet_v1(kin, use_dropout=True)
        assert isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == 0.5
        m.load_state_dict(mirror.state_dict(), strict=True)
        m = m.double().train()
        _, info, _ = make_pair(c['N'], c['M'], c['S'], c['pts'], c['seed'], c['ragged'], reflectivity=bool(c['refl']))
        split = info['points_split'].reshape(-1).long()
        cnt = (split[1:] - split[:-1]).tolist()
        assert 1 in cnt and max(cnt) > 1, cnt
        P = int(split[-1])
        keep = dropout_ref.mask(c['mask_seed'], 0x80000000, P, 512)
        m.dropout = Factor(torch.from_numpy(keep.T.astype(np.float64) * 2.0).unsqueeze(0))
        out, trans = m(info['points'].double().transpose(-1, -2), split)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).double()
        wt = torch.randn(64, 64, generator=torch.Generator().manual_seed(4)).double()
        ((out * w).sum() + (trans[1][0] * wt).sum()).backward()
        keys, norms, full = [], [], {}
        for k, p in m.named_parameters():
            if p.grad is None:
                continue
            g = p.grad.numpy()
            keys.append('point_net.' + k)
            norms.append([g.sum(), (g ** 2).sum(), np.abs(g).max()])
            if g.size <= SMALL:
                full['g:point_net.' + k] = g
        case = {k: v for k, v in c.items() if k not in ('name', 'mask_seed')}
        path = os.path.join(GOLDEN, 'pointnet_dropout_%s.npz' % c['name'])
        np.savez_compressed(path, case=repr(case), mask_seed=np.uint64(c['mask_seed']), counts=np.asarray(cnt),
                            keep_fraction=keep.mean(), out=out.detach().numpy(), grad_keys=np.asarray(keys),
                            grad_norms=np.asarray(norms), **full)
        print('%s: P = %d, counts %s, kept %.4f, %d gradients (%d in full), %d bytes' % (
            path, P, cnt, keep.mean(), len(keys), len(full), os.path.getsize(path)))


if __name__ == '__main__':
    main()
