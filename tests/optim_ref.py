"""Executable specifications of the optimizer step (mmmot_amd/optim.py, csrc/adam_step.hip); not a test module.

* ``RefOptim``: the fastai ``OptimWrapper`` over torch's Adam restated in NumPy float64 - what
  tests/golden/optim_adam.npz (made by running the reference's wrapper over ``torch.optim.Adam``:
  tools/gen_golden_optim.py) pins, and the float64 yardstick of the GPU tests.
* ``one_cycle``: lr and momentum of the reference's ``OneCycle`` at an iteration, as plain functions.
* ``EmuOps``: an emulation of ``mmmot_adam_step`` that the CPU tests inject as the optimizer's backend.  Like the kernel
  it is handed ADDRESSES and writes through them, chunk by chunk of the chunk table - so nothing it does advances a
  version counter, and a test of ``optim.Adam`` through it sees what the optimizer itself does about that.
* ``make_tree``: the module tree of the fixture (every grouping quirk the wrapper has, in miniature).
* ``TorchWrapper``: the parent's path - the restated wrapper's decay loop over a ``torch.optim.Adam``.
"""
import ctypes
import os

import numpy as np
import torch
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optim_adam.npz')
CASES = [(True, True), (True, False), (False, True), (False, False)]  # (true_wd, bn_wd)
SCHEDULE = dict(total_step=20, lr_max=6e-4, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)
WD, BASE_LR, BETAS, EPS = 0.01, 3e-4, (0.9, 0.99), 1e-8
NONE_GRAD = ('stem.0.weight', 7)  # this parameter's .grad is None at this step


def case_name(true_wd, bn_wd):
    return 'tw%d_bn%d' % (int(true_wd), int(bn_wd))


# ---- the module tree ---------------------------------------------------------------------------------------------------
class Scaled(nn.Module):
    """A parent that holds a parameter of its own beside its children: the wrapper's groups miss it."""

    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(3))
        self.lin = nn.Linear(4, 3)
        self.norm = nn.LayerNorm(3)  # counts as a non-norm leaf


class Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(2, 3, 3), nn.BatchNorm2d(3),
                                  nn.Sequential(nn.Conv1d(3, 4, 1), nn.BatchNorm1d(4), nn.GroupNorm(2, 4)))
        self.block = Scaled()
        self.head = nn.Linear(3, 1)  # its bias: a parameter of one element
        self.frozen = nn.Linear(2, 2)
        self.frozen.weight.requires_grad_(False)


def make_tree(init=None, dtype=torch.float64):
    """The fixture's tree; ``init``: {name: array} to start from (the fixture's ``init/<name>``)."""
    m = Tree().to(dtype)
    if init is not None:
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(torch.as_tensor(np.asarray(init[k])).to(dtype))
    return m


# ---- the schedule ------------------------------------------------------------------------------------------------------
def _cos(start, end, pct):
    return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)


def one_cycle(it, total_step, lr_max, moms, div_factor, pct_start):
    """(lr, mom) that ``OneCycle.step(it)`` leaves behind: the last phase whose start has been reached."""
    a1 = int(pct_start * total_step)
    low = lr_max / div_factor
    if it >= a1:
        pct = (it - a1) / (total_step - a1)
        return float(_cos(lr_max, low / 1e4, pct)), float(_cos(moms[1], moms[0], pct))
    pct = (it - 0) / (a1 - 0)
    return float(_cos(low, lr_max, pct)), float(_cos(moms[0], moms[1], pct))


# ---- wrapper + Adam in float64 -----------------------------------------------------------------------------------------
class RefOptim:
    """params: {name: float64 array}, updated in place; groups: [names of the non-norm group, names of the norm group]."""

    def __init__(self, params, groups, wd, true_wd, bn_wd, beta2=BETAS[1], eps=EPS):
        self.p, self.groups, self.wd, self.true_wd, self.bn_wd, self.beta2, self.eps = params, groups, wd, true_wd, bn_wd, beta2, eps
        self.m, self.v, self.t = {}, {}, {}
        # the inner optimizer's weight_decay per group: the constructor's 0 unless the wrapper's wd setter wrote it
        self.l2 = [0.0, 0.0] if true_wd else [wd, wd if bn_wd else 0.0]

    def step(self, grads, lr, mom):
        if self.true_wd:
            f = 1 - self.wd * lr
            for k in self.groups[0] + (self.groups[1] if self.bn_wd else []):
                self.p[k] *= f
            self.l2 = [0.0, 0.0]
        b1, b2 = mom, self.beta2
        for names, l2 in zip(self.groups, self.l2):
            for k in names:
                g = grads.get(k)
                if g is None:
                    continue
                g = np.asarray(g, dtype=np.float64)
                if k not in self.t:
                    self.m[k], self.v[k], self.t[k] = np.zeros_like(self.p[k]), np.zeros_like(self.p[k]), 0
                t = self.t[k] = self.t[k] + 1
                if l2 != 0:
                    g = g + l2 * self.p[k]
                self.m[k] += (1 - b1) * (g - self.m[k])
                self.v[k] = self.v[k] * b2 + (1 - b2) * g * g
                step_size = lr / (1 - b1 ** t)
                denom = np.sqrt(self.v[k]) / (1 - b2 ** t) ** 0.5 + self.eps
                self.p[k] -= step_size * (self.m[k] / denom)


# ---- the parent's path: decay loop + torch.optim.Adam ------------------------------------------------------------------
class TorchWrapper:
    """What a training loop ran before optim.Adam: under ``true_wd`` one ``mul_`` per parameter, then torch's Adam.
    groups: [non-norm tensors, norm tensors]."""

    def __init__(self, groups, wd, true_wd, bn_wd, **adam_kw):
        self.opt = torch.optim.Adam([{'params': list(g), 'lr': BASE_LR} for g in groups], betas=BETAS, eps=EPS, **adam_kw)
        self.wd, self.true_wd, self.bn_wd = wd, true_wd, bn_wd
        if not true_wd:
            self.opt.param_groups[0]['weight_decay'] = wd
            if bn_wd:
                self.opt.param_groups[1]['weight_decay'] = wd

    def step(self, lr, mom):
        g = self.opt.param_groups
        for x in g:
            x['lr'], x['betas'] = lr, (mom, x['betas'][1])
        if self.true_wd:
            f = 1 - self.wd * lr
            with torch.no_grad():
                for p in g[0]['params'] + (g[1]['params'] if self.bn_wd else []):
                    p.mul_(f)
            for x in g:
                x['weight_decay'] = 0
        self.opt.step()


# ---- emulation of mmmot_adam_step ---------------------------------------------------------------------------------------
class EmuOps:
    """``adam_step`` with the signature of HipOps.adam_step, all tables on the host: chunks int32 [n, 2], ptrs int64 [T, 6]
    (p, g, m, v, numel, flags), scal float64 [T, 4] (step_size, bc2_sqrt, decay, l2).  ``dtype``: float32 = the kernel's
    arithmetic (scalars rounded to fp32 once), float64 = the same sequence in double, for the fixture."""
    name = 'emu'

    def __init__(self, dtype=torch.float32):
        from mmmot_amd import optim
        self.dtype, self.chunk, self.calls = dtype, optim.chunk_elems(), 0

    def _view(self, addr, off, n):
        ct = ctypes.c_double if self.dtype == torch.float64 else ctypes.c_float
        return torch.frombuffer((ct * n).from_address(int(addr) + off * ctypes.sizeof(ct)), dtype=self.dtype)

    def adam_step(self, chunks, ptrs, scal, beta1, beta2, eps):
        self.calls += 1
        r = (lambda x: float(np.float32(x))) if self.dtype == torch.float32 else float
        omb1, b2, omb2, eps = r(1.0 - beta1), r(beta2), r(1.0 - beta2), r(eps)
        for ti, ci in chunks.tolist():
            pa, ga, ma, va, numel, flags = ptrs[ti].tolist()
            step_size, bc2_sqrt, decay, l2 = (r(x) for x in scal[ti].tolist())
            off = ci * self.chunk
            if off >= numel or (not flags & 1 and decay == 1.0):
                continue
            n = min(self.chunk, numel - off)
            p = self._view(pa, off, n)
            if decay != 1.0:
                p.mul_(decay)
            if not flags & 1:
                continue
            g, m, v = self._view(ga, off, n), self._view(ma, off, n), self._view(va, off, n)
            if l2 != 0.0:
                g = g + l2 * p
            m.add_(omb1 * (g - m))
            v.mul_(b2).add_((omb2 * g) * g)
            p.sub_(step_size * (m / (v.sqrt() / bc2_sqrt + eps)))
