#!/usr/bin/env python
"""Generate tests/golden/optim_adam.npz by running the REFERENCE's optimizer wrapper and schedule over torch's Adam.

    python tools/gen_golden_optim.py --reference <checkout of the reference project>

``utils/optim_util.py`` (OptimWrapper), ``utils/learning_schedules_fastai.py`` (OneCycle) and ``utils/build_util.py``
(get_layer_groups, build_optim) are loaded from the checkout by file path and called as they are; nothing of them is
copied, only data is written.  Two harness-side shims, no edits to the reference: ``collections.Iterable`` is set to
``collections.abc.Iterable`` first (optim_util.py imports the name Python 3.10 removed), and the modules build_util.py
imports at its top and the functions used here never touch (``cost``, ``dataset``, ``modules``, ``torchvision``) are
replaced by empty stand-ins.  CPU, float64.

The tree (tests/optim_ref.make_tree): nested Sequential; Linear, Conv1d, Conv2d; BatchNorm1d, BatchNorm2d, GroupNorm; a
LayerNorm; a parent with a direct parameter; a requires_grad=False parameter; a parameter of one element.  Gradients are
seeded normal draws, the same for every case; one parameter's .grad is None at one step (optim_ref.NONE_GRAD).  Cases:
true_wd on / off x bn_wd on / off; the case (true_wd, bn_wd=True) goes through the reference's build_optim itself.
Schedule: OneCycle(total 20, 6e-4, [0.95, 0.85], 10.0, 0.4), stepped through both phases as the training loop does -
``lr_scheduler.step(it)``, then the gradients, then ``optimizer.step()``.

Keys: names; init/<name>; grad/<name> [20, ..]; per case c = tw<0|1>_bn<0|1>: lr/c, mom/c [20] (read from the wrapper
after the scheduler stepped), param/c/<name> [20, ..] (every parameter after every step), group0/c, group1/c (names),
steps/c (the final state_dict's step counts, -1 = no state) in the order of group0 + group1.
"""
import argparse
import collections
import collections.abc
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True
import optim_ref  # noqa: E402


def import_reference(path):
    collections.Iterable = collections.abc.Iterable
    for name, attrs in (('cost', ['TrackingLoss']), ('dataset', ['PatchwiseDataset', 'TestSequenceDataset']),
                        ('modules', ['TrackingNet'])):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    try:
        import torchvision.transforms  # noqa: F401
    except Exception:
        tv = types.ModuleType('torchvision')
        tv.transforms = types.ModuleType('torchvision.transforms')
        sys.modules['torchvision'], sys.modules['torchvision.transforms'] = tv, tv.transforms
    pkg = types.ModuleType('refutils')  # a package of its own: utils/__init__.py imports the whole project
    pkg.__path__ = [os.path.join(path, 'utils')]
    sys.modules['refutils'] = pkg
    out = {}
    for name in ('optim_util', 'learning_schedules_fastai', 'build_util'):
        spec = importlib.util.spec_from_file_location('refutils.' + name, os.path.join(path, 'utils', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        out[name] = mod
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=optim_ref.GOLDEN)
    args = ap.parse_args()
    ref = import_reference(args.reference)
    S = optim_ref.SCHEDULE
    steps = S['total_step']

    torch.manual_seed(20)
    tree0 = optim_ref.make_tree()
    rng = np.random.default_rng(11)
    with torch.no_grad():
        for p in tree0.parameters():  # away from the constructors' ones and zeros
            p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)) * 0.5 + 0.1))
    names = [k for k, _ in tree0.named_parameters()]
    out = {'names': np.array(names)}
    init = {k: p.detach().numpy().copy() for k, p in tree0.named_parameters()}
    grads = {k: rng.standard_normal((steps,) + init[k].shape) * np.exp(rng.uniform(-4, 1)) for k in names}
    for k in names:
        out['init/' + k], out['grad/' + k] = init[k], grads[k]

    for true_wd, bn_wd in optim_ref.CASES:
        c = optim_ref.case_name(true_wd, bn_wd)
        net = optim_ref.make_tree(init)
        if bn_wd:
            cfg = types.SimpleNamespace(lr_scheduler=types.SimpleNamespace(optim='Adam', base_lr=optim_ref.BASE_LR),
                                        weight_decay=optim_ref.WD, fixed_wd=true_wd)
            opt = ref['build_util'].build_optim(net, cfg)
        else:
            opt = ref['optim_util'].OptimWrapper.create(
                functools.partial(torch.optim.Adam, betas=optim_ref.BETAS), optim_ref.BASE_LR,
                ref['build_util'].get_layer_groups(net), wd=optim_ref.WD, true_wd=true_wd, bn_wd=False)
        sched = ref['learning_schedules_fastai'].OneCycle(opt, steps, S['lr_max'], list(S['moms']), S['div_factor'],
                                                          S['pct_start'])
        by_id = {id(p): k for k, p in net.named_parameters()}
        groups = [[by_id[id(p)] for p in g['params']] for g in opt.param_groups]
        assert len(groups) == 2
        out['group0/' + c], out['group1/' + c] = np.array(groups[0]), np.array(groups[1])
        lrs, moms = [], []
        track = {k: [] for k in names}
        for it in range(steps):
            sched.step(it)
            lrs.append(float(opt.lr))
            moms.append(float(opt.mom))
            opt.zero_grad()
            for k, p in net.named_parameters():
                if p.requires_grad:
                    p.grad = None if (k, it) == optim_ref.NONE_GRAD else torch.from_numpy(grads[k][it].copy())
            opt.step()
            for k, p in net.named_parameters():
                track[k].append(p.detach().numpy().copy())
        out['lr/' + c], out['mom/' + c] = np.array(lrs), np.array(moms)
        for k in names:
            out['param/%s/%s' % (c, k)] = np.stack(track[k])
        sd = opt.state_dict()
        order = [i for g in sd['param_groups'] for i in g['params']]
        out['steps/' + c] = np.array([int(sd['state'][i]['step']) if i in sd['state'] else -1 for i in order])
        print('%s: groups %d + %d tensors, lr %.3e .. %.3e, final steps %s' % (
            c, len(groups[0]), len(groups[1]), min(lrs), max(lrs), sorted(set(out['steps/' + c].tolist()))))
    np.savez_compressed(args.out, **out)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
