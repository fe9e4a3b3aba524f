"""Optimizer step on the device: one-launch Adam behind the fastai-style ``OptimWrapper``.

Drop-ins for what the reference's ``TrackingModule`` builds its optimizer from (``utils/build_util.py:28-59``,
``utils/optim_util.py:90-234``, ``utils/learning_schedules_fastai.py:8-86``), written from their behaviour:

    optimizer = mmmot_amd.build_optim(model, config)                      # OptimWrapper over optim.Adam
    lr_scheduler = mmmot_amd.build_lr_scheduler(config.lr_scheduler, optimizer)
    ...
    lr_scheduler.step(it); optimizer.zero_grad(); loss.backward(); optimizer.step()

``Adam`` has the shape of ``torch.optim.Adam`` (``param_groups``, ``state``, ``step``, ``zero_grad``, ``state_dict``,
``load_state_dict`` in torch's format) and takes its step in ONE launch of ``mmmot_adam_step`` (csrc/adam_step.hip) over
every tensor; under the wrapper's ``true_wd`` the decoupled decay ``p *= 1 - wd*lr`` rides in the same launch instead of
a Python loop of one ``mul_`` per parameter.  The kernel writes the parameters through raw pointers, so ``step()``
advances ``Tensor._version`` of every parameter it had written: that is how ``TrackingNet`` and the weight tape notice
that their packed copies are stale.  DESIGN.md section 16 has the layout of the tables and the arithmetic order.
"""
import collections
import collections.abc
import ctypes
import functools

import numpy as np
import torch
from torch import nn

from . import torch_ops

NORM_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.GroupNorm)  # LayerNorm is not among them (kept)
_TORCH_ONLY = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                   decoupled_weight_decay=False)  # carried in the groups so that torch.optim.Adam can load our dicts


def _chunk_table(numels):
    """The host int32 [n, 2] chunk table of tensors of these sizes (mmmot_adam_chunks)."""
    from . import _lib
    lib = _lib.load()
    sizes = np.ascontiguousarray(numels, dtype=np.int64)
    count = ctypes.c_longlong(0)
    _lib.check(lib.mmmot_adam_chunks(sizes.ctypes.data, len(sizes), None, 0, ctypes.addressof(count)), 'mmmot_adam_chunks')
    table = torch.empty((count.value, 2), dtype=torch.int32)
    _lib.check(lib.mmmot_adam_chunks(sizes.ctypes.data, len(sizes), table.data_ptr(), count.value,
                                     ctypes.addressof(count)), 'mmmot_adam_chunks')
    return table


def chunk_elems():
    """Elements per chunk (per workgroup) of the loaded library's mmmot_adam_step."""
    from . import _lib
    return int(_lib.load().mmmot_adam_chunk_elems())


class Adam:
    """``torch.optim.Adam`` (single-tensor arithmetic, fp32) with the step taken by one launch of ``mmmot_adam_step``.

    ``step(decay=[f_0, ..])`` multiplies the parameters of group i by f_i before the update, in the same launch - the
    decoupled decay of ``OptimWrapper`` - a parameter without a gradient included, as the wrapper's loop does."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, amsgrad=False, maximize=False,
                 capturable=False, foreach=None, ops=None):
        if amsgrad or maximize or capturable or foreach is not None:
            raise ValueError('optim.Adam: amsgrad, maximize, capturable and foreach= are not supported')
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **_TORCH_ONLY)
        self.ops = ops  # operator backend (HipOps unless a test injects another)
        self.state = {}
        self.param_groups = []
        self._chunks = None  # (key, host table, device table, first chunk of every tensor)
        groups = list(params)
        if not groups:
            raise ValueError('optim.Adam: got an empty parameter list')
        if not isinstance(groups[0], dict):
            groups = [{'params': groups}]
        seen = set()
        for g in groups:
            g = dict(g)
            ps = g['params']
            g['params'] = [ps] if torch.is_tensor(ps) else list(ps)
            for k, v in self.defaults.items():
                g.setdefault(k, v)
            for p in g['params']:
                if id(p) in seen:
                    raise ValueError('optim.Adam: some parameters appear in more than one parameter group')
                seen.add(id(p))
            self._check_group(g)
            self.param_groups.append(g)
        self._check_params()

    # ---- checks ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_group(g):
        b1, b2 = g['betas']
        if not g['lr'] >= 0.0:
            raise ValueError('optim.Adam: invalid learning rate %r' % (g['lr'],))
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError('optim.Adam: betas must lie in [0, 1), got %r' % (g['betas'],))
        if not g['eps'] >= 0.0:
            raise ValueError('optim.Adam: invalid eps %r' % (g['eps'],))
        if not g['weight_decay'] >= 0.0:
            raise ValueError('optim.Adam: invalid weight_decay %r' % (g['weight_decay'],))
        if g.get('amsgrad') or g.get('maximize') or g.get('capturable') or g.get('foreach') is not None or \
                g.get('fused') or g.get('differentiable') or g.get('decoupled_weight_decay'):
            raise ValueError('optim.Adam: amsgrad, maximize, capturable, foreach, fused, differentiable and '
                             'decoupled_weight_decay are not supported')

    def _dtype(self):
        return getattr(self.ops, 'dtype', torch.float32) if self.ops is not None else torch.float32

    def _check_params(self):
        dt, dev = self._dtype(), None
        for g in self.param_groups:
            for p in g['params']:
                if not torch.is_tensor(p):
                    raise ValueError('optim.Adam: parameters must be tensors, got %s' % type(p).__name__)
                if p.dtype != dt or not p.is_contiguous() or p.numel() < 1:
                    raise ValueError('optim.Adam: parameters must be contiguous %s tensors of at least one element, got '
                                     '%s %s (contiguous: %s)' % (dt, p.dtype, tuple(p.shape), p.is_contiguous()))
                dev = p.device if dev is None else dev
                if p.device != dev:
                    raise ValueError('optim.Adam: parameters must live on one device, got %s and %s' % (dev, p.device))
        return dev

    def _ops(self):
        if self.ops is None:
            from .ops import HipOps
            self.ops = HipOps()
        return self.ops

    # ---- the step ----------------------------------------------------------------------------------------------------
    def _new_state(self, params):
        """exp_avg / exp_avg_sq of the parameters that meet their first gradient now: views of ONE zero-filled block,
        each starting on a 16-byte boundary."""
        pad = lambda n: (n + 3) & ~3
        total = sum(pad(p.numel()) for p in params)
        flat = torch.zeros(2 * total, dtype=params[0].dtype, device=params[0].device)
        o = 0
        for p in params:
            n = p.numel()
            self.state[p] = {'step': 0, 'exp_avg': flat[o:o + n].view_as(p), 'exp_avg_sq': flat[total + o:total + o + n].view_as(p)}
            o += pad(n)

    def _chunk_tables(self, numels, dev, hip):
        key = (tuple(numels), dev, hip)
        if self._chunks is None or self._chunks[0] != key:
            host = _chunk_table(key[0])
            first = np.concatenate([[0], np.cumsum((np.asarray(key[0], dtype=np.int64) - 1) // chunk_elems() + 1)])
            self._chunks = (key, host, host.to(dev) if hip else host, first)  # depends on the sizes only: uploaded once
        return self._chunks[2], self._chunks[3]

    @torch.no_grad()
    def step(self, closure=None, decay=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self.param_groups
        if decay is None:
            decay = [1.0] * len(groups)
        if len(decay) != len(groups):
            raise ValueError('optim.Adam.step: decay needs one factor per parameter group (%d, %d)' % (len(decay), len(groups)))
        if not any(g['params'] for g in groups):
            return loss
        ops = self._ops()
        hip = ops.name == 'hip'
        dt, state, has_grad = self._dtype(), self.state, torch_ops.ADAM_HAS_GRAD
        # every tensor is checked on every step, before anything is changed: the kernel follows the addresses, and a
        # parameter's storage can be replaced under the same object (module.to(), .half(), p.data = ..)
        dev = None
        for g in groups:
            for p in g['params']:
                dev = p.device if dev is None else dev
                if p.dtype != dt or p.device != dev or not p.is_contiguous() or p.numel() < 1:
                    self._check_params()  # says what is wrong
                gr = p.grad
                if gr is not None and (gr.dtype != dt or gr.device != dev or gr.shape != p.shape or not gr.is_contiguous()
                                       or gr.layout != torch.strided):
                    raise ValueError('optim.Adam: gradients must be contiguous %s tensors on the device of their '
                                     'parameter, got %s %s on %s' % (p.dtype, gr.dtype, tuple(gr.shape), gr.device))
                st = state.get(p) if gr is not None else None
                if st is not None:
                    n = p.numel()
                    for x in (st['exp_avg'], st['exp_avg_sq']):
                        if x.numel() != n or x.dtype != dt or x.device != dev or not x.is_contiguous():
                            raise ValueError('optim.Adam: exp_avg / exp_avg_sq must be contiguous %s tensors of their '
                                             'parameter\'s size on its device' % (dt,))
        fresh = [p for g in groups for p in g['params'] if p.grad is not None and p not in state]
        if fresh:
            self._new_state(fresh)
        prow, srow, numels, written, runs, advance = [], [], [], [], [], []
        for g, f in zip(groups, decay):
            for k in _TORCH_ONLY:  # a loaded or edited group may carry them
                if g.get(k):
                    self._check_group(g)
            lr, (b1, b2), eps, wd = g['lr'], g['betas'], g['eps'], g['weight_decay']
            hyper = (float(b1), float(b2), float(eps))
            f, wd = float(f), float(wd)
            scalars = {}  # step count -> (step_size, bc2_sqrt): torch's _single_tensor_adam, in Python doubles
            i0 = len(prow)
            for p in g['params']:
                n = p.numel()
                numels.append(n)
                gr = p.grad
                if gr is None:
                    prow.append((p.data_ptr(), 0, 0, 0, n, 0))
                    srow.append((1.0, 1.0, f, 0.0))
                    if f != 1.0:
                        written.append(p)
                    continue
                st = state[p]
                t = st['step'] + 1
                advance.append((st, t))
                s = scalars.get(t)
                if s is None:
                    s = scalars[t] = (lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5)
                prow.append((p.data_ptr(), gr.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), n, has_grad))
                srow.append((s[0], s[1], f, wd))
                written.append(p)
            i = len(prow)
            if i > i0:
                if runs and runs[-1][0] == hyper and runs[-1][2] == i0:
                    runs[-1][2] = i
                else:
                    runs.append([hyper, i0, i])
        if not written:
            return loss
        ptrs, scal = torch.tensor(prow, dtype=torch.int64), torch.tensor(srow, dtype=torch.float64)
        chunks, first = self._chunk_tables(numels, dev, hip)
        for st, t in advance:  # the counts move once the whole table stands: a refusal above leaves them alone
            st['step'] = t
        for (b1, b2, eps), a, b in runs:  # one launch per run of groups that share betas and eps: one, as a rule
            if not any(r[5] or q[2] != 1.0 for r, q in zip(prow[a:b], srow[a:b])):
                continue
            # rows keep their place in the tensor table (the chunk table names them by index): a run passes the whole
            # table and its own chunks; the rows of the other runs are not named by them
            ch = chunks[int(first[a]):int(first[b])]
            if hip:
                torch.ops.mmmot.adam_step(ch, ptrs, scal, b1, b2, eps)
            else:  # an injected backend (tests: the emulation of the C-ABI): the same call, HipOps.adam_step's signature
                ops.adam_step(ch, ptrs, scal, b1, b2, eps)
        # written through raw pointers: autograd and everything that keys on Tensor._version has to be told
        torch.autograd.graph.increment_version(written)
        return loss

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g['params']:
                if p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.requires_grad_(False)
                    p.grad.zero_()

    # ---- state in torch's format -------------------------------------------------------------------------------------
    def state_dict(self):
        index, groups, n = {}, [], 0
        for g in self.param_groups:
            packed = {k: v for k, v in g.items() if k != 'params'}
            packed['params'] = list(range(n, n + len(g['params'])))
            for j, p in enumerate(g['params']):
                index[id(p)] = n + j
            n += len(g['params'])
            groups.append(packed)
        state = {}
        for p, st in self.state.items():
            state[index[id(p)]] = {'step': torch.tensor(float(st['step'])), 'exp_avg': st['exp_avg'],
                                   'exp_avg_sq': st['exp_avg_sq']}
        return {'state': dict(sorted(state.items())), 'param_groups': groups}

    def load_state_dict(self, state_dict):
        saved = state_dict['param_groups']
        if len(saved) != len(self.param_groups):
            raise ValueError('optim.Adam: loaded state dict has a different number of parameter groups')
        if any(len(s['params']) != len(g['params']) for s, g in zip(saved, self.param_groups)):
            raise ValueError("optim.Adam: loaded state dict contains a parameter group that doesn't match the size of "
                             "optimizer's group")
        by_index, groups = {}, []
        for s, g in zip(saved, self.param_groups):
            new = {k: v for k, v in s.items() if k != 'params'}
            for k, v in self.defaults.items():
                new.setdefault(k, v)
            new['betas'] = tuple(new['betas'])
            new['params'] = g['params']
            self._check_group(new)
            groups.append(new)
            by_index.update(zip(s['params'], g['params']))
        state = {}
        for idx, st in state_dict['state'].items():
            p = by_index[idx]
            if 'max_exp_avg_sq' in st:
                raise ValueError('optim.Adam: the loaded state is that of amsgrad, which is not supported')
            step = st['step']  # a scalar tensor, or a plain int in older checkpoints
            step = float(step.item()) if torch.is_tensor(step) else float(step)
            if step != int(step) or step < 0:
                raise ValueError('optim.Adam: step count %r of parameter %r is not a whole number' % (step, idx))
            mv = [st[k].detach().to(device=p.device, dtype=p.dtype).contiguous().clone().view_as(p)
                  for k in ('exp_avg', 'exp_avg_sq')]
            state[p] = {'step': int(step), 'exp_avg': mv[0], 'exp_avg_sq': mv[1]}
        self.param_groups, self.state = groups, state

    def __repr__(self):
        return 'mmmot_amd.optim.Adam(%s)' % ', '.join(
            'group %d: %d tensors, lr %r, betas %r, eps %r, weight_decay %r' % (
                i, len(g['params']), g['lr'], g['betas'], g['eps'], g['weight_decay']) for i, g in enumerate(self.param_groups))


# ======================================================================================================================
# the wrapper: hyper-parameters of (non-norm, norm) group pairs and the decoupled decay
# (stands in for the OptimWrapper of reference utils/optim_util.py; written from its behaviour)
# ======================================================================================================================
def listify(p=None, q=None):
    """``p`` as a list with one entry per slot of ``q`` (a count, something sized, or None = as many as ``p`` has); a
    lone entry fills every slot.  Strings count as one value."""
    if p is None:
        items = []
    elif isinstance(p, str) or not isinstance(p, collections.abc.Iterable):
        items = [p]
    else:
        items = list(p)
    if q is None:
        slots = len(items)
    elif type(q) is int:
        slots = q
    else:
        slots = len(q)
    if len(items) == 1:
        items = items * slots
    if len(items) != slots:
        raise AssertionError('listify: %d values for %d slots' % (len(items), slots))
    return items


def leaf_modules(m):
    """The leaf modules of ``m`` in tree order; a module that has children contributes only them."""
    kids = list(m.children())
    return [m] if not kids else [leaf for c in kids for leaf in leaf_modules(c)]


def get_layer_groups(m):
    """ONE layer group holding the leaves of ``m``.  Parameters that a module with children holds directly are therefore
    in no group (kept as the reference has it)."""
    return [nn.Sequential(*leaf_modules(m))]


def _group_pair(layer_group):
    """(trainable parameters of the non-norm children, of the norm children) of one layer group."""
    plain, norm = [], []
    for child in layer_group.children():
        (norm if isinstance(child, NORM_TYPES) else plain).append(child)
    take = lambda mods: [p for p in nn.Sequential(*mods).parameters() if p.requires_grad]  # each tensor once
    return take(plain), take(norm)


class _Hyper:
    """One hyper-parameter of an OptimWrapper: reads as the LAST pair's value, a write goes to every pair (a scalar) or
    pair by pair (a sequence) and on into the inner optimizer's groups by the rule of ``OptimWrapper._push``."""

    def __init__(self, name):
        self.name = name

    def __get__(self, wrapper, owner=None):
        if wrapper is None:
            return self
        values = wrapper._hyper[self.name]
        return None if values is None else values[-1]

    def __set__(self, wrapper, value):
        if value is None and self.name == 'beta':
            return
        values = listify(value, len(wrapper._pairs))
        wrapper._hyper[self.name] = values
        wrapper._push(self.name)


class OptimWrapper:
    """An optimizer whose parameter groups come in (non-norm, norm) pairs, with ``lr``, ``mom``, ``beta`` and ``wd`` as
    attributes - one value per pair - and, with ``true_wd``, weight decay applied to the parameters themselves
    (``p *= 1 - wd*lr``) instead of through the gradient; ``bn_wd`` says whether the norm group of a pair decays."""
    lr, mom, beta, wd = _Hyper('lr'), _Hyper('mom'), _Hyper('beta'), _Hyper('wd')

    def __init__(self, opt, wd, true_wd=False, bn_wd=True):
        groups = opt.param_groups
        if len(groups) % 2:
            raise ValueError('OptimWrapper: the parameter groups must come in (non-norm, norm) pairs, got %d' % len(groups))
        self.opt, self.true_wd, self.bn_wd = opt, bool(true_wd), bool(bn_wd)
        self._pairs = [(i, i + 1) for i in range(0, len(groups), 2)]
        self.opt_keys = [k for k in groups[0] if k != 'params']
        first = [groups[i] for i, _ in self._pairs]  # the non-norm group speaks for its pair
        column = lambda key: [g[key] for g in first] if key in self.opt_keys else None
        betas = column('betas')
        self._hyper = {
            'lr': column('lr'),
            'mom': column('momentum') if betas is None else [b[0] for b in betas],
            'beta': column('alpha') if betas is None else [b[1] for b in betas],
            'wd': column('weight_decay'),
        }
        self.wd = wd

    # which key of the inner groups a hyper-parameter lands in: the first one the optimizer has
    _TARGETS = {'lr': ('lr',), 'mom': ('momentum', 'betas'), 'beta': ('betas', 'alpha'), 'wd': ('weight_decay',)}

    def _push(self, name):
        """Write the wrapper's values of ``name`` into the inner optimizer's groups."""
        key = next((k for k in self._TARGETS[name] if k in self.opt_keys), None)
        if key is None or (name == 'wd' and self.true_wd):  # decoupled decay never reaches the inner optimizer
            return
        if key == 'betas':
            values = list(zip(self._hyper['mom'], self._hyper['beta']))
        else:
            values = self._hyper[name]
        self._write(key, values, norm_too=self.bn_wd if name == 'wd' else True)

    def _write(self, key, values, norm_too=True):
        groups = self.opt.param_groups
        for value, (i, j) in zip(values, self._pairs):
            groups[i][key] = value
            if norm_too:
                groups[j][key] = value

    @classmethod
    def create(cls, opt_func, lr, layer_groups, **kwargs):
        """``opt_func(param_groups)`` over the (non-norm, norm) split of every layer group, wrapped."""
        rates = listify(lr, layer_groups)
        groups = []
        for rate, layer_group in zip(rates, layer_groups):
            groups += [{'params': ps, 'lr': rate} for ps in _group_pair(layer_group)]
        wrapper = cls(opt_func(groups), **kwargs)
        wrapper.lr = rates
        wrapper.opt_func = opt_func
        return wrapper

    def new(self, layer_groups):
        """The same optimizer kind and hyper-parameters over other layer groups."""
        return type(self).create(self.__dict__.get('opt_func', type(self.opt)), self.lr, layer_groups, wd=self.wd,
                                 true_wd=self.true_wd, bn_wd=self.bn_wd)

    def step(self):
        if not self.true_wd:
            return self.opt.step()
        groups = self.opt.param_groups
        fused = isinstance(self.opt, Adam)
        factors = [1.0] * len(groups)
        for lr, wd, (i, j) in zip(self._hyper['lr'], self._hyper['wd'], self._pairs):
            for k in (i, j) if self.bn_wd else (i,):
                factors[k] = 1 - wd * lr
        self._write('weight_decay', [0] * len(self._pairs))
        if fused:  # the decay rides in the step's launch
            return self.opt.step(decay=factors)
        with torch.no_grad():  # any other optimizer: one multiplication per parameter, then its own step
            for group, f in zip(groups, factors):
                if f != 1.0:
                    for p in group['params']:
                        p.mul_(f)
        return self.opt.step()

    def zero_grad(self):
        self.opt.zero_grad()

    def clear(self):
        """Forget the inner optimizer's state, keep its groups."""
        self.opt.load_state_dict({'state': {}, 'param_groups': self.opt.state_dict()['param_groups']})

    def __getattr__(self, name):
        # whatever the wrapper does not have is the inner optimizer's (param_groups, state_dict, ...); a name that one
        # lacks as well reads as None, as training scripts of the reference probe for optional attributes this way
        inner = self.__dict__.get('opt')
        if inner is None or name.startswith('__'):
            raise AttributeError(name)
        return getattr(inner, name, None)

    def __repr__(self):
        return 'OptimWrapper(true_wd=%s, bn_wd=%s) over %r' % (self.true_wd, self.bn_wd, self.opt)


# ======================================================================================================================
# the schedule: one cycle of lr and momentum (stands in for OneCycle of reference utils/learning_schedules_fastai.py)
# ======================================================================================================================
_Phase = collections.namedtuple('_Phase', 'begin end first last')  # iterations [begin, end), value first -> last


def _cosine(first, last, frac):
    """Half a cosine from ``first`` (frac = 0) to ``last`` (frac = 1).  The operation order is the reference's, so that
    the doubles are the same ones: tests/test_optim_cpu.py compares them with its recorded sequence to 1e-15."""
    swing = np.cos(np.pi * frac) + 1
    return float(last + (first - last) / 2 * swing)


def _track(total_step, knots, spans):
    """Phases of one quantity: ``knots`` are the fractions of ``total_step`` at which a phase begins, ``spans`` its (first,
    last) values; a phase ends where the next begins, the last one at ``total_step``."""
    if knots[0] != 0 or any(a >= b for a, b in zip(knots, knots[1:])):
        raise ValueError('phases must begin at 0 and in increasing order, got %r' % (knots,))
    edges = [int(k * total_step) for k in knots] + [total_step]
    return [_Phase(edges[i], edges[i + 1], *spans[i]) for i in range(len(knots))]


class OneCycle:
    """lr: lr_max / div_factor -> lr_max over the first ``pct_start`` of ``total_step`` iterations, then down to a
    ten-thousandth of the start value; momentum: moms[0] -> moms[1] and back - half cosines, set on ``fai_optimizer``
    (an OptimWrapper) by ``step(iteration)``."""

    def __init__(self, fai_optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.optimizer, self.total_step = fai_optimizer, total_step
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, moms, div_factor, pct_start
        low = lr_max / div_factor
        knots = [0, pct_start]
        self._tracks = {'lr': _track(total_step, knots, [(low, lr_max), (lr_max, low / 1e4)]),
                        'mom': _track(total_step, knots, [(moms[0], moms[1]), (moms[1], moms[0])])}
        self.current_lr = 0
        fai_optimizer.lr, fai_optimizer.mom = low, moms[0]

    def step(self, step):
        # every phase that has begun is evaluated and set, in order, so the latest one stands - and an earlier one is
        # still evaluated past its end (frac > 1) on the way: kept, the optimizer sees the same sequence of writes
        for name, phases in self._tracks.items():
            for ph in phases:
                if step < ph.begin:
                    continue
                value = _cosine(ph.first, ph.last, (step - ph.begin) / (ph.end - ph.begin))
                setattr(self.optimizer, name, value)
                if name == 'lr':
                    self.current_lr = value

    def get_lr(self):
        return self.current_lr


# ======================================================================================================================
# builders (reference utils/build_util.py:28-59)
# ======================================================================================================================
def _cfg(c, k):
    return c[k] if isinstance(c, dict) else getattr(c, k)


def build_lr_scheduler(config, optimizer):
    """``config``: the ``lr_scheduler`` section of the experiment's config (EasyDict or dict)."""
    kind = _cfg(config, 'type')
    if kind == 'one_cycle':
        return OneCycle(optimizer, _cfg(config, 'max_iter'), _cfg(config, 'lr_max'), list(_cfg(config, 'moms')),
                        _cfg(config, 'div_factor'), _cfg(config, 'pct_start'))
    if kind == 'constant':
        return None
    raise ValueError('build_lr_scheduler: unknown scheduler type %r' % (kind,))


def build_optim(net, config, ops=None):
    """``config``: the ``train`` section (``lr_scheduler.optim``, ``lr_scheduler.base_lr``, ``weight_decay``,
    ``fixed_wd``).  ``ops``: an injected operator backend (tests)."""
    sched = _cfg(config, 'lr_scheduler')
    name = _cfg(sched, 'optim')
    if name == 'AdaBound':
        raise NotImplementedError("optim 'AdaBound' is not available: the reference imports a module for it that it "
                                  "does not ship")
    if name != 'Adam':
        raise ValueError('build_optim: unknown optimizer %r' % (name,))
    opt_func = functools.partial(Adam, betas=(0.9, 0.99), ops=ops)
    return OptimWrapper.create(opt_func, _cfg(sched, 'base_lr'), get_layer_groups(net), wd=_cfg(config, 'weight_decay'),
                               true_wd=_cfg(config, 'fixed_wd'), bn_wd=True)
