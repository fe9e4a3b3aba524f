#!/usr/bin/env python
"""CPU trace (no GPU) of the engine's launch schedule through the torch emulation of the C-ABI (tests/fake_ops.py): one
line per operator call - method name, scalar arguments, and for every tensor argument dtype, shape, strides, storage
offset and WHICH storage it is (the `eng.ws` key, the path inside the packed weights, 'input', 'range_block' or
'fresh').  A host-side change of mmmot_amd/engine.py that claims "the same launches, in the same order, with the same
arguments, on the same workspace buffers" gives the same output byte for byte before and after; the last line is the
count of configurations and lines and the SHA-256 of everything above it.

    python tools/launch_trace.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys
import warnings
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from common import build_model, case_inputs, get_case, u8_crops  # noqa: E402
from fake_ops import TorchOps  # noqa: E402
from mmmot_amd import TrackingNet  # noqa: E402
from mmmot_amd.synth import make_pair  # noqa: E402
from mmmot_amd.weights import generate_state_dict_trained  # noqa: E402


def _storage(t):
    return t.untyped_storage().data_ptr()


def _paths(obj, prefix, out):
    """storage -> path of every tensor inside the packed weights (dicts / lists of tensors)"""
    if torch.is_tensor(obj):
        out.setdefault(_storage(obj), prefix)
    elif isinstance(obj, dict):
        for k in obj:
            _paths(obj[k], '%s.%s' % (prefix, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _paths(v, '%s.%d' % (prefix, i), out)
    return out


class LaunchTrace:
    """Operator backend proxy like tests/common.py::CallLog that records the arguments too."""
    _quiet = ('name', 'on_current_stream', 'on_stream')

    def __init__(self, ops, eng, lines):
        self.ops, self.eng, self.lines = ops, eng, lines
        self.inputs = {}

    def __getattr__(self, k):
        v = getattr(self.ops, k)
        if k in self._quiet or k.startswith('_') or not callable(v):
            return v

        def call(*a, **kw):
            weights = _paths(self.eng.P, 'weights', {})
            args = [self._show(k, x, weights) for x in a] + ['%s=%s' % (n, self._show(k, kw[n], weights)) for n in sorted(kw)]
            self.lines.append('%s(%s)' % (k, ', '.join(args)))
            return v(*a, **kw)
        return call

    def _show(self, method, x, weights):
        if torch.is_tensor(x):
            s = _storage(x)
            where = next((repr(key) for key, t in self.eng.ws.items() if _storage(t) == s), None)
            if where is None:
                where = 'range_block' if method == 'trunk_range_bind' else weights.get(s) or self.inputs.get(s, 'fresh')
            return '<%s %s %s +%d @%s>' % (str(x.dtype)[6:], list(x.shape), list(x.stride()), x.storage_offset(), where)
        if isinstance(x, dict):
            return '{%s}' % ', '.join('%s: %s' % (n, self._show(method, x[n], weights)) for n in sorted(x))
        if isinstance(x, (list, tuple)):
            return '[%s]' % ', '.join(self._show(method, v, weights) for v in x)
        if x is None or isinstance(x, (bool, int, float, str)):
            return repr(x)
        # a tile / segment table of the plan: its class, sizes and a checksum of its host arrays
        crc, sizes = 0, []
        for n in sorted(vars(x)):
            v = getattr(x, n)
            if n.startswith('h_') and isinstance(v, np.ndarray):
                crc = zlib.crc32(np.ascontiguousarray(v).tobytes(), zlib.crc32(n.encode(), crc))
            elif isinstance(v, (bool, int)):
                sizes.append('%s=%d' % (n, v))
        return '%s(%s #%08x)' % (type(x).__name__, ' '.join(sizes), crc)


def _crc(out):
    c = 0
    for t in out:
        for u in (t if isinstance(t, (list, tuple)) else [t]):
            if torch.is_tensor(u):
                c = zlib.crc32(u.detach().contiguous().numpy().tobytes(), c)
    return '%08x' % c


def traced(name, trunk, lines, env=None, **knobs):
    """model of golden case `name` on a traced TorchOps backend; `env`: MMMOT_* switches read when the engine is built"""
    c, base = get_case(name)
    m = build_model(c, base, ops=TorchOps())
    return _trace(m, trunk, lines, env, knobs), c


def _trace(m, trunk, lines, env, knobs):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        m.set_trunk(trunk)
        eng = m.engine()
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    for k, v in knobs.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    eng.ops = LaunchTrace(eng.ops, eng, lines)
    return m


def step(m, lines, what, call, *inputs):
    """one traced call: its launches, then the checksum of what it returned and the guard's results"""
    eng = m.engine()
    eng.ops.inputs = {}
    for t in inputs:
        for u in (t.values() if isinstance(t, dict) else [t]):
            if torch.is_tensor(u):
                eng.ops.inputs[_storage(u)] = 'input'
    lines.append('-- ' + what)
    with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = call()
    for w in caught:
        lines.append('warning at %s: %s' % (os.path.basename(w.filename), w.message))
    out = list(out.values()) if isinstance(out, dict) else [out.rows] if hasattr(out, 'rows') else out
    out = out if isinstance(out, (list, tuple)) else [out]
    lines.append('-> %s trunk=%s events=%d window=%r last=%r' % (_crc(out), eng.trunk, len(eng.range_events),
                                                                eng.out_of_range_window, eng.last_out_of_range_forward))
    return out


MATRIX = [  # tests/test_workspace_poison_cpu.py CASES, and the switches it leaves out
    ('s1_C_minus_abs_dual_add', 'f16x3', {}),
    ('s6_endmax_A', 'f32', {}),
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0}),
    ('s5_3frames_B', 'f16x3', {}),
    ('s6_endmax_C', 'f16x3', {'pn_gram': False}),
    ('s6_endmax_C', 'f16x3', {'pn_fused': False}),
    ('s6_endmax_C', 'f16x3', {'fuse_conv1': False, 'sp_fused': False}),
    ('s6_endmax_C', 'f16x3', {'pn_mlp64': False}),
    ('s6_endmax_C', 'f32', {'pn_fused': False}),
    ('s6_endmax_C', 'f16q8', {}),
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0, 'q8_layers': None}),
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0, 'fuse_conv1': False}),
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0, 'q8_layers': None, 'fuse_conv1': False}),
    ('s6_endmax_C', 'f16q8', {'q8_min_crop': 0, 'q8_layers': {1, 2, 5, 6, 12}}),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    args = ap.parse_args()
    torch.set_num_threads(8)
    lines, n = [], 0

    def config(title):
        nonlocal n
        n += 1
        lines.append('==== %d: %s' % (n, title))

    for name, trunk, knobs in MATRIX:
        config('%s %s %r, two forwards' % (name, trunk, sorted(knobs.items(), key=str)))
        m, c = traced(name, trunk, lines, **knobs)
        dets, info, ds = case_inputs(c)
        for i in range(2):
            step(m, lines, 'forward %d' % i, lambda: m(dets, info, ds), dets, info)

    for trunk, knobs in (('f16x3', {}), ('f16x3', {'fuse_conv1': False}), ('f32', {}),
                         ('f16q8', {'q8_min_crop': 0, 'q8_layers': None}),
                         ('f16q8', {'q8_min_crop': 0, 'fuse_conv1': False})):
        config('uint8 crops %s %r' % (trunk, sorted(knobs.items())))
        m, c = traced('s6_endmax_C', trunk, lines, **knobs)
        dets, info, ds = case_inputs(c)
        u8 = u8_crops(dets)
        for i in range(2):
            step(m, lines, 'forward %d' % i, lambda: m(u8, info, ds), u8, info)

    for rows in ((0,), (1,)):
        config('rows %r' % (rows,))
        m, c = traced('s6_endmax_C', 'f16x3', lines)
        dets, info, ds = case_inputs(c)
        step(m, lines, 'forward_rows', lambda: m.forward_rows(dets, info, ds, rows=rows), dets, info)

    config('appearance rows: encode, forward(appearance=) shapes (a) and (b), forward_appearance, image_first')
    m, c = traced('s6_endmax_C', 'f16x3', lines)
    dets, info, ds = case_inputs(c)
    N = int(ds[0])
    pts = info['points'].reshape(-1, 3).contiguous()
    plan = m.make_plan([([int(d) for d in ds], info['points_split'].reshape(-1).long().numpy())], c['S'])
    eng = m.engine()
    enc = step(m, lines, 'encode_appearance', lambda: m.encode_appearance(dets), dets)[0]
    step(m, lines, 'shape (a)', lambda: eng.forward(plan, None, pts, appearance=enc), pts, enc)
    head, tail = enc[:N].clone(), dets[N:].contiguous()
    step(m, lines, 'shape (b)', lambda: eng.forward(plan, tail, pts, appearance=head), pts, tail, head)
    step(m, lines, 'forward_appearance', lambda: m.forward_appearance(m.encode_appearance(dets[:N]), dets[N:], info, ds),
         dets, info)
    step(m, lines, 'image_first + forward', lambda: (eng.image_first(plan, dets), eng.forward(plan, dets, pts))[1],
         dets, pts)
    step(m, lines, 'image_first (b) + forward', lambda: (eng.image_first(plan, tail, appearance=head),
                                                         eng.forward(plan, tail, pts, appearance=head))[1], pts, tail, head)
    step(m, lines, 'Engine.encode', lambda: eng.encode(plan, dets)[0], dets)

    for trunk, env in (('f16x3', {}), ('f16q8', {}), ('f16q8', {'MMMOT_RANGE_CHECK_EVERY': '2'}),
                       ('f16q8', {'MMMOT_RANGE_GUARD': '0'})):
        config('consecutive forwards %s %r' % (trunk, sorted(env.items())))
        m, c = traced('s6_endmax_C', trunk, lines, env=env, q8_min_crop=0)
        dets, info, ds = case_inputs(c)
        for i in range(5 if env else 3):
            step(m, lines, 'forward %d' % i, lambda: m(dets, info, ds), dets, info)

    # weights that leave the fp16 range (the 'wild' profile of tests/test_robust_cpu.py): the guard recomputes the first
    # forward; then a model that leaves the range later (bias of conv3_1 raised under the live engine): detected late
    kw = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True,
              appear_fpn=False, point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg',
              test_mode=2, neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='A',
              affinity_op='multiply', softmax_mode='none')
    for title, profile, late in (('wild weights trip the guard on the first forward', 'wild', False),
                                 ('weights leave the range at the third forward', 'calibrated', True)):
        config(title)
        m = TrackingNet(**kw)
        sd = generate_state_dict_trained(m.state_dict(), 0, profile)
        dets, info, ds = make_pair(2, 2, 64, 12, seed=4000, ragged=True)
        if late:
            from mmmot_amd.weights import calibrate_bn
            calibrate_bn(sd, make_pair(4, 4, 64, 4, seed=4100)[0])
        m.load_state_dict(sd)
        m.eval()
        m.set_ops(TorchOps())
        m = _trace(m, 'f16q8', lines, None, {})
        for i in range(5 if late else 2):
            if late and i == 2:
                cv = m.engine().P['vgg'][4]
                cv['bias'] = cv['bias'] + 3000.0
            step(m, lines, 'forward %d' % i, lambda: m(dets, info, ds), dets, info)
        if late:
            step(m, lines, 'encode_appearance', lambda: m.encode_appearance(dets), dets)
            lines.append('appearance_is_current %r' % m.appearance_is_current(m.encode_appearance(dets)))

    body = '\n'.join(lines) + '\n'
    body += '%d configurations, %d lines, sha256 %s\n' % (n, len(lines), hashlib.sha256(body.encode()).hexdigest())
    if args.out:
        with open(args.out, 'w') as f:
            f.write(body)
    else:
        sys.stdout.write(body)
    sys.stderr.write(body.splitlines()[-1] + '\n')


if __name__ == '__main__':
    main()
