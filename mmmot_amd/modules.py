"""Drop-in ``nn.Module`` mirror of the reference network API.

Same constructor keywords, same ``state_dict`` keys / shapes, same
``forward(dets, det_info, dets_split)`` signature and return tuple as reference
modules/tracking_net.py:17-35,165-193 - so ``tracking_model.py`` /
``eval_seq.py`` keep working when ``build_model`` imports ``TrackingNet`` from
here.  The torch sub-modules below are *parameter containers only* (they give
the reference key names and ``load_state_dict`` semantics); none of their
``forward`` methods is ever called.  All arithmetic happens in
libmmmot_hip.so through ``Engine``; CPU tensors are rejected (no fallback).

The north-star path is the eval-mode forward.  ``train()`` / ``eval()`` record
the flag like any ``nn.Module`` (the reference's ``TrackingModule`` toggles them
around validation, tracking_model.py:32-48, eval_seq.py:127).  In training mode
``forward`` is the differentiable forward of mmmot_amd/train.py (batch-statistics
BatchNorm, backward kernels behind autograd); the batched, single-modality and
appearance-row entry points stay eval-only and raise.  After an optimizer step
``refresh_head`` / ``refresh_head_device`` bring the packed head up to date; the
next eval-mode forward re-packs whatever else was trained.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import torch_ops
from .engine import Engine, check_crop_layout
from .pack import FUSION_LAYOUT, LINK_LAYOUT, VGG_STAGES, build_head, pack_weights
from .plan import BatchPlan, CropPlan, PlanCache


def _gn(groups, ch):
    return nn.GroupNorm(groups, ch)


class SkipPool(nn.Module):
    """Parameter layout of reference modules/appear_net.py:9-32 (``fc`` indices 0,1,2,4,5)."""

    def __init__(self, channels, reduction, out_channels, dropblock_size=0):
        super().__init__()
        mid = max(channels // reduction, 64)
        self.channels = channels
        self.fc = nn.Sequential(_gn(1, channels), nn.Conv2d(channels, mid, 1), _gn(1, mid), nn.ReLU(inplace=True),
                                nn.Conv2d(mid, out_channels, 1), _gn(1, out_channels), nn.ReLU(inplace=True))


class AppearanceNet(nn.Module):
    """VGG16-BN + SkipPool image-crop encoder (reference modules/appear_net.py:35-59,130-190)."""

    def __init__(self, arch='vgg', out_channels=512, skippool=True, fpn=False, dropblock=0):
        super().__init__()
        if arch != 'vgg' or not skippool or fpn or out_channels != 512:
            raise NotImplementedError('HIP path builds the vgg16_bn_512 + skippool encoder only '
                                      '(every shipped config; resnet/fpn branches need torchvision downloads)')
        self.arch, self.skippool, self.fpn, self.out_channels, self.dropblock = arch, skippool, fpn, out_channels, dropblock
        stages, heads = [], []
        for stage in VGG_STAGES:
            mods = []
            for (_, cin, cout, pool) in stage:
                mods += [nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU(inplace=True)]
                if pool:
                    mods.append(nn.MaxPool2d(2, 2))
            stages.append(nn.Sequential(*mods))
            heads.append(SkipPool(stage[-1][2], 4, out_channels // 4, 0))
        self.layers = nn.ModuleList(stages)
        self.global_pool = nn.ModuleList(heads)
        self._engine = None

    def forward(self, x):
        """x: L x 3 x S x S crops -> L x 512 (HIP)."""
        eng = _standalone_engine(self, 'appearance.')
        L, S = x.shape[0], x.shape[-1]
        plan = BatchPlan(_dummy_samples(L), S, x.device, use_points=False)
        return torch.ops.mmmot.appearance(x.contiguous(), torch_ops.engine_handle(eng), torch_ops.plan_handle(plan))


class STN3d(nn.Module):
    """Parameter layout of reference modules/point_net.py:47-70."""

    def __init__(self, in_channels, out_size=3, feature_channels=512):
        super().__init__()
        self.out_size = out_size
        self.conv1 = nn.Conv1d(in_channels, 64, 1)
        self.bn1 = _gn(64, 64)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.bn2 = _gn(128, 128)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.bn3 = _gn(1024, 1024)
        self.idt = nn.Parameter(torch.eye(out_size), requires_grad=False)
        self.fc1 = nn.Linear(1024, 512)
        self.fc_bn1 = _gn(512, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc_bn2 = _gn(256, 256)
        self.output = nn.Linear(256, out_size * out_size)
        nn.init.zeros_(self.output.weight)
        nn.init.zeros_(self.output.bias)


class PointNetfeatGN(nn.Module):
    """Parameter layout of reference modules/point_net.py:89-113."""

    def __init__(self, in_channels=3, out_channels=512, global_feat=True):
        super().__init__()
        self.stn1 = STN3d(in_channels, in_channels, out_channels)
        self.conv1 = nn.Conv1d(in_channels, 64, 1)
        self.bn1 = _gn(64, 64)
        self.conv2 = nn.Conv1d(64, 64, 1)
        self.bn2 = _gn(64, 64)
        self.stn2 = STN3d(64, 64, out_channels)
        self.conv3 = nn.Conv1d(64, 64, 1)
        self.bn3 = _gn(64, 64)
        self.conv4 = nn.Conv1d(64, 128, 1)
        self.bn4 = _gn(128, 128)
        self.conv5 = nn.Conv1d(128, 1024, 1)
        self.bn5 = _gn(1024, 1024)


class PointNet_v1(nn.Module):
    """LiDAR encoder (reference modules/point_net.py:5-44)."""

    def __init__(self, in_channels, out_channels=512, use_dropout=False):
        super().__init__()
        if in_channels not in (3, 4) or out_channels != 512:
            raise NotImplementedError('HIP path builds PointNet_v1(3 | 4 -> 512) (point_len=512)')
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.feat = PointNetfeatGN(in_channels, out_channels)
        self.conv1 = nn.Conv1d(1088, 512, 1)
        self.conv2 = nn.Conv1d(512, out_channels, 1)
        self.bn1 = _gn(512, 512)
        self.bn2 = _gn(16, out_channels)
        self.avg_bn = _gn(512, 512)  # unused by the reference forward too; kept for key parity
        # point_net.py:18-21,29-30: identity in eval mode; in training mode the pool behind it drops on the device
        # (mmmot_amd/train.py).  No parameters: the state_dict keys do not depend on the flag
        self.dropout = nn.Dropout(p=0.5) if use_dropout else None

    def forward(self, x, point_split):
        """x: 1 x 3 x P, point_split: (L+1,) -> (L x 512, [1x3x3, 1x64x64]) (HIP)."""
        eng = _standalone_engine(self, 'point_net.')
        ps = point_split.detach().cpu().numpy().astype(np.int64)
        L = ps.shape[0] - 1
        plan = BatchPlan([(_dummy_samples(L)[0][0], ps)], 32, x.device)
        feat = torch.ops.mmmot.pointnet(x[0].t().contiguous(), torch_ops.engine_handle(eng), torch_ops.plan_handle(plan))
        pn = eng.P['pointnet']
        return feat, [pn['trans1'].unsqueeze(0).clone(), pn['trans2'].unsqueeze(0).clone()]


def _conv_gn(cin, cout, groups):
    return nn.Sequential(nn.Conv1d(cin, cout, 1, 1), _gn(groups, cout))


class _FusionBase(nn.Module):
    mode = None

    def forward(self, objs):
        """objs: 1 x 2D x L -> 3 x D x L (HIP)."""
        eng = _standalone_engine(self, 'fusion_module.', fusion=self.mode)
        L = objs.shape[-1]
        plan = BatchPlan(_dummy_samples(L), 32, objs.device, use_points=False)
        eng.dev = objs.device
        cat = eng.buf('cat', L, 1024)
        cat.copy_(objs[0].t())
        F = eng.buf('F', 3, L, 512)
        eng.fuse(plan, cat, F)
        return F.permute(0, 2, 1).contiguous()


class fusion_module_A(_FusionBase):
    """reference modules/fusion_net.py:73-92"""
    mode = 'A'

    def __init__(self, appear_len, point_len, out_channels):
        super().__init__()
        self.appear_len, self.point_len = appear_len, point_len
        self.input_w = _conv_gn(out_channels * 2, out_channels, out_channels)


class fusion_module_B(_FusionBase):
    """reference modules/fusion_net.py:45-70"""
    mode = 'B'

    def __init__(self, appear_len, point_len, out_channels):
        super().__init__()
        self.appear_len, self.point_len = appear_len, point_len
        self.input_p = _conv_gn(out_channels, out_channels, out_channels)
        self.input_i = _conv_gn(out_channels, out_channels, out_channels)


class fusion_module_C(_FusionBase):
    """reference modules/fusion_net.py:6-42"""
    mode = 'C'

    def __init__(self, appear_len, point_len, out_channels):
        super().__init__()
        self.appear_len, self.point_len = appear_len, point_len
        self.gate_p = nn.Sequential(nn.Conv1d(point_len, point_len, 1, 1), nn.Sigmoid())
        self.gate_i = nn.Sequential(nn.Conv1d(appear_len, appear_len, 1, 1), nn.Sigmoid())
        self.input_p = _conv_gn(point_len, out_channels, out_channels)
        self.input_i = _conv_gn(appear_len, out_channels, out_channels)


FUSION_CLASSES = {'A': fusion_module_A, 'B': fusion_module_B, 'C': fusion_module_C}


class NewEndIndicator_v2(nn.Module):
    """Parameter layout of reference modules/new_end.py:43-60."""

    def __init__(self, in_channels, kernel_size=5, reduction=4, mode='avg'):
        super().__init__()
        self.mode = mode
        mid = min(in_channels, 512)
        self.conv0 = nn.Sequential(nn.Conv2d(in_channels, in_channels, 1, 1), _gn(1, in_channels), nn.ReLU(inplace=True))
        self.conv1 = nn.Sequential(nn.Conv1d(in_channels, mid, 1, 1), _gn(1, mid), nn.ReLU(inplace=True),
                                   nn.Conv1d(mid, in_channels // reduction, 1, 1), _gn(1, in_channels // reduction),
                                   nn.ReLU(inplace=True), nn.Conv1d(in_channels // reduction, 1, 1, 1), nn.Sigmoid())


class affinity_module(nn.Module):
    """Pairwise affinity + new/end heads (reference modules/gcn.py:45-82)."""

    def __init__(self, in_channels, new_end=None, affinity_op='multiply'):
        super().__init__()
        if in_channels != 512:
            raise NotImplementedError('HIP path builds the 512-channel affinity module')
        self.in_channels = in_channels
        self.affinity_op = affinity_op
        self.w_new_end = new_end(in_channels) if new_end is not None else NewEndIndicator_v2(in_channels)
        c = in_channels
        self.conv1 = nn.Sequential(nn.Conv2d(c, c, 1, 1), _gn(c, c), nn.ReLU(inplace=True),
                                   nn.Conv2d(c, c, 1, 1), _gn(c, c), nn.ReLU(inplace=True),
                                   nn.Conv2d(c, c // 4, 1, 1), _gn(c // 4, c // 4), nn.ReLU(inplace=True),
                                   nn.Conv2d(c // 4, 1, 1, 1))

    def forward(self, objs, dets):
        """objs R x D x N, dets R x D x M -> (R x 1 x N x M logits, R x M new, R x N end) (HIP)."""
        eng = _standalone_engine(self, 'w_link.', affinity_op=self.affinity_op)
        R, _, N = objs.shape
        M = dets.shape[-1]
        plan = BatchPlan([([N, M], None)], 32, objs.device, rows=tuple(range(R)), use_points=False)
        eng.dev = objs.device
        F = eng.buf('F', R, N + M, 512)
        F[:, :N].copy_(objs.permute(0, 2, 1))
        F[:, N:].copy_(dets.permute(0, 2, 1))
        link, new, end = eng.affinity(plan, F)
        return link.view(R, 1, N, M), new[:, N:].clone(), end[:, :N].clone()


def _dummy_samples(L):
    """One sample of L detections split over two frames (sub-module calls carry no frame split)."""
    if L < 2:
        raise ValueError('stand-alone sub-module calls need >= 2 detections')
    return [([L // 2, L - L // 2], None)]


def _standalone_engine(module, prefix, **cfg):
    """Engine for calling a sub-module on its own (module-level parity tests)."""
    ver = tuple(p._version for p in module.state_dict().values())
    cache = getattr(module, '_eng_cache', None)
    if cache is None or cache[0] != ver:
        from .ops import HipOps
        dev = next(module.parameters()).device
        sd = {prefix + k: v for k, v in module.state_dict().items()}
        packed = pack_weights(sd, cfg.get('fusion', 'A'), dev)
        eng = Engine(packed, HipOps(), **cfg)
        object.__setattr__(module, '_eng_cache', (ver, eng))
        cache = module._eng_cache
    return cache[1]


def _collect_tensors(obj, out=None):
    """every tensor reachable through dicts / lists / tuples of a packed-weight tree"""
    out = [] if out is None else out
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _collect_tensors(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _collect_tensors(v, out)
    return out


def _copy_packed_(dst, src):
    """Copy the packed tree ``src`` into ``dst`` in place (same keys / shapes / dtypes); False when they differ."""
    if torch.is_tensor(dst):
        if not torch.is_tensor(src) or dst.shape != src.shape or dst.dtype != src.dtype or dst.device != src.device:
            return False
        dst.copy_(src)
        return True
    if isinstance(dst, dict):
        if not isinstance(src, dict) or dst.keys() != src.keys():
            return False
        ok = True
        for k in dst:
            if torch.is_tensor(dst[k]) or isinstance(dst[k], (dict, list, tuple)):
                ok = _copy_packed_(dst[k], src[k]) and ok
            elif dst[k] != src[k]:
                dst[k] = src[k]  # python scalars (scales): the kernels take them by value at launch time ...
                ok = False       # ... so a captured launch keeps the old one
        return ok
    if isinstance(dst, (list, tuple)):
        if not isinstance(src, (list, tuple)) or len(dst) != len(src):
            return False
        return all([_copy_packed_(d, s_) for d, s_ in zip(dst, src)])
    return dst == src


class PackSnapshot:
    """What a live engine was packed from: EVERY parameter and buffer of the model, their versions at packing time, and
    which of them belong to the head modules (the head's versions alone miss encoder-only training and the
    'eval, one training step, eval' flow).  The tensor list is kept so that the per-forward check is one list
    comprehension (25 us), not a module walk (0.4 ms)."""

    def __init__(self, model, heads):
        head = set()
        for name in heads:
            m = getattr(model, name)
            head.update(id(t) for t in list(m.parameters()) + list(m.buffers()))
        self.tensors = list(model.parameters()) + list(model.buffers())
        self.versions = [t._version for t in self.tensors]
        self.head = [i for i, t in enumerate(self.tensors) if id(t) in head]

    def head_is_current(self):
        return all(self.tensors[i]._version == self.versions[i] for i in self.head)

    def head_refreshed(self):
        """the head was packed again from the live tensors; the encoders keep their versions"""
        for i in self.head:
            self.versions[i] = self.tensors[i]._version


def graph_stale_reason(engine_then, engine_now, pack_version_then, pack_version_now, trained_since_pack, packed_is_current):
    """Why a captured forward may not be replayed any more (None: it may).  A replay launches exactly what was captured,
    on the packed weights of capture time, and runs none of the eval entry points' checks - so everything they guard
    against (``TrackingNet._repack_if_trained``) has to be refused here:
      - the engine was replaced or its packed tensors were (load_state_dict / invalidate / set_trunk / .to(), a head
        refresh that could not be done in place, refresh_head_device): the graph computes with tensors the model dropped;
      - ``trained_since_pack``: a training step refreshed the fp32 head on the device, the fp16-split copies are stale;
      - not ``packed_is_current``: a parameter or buffer was modified in place (optimizer.step(), a training-mode
        BatchNorm update, by hand) and nothing was re-packed yet - the replay would return the OLD weights' scores."""
    if engine_now is not engine_then or pack_version_now != pack_version_then:
        return ('the model was re-packed (load_state_dict / invalidate / set_trunk / .to() / a training step) after '
                'capture(); capture again')
    if trained_since_pack:
        return ('a training step left the packed fp16-split copies of the head stale (refresh_head() does not clear '
                'that); the next eval forward re-packs the model - capture again after it')
    if not packed_is_current:
        return ('a parameter or buffer was modified in place after it was packed; call refresh_head() if only the head '
                '(fusion_module, w_det, w_link) changed, else run an eval forward (which re-packs) and capture again')
    return None


def check_graph_inputs(crops_buf, points_buf, crops, points):
    """Host check of the inputs of a replay against the captured buffers, BEFORE anything is copied: ``copy_`` would
    broadcast a [1,3,S,S] tensor over [Lt,3,S,S] and convert fp32 crops into a uint8 buffer (and back) without a word,
    where the eager forward refuses both (Engine._check_crops).  None = keep what the buffer holds."""
    for name, buf, t in (('crops', crops_buf, crops), ('points', points_buf, points)):
        if t is None:
            continue
        if buf is None:
            raise ValueError('%s given to a captured forward that was captured without %s' % (name, name))
        if not torch.is_tensor(t) or t.shape != buf.shape or t.dtype != buf.dtype:
            raise ValueError('%s of a captured forward must be a %s %s tensor (the shape and type it was captured with), '
                             'got %s' % (name, buf.dtype, list(buf.shape),
                                         '%s %s' % (t.dtype, list(t.shape)) if torch.is_tensor(t) else type(t).__name__))


class GraphedForward:
    """See ``TrackingNet.capture``."""

    def __init__(self, model, plan, crops, points):
        self.plan = plan
        self.crops = None if crops is None else crops.clone()
        self.points = None if points is None else points.clone()
        model._repack_if_trained()  # here, not inside the warm-up: the engine taken below is the one that gets captured
        eng = model.engine()
        with torch.no_grad():
            model.forward_batch(plan, self.crops, self.points)   # warm-up: workspace allocation, range-guard check
            torch.cuda.synchronize()
            # (the range guard sees the capture and only binds the engine's counter block: check_range() reads it)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.result = model.forward_batch(plan, self.crops, self.points)
        # the graph holds raw pointers into the engine's packed weights and workspace arena: keep BOTH alive (every
        # tensor of eng.P and eng.ws at capture time) even if the model is re-packed or a later, larger forward
        # re-allocates workspace buffers - a replay then reads valid memory.  It would still compute with the weights
        # of capture time, so a re-pack that could not be done in place (invalidate / load_state_dict / set_trunk / a
        # head refresh that changed shapes) marks the graph stale: __call__ raises instead of silently replaying it.
        # refresh_head() itself copies into the packed tensors IN PLACE, so a graph follows an optimizer step once
        # refresh_head() was called; until then (parameters edited, nothing re-packed) the graph is stale as well.
        self._engine = eng
        self._model = model
        self._pack_version = model._pack_version
        self._keep = list(eng.ws.values()) + _collect_tensors(eng.P) + [eng.guard.block]

    def stale_reason(self):
        m = self._model
        return graph_stale_reason(self._engine, m._engine, self._pack_version, m._pack_version,
                                  m._trained_since_pack, m._packed_is_current())

    def stale(self):
        return self.stale_reason() is not None

    def check_range(self):
        """The trunk's range guard never runs inside a replay (its counter read synchronises): call this now and then
        when serving from a graph.  Returns the counters (e4m3-saturated, fp16-clamped, conv1_1 hits) accumulated by
        this engine since the last check and raises if the captured arithmetic left its range (re-capture after
        ``model.set_trunk('f32')`` or with rescaled inputs)."""
        eng = self._engine
        sat, clamp, c11 = eng.guard.read(reset=True)
        if clamp > 0 or (c11 > 0 and eng.trunk != 'f16q8'):
            raise RuntimeError('mmmot_amd: %d activation elements left the fp16 range inside a captured forward (trunk %s): '
                               'the replayed results are wrong; lower the trunk (set_trunk) and capture again'
                               % (clamp + c11, eng.trunk))
        return sat, clamp, c11

    def __call__(self, crops=None, points=None):
        why = self.stale_reason()
        if why is not None:
            raise RuntimeError('mmmot_amd: this captured forward is stale - ' + why)
        check_graph_inputs(self.crops, self.points, crops, points)
        if crops is not None and crops.data_ptr() != self.crops.data_ptr():
            self.crops.copy_(crops, non_blocking=True)
        if points is not None and points.data_ptr() != self.points.data_ptr():
            self.points.copy_(points, non_blocking=True)
        self.graph.replay()
        return self.result


class StaleAppearanceError(ValueError):
    """Appearance rows whose stamp no longer holds (TrackingNet.appearance_is_current): encode the frame again."""


class AppearanceRows:
    """Owned appearance rows of one frame's crops (``rows``: fp32 [L, 512] on the model's device, the image branch's
    output) and the stamp they are valid under: ``stamp`` = (pack version, engine serial, trunk arithmetic, engine
    forward index the rows were computed in, range events recorded by then).  See TrackingNet.encode_appearance."""
    __slots__ = ('rows', 'stamp')

    def __init__(self, rows, stamp):
        self.rows, self.stamp = rows, stamp

    def __len__(self):
        return int(self.rows.shape[0])

    def split(self, counts):
        """per-frame AppearanceRows of rows encoded for several frames at once (views of this owned tensor)"""
        out, r = [], 0
        for n in counts:
            out.append(AppearanceRows(self.rows[r:r + int(n)], self.stamp))
            r += int(n)
        return out


class TrackingNet(nn.Module):
    """Reference-compatible tracking network (modules/tracking_net.py:15-193), HIP forward."""

    def __init__(self, seq_len, appear_len=512, appear_skippool=False, appear_fpn=False, score_arch='vgg',
                 score_fusion_arch='C', appear_arch='vgg', point_arch='v1', point_len=512,
                 softmax_mode='single', test_mode=0, affinity_op='multiply', dropblock=5, end_arch='v2',
                 end_mode='avg', without_reflectivity=True, neg_threshold=0, use_dropout=False):
        super().__init__()
        if appear_len != 512 or point_len != 512 or point_arch != 'v1' or end_arch != 'v2':
            raise NotImplementedError('HIP path covers appear_len=point_len=512, point_arch=v1, end_arch=v2 '
                                      '(all shipped configs); single-modality runs use forward_rows()')
        if score_arch not in ('branch_cls', 'branch_reg'):
            raise NotImplementedError("score_arch must be 'branch_cls' or 'branch_reg' (reference builds no w_det otherwise)")
        if score_fusion_arch not in FUSION_CLASSES:
            raise ValueError('unknown score_fusion_arch %r' % (score_fusion_arch,))
        self.seq_len = seq_len
        self.score_arch = score_arch
        self.neg_threshold = neg_threshold
        self.test_mode = test_mode  # read by the host tracker (tracking_model.py:19-22)
        self.softmax_mode = softmax_mode
        self.affinity_op = affinity_op
        self.score_fusion_arch = score_fusion_arch
        self.end_mode = end_mode
        self.fusion_module = FUSION_CLASSES[score_fusion_arch](appear_len, point_len, out_channels=point_len)
        self.appearance = AppearanceNet(appear_arch, appear_len, skippool=appear_skippool, fpn=appear_fpn,
                                        dropblock=dropblock)
        self.point_net = PointNet_v1(4 - int(without_reflectivity), out_channels=point_len, use_dropout=use_dropout)
        self.w_link = affinity_module(
            point_len, new_end=lambda c: NewEndIndicator_v2(c, kernel_size=5, reduction=4, mode=end_mode),
            affinity_op=affinity_op)
        c = point_len
        self.w_det = nn.Sequential(nn.Conv1d(c, c, 1, 1), nn.BatchNorm1d(c), nn.ReLU(inplace=True),
                                   nn.Conv1d(c, c // 2, 1, 1), nn.BatchNorm1d(c // 2), nn.ReLU(inplace=True),
                                   nn.Conv1d(c // 2, 1, 1, 1))
        self.trunk = os.environ.get('MMMOT_TRUNK', 'f16x3')
        self._ops = None       # operator backend (HipOps unless a test injects another)
        self._engine = None
        self._engine_key = None
        self._plans = PlanCache(64)        # BatchPlans of the reference-shaped call, keyed by the whole sample layout
        self._img_plans = PlanCache(256)   # image-only plans of forward()'s trunk-first launch, by (frame counts, crop side)
        self._crop_plans = PlanCache(256)  # CropPlans of encode_appearance, keyed by (crops, crop side, device)
        self._train_plans = PlanCache(os.environ.get('MMMOT_TRAIN_PLAN_CACHE', '8'))  # mmmot_amd/train.py::forward_train
        # forward(): launch the trunk before the point split is read back and the plan is built (MMMOT_IMAGE_FIRST=0: after)
        self.image_first = os.environ.get('MMMOT_IMAGE_FIRST', '1') != '0'
        self.freeze_appearance = False  # training mode: True = frozen eval-mode image features instead of the training trunk
        self._pack_version = 0     # bumped whenever packed weights are REPLACED (captured graphs go stale)
        self._packed = None        # PackSnapshot of the live engine
        self._trained_since_pack = False  # refresh_head_device(): the head's fp16-split copies are stale

    # ---- backend / packing ---------------------------------------------------
    def set_ops(self, ops):
        """Inject an operator backend (tests use a torch emulation of the C-ABI to
        check the host logic on CPU; the product default is HipOps)."""
        self._ops = ops
        self._engine = None

    def engine(self):
        """Packed-weight engine; rebuilt after load_state_dict / .to() / .cuda() (call
        ``invalidate()`` after editing parameters in place)."""
        if self._engine is None:
            dev = next(self.parameters()).device
            if self._ops is None:
                from .ops import HipOps
                self._ops = HipOps()  # raises if libmmmot_hip.so is missing: no fallback
            packed = pack_weights(self.state_dict(), self.score_fusion_arch, dev)
            self._engine = Engine(packed, self._ops, fusion=self.score_fusion_arch, affinity_op=self.affinity_op,
                                  softmax_mode=self.softmax_mode, neg_threshold=self.neg_threshold,
                                  score_arch=self.score_arch, end_mode=self.end_mode, trunk=self.trunk)
            self._plans.clear()
            self._pack_version += 1
            self._packed = PackSnapshot(self, self._HEADS)
            self._trained_since_pack = False
        return self._engine

    def _packed_is_current(self):
        p = self._packed  # (compared here, not behind another call: this runs in every forward)
        return self._engine is None or [t._version for t in p.tensors] == p.versions

    def _repack_if_trained(self):
        """Eval-mode entry points: everything the inference engine holds (folded BatchNorm, fp16-split copies, folded
        transforms) is stale once any parameter / buffer was modified in place since it was packed - by an optimizer step,
        a training-mode BatchNorm update, or by hand."""
        if self._trained_since_pack or not self._packed_is_current():
            self.invalidate()

    _HEADS = ('fusion_module', 'w_det', 'w_link')

    def refresh_head_device(self):
        """What a TRAINING step needs after ``optimizer.step()``: the fp32 packed tensors of fusion_module and w_link
        recomputed from the live parameters ON THE DEVICE (concatenations and reshapes - no host round trip except the
        two scalar output biases) and copied into the engine's tensors in place.  refresh_head() does the same on the
        host in float64 and also rebuilds the fp16-split copies (0.2 s per call: 95 % of a training step, measured);
        here those copies go stale, so the training forward runs its GEMMs on the fp32 weights (Engine.fp32_mlp) and the
        next EVAL forward re-packs everything (``_trained_since_pack``)."""
        eng = self.engine()
        with torch.no_grad():
            live = {k: p for name in ('fusion_module', 'w_link') for k, p in getattr(self, name).named_parameters(name)}
            for section, layout in (('fusion', FUSION_LAYOUT[self.score_fusion_arch]), ('w_link', LINK_LAYOUT)):
                P = eng.P[section]
                for k, v in build_head(layout, live.__getitem__).items():
                    if torch.is_tensor(v):
                        P[k].copy_(v)
                    else:
                        P[k] = v  # the two scalar output biases: one .item() each
        self._trained_since_pack = True
        self._pack_version += 1  # a captured eval graph would replay the stale fp16-split copies
        self._packed.head_refreshed()
        return eng

    def head_is_current(self):
        """False once a head parameter / buffer was modified in place (``optimizer.step()``, the BatchNorm momentum
        update) after the engine packed it."""
        return self._engine is not None and self._packed.head_is_current()

    def set_trunk(self, trunk):
        """Arithmetic of the VGG trunk (the other GEMMs follow: f16x3, or exact fp32 with 'f32'):
        'f16x3' (default): fp16 matrix cores, 3-term hi/lo split - fp32-class, score error ~3e-5 against the fp32
                 reference (indistinguishable from fp32 summation-order noise);
        'f16q8': opt-in: fp16 main term + both correction terms in one block-scaled fp8 MFMA on the trunk layers
                 ``Engine.q8_layers`` (+20 % throughput; score error 3e-4 on He-normal weights, up to 9e-4 on
                 trained-like statistics with every layer in fp8; crops under 64 pixels run f16x3);
        'f32':   exact fp32 MFMA everywhere.
        The engine's range guard lowers f16q8 -> f16x3 -> f32 by itself when activations leave the e4m3 / fp16 range
        (``engine().range_events``)."""
        self.trunk = trunk
        self.invalidate()

    def invalidate(self):
        self._engine = None
        for cache in (self._plans, self._img_plans, self._crop_plans, self._train_plans):
            cache.clear()
        self._pack_version += 1

    def refresh_head(self):
        """Re-pack only the head's weights (fusion_module, w_det, w_link: 3 M of the 21 M parameters) into the live
        engine - what a training step on the head needs after ``optimizer.step()`` (mmmot_amd/backward.py); the
        encoders' packed weights (VGG hl16 / hq8 copies, PointNet) stay as they are."""
        eng = self.engine()
        sd = {k: v for k, v in self.state_dict().items() if k.split('.')[0] in self._HEADS}
        P = pack_weights(sd, self.score_fusion_arch, next(self.parameters()).device)
        # in place where the packed layout is unchanged (always, for a pure weight update): the packed tensors keep
        # their addresses, so a captured hipGraph (GraphedForward) computes with the new weights on its next replay;
        # anything that cannot be copied in place replaces the entry and marks captured graphs stale
        inplace = True
        for k in ('fusion', 'w_det', 'w_link'):
            if not _copy_packed_(eng.P[k], P[k]):
                eng.P[k] = P[k]
                inplace = False
        if not inplace:
            self._pack_version += 1
        self._packed.head_refreshed()
        return eng

    def _apply(self, fn, *a, **k):
        self.invalidate()  # .to() / .cuda(): packed weights and the cached plans' tables live on the old device
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict=True, **k):
        self._engine = None
        self._pack_version += 1
        return super().load_state_dict(state_dict, strict=strict, **k)

    def make_plan(self, samples, crop_hw, rows=(0, 1, 2)):
        """samples: list of (frame_counts, points_split) - see BatchPlan."""
        dev = next(self.parameters()).device
        return BatchPlan(samples, crop_hw, dev, rows=rows, use_points=(1 in rows or 2 in rows))

    # ---- batched entry (no reference counterpart: the reference batch is 1) --
    def forward_batch(self, plan, crops, points, appearance=None):
        """crops [Lt,3,S,S], points [P,3] (device, concatenated over the plan's samples).
        Returns per-sample reference-shaped tuples.  ``appearance``: the detections' appearance rows [Lt, 512]
        (``encode_appearance``; AppearanceRows or a tensor) in place of the crops (crops=None): the trunk and the SkipPool
        heads do not run."""
        return self._forward_batch(plan, crops, points, appearance)[0]

    def _forward_batch(self, plan, crops, points, appearance=None):
        """forward_batch -> (per-sample tuples, the trunk's rows [M, 512] of shape (b), else None)"""
        if appearance is not None:
            appearance = self._appearance_tensor(appearance)
        self._repack_if_trained()
        if self.training:
            raise NotImplementedError('forward_batch / forward_rows compute the eval-mode forward (call .eval()); the '
                                      'training-mode forward of tracking_model.py:50-66 is model(dets, det_info, dets_split) '
                                      'after .train() - mmmot_amd/train.py')
        eng = self.engine()
        tail = None
        if eng.ops.name == 'hip':
            # the registered PyTorch-ROCm operator (mmmot_amd/torch_ops.py): CUDA dispatch key only, no CPU kernel
            h = (torch_ops.engine_handle(eng), torch_ops.plan_handle(plan))
            if appearance is None:
                det_t, link_t, new_t, end_t = torch.ops.mmmot.forward_batch(crops, points, *h)
            elif crops is None:
                det_t, link_t, new_t, end_t = torch.ops.mmmot.forward_batch_appearance(appearance, points, *h)
            else:
                det_t, link_t, new_t, end_t, tail = torch.ops.mmmot.forward_pair_appearance(appearance, crops, points, *h)
            out = dict(det=det_t, link=link_t, new=new_t, end=end_t)
        else:  # an injected backend (tests: the torch emulation of the C-ABI)
            out = eng.forward(plan, crops, points, appearance=appearance)
            if appearance is not None and crops is not None:
                tail = out['cat'][int(appearance.shape[0]):, 0:512].clone()
        res = []
        pi = 0
        nR = plan.nR
        for b, fc in enumerate(plan.frame_counts):
            d0, d1 = int(plan.det_off[b]), int(plan.det_off[b + 1])
            links = []
            for f in range(len(fc) - 1):
                _, _, N, _, M = plan.pairs[pi]
                o = plan.link_off[pi]
                links.append(out['link'][o:o + nR * N * M].view(nR, N, M))
                pi += 1
            res.append((out['det'][:, d0:d1], links, out['new'][:, d0:d1], out['end'][:, d0:d1]))
        return res, tail

    # ---- appearance rows reused across the pairs of a sequence ---------------------------------------------------
    def encode_appearance(self, crops):
        """The image branch (VGG trunk + SkipPool heads) of one frame's crops - fp32 [L,3,S,S] or uint8 [L,S,S,3], like
        ``forward`` - under the same range guard as a forward.  Returns AppearanceRows: owned rows [L, 512] (not a view of
        the workspace) and their stamp.  In eval mode every crop's row is independent of the crops beside it (folded
        BatchNorm, one-detection GroupNorm in SkipPool, fixed 256-row pooling chunks), so the rows equal bit for bit the
        appearance half of a forward over any pair that holds these crops: ``forward_appearance`` / ``forward_batch(...,
        appearance=)`` use them while ``appearance_is_current``."""
        self._repack_if_trained()
        if self.training:
            raise NotImplementedError('encode_appearance computes the eval-mode image features (call .eval())')
        S = check_crop_layout(crops)
        crops = crops.contiguous()
        eng = self.engine()
        key = (int(crops.shape[0]), S, str(crops.device))
        plan = self._crop_plans.get(key, lambda: CropPlan(key[0], S, crops.device))
        if eng.ops.name == 'hip':
            rows = torch.ops.mmmot.encode_appearance(crops, torch_ops.engine_handle(eng), torch_ops.plan_handle(plan))
        else:
            rows = eng.encode(plan, crops)[0]
        return AppearanceRows(rows, self._stamp(eng))

    def _stamp(self, eng):
        """validity stamp of rows the engine's latest trunk launch computed (read after it: a synchronous recompute in a
        lowered arithmetic is what the rows hold)"""
        return (self._pack_version, eng.serial, eng.trunk, eng.guard.n_forward - 1, len(eng.range_events))

    def appearance_is_current(self, rows):
        """True while AppearanceRows may stand in for their crops: same packed weights (no load_state_dict / invalidate
        / set_trunk / .to() / training re-pack since), same trunk arithmetic, no range event recorded since they were
        computed, eval mode.  The range guard's asynchronous check lags one forward, so its verdict on the forward that
        made the rows is taken here first (RangeGuard.settle: waits for that forward's read-back - free once its results
        were read - or reads the counters).  Stale rows are encoded again, never reused: the forwards that take
        AppearanceRows refuse them (StaleAppearanceError) before any launch."""
        eng = self._engine
        pv, serial, trunk, fwd, n_events = rows.stamp
        if (self.training or eng is None or pv != self._pack_version or eng.serial != serial or eng.trunk != trunk
                or self._trained_since_pack or not self._packed_is_current()):
            return False
        eng.guard.settle(upto=fwd)
        return eng.trunk == trunk and len(eng.range_events) == n_events

    def _appearance_tensor(self, appearance):
        if isinstance(appearance, AppearanceRows):
            if not self.appearance_is_current(appearance):
                raise StaleAppearanceError('appearance rows are stale (weights re-packed, trunk arithmetic changed, a range '
                                           'event since they were computed, or training mode): encode the frame again')
            return appearance.rows
        if not torch.is_tensor(appearance):
            raise ValueError('appearance must be AppearanceRows (encode_appearance) or a tensor, got %s'
                             % type(appearance).__name__)
        return appearance

    def forward_appearance(self, prev_rows, curr_crops, det_info, dets_split, return_rows=False):
        """``forward(dets, det_info, dets_split)`` of one frame pair with the first frame's appearance rows (AppearanceRows
        of ``encode_appearance`` or of the previous call) in place of its crops: the trunk runs on the second frame's crops
        only.  ``det_info`` / ``dets_split`` are the pair's, as for ``forward``.  Returns the same tuple as ``forward``;
        with return_rows=True also the second frame's AppearanceRows - the first frame's rows of the next pair."""
        if self.training:
            raise NotImplementedError('forward_appearance computes the eval-mode forward (call .eval())')
        if prev_rows is None or curr_crops is None:
            raise ValueError('forward_appearance needs the first frame\'s rows and the second frame\'s crops')
        prev = self._appearance_tensor(prev_rows)
        out, tail = self._forward_rows(curr_crops, det_info, dets_split, (0, 1, 2), prev)
        if not return_rows:
            return out
        return out, AppearanceRows(tail, self._stamp(self._engine))

    def capture(self, plan, crops, points):
        """hipGraph of one ``forward_batch`` for a FIXED plan (the C-ABI entry points only launch: no allocation, no
        synchronisation, so the whole step is capturable).  Returns a ``GraphedForward``; its ``__call__(crops,
        points)`` copies the inputs into the captured buffers, replays the graph and returns the same per-sample
        tuples as ``forward_batch`` (views of static output buffers, overwritten by the next replay or forward of this
        engine).  Use it when consecutive calls share the batch shape (throughput serving of fixed-size batches, the
        benchmark); a tracker whose detections change every frame calls ``forward`` / ``forward_batch`` instead.
        ``__call__`` refuses inputs of another shape or type than the captured ones (ValueError; None keeps a buffer)
        and raises once the graph is stale: the model was re-packed, or a parameter / buffer was modified in place
        and not packed again (``refresh_head()`` after a head-only edit lets the graph follow).  A replay cannot lower
        its arithmetic: ``check_range()`` is its only range protection ("Captured forward")."""
        return GraphedForward(self, plan, crops, points)

    def trans(self):
        pn = self.engine().P['pointnet']
        return [pn['trans1'].unsqueeze(0), pn['trans2'].unsqueeze(0)]

    # ---- reference entry ------------------------------------------------------
    def forward(self, dets, det_info, dets_split):
        """Same contract as reference modules/tracking_net.py:165-193: in eval mode
        (det_scores 3xL, [link_scores 3xNxM ...], new_scores 3xL, end_scores 3xL, trans); in training mode
        (``.train()``) the differentiable forward of mmmot_amd/train.py - raw det scores, new / end scores without the
        eval padding, batch-statistics BatchNorm in the trunk and w_det (``self.freeze_appearance = True`` runs the image
        branch frozen in eval mode instead)."""
        if self.training:
            from .train import forward_train
            return forward_train(self, dets, det_info, dets_split)
        return self.forward_rows(dets, det_info, dets_split, rows=(0, 1, 2))

    def _trunk_first(self, fc, S, crops, appearance=None):
        """The point split is on the HOST already (a pipeline that prepared the points itself, mmmot_amd/pipeline.py): no
        read-back to hide, but the image branch still launches first so that PointNet's small launches run on the engine's
        side stream beside the trunk instead of behind it.  Returns False when the engine is not the HIP one."""
        self._repack_if_trained()
        eng = self.engine()
        if eng.ops.name != 'hip':
            return False
        eng.image_first(self._image_plan(fc, S, crops.device), crops, appearance)
        return True

    def _image_plan(self, fc, S, dev):
        """the image-only plan of Engine.image_first: its tables depend on the frame counts and the crop side only"""
        return self._img_plans.get((tuple(fc), S, str(dev)),
                                   lambda: BatchPlan([(fc, None)], S, dev, rows=(0,), use_points=False))

    def _split_behind_trunk(self, ps_t, fc, S, crops, appearance=None):
        """The point split (device tensor) is needed on the host to build the plan; the trunk is not waiting for it.  Copy it
        on a side stream, launch the image branch (Engine.image_first: its tables depend on the frame counts only and are
        cached per (counts, crop side)), then wait for the copy alone: the read-back and the plan build that follows run
        beside ~2 ms of trunk time instead of in front of it.  Returns the split as int64 numpy, or None when the engine is
        not the HIP one (injected test backends take the plain path)."""
        self._repack_if_trained()
        eng = self.engine()
        if eng.ops.name != 'hip':
            return None
        dev = crops.device
        n = int(ps_t.numel())
        st = getattr(self, '_split_stage', None)
        if st is None or st[0].numel() < n or st[0].dtype != ps_t.dtype or st[1].device != dev:
            st = (torch.empty(max(64, 2 * n), dtype=ps_t.dtype).pin_memory(), torch.cuda.Stream(dev), torch.cuda.Event())
            self._split_stage = st
        host, side, ev = st
        cur = torch.cuda.current_stream(dev)
        side.wait_stream(cur)  # the producer of points_split is ordered before the copy; nothing of this forward is queued yet
        with torch.cuda.stream(side):
            host[:n].copy_(ps_t.detach(), non_blocking=True)
            ev.record(side)
        eng.image_first(self._image_plan(fc, S, dev), crops, appearance)
        ev.synchronize()
        return host[:n].numpy().astype(np.int64)

    def forward_rows(self, dets, det_info, dets_split, rows=(0, 1, 2)):
        """Single-modality variant: rows=(0,) image-only skips PointNet+fusion, rows=(1,) LiDAR-only
        skips VGG+fusion; the returned tensors hold only the requested modality rows."""
        return self._forward_rows(dets, det_info, dets_split, rows)[0]

    def _forward_rows(self, dets, det_info, dets_split, rows, appearance=None):
        """forward_rows; `appearance`: the first frame's rows, `dets` the second frame's crops (forward_appearance).
        Returns (the forward's tuple, the second frame's rows when appearance is given)."""
        fc = [int(d.item()) if torch.is_tensor(d) else int(d) for d in dets_split]
        rows = tuple(rows)
        need_pts = (1 in rows) or (2 in rows)
        need_img = (0 in rows) or (2 in rows)
        # dets: the reference's normalised fp32 [L,3,S,S] crops, or the uint8 [L,S,S,3] crops of the resize
        # (mmmot_amd.crops.crop_resize_u8): ToTensor / Normalize then happen inside the first trunk launch
        # (checked on the host before anything is queued: a wrong layout or side must not reach the D2H copy of the point
        # split or the trunk of Engine.image_first)
        if need_img and dets is not None:
            S = check_crop_layout(dets)
        else:
            S = (int(dets.shape[1]) if dets.dtype == torch.uint8 else int(dets.shape[-1])) if dets is not None else 0
        ps = None
        points = None
        crops = dets.contiguous() if need_img else None
        beside = False  # the trunk of this call is already running (Engine.image_first)
        if need_pts:
            # (before the trunk is launched: a layout copy queued behind it would not be seen by the LiDAR branch, which
            # runs on a side stream beside the trunk)
            points = det_info['points']
            points = points.reshape(-1, points.shape[-1]).contiguous()  # [P][3] or [P][4] (with reflectivity)
            ps_t = det_info['points_split'].reshape(-1)
            if (need_img and ps_t.is_cuda and crops.is_cuda and self.image_first and not self.training
                    and not torch.cuda.is_current_stream_capturing()):
                ps = self._split_behind_trunk(ps_t, fc, S, crops, appearance)
                beside = ps is not None
            elif (need_img and not ps_t.is_cuda and crops.is_cuda and points.is_cuda and self.image_first
                  and not self.training and not torch.cuda.is_current_stream_capturing()):
                beside = self._trunk_first(fc, S, crops, appearance)
            if ps is None:
                ps = ps_t.detach().to('cpu').numpy().astype(np.int64)  # one D2H copy (reference: 2 .item() per detection)
        try:
            return self._forward_rows_tail(fc, ps, S, rows, need_pts, crops, points, dets, beside, appearance)
        except BaseException:
            if beside and self._engine is not None:  # the image branch that was issued belongs to no forward any more
                self._engine.drop_head_start()
            raise

    def _forward_rows_tail(self, fc, ps, S, rows, need_pts, crops, points, dets, beside, appearance=None):
        dev = points.device if points is not None else dets.device
        key = (tuple(fc), None if ps is None else ps.tobytes(), S, rows, str(dev))

        def build():
            if not beside:
                return BatchPlan([(fc, ps)], S, dev, rows=rows, use_points=need_pts)
            # the plan's tables are uploaded on the engine's side stream - the stream the LiDAR branch will run on -
            # instead of behind the trunk; the main stream (pairwise head) waits for that upload alone
            side = self.engine()._side_stream(dev)
            with torch.cuda.stream(side):
                plan = BatchPlan([(fc, ps)], S, dev, rows=rows, use_points=need_pts)
            torch.cuda.current_stream(dev).wait_stream(side)
            return plan

        res, tail = self._forward_batch(self._plans.get(key, build), crops, points, appearance)
        det, links, new, end = res[0]
        trans = self.trans() if need_pts else None
        return (det, links, new, end, trans), tail
