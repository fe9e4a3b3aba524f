"""One training run, sample by sample: the training counterpart of ``pipeline.SequencePipeline``.

The reference builds a training sample on the host, per frame of the sample (dataset/patchwise_dataset.py:115-190):
``bbox_jitter`` -> ``get_pointcloud(.., shift_bbox=..)`` -> ``align_points`` to the sample's first frame ->
``generate_det_id_matrix(shift_bbox, gt)`` -> per detection ``train_transform(img.crop(shift_bbox).resize((224, 224)))``,
and then runs ``TrackingModule.step`` (tracking_model.py:50-66) on it.  Here, per sample:

    prepare:  H2D (T images, T sweeps)  ->  ``prep_points_batched``  ->  ``align_points_batched`` (frames 1 .. T-1, k-step
              records; with poses)  ->  ``crop_resize_u8`` per frame  ->  ``augment_crops`` over the joined crops (one
              launch; ``augment=None``: ``u8_normalize``)  ->  ``labels.match_dets_batch``
    step:     ``lr_scheduler.step(it)``  ->  training-mode forward  ->  ``labels.generate_gt``  ->  criterion  ->
              ``zero_grad``, ``backward``, ``optimizer.step()``

``overlap=True`` queues ``prepare`` of sample k+1 on a side stream before the host waits on anything of step k, so the
upload, the gather, the resamplings and the matching run beside the step.  Both orders launch the same kernels on the
same inputs and return the same bits (tests/test_train_pipeline_gpu.py).  ``bbox_jitter`` stays the caller's host code
(DESIGN section 15): a sample carries the jittered boxes, which are used for the crops, for the frustum gather and for
the matching, as in the reference.  One sample per step, like the reference's batch size 1.

The augmentation parameters come from the pipeline's own host ``torch.Generator(seed)``, drawn in sample order at
``prepare`` - the global generator, which carries DropBlock's and dropout's draws inside the forward, is not touched, and
both overlap settings see the same numbers.  No CPU fallback: every stage is a C-ABI kernel sequence on the device.
"""
import numpy as np
import torch

from . import ego, labels
from .crops import augment_crops, crop_resize_u8, u8_normalize
from .pipeline import FrameFeed, _window_records  # noqa: F401  (FrameFeed: what a TrainSample is made of)
from .points import align_points_batched, prep_points_batched


class TrainSample:
    """Host side of one training sample: T = ``sample_max_len`` FrameFeeds (every one with ``pose=`` or none), per frame
    the ground-truth dict {'bbox', 'id', 'name'} that ``labels.match_dets`` takes, and optionally per frame the jittered
    detection boxes [n_t, 4] (``bbox_jitter`` of the frame's ``dets['bbox']``; None: the boxes themselves)."""

    def __init__(self, feeds, gts, shift_bboxes=None):
        feeds, gts = list(feeds), list(gts)
        if len(feeds) < 2:
            raise ValueError('TrainSample: a sample has at least 2 frames, got %d' % len(feeds))
        if len(gts) != len(feeds):
            raise ValueError('TrainSample: %d frames need %d ground-truth dicts, got %d' % (len(feeds), len(feeds), len(gts)))
        n = sum(1 for f in feeds if f.pose is not None)
        if 0 < n < len(feeds):
            raise ValueError('TrainSample: %d of %d frames carry a pose; the alignment to the first frame needs the pose '
                             'of every frame (or of none)' % (n, len(feeds)))
        if n and len(feeds) - 1 > ego.MAX_CHAIN:
            raise ValueError('TrainSample: %d frames with poses need a chain of %d alignment steps; at most %d'
                             % (len(feeds), len(feeds) - 1, ego.MAX_CHAIN))
        if any(f.point_transform is not None for f in feeds):
            raise ValueError('TrainSample: point_transform= is not used in training; give pose= for the alignment')
        for t, g in enumerate(gts):
            if not all(k in g for k in ('bbox', 'id', 'name')):
                raise ValueError("TrainSample: ground truth of frame %d needs 'bbox', 'id' and 'name'" % t)
        boxes = [np.asarray(f.dets['bbox'], dtype=np.float64).reshape(-1, 4) for f in feeds]
        if shift_bboxes is not None:
            shift_bboxes = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in shift_bboxes]
            if len(shift_bboxes) != len(feeds) or any(s.shape != b.shape for s, b in zip(shift_bboxes, boxes)):
                raise ValueError('TrainSample: shift_bboxes holds one [n_t, 4] array per frame, as many boxes as detections')
        if any(b.shape[0] == 0 for b in boxes):
            raise ValueError('TrainSample: every frame needs a detection (the reference asserts it)')
        self.feeds, self.gts, self.shift_bboxes = feeds, gts, shift_bboxes
        self.moving = n > 0
        self.boxes = shift_bboxes if shift_bboxes is not None else boxes  # crops, frustum gather and matching use these


def _upload(arrays, dtype, dev):
    """host arrays -> their device copies, views of ONE buffer that travels in one asynchronous copy"""
    flat = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays]
    n = sum(a.size for a in flat)
    stage = torch.empty(n, dtype={np.float64: torch.float64, np.int32: torch.int32}[dtype], pin_memory=True)
    if n:
        stage.numpy()[:] = np.concatenate(flat)
    d = stage.to(dev, non_blocking=True)
    out, o = [], 0
    for a in flat:
        out.append(d[o:o + a.size])
        o += a.size
    return out


class TrainingPipeline:
    def __init__(self, model, criterion, optimizer, size=224, augment=None, seed=0, overlap=True, lr_scheduler=None,
                 use_frustum=False, det_type='3D', without_reflectivity=True):
        if augment is not None and int(augment.size) != int(size):
            raise ValueError('TrainingPipeline: the augmentation is made for %d-pixel crops, size is %d' % (augment.size, size))
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        self.size, self.augment, self.overlap = int(size), augment, bool(overlap)
        self.lr_scheduler = lr_scheduler
        self.use_frustum, self.det_type, self.wo_refl = bool(use_frustum), det_type, without_reflectivity
        self.dev = next(model.parameters()).device
        self.side = torch.cuda.Stream(self.dev) if overlap else None
        self.generator = torch.Generator().manual_seed(int(seed))  # the augmentation's draws, in sample order
        self.it = 0                                                # iterations stepped: what lr_scheduler.step takes

    # ---- one sample onto the device and through the preparation kernels ----------------------------------------------
    def _prepare(self, sample):
        feeds, T, dev = sample.feeds, len(sample.feeds), self.dev
        boxes = sample.boxes
        counts = [int(b.shape[0]) for b in boxes]
        # drawn first: the table depends on the sample's order alone, not on what the device does
        params = None if self.augment is None else self.augment.draw(sum(counts), self.generator)
        imgs = [f.img.to(dev, non_blocking=True) for f in feeds]
        sweeps = [f.sweep.to(dev, non_blocking=True) for f in feeds]
        # the T frames' gather in ONE launch sequence, one split read-back - the one host wait of prepare
        pcs = prep_points_batched(sweeps, [f.info for f in feeds], [f.dets for f in feeds], use_frustum=self.use_frustum,
                                  without_reflectivity=self.wo_refl, det_type=self.det_type,
                                  shift_bboxes=sample.shift_bboxes)
        pts = [pc['points'] for pc in pcs]
        if sample.moving:  # frame k aligned to frame 0 by its k-step record, frames 1 .. T-1 in one launch; frame 0 raw
            n0 = int(pts[0].shape[0])
            rows = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in pts[1:]])])
            points = torch.empty((n0 + int(rows[-1]), int(pts[0].shape[1])), dtype=torch.float32, device=dev)
            points[:n0] = pts[0]
            align_points_batched(torch.cat(pts[1:]), rows, _window_records(feeds, T - 1), T - 1, out=points, out_row0=n0)
        else:
            points = torch.cat(pts)
        split = np.asarray(pcs[0]['points_split'], dtype=np.int64)
        for pc in pcs[1:]:
            split = np.concatenate([split, split[-1] + np.asarray(pc['points_split'][1:], dtype=np.int64)])
        u8 = torch.cat([crop_resize_u8(img, b, self.size) for img, b in zip(imgs, boxes)])
        crops = u8_normalize(u8) if params is None else augment_crops(u8, params)
        # detections -> ground-truth identities, all frames in one launch, inputs and results on the device
        gts = sample.gts
        fb = _upload(list(boxes) + [np.asarray(g['bbox']).reshape(-1, 4) for g in gts], np.float64, dev)
        codes = _upload([g['id'] for g in gts] + [g['name'] for g in gts], np.int32, dev)
        matched = labels.match_dets_batch([b.view(-1, 4) for b in fb[:T]], [b.view(-1, 4) for b in fb[T:]], codes[:T],
                                          codes[T:])
        return {'crops': crops,
                'det_info': {'points': points.unsqueeze(0),
                             # on the host already (the gather read it back): a CPU tensor - no D2H in the forward
                             'points_split': torch.from_numpy(split.astype(np.float32)).unsqueeze(0)},
                'det_id': [m[0].unsqueeze(0) for m in matched], 'det_cls': [m[1].unsqueeze(0) for m in matched],
                'det_split': [torch.tensor([n]) for n in counts], 'params': params, 'ready': None}

    def prepare(self, sample):
        """The sample as the arguments of ``TrackingModule.step`` on the device: 'crops' fp32 [L, 3, S, S], 'det_info'
        ('points' [1, Q, 3|4], 'points_split' [1, L + 1] on the host), 'det_id' / 'det_cls' per frame [1, n_t, 1] long,
        'det_split'; 'params' the augmentation table it drew, 'ready' the event ``step`` waits for (overlap)."""
        if not self.overlap:
            return self._prepare(sample)
        cur = torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(self.side):
            a = self._prepare(sample)
            a['ready'] = torch.cuda.Event()
            a['ready'].record(self.side)
        for t in [a['crops'], a['det_info']['points']] + a['det_id'] + a['det_cls']:
            t.record_stream(cur)   # allocated on the side stream, consumed on the main one
        return a

    # ---- tracking_model.py:50-66 ---------------------------------------------------------------------------------------
    def step(self, prepared):
        """One training step on a prepared sample; returns the loss as a device scalar, nothing waits on the host."""
        if not self.model.training:
            raise RuntimeError('TrainingPipeline.step: the model is in eval mode; call model.train() first')
        if prepared['ready'] is not None:
            torch.cuda.current_stream(self.dev).wait_event(prepared['ready'])
        if self.lr_scheduler is not None:
            self.lr_scheduler.step(self.it)
        self.it += 1
        ds = prepared['det_split']
        det, link, new, end, trans = self.model(prepared['crops'], prepared['det_info'], ds)
        gt_det, gt_link, gt_new, gt_end = labels.generate_gt(det[0], prepared['det_cls'], prepared['det_id'], ds)
        loss = self.criterion(ds, gt_det, gt_link, gt_new, gt_end, det, link, new, end, trans)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def run(self, samples, log_every=None, on_log=None):
        """``step`` over ``samples`` (any iterable of TrainSamples), sample k+1 prepared before the host first waits on
        anything of step k.  Returns the losses as a host fp32 tensor, copied once at the end - or every ``log_every``
        steps, when ``on_log(first step, losses)`` is called with each batch of them."""
        it = iter(samples)
        nxt = next(it, None)
        nxt = None if nxt is None else self.prepare(nxt)
        done, pending, k = [], [], 0
        while nxt is not None:
            cur = nxt
            pending.append(self.step(cur))
            s = next(it, None)
            nxt = None if s is None else self.prepare(s)
            k += 1
            if log_every and len(pending) >= int(log_every):
                done.append(torch.stack(pending).cpu())
                if on_log is not None:
                    on_log(k - len(pending), done[-1])
                pending = []
        if pending:
            done.append(torch.stack(pending).cpu())
            if on_log is not None and log_every:
                on_log(k - len(pending), done[-1])
        return torch.cat(done) if done else torch.zeros(0)
