"""Training labels on the device: drop-ins for the reference's two host loops in front of ``TrackingLoss``.

``TrackingModule.step`` (reference tracking_model.py:50-66) is forward -> ``generate_gt`` -> loss -> backward ->
optimizer.  ``generate_gt`` (tracking_model.py:294-351) is a triple Python loop over 1-element tensors that writes the
targets one element at a time; its inputs come from ``generate_det_id_matrix`` (dataset/common.py:95-111), a host loop of
the same kind per frame.  Both are restated literally - quirks included, DESIGN.md section 15 - as one kernel launch each
(csrc/labels.hip), and the targets come out in the block layout the chain solver and the loss already use:

    from mmmot_amd.labels import generate_gt, as_solver_gt, match_dets
    gt_det, gt_link, gt_new, gt_end = generate_gt(det_score[0], det_cls, det_id, det_split)   # tracking_model.py:54-55
    assignment = associate_chain(det, links, new, end, det_split, gt=as_solver_gt((gt_det, gt_link, gt_new, gt_end)))
    frame_ids, frame_cls = match_dets(shift_bbox, gt['bbox'], gt['id'], gt['name'])           # patchwise_dataset.py:97

Host inputs go to the device in one copy; device inputs stay there (joined and converted to int32 by two small torch
kernels in front of the launch) and nothing waits on the host.  ``bbox_jitter`` stays
on the host (its NumPy random stream is part of the reference's behaviour).  There is no CPU implementation.
"""
import numpy as np
import torch

from . import torch_ops  # noqa: F401  (registers mmmot::generate_gt and mmmot::match_dets)
from .association import chain_block_size, chain_of, chains_table, unpack_chain

CAR, DONTCARE = 0, -1  # LABEL['Car'], LABEL['DontCare'] (reference utils/data_util.py:14-24)
_DEVICE = 'cuda'       # where host inputs are sent


def _op_generate_gt(ids, cls, chains):
    return torch.ops.mmmot.generate_gt(ids, cls, chains)


def _op_match_dets(det_xywh, gt_xywh, gt_id, gt_name, frames, car, dontcare, max_iou):
    return torch.ops.mmmot.match_dets(det_xywh, gt_xywh, gt_id, gt_name, frames, car, dontcare, max_iou)


def _int32(t, what):
    """integer tensor -> int32 (one conversion); on the host the range is checked first (a device tensor is converted as it
    is: looking at its values would wait for the device)"""
    if t.is_floating_point() or t.dtype == torch.bool or t.is_complex():
        raise ValueError('%s must be an integer tensor, got %s' % (what, t.dtype))
    if t.dtype == torch.int32:
        return t
    if not t.is_cuda and t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
        raise ValueError('%s outside the int32 range' % what)
    return t.to(torch.int32)


def _frames_flat(per_frame, split, what):
    """the T per-frame tensors ([1, n_t, 1] in the reference) of one sample -> the list of flat [n_t] views"""
    if len(per_frame) != len(split):
        raise ValueError('generate_gt: %s has %d frames, det_split %d' % (what, len(per_frame), len(split)))
    flat = [torch.as_tensor(t).reshape(-1) for t in per_frame]
    if any(f.numel() != n for f, n in zip(flat, split)):
        raise ValueError('generate_gt: %s does not match det_split %s' % (what, split))
    return flat


def _launch_device(tensors, like=None):
    for t in tensors:
        if t.is_cuda:
            return t.device
    return like.device if like is not None and like.is_cuda else torch.device(_DEVICE)


def _to_device(ids, cls, dev):
    """[ids | cls] as int32 on ``dev``: the per-frame tensors are joined first, so that host inputs travel in ONE copy and
    device inputs cost one concatenation and one conversion, whatever the number of frames"""
    parts = ids + cls
    if any(p.is_cuda for p in parts):
        parts = [p if p.device == dev else p.to(dev) for p in parts]
        both = _int32(torch.cat(parts), 'generate_gt: det_id / det_cls')
    else:
        both = _int32(torch.cat(parts), 'generate_gt: det_id / det_cls').to(dev)  # one host-to-device copy
    n = both.numel() // 2
    return both[:n], both[n:]


def generate_gt_batch(det_cls, det_id, det_splits, like=None):
    """The targets of B samples in one launch.  Per sample b: det_cls[b] / det_id[b] = its T_b per-frame integer tensors
    (n_t values each, any shape), det_splits[b] its split; every sample needs a detection.  Returns (block, offsets,
    labels): the flat fp32 device block, sample b's [gt_det L | gt_new L | gt_end L | link_0 | ..] at offsets[b], and per
    sample the tuple (gt_det [L], [gt_link 1 x n_t x n_{t+1} ...], gt_new [L], gt_end [L]) - views of the block, or
    copies with the dtype and device of ``like`` when given."""
    splits = [chain_of(s) for s in det_splits]
    if not splits:
        raise ValueError('generate_gt_batch: no samples')
    if any(sum(s) == 0 for s in splits):
        raise ValueError('generate_gt_batch: every sample needs a detection (use generate_gt for empty samples)')
    if len(det_cls) != len(splits) or len(det_id) != len(splits):
        raise ValueError('generate_gt_batch: det_cls, det_id and det_splits must have one entry per sample')
    ids = [f for d, s in zip(det_id, splits) for f in _frames_flat(d, s, 'det_id')]
    cls = [f for d, s in zip(det_cls, splits) for f in _frames_flat(d, s, 'det_cls')]
    chains, offs = chains_table(splits)
    torch_ops.chain_layout(chains, op='generate_gt')  # the limits, before anything is copied
    ids_d, cls_d = _to_device(ids, cls, _launch_device(ids + cls, like))
    block = _op_generate_gt(ids_d, cls_d, chains)
    labels = []
    for s, o in zip(splits, offs):
        b = block[o:o + chain_block_size(s)]
        if like is not None:
            b = b.to(device=like.device, dtype=like.dtype)
        labels.append(unpack_chain(b, s))
    return block, offs, labels


def generate_gt(det_score, det_cls, det_id, det_split):
    """Drop-in for reference ``TrackingModule.generate_gt(det_score, det_cls, det_id, det_split)``: det_score [L] (only
    its size, dtype and device are used), det_cls / det_id the per-frame ``[1, n_t, 1]`` long tensors (host or device),
    det_split ints or 1-element tensors.  Returns (gt_det, gt_link, gt_new, gt_end) with the dtype, device and shape of
    det_score, gt_link[t] as [1, n_t, n_{t+1}]."""
    split = chain_of(det_split)
    L = sum(split)
    if det_score.numel() != L:
        raise ValueError('generate_gt: det_score has %d elements, det_split %s' % (det_score.numel(), split))
    ids, cls = _frames_flat(det_id, split, 'det_id'), _frames_flat(det_cls, split, 'det_cls')
    if L == 0:
        z = det_score.new_zeros(det_score.size())
        return z, [det_score.new_zeros((1, a, b)) for a, b in zip(split[:-1], split[1:])], z.clone(), z.clone()
    chains, _ = chains_table([split])
    torch_ops.chain_layout(chains, op='generate_gt')  # the limits, before anything is copied
    ids_d, cls_d = _to_device(ids, cls, _launch_device(ids + cls, det_score))
    block = _op_generate_gt(ids_d, cls_d, chains).to(device=det_score.device, dtype=det_score.dtype)
    det, links, new, end = unpack_chain(block, split)
    return det.view(det_score.size()), links, new.view(det_score.size()), end.view(det_score.size())


def as_solver_gt(labels):
    """(gt_det, gt_link, gt_new, gt_end), the order of ``generate_gt`` and of ``TrackingLoss`` -> (gt_det, gt_new, gt_end,
    [gt_link ...]), the order ``associate_chain(gt=...)`` and the reference's ``ortools_solve(gt=...)`` take."""
    gt_det, gt_link, gt_new, gt_end = labels
    return gt_det, gt_new, gt_end, list(gt_link)


# ---- detections -> ground-truth identities --------------------------------------------------------------------------
def _xywh(boxes, what):
    """x1, y1, x2, y2 boxes [n, 4] -> x, y, w, h in fp64; the subtraction runs in the INPUT's dtype before widening, as
    ``calculate_distance`` (dataset/common.py:88-91) does"""
    b = boxes if torch.is_tensor(boxes) else torch.from_numpy(np.ascontiguousarray(boxes))
    if b.numel() == 0:
        b = b.reshape(0, 4)
    if b.dim() != 2 or b.shape[1] != 4:
        raise ValueError('match_dets: %s must be [n, 4] boxes (x1, y1, x2, y2), got %s' % (what, tuple(b.shape)))
    return torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], dim=1).to(torch.float64)


def _codes(v, n, what):
    t = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
    t = t.reshape(-1)
    if t.numel() != n:
        raise ValueError('match_dets: %s has %d entries for %d ground-truth boxes' % (what, t.numel(), n))
    if t.is_floating_point():  # the reference's int(gt_dets['id'][i]); a device tensor is converted as it is
        if not t.is_cuda and n and not bool(torch.isfinite(t).all()):
            raise ValueError('match_dets: %s is not finite' % what)
        t = t.to(torch.int64)
    return _int32(t, 'match_dets: %s' % what)


def match_dets_batch(det_bbox, gt_bbox, gt_id, gt_name, car=CAR, dontcare=DONTCARE, max_iou=0.5):
    """``generate_det_id_matrix`` for NF frames (the frames of a sample, or of several samples) in one launch: four lists
    with one entry per frame, as ``match_dets`` takes them.  Returns the list of per-frame (gt_id [n, 1] long, gt_cls
    [n, 1] long), on the device of the detection boxes when those are device tensors, else on the host."""
    NF = len(det_bbox)
    if NF < 1 or len(gt_bbox) != NF or len(gt_id) != NF or len(gt_name) != NF:
        raise ValueError('match_dets_batch: four lists with one entry per frame (at least one frame)')
    det = [_xywh(b, 'det_bbox') for b in det_bbox]
    gt = [_xywh(b, 'gt_bbox') for b in gt_bbox]
    nd, ng = [int(b.shape[0]) for b in det], [int(b.shape[0]) for b in gt]
    ids = [_codes(v, n, 'gt_id') for v, n in zip(gt_id, ng)]
    names = [_codes(v, n, 'gt_name') for v, n in zip(gt_name, ng)]
    out_dev = det[0].device
    if sum(nd) == 0:
        return [(torch.zeros((0, 1), dtype=torch.long, device=out_dev),) * 2 for _ in range(NF)]
    rows, do, go = [], 0, 0
    for a, b in zip(nd, ng):
        rows.append((do, a, go, b))
        do += a
        go += b
    frames = torch.tensor(rows, dtype=torch.int32)
    torch_ops.match_layout(frames, do, go)  # the limits, before anything is copied
    dev = _launch_device(det + gt + ids + names)
    if not any(t.is_cuda for t in det + gt + ids + names):
        # one host-to-device copy: the boxes as their bit patterns in front of the codes
        packed = torch.cat([torch.cat(det + gt).reshape(-1).view(torch.int32), torch.cat(ids + names)]).to(dev)
        nb = 8 * (do + go)
        boxes = packed[:nb].view(torch.float64).view(-1, 4)
        codes = packed[nb:]
    else:
        boxes = torch.cat([t.to(dev) for t in det + gt])
        codes = torch.cat([t.to(dev) for t in ids + names])
    res = _op_match_dets(boxes[:do], boxes[do:], codes[:go], codes[go:], frames, int(car), int(dontcare), float(max_iou))
    res = res.to(device=out_dev, dtype=torch.long)
    out, o = [], 0
    for a in nd:
        out.append((res[0, o:o + a].reshape(a, 1), res[1, o:o + a].reshape(a, 1)))
        o += a
    return out


def match_dets(det_bbox, gt_bbox, gt_id, gt_name, car=CAR, dontcare=DONTCARE, max_iou=0.5):
    """Drop-in for reference ``generate_det_id_matrix(dets_bbox, gt_dets)`` with ``gt_dets`` = {'bbox': gt_bbox, 'id':
    gt_id, 'name': gt_name}: x1, y1, x2, y2 boxes [n, 4] / [n_gt, 4] (arrays or tensors, host or device), integer ids and
    class codes (``car`` / ``dontcare``: the codes of LABEL['Car'] / LABEL['DontCare']).  Returns (gt_id [n, 1] long,
    gt_cls [n, 1] long)."""
    return match_dets_batch([det_bbox], [gt_bbox], [gt_id], [gt_name], car, dontcare, max_iou)[0]
