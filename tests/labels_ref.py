"""Host specification of the two label kernels (csrc/labels.hip) in NumPy: integer / float64 restatements of the
reference's ``TrackingModule.generate_gt`` (tracking_model.py:294-351) and ``generate_det_id_matrix``
(dataset/common.py:82-111), written from their semantics as array expressions.  Imports nothing from the reference;
tests/test_labels_cpu.py pins both against fixtures made by running the imported reference (tools/gen_golden_labels.py):
crafted cases, 200 seeded random chains and 60 seeded random frames."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def generate_gt(cls, ids, split):
    """cls / ids: per frame an integer array of n_t values.  Returns (gt_det [L], [gt_link n_t x n_{t+1} ...], gt_new [L],
    gt_end [L]) as float32 0 / 1 arrays."""
    split = [int(n) for n in split]
    T, L = len(split), sum(split)
    cls = [np.asarray(c).reshape(-1).astype(np.int64) for c in cls]
    ids = [np.asarray(i).reshape(-1).astype(np.int64) for i in ids]
    assert all(len(c) == n and len(i) == n for c, i, n in zip(cls, ids, split))
    st = np.concatenate([[0], np.cumsum(split)]).astype(int)
    gt_det, gt_new, gt_end = (np.zeros(L, np.float32) for _ in range(3))
    links = [np.zeros((a, b), np.float32) for a, b in zip(split[:-1], split[1:])]
    for t in range(T):
        pos = cls[t] == 1
        gt_det[st[t]:st[t + 1]] = pos
        if t < T - 1 and split[t] and split[t + 1]:
            eq = ids[t][:, None] == ids[t + 1][None, :]
            has, succ = eq.any(1), eq.argmax(1)  # argmax: the first True
            rows = np.nonzero(pos & has)[0]
            links[t][rows, succ[rows]] = 1
        else:
            has = np.zeros(split[t], bool)
        gt_end[st[t]:st[t + 1]] = pos & ~has
        if t > 0 and split[t] and split[t - 1]:
            prev = (ids[t][:, None] == ids[t - 1][None, :]).any(1)
        else:
            prev = np.zeros(split[t], bool)
        gt_new[st[t]:st[t + 1]] = pos & ~prev
    return gt_det, links, gt_new, gt_end


def block_of(labels):
    """(gt_det, links, gt_new, gt_end) -> the flat block [gt_det | gt_new | gt_end | link_0 | ..] of the kernel"""
    d, links, n, e = labels
    return np.concatenate([d, n, e] + [l.reshape(-1) for l in links]).astype(np.float32)


def iou_distance(gt_xywh, det_xywh, max_iou=0.5):
    """``motmetrics.distances.iou_matrix(objs, hyps, max_iou)`` from its definition: 1 - IoU of x, y, w, h boxes in
    float64, NaN where the union is empty or the distance exceeds ``max_iou``; [n_gt, n_det]."""
    g, d = np.asarray(gt_xywh, np.float64).reshape(-1, 4), np.asarray(det_xywh, np.float64).reshape(-1, 4)
    if g.size == 0 or d.size == 0:
        return np.empty((0, 0))
    g, d = g[:, None, :], d[None, :, :]
    g_br, d_br = g[..., :2] + g[..., 2:], d[..., :2] + d[..., 2:]
    ext = np.maximum(np.minimum(g_br, d_br) - np.maximum(g[..., :2], d[..., :2]), 0.0)
    isect = ext[..., 0] * ext[..., 1]
    union = g[..., 2] * g[..., 3] + d[..., 2] * d[..., 3] - isect
    with np.errstate(divide='ignore', invalid='ignore'):
        dist = np.where(union == 0, np.nan, 1.0 - isect / union)
        return np.where(dist > max_iou, np.nan, dist)


def xywh(boxes):
    """x1, y1, x2, y2 -> x, y, w, h with the subtraction in the array's own dtype (calculate_distance)"""
    b = np.array(boxes, copy=True).reshape(-1, 4)
    b[:, 2:] = b[:, 2:] - b[:, :2]
    return b


def match_xywh(det, gt, gt_id, gt_name, car=0, dontcare=-1, max_iou=0.5):
    """x, y, w, h boxes -> (det_id [n] int64, det_cls [n] int64): the contract of mmmot_match_dets for one frame"""
    det, gt = np.asarray(det).reshape(-1, 4), np.asarray(gt).reshape(-1, 4)
    n, ng = det.shape[0], gt.shape[0]
    det_id, det_cls = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    if n == 0 or ng == 0:
        return det_id, det_cls
    mat = iou_distance(gt, det, max_iou)
    mat[np.isnan(mat)] = 10
    mat = mat.astype(np.float32)
    arg = mat.argmin(1)  # the first minimum
    for i in range(ng):  # sequential overwrite: the last gt that points at a det stays
        det_id[arg[i]] = int(gt_id[i])
        det_cls[arg[i]] = 1 if gt_name[i] == car else (-1 if gt_name[i] == dontcare else 0)
    return det_id, det_cls


def match_dets(det_bbox, gt_bbox, gt_id, gt_name, car=0, dontcare=-1, max_iou=0.5):
    """x1, y1, x2, y2 boxes -> (det_id [n] int64, det_cls [n] int64)"""
    return match_xywh(xywh(det_bbox), xywh(gt_bbox), gt_id, gt_name, car, dontcare, max_iou)


# ---- seeded inputs shared by the CPU and the GPU tests ----------------------------------------------------------------
def random_chain(rng, split, n_ids=None):
    """per-frame (cls, ids) with classes in {-1, 0, 1} and ids drawn from a small pool (duplicates inside a frame and
    -1 included), so that every branch of generate_gt is met"""
    n_ids = n_ids or max(3, max(split) if split else 3)
    cls = [rng.choice([-1, 0, 1, 1], n).astype(np.int64) for n in split]
    ids = [rng.integers(-1, n_ids, n).astype(np.int64) for n in split]
    return cls, ids


def random_boxes(rng, n, size=200.0):
    """n x1, y1, x2, y2 float64 boxes on a size x size canvas, 20 - 60 wide and high"""
    tl = rng.uniform(0, size, (n, 2))
    return np.concatenate([tl, tl + rng.uniform(20, 60, (n, 2))], 1)


def random_frame(rng, n_det, n_gt):
    """(det_bbox, gt_bbox, gt_id, gt_name): the first gts are detections moved by a few pixels (close matches, two gts on
    one detection when n_gt > n_det), the rest lie anywhere; names from Car (0), DontCare (-1), others"""
    det = random_boxes(rng, n_det)
    gt = random_boxes(rng, n_gt)
    if n_det:
        for i in range(n_gt):
            if i % 3 != 2:
                gt[i] = det[i % n_det] + rng.uniform(-6, 6, 4)
    gt_id = rng.permutation(n_gt + 5)[:n_gt].astype(np.int64)
    gt_name = rng.choice([0, 0, -1, 3, 1], n_gt).astype(np.int64)
    return det, gt, gt_id, gt_name


# ---- readers of the fixtures (tools/gen_golden_labels.py) -------------------------------------------------------------
def gt_fixture():
    """the crafted chains: (name, split, cls per frame, ids per frame, expected block)"""
    z = np.load(os.path.join(GOLDEN, 'labels_gt.npz'))
    for name in z['names']:
        split = [int(n) for n in z[name + ':split']]
        cut = np.cumsum(split)[:-1]
        yield str(name), split, np.split(z[name + ':cls'], cut), np.split(z[name + ':ids'], cut), z[name + ':block']


def gt_fixture_random():
    """the seeded random chains (T <= 8, n <= 12): (k, split, cls per frame, ids per frame, expected block)"""
    z = np.load(os.path.join(GOLDEN, 'labels_gt.npz'))
    cls, ids, block = z['random:cls'], z['random:ids'], z['random:block'].astype(np.float32)
    so = bo = 0
    for k, row in enumerate(z['random:splits']):
        split = [int(n) for n in row if n >= 0]
        L = sum(split)
        nb = 3 * L + sum(a * b for a, b in zip(split[:-1], split[1:]))
        cut = np.cumsum(split)[:-1]
        yield k, split, np.split(cls[so:so + L], cut), np.split(ids[so:so + L], cut), block[bo:bo + nb]
        so, bo = so + L, bo + nb
    assert so == len(cls) and bo == len(block)


def match_fixture():
    """the crafted frames: (name, det, gt, gt_id, gt_name, expected det_id, expected det_cls)"""
    z = np.load(os.path.join(GOLDEN, 'labels_match.npz'))
    for name in z['names']:
        g = lambda k: z['%s:%s' % (name, k)]
        yield str(name), g('det'), g('gt'), g('gt_id'), g('gt_name'), g('det_id'), g('det_cls')


def match_fixture_random():
    """the seeded random frames (n_det, n_gt <= 12; every second one with float32 boxes): same tuple, name = index"""
    z = np.load(os.path.join(GOLDEN, 'labels_match.npz'))
    do = go = 0
    for k, (nd, ng, f32) in enumerate(zip(z['random:nd'], z['random:ng'], z['random:f32'])):
        dt = np.float32 if f32 else np.float64
        yield (k, z['random:det'][do:do + nd].astype(dt), z['random:gt'][go:go + ng].astype(dt),
               z['random:gt_id'][go:go + ng], z['random:gt_name'][go:go + ng], z['random:det_id'][do:do + nd],
               z['random:det_cls'][do:do + nd])
        do, go = do + nd, go + ng
    assert do == len(z['random:det']) and go == len(z['random:gt'])
