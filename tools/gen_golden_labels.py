#!/usr/bin/env python
"""Generate tests/golden/labels_gt.npz and tests/golden/labels_match.npz by running the REFERENCE's label code.

    python tools/gen_golden_labels.py --reference <checkout of the reference project>

``TrackingModule.generate_gt`` (tracking_model.py:294-351) and ``generate_det_id_matrix`` (dataset/common.py:95-111) are
imported from the checkout and called as they are; nothing of them is copied, only data is written.  Modules their
imports pull in and these two functions never touch (``solvers``, ``pyproj``, ``cv2``, ``numba``, ``torchvision``) are
replaced by empty stand-ins, and dataset/common.py is loaded on its own (the ``dataset`` package's __init__ imports the
whole data pipeline).

``motmetrics`` IS touched - ``calculate_distance`` calls ``motmetrics.distances.iou_matrix`` - and is not installed
here.  The generator installs a stand-in written from that function's definition (1 - IoU of x, y, w, h boxes in
float64, NaN where the distance exceeds ``max_iou``: tests/labels_ref.iou_distance).  What labels_match.npz pins against
the reference is therefore everything AROUND that call: the x2 - x1 conversion in the input's dtype, NaN -> 10, the
rounding to float32, ``torch.min``'s arg-min, the sequential overwrite and the class codes.  So that the fixture does
not depend on the library's version or on rounding, the generator asserts that every distance is more than 1e-6 away
from the 0.5 gate and that the float32 minimum of every row is either more than 1e-6 below the runner-up or exactly
equal to it (identical detection boxes: the one tie admitted) - and fails otherwise.

labels_gt.npz: chains of T = 2 with n = (1,1), (3,0), (0,2), (5,7), T = 3 and T = 8 with ragged n and an empty middle
frame; duplicate ids inside a frame (the first k wins), a positive detection linked to a cls 0 successor, classes in
{-1, 0, 1}, a positive detection with id -1 facing a -1 in both neighbour frames - each asserted to occur.
labels_match.npz: two gts on one detection, a gt overlapping nothing (-> det 0), Car / DontCare / other names, n_gt = 0
(the reference cannot run that one - ``torch.min`` over an empty row raises - so its expectation is the literal "no gt
assigns anything": -1 / 0), identical detection boxes, float32 boxes and a seeded frame of 9 x 11.

Both files also hold seeded random inputs with what the reference made of them, stored joined: 200 chains (T = 2 .. 8,
n <= 12, ``random:*`` in labels_gt.npz) and 60 frames (n_det, n_gt <= 12, every second one float32; a draw that misses
the margins above is drawn again; ``random:*`` in labels_match.npz).  tests/labels_ref.py reads them back.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True
import labels_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def import_reference(path):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def njit(*a, **k):
        return a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f)
    stub('solvers', ortools_solve=None)
    stub('pyproj')
    stub('cv2')
    stub('numba', njit=njit, jit=njit)
    stub('torchvision')
    mm = stub('motmetrics')
    mm.distances = stub('motmetrics.distances', iou_matrix=labels_ref.iou_distance)
    sys.path.insert(0, os.path.abspath(path))
    from tracking_model import TrackingModule
    spec = importlib.util.spec_from_file_location('reference_dataset_common', os.path.join(path, 'dataset', 'common.py'))
    common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(common)
    return TrackingModule, common


# ---- generate_gt ------------------------------------------------------------------------------------------------------
def gt_cases():
    rng = np.random.default_rng(20261)
    a = lambda *v: np.asarray(v, np.int64)
    cases = [
        ('t2_1_1', [a(1), a(1)], [a(7), a(7)]),
        ('t2_3_0', [a(1, 0, 1), a()], [a(3, 4, 5), a()]),
        ('t2_0_2', [a(), a(1, -1)], [a(), a(2, 2)]),
        # duplicates in frame 1 (ids 4, 4: the first wins), a positive linked to a cls 0 (id 9) and a cls -1 (id 6)
        # successor, a positive with id -1 facing -1s
        ('t2_5_7', [a(1, 1, 0, 1, -1), a(1, 1, 0, 1, -1, 1, 0)], [a(4, 9, 4, -1, 6), a(5, 4, 9, 4, 6, -1, -1)]),
        ('t3_4_0_3', [a(1, 1, 0, 1), a(), a(1, 1, 0)], [a(1, 2, 3, -1), a(), a(1, -1, 3)]),
        # id -1 positive in the middle frame with -1 in both neighbours; duplicates inside frames 0 and 2
        ('t3_3_5_2', [a(1, 0, 1), a(1, 1, 1, -1, 0), a(1, 1)], [a(-1, 2, 2), a(-1, 2, 8, 8, 2), a(8, 8)]),
    ]
    split8 = [2, 3, 0, 4, 1, 5, 2, 3]
    cls, ids = labels_ref.random_chain(rng, split8, 4)
    cases.append(('t8_ragged', cls, ids))
    split8b = [3, 1, 4, 2, 5, 3, 1, 2]
    cls, ids = labels_ref.random_chain(rng, split8b, 3)
    cases.append(('t8_full', cls, ids))
    return cases


def run_generate_gt(TrackingModule, cls, ids):
    split = [len(c) for c in cls]
    L = sum(split)
    t = lambda v: torch.from_numpy(np.asarray(v, np.int64)).view(1, -1, 1)
    got = TrackingModule.generate_gt(None, torch.zeros(L), [t(c) for c in cls], [t(i) for i in ids],
                                     [torch.tensor([n]) for n in split])
    gt_det, gt_link, gt_new, gt_end = got
    assert [tuple(l.shape) for l in gt_link] == [(1, a, b) for a, b in zip(split[:-1], split[1:])]
    return gt_det.numpy(), [l[0].numpy() for l in gt_link], gt_new.numpy(), gt_end.numpy()


def gen_gt(TrackingModule):
    out, names = {}, []
    seen = dict(dup=False, cls0_succ=False, neg1=False, classes=set(), empty_mid=False)
    for name, cls, ids in gt_cases():
        split = [len(c) for c in cls]
        d, links, n, e = run_generate_gt(TrackingModule, cls, ids)
        names.append(name)
        out[name + ':split'] = np.asarray(split, np.int64)
        out[name + ':cls'] = np.concatenate(cls).astype(np.int64)
        out[name + ':ids'] = np.concatenate(ids).astype(np.int64)
        out[name + ':block'] = labels_ref.block_of((d, links, n, e))
        seen['empty_mid'] |= any(s == 0 for s in split[1:-1])
        for t in range(len(split)):
            seen['classes'] |= set(int(c) for c in cls[t])
            for j in range(split[t]):
                if cls[t][j] != 1 or t == len(split) - 1:
                    continue
                ks = np.nonzero(ids[t + 1] == ids[t][j])[0]
                if len(ks) > 1:
                    seen['dup'] = True
                    assert links[t][j, ks[0]] == 1 and links[t][j].sum() == 1
                if len(ks) and cls[t + 1][ks[0]] == 0:
                    seen['cls0_succ'] = True
                if len(ks) and ids[t][j] == -1:
                    seen['neg1'] = True
    assert seen['dup'] and seen['cls0_succ'] and seen['neg1'] and seen['empty_mid'] and seen['classes'] == {-1, 0, 1}, seen
    out['names'] = np.asarray(names)
    # 200 seeded random chains, T <= 8, n <= 12, stored joined (the blocks hold 0 / 1 only: uint8)
    rng = np.random.default_rng(20261018)
    splits, r_cls, r_ids, r_block = [], [], [], []
    for k in range(200):
        T = 2 + k % 7
        split = [int(n) for n in rng.integers(0, 13, T)]
        cls, ids = labels_ref.random_chain(rng, split, int(rng.integers(2, 8)))
        block = labels_ref.block_of(run_generate_gt(TrackingModule, cls, ids))
        assert set(np.unique(block)) <= {0.0, 1.0}
        splits.append(split + [-1] * (8 - T))
        r_cls += cls
        r_ids += ids
        r_block.append(block.astype(np.uint8))
    out['random:splits'] = np.asarray(splits, np.int8)
    out['random:cls'] = np.concatenate(r_cls).astype(np.int8)
    out['random:ids'] = np.concatenate(r_ids).astype(np.int8)
    out['random:block'] = np.concatenate(r_block)
    path = os.path.join(GOLDEN, 'labels_gt.npz')
    np.savez_compressed(path, **out)
    print('%s: %d crafted and %d random chains, %d bytes' % (path, len(names), len(splits), os.path.getsize(path)))


# ---- generate_det_id_matrix -------------------------------------------------------------------------------------------
def match_cases():
    rng = np.random.default_rng(20262)
    b = lambda *rows: np.asarray(rows, np.float64).reshape(-1, 4)
    i = lambda *v: np.asarray(v, np.int64)
    det3 = b([10, 10, 60, 50], [100, 20, 150, 70], [200, 30, 260, 90])
    cases = [
        # gts 0 and 2 both sit on det 1 (the later one stays), gt 1 on det 2
        ('two_on_one', det3, b([102, 22, 151, 69], [203, 31, 258, 92], [98, 18, 149, 72]), i(11, 12, 13), i(0, 0, 3)),
        # gt 1 overlaps nothing: a row of 10s, which lands on det 0 and overwrites gt 0's entry there
        ('no_overlap', det3, b([12, 11, 61, 52], [500, 500, 540, 560]), i(21, 22), i(0, -1)),
        ('names', det3, b([11, 9, 59, 51], [101, 21, 152, 69], [198, 33, 262, 88]), i(31, 32, 33), i(0, -1, 5)),
        ('no_gt', det3, b(), i(), i()),
        # dets 0 and 1 are the same box: bitwise-equal distances, the smaller index takes the gt
        ('identical_dets', b([100, 20, 150, 70], [100, 20, 150, 70], [300, 30, 360, 90]),
         b([103, 22, 152, 71], [301, 28, 358, 93]), i(41, 42), i(0, 0)),
    ]
    det, gt, gid, gname = labels_ref.random_frame(rng, 9, 11)
    cases.append(('seeded_9x11', det, gt, gid, gname))
    det, gt, gid, gname = labels_ref.random_frame(rng, 6, 4)
    cases.append(('float32_6x4', (det + 0.3).astype(np.float32), (gt + 0.7).astype(np.float32), gid, gname))
    return cases


def check_margins(name, det, gt):
    """the conditions that make the expectation independent of library version and rounding"""
    if len(gt) == 0 or len(det) == 0:
        return
    raw = labels_ref.iou_distance(labels_ref.xywh(gt), labels_ref.xywh(det), max_iou=np.inf)
    assert np.all(np.abs(raw[~np.isnan(raw)] - 0.5) > 1e-6), (name, 'a distance within 1e-6 of the gate')
    mat = labels_ref.iou_distance(labels_ref.xywh(gt), labels_ref.xywh(det), max_iou=0.5)
    mat[np.isnan(mat)] = 10
    mat = mat.astype(np.float32).astype(np.float64)
    for r, row in enumerate(mat):
        if len(row) < 2 or row.min() == 10:
            continue  # one detection, or a row of 10s: the arg-min is index 0 by definition
        s = np.sort(row)
        assert s[1] - s[0] > 1e-6 or s[1] == s[0], (name, r, 'minimum and runner-up closer than 1e-6')


def gen_match(common):
    out, names = {}, []
    for name, det, gt, gid, gname in match_cases():
        check_margins(name, det, gt)
        if len(gt):
            rid, rcls = common.generate_det_id_matrix(det.copy(), {'bbox': gt.copy(), 'id': gid, 'name': gname})
            assert rid.dtype == torch.long and tuple(rid.shape) == (len(det), 1) == tuple(rcls.shape)
            rid, rcls = rid.numpy().reshape(-1), rcls.numpy().reshape(-1)
        else:  # the reference raises on an empty gt set: no gt assigns anything
            rid, rcls = np.full(len(det), -1, np.int64), np.zeros(len(det), np.int64)
        names.append(name)
        out[name + ':det'], out[name + ':gt'] = det, gt
        out[name + ':gt_id'], out[name + ':gt_name'] = gid, gname
        out[name + ':det_id'], out[name + ':det_cls'] = rid, rcls
    out['names'] = np.asarray(names)
    # 60 seeded random frames, n_det and n_gt in 1 .. 12, every second one with float32 boxes, stored joined (float32
    # values are exact in the float64 array).  A draw that misses the margins is drawn again.
    rng = np.random.default_rng(77)
    cols = {k: [] for k in ('nd', 'ng', 'f32', 'det', 'gt', 'gt_id', 'gt_name', 'det_id', 'det_cls')}
    while len(cols['nd']) < 60:
        k = len(cols['nd'])
        nd, ng = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        det, gt, gid, gname = labels_ref.random_frame(rng, nd, ng)
        if k % 2:
            det, gt = det.astype(np.float32), gt.astype(np.float32)
        try:
            check_margins('random %d' % k, det, gt)
        except AssertionError:
            continue
        rid, rcls = common.generate_det_id_matrix(det.copy(), {'bbox': gt.copy(), 'id': gid, 'name': gname})
        for key, v in (('nd', nd), ('ng', ng), ('f32', k % 2 == 1), ('det', det.astype(np.float64)),
                       ('gt', gt.astype(np.float64)), ('gt_id', gid), ('gt_name', gname),
                       ('det_id', rid.numpy().reshape(-1)), ('det_cls', rcls.numpy().reshape(-1))):
            cols[key].append(v)
    for key in ('nd', 'ng', 'f32'):
        out['random:' + key] = np.asarray(cols[key])
    for key in ('det', 'gt', 'gt_id', 'gt_name', 'det_id', 'det_cls'):
        out['random:' + key] = np.concatenate(cols[key])
    out['car'], out['dontcare'] = np.int64(common.LABEL['Car']), np.int64(common.LABEL['DontCare'])
    path = os.path.join(GOLDEN, 'labels_match.npz')
    np.savez_compressed(path, **out)
    print('%s: %d crafted and %d random frames, %d bytes' % (path, len(names), len(cols['nd']), os.path.getsize(path)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference project')
    args = ap.parse_args()
    TrackingModule, common = import_reference(args.reference)
    gen_gt(TrackingModule)
    gen_match(common)


if __name__ == '__main__':
    main()
