"""CLEAR-MOT evaluation of tracked sequences on the device: the reference's ``kitti_devkit.evaluate_tracking.evaluate``
(the call behind every validation epoch of main.py and eval_seq.py:124), which turns a KITTI result file into MOTA,
MOTP, ID switches, fragments and MT / PT / ML.

    from mmmot_amd.evaluate import evaluate            # instead of kitti_devkit.evaluate_tracking
    MOTA, MOTP, recall, prec, F1, fp, fn, id_switches = evaluate(step, result_path, part, gt_path='./data/tracking')

or, without files, straight from what the pipeline holds:

    tr = labels_from_tracks(feed_dets, pipe.tracks)
    m = evaluate_sequences(load_kitti(label_file, 'car', n_frames, True), tr)     # m.MOTA, m.id_switches, ...

The Hungarian association of every frame, the ignore logic, the per-frame counters and the trajectory scan run in
csrc/clear_mot.hip (one workgroup per frame, one lane per ground-truth trajectory); a call is one upload, four
launches and one read-back.  The host parses the label files into packed tables (``Labels``), sorts the ground-truth
objects into trajectories, and forms the dozen ratios of evaluate_tracking.py:745-791 from the totals.

Kept from the reference: class selection by substring (car + van, pedestrian + person_sitting, always DontCare);
non-DontCare rows with track ID -1 are dropped; tracker frames past the ground truth's are loaded (they count for the
tracker's trajectories) but not evaluated; FAR and MODP divide by the seqmap's frame counts.  Different: a tracker
file that repeats a (frame, ID) raises ``ValueError`` (there: ``return False``), and so does a frame with more than 128
boxes on a side or 64 DontCare areas.  Equal-cost matchings are broken by column index, not munkres's way.

HOTA and IDF1 (``hota_sequences`` / ``evaluate_hota`` -> ``Hota``; csrc/hota.hip) are built from the rules written down
in DESIGN.md section 13 and restated in tests/hota_ref.py, on the same packed tables:

    h = hota_sequences(gt, tr)                         # h.HOTA, h.AssA, h.IDF1, h.summary()
    h = evaluate_hota(step, result_path, part, gt_path='./data/tracking', cls='car')

No agreement with any published implementation of these metrics is claimed.

3D evaluation (``evaluate_3d_sequences`` / ``evaluate_3d`` -> ``Mot3D``; csrc/mot3d.hip): the CLEAR-MOT evaluation above
with the cost 1 - IoU of the rotated 3D boxes (or of their bird's-eye-view footprints) in place of the image-plane IoU,
and its sweep over 40 recall levels, thresholding the tracks by their mean score (AMOTA, sAMOTA, AMOTP).  The labels
carry the 3D boxes and scores in ``Labels.box3d``:

    gt = load_kitti(label_file, 'car', n_frames, True, box3d=True)
    tr = labels_from_tracks(feed_dets, pipe.tracks, box3d=True, scores=scores)
    m = evaluate_3d_sequences(gt, tr)                  # m.AMOTA, m.sAMOTA, m.AMOTP, m.all.MOTA, m.best, m.summary()

The rules are written down in DESIGN.md section 13 "3D / AMOTA" and restated in tests/mot3d_ref.py.  No agreement with
any published 3D evaluator is claimed.
"""
import math
import os
from dataclasses import dataclass, field

import numpy as np

from .torch_ops import CLEAR_MOT_MAX_BOXES, CLEAR_MOT_MAX_DONTCARE, CLEAR_MOT_SEQ_INTS, clear_mot_layout
from .torch_ops import FP64_SECTIONS, sections
from .torch_ops import (HOTA_ALPHAS, HOTA_FRAME_D, HOTA_FRAME_I, HOTA_MAX_CELLS, HOTA_MAX_IDS, HOTA_SEQ_D, HOTA_SEQ_I,
                        hota_layout)
from .torch_ops import MOT3D_BOX, MOT3D_MAX_LEVELS, MOT3D_MODES, mot3d_layout

TRAIN_SEQ_ID = ['0003', '0001', '0013', '0009', '0004', '0020', '0006', '0015', '0008', '0012']
VALID_SEQ_ID = ['0005', '0007', '0017', '0011', '0002', '0014', '0000', '0010', '0016', '0019', '0018']
TRAINVAL_SEQ_ID = ['%04d' % i for i in range(21)]
# columns of Labels.rows
SEQ, FRAME, TID, CLS, TRUNC, OCC, X1, Y1, X2, Y2 = range(10)
MAIN, NEIGHBOUR, DONTCARE = 0, 1, 2  # class codes


def class_names(cls):
    """(loaded class substrings, the neighbouring class) of evaluate_tracking.py:257-263 / :521"""
    c = cls.lower()
    if 'car' in c:
        return ['car', 'van', 'dontcare'], 'van' if c == 'car' else None
    if 'pedestrian' in c:
        return ['pedestrian', 'person_sitting', 'dontcare'], 'person_sitting' if c == 'pedestrian' else None
    return [c, 'dontcare'], None


def class_code(name, cls):
    """class code of a lower-case object type, or None when the evaluation of ``cls`` does not load it"""
    loaded, neighbour = class_names(cls)
    if not any(s in name for s in loaded):
        return None
    return DONTCARE if name == 'dontcare' else (NEIGHBOUR if name == neighbour else MAIN)


@dataclass
class Labels:
    """Packed label tables of S sequences.  rows: float64 [n, 10] = sequence, frame, track ID, class code, truncation,
    occlusion, x1, y1, x2, y2 in file order; n_frames: the seqmap's frame counts; length: frames held (n_frames, or more
    where a row lies beyond); n_traj: distinct non-DontCare track IDs per sequence; box3d: None, or float64 [n, 8] = h, w,
    l, x, y, z, rotation_y, score, row for row beside ``rows`` (KITTI camera coordinates; the score of ground truth is 0)."""
    rows: np.ndarray
    n_frames: np.ndarray
    length: np.ndarray
    n_traj: np.ndarray
    cls: str = 'car'
    ground_truth: bool = False
    box3d: np.ndarray = None

    @property
    def n_sequences(self):
        return len(self.n_frames)


def concat(labels):
    """several Labels (one per sequence, say) as one"""
    labels = list(labels)
    rows, o = [], 0
    for lb in labels:
        r = lb.rows.copy()
        r[:, SEQ] += o
        o += lb.n_sequences
        rows.append(r)
    cat = lambda k: np.concatenate([getattr(lb, k) for lb in labels])
    has3d = [lb.box3d is not None for lb in labels]
    if any(has3d) and not all(has3d):
        raise ValueError('concat: some Labels hold box3d and some do not')
    return Labels(np.concatenate(rows).reshape(-1, 10), cat('n_frames'), cat('length'), cat('n_traj'), labels[0].cls,
                  labels[0].ground_truth, cat('box3d').reshape(-1, 8) if all(has3d) and labels else None)


def _finish(parsed, cls, n_frames, ground_truth, what, b3=None):
    """rows (frame, id, code, trunc, occ, box) of ONE sequence -> Labels: the bookkeeping of _loadData :293-328.  b3: None,
    or per parsed row its eight box3d values."""
    length, seen, ids, rows, kept3 = int(n_frames), set(), set(), [], []
    for k, (frame, tid, code, trunc, occ, box) in enumerate(parsed):
        if tid == -1 and code != DONTCARE:
            continue
        if b3 is not None:
            kept3.append(b3[k])
        if frame < 0:
            raise ValueError('%s: negative frame index %d' % (what, frame))
        if frame >= length:
            if frame - length >= 500:  # the reference's list grows by max(500, frame - length) and then misses the frame
                raise ValueError('%s: frame %d lies 500 or more frames past the sequence (%d)' % (what, frame, length))
            length += 500
        if not ground_truth:
            if (frame, tid) in seen:
                raise ValueError('%s: track ids are not unique: id %d occurs twice in frame %d' % (what, tid, frame))
            seen.add((frame, tid))
        if code != DONTCARE:
            ids.add(tid)
        rows.append([0, frame, tid, code, trunc, occ] + list(box))
    return Labels(np.asarray(rows, np.float64).reshape(-1, 10), np.asarray([n_frames], np.int64),
                  np.asarray([length], np.int64), np.asarray([len(ids)], np.int64), cls, bool(ground_truth),
                  None if b3 is None else np.asarray(kept3, np.float64).reshape(-1, 8))


def load_kitti(path, cls, n_frames, ground_truth, box3d=False):
    """One KITTI tracking label / result file as Labels (evaluate_tracking.py:227-361 _loadData for one sequence).
    ``box3d``: also read columns 10..16 (h, w, l, x, y, z, rotation_y) and, of a result file, column 17 as the score (0
    for ground truth or where the column is absent) into ``Labels.box3d``."""
    parsed, b3 = [], [] if box3d else None
    with open(path, 'r') as f:
        for line in f:
            fields = line.strip().split(' ')
            if len(fields) < 3:
                continue
            code = class_code(fields[2].lower(), cls)
            if code is None:
                continue
            if len(fields) < 17 or (not ground_truth and len(fields) > 18):
                raise ValueError('%s: file is not in KITTI format' % path)
            parsed.append((int(float(fields[0])), int(float(fields[1])), code, int(float(fields[3])),
                           int(float(fields[4])), [float(v) for v in fields[6:10]]))
            if box3d:
                score = float(fields[17]) if not ground_truth and len(fields) > 17 else 0.
                b3.append([float(v) for v in fields[10:17]] + [score])
    return _finish(parsed, cls, n_frames, ground_truth, path, b3)


def labels_from_tracks(frames, ids, frame_idx=None, cls='car', n_frames=None, ground_truth=False, box3d=False,
                       scores=None):
    """The Labels that ``load_kitti`` reads from the file ``tracks.write_kitti_tracks(path, frames, ids, frame_idx)``
    writes, without the file: kept detections only, values through the same '{:.4f}' of the fp32 value.  ``n_frames``:
    the sequence's frame count (default: one past the last frame).  ``box3d``: also fill ``Labels.box3d`` from
    ``dimensions`` (lhw -> hwl), ``location``, ``rotation_y`` and ``scores[t][j]`` (default 0.9; 0 for ground truth), as
    ``load_kitti(box3d=True)`` reads them from the file ``write_kitti_tracks(..., scores=scores)`` writes."""
    from .tracks import KITTI_NAMES
    f4 = lambda v: float('{:.4f}'.format(float(np.float32(v))))
    parsed, last, b3 = [], -1, [] if box3d else None
    for t, (d, fid) in enumerate(zip(frames, ids)):
        frame = t if frame_idx is None else int(frame_idx[t])
        last = max(last, frame)
        fid = np.asarray(fid)
        for j in np.flatnonzero(fid >= 0):
            name = d['name'][j] if 'name' in d else 0
            name = name if isinstance(name, str) else KITTI_NAMES[int(name)]
            code = class_code(name.lower(), cls)
            if code is None:
                continue
            trunc = int(f4(d['truncated'][j])) if 'truncated' in d else -1
            occ = int(d['occluded'][j]) if 'occluded' in d else -1
            parsed.append((frame, int(fid[j]), code, trunc, occ, [f4(v) for v in np.asarray(d['bbox'][j]).reshape(-1)]))
            if box3d:
                score = 0. if ground_truth else f4(0.9 if scores is None else scores[t][j])
                b3.append([f4(v) for v in np.asarray(d['dimensions'][j])[[1, 2, 0]]] +
                          [f4(v) for v in np.asarray(d['location'][j]).reshape(-1)] + [f4(d['rotation_y'][j]), score])
    return _finish(parsed, cls, last + 1 if n_frames is None else n_frames, ground_truth, 'labels_from_tracks', b3)


@dataclass
class ClearMot:
    """What compute3rdPartyMetrics leaves on the reference's evaluation object, under the same names."""
    cls: str = 'car'
    MOTA: float = 0.0
    MOTP: float = 0.0
    MOTAL: float = 0.0
    MODA: float = 0.0
    MODP: object = 0.0
    recall: float = 0.0
    precision: float = 0.0
    F1: float = 0.0
    FAR: object = 0.0
    MT: float = 0.0
    PT: float = 0.0
    ML: float = 0.0
    tp: int = 0
    fp: int = 0
    fn: int = 0
    id_switches: int = 0
    fragments: int = 0
    n_gt: int = 0
    n_gt_trajectories: int = 0
    n_tr: int = 0
    n_tr_trajectories: int = 0
    itp: int = 0
    ifn: int = 0
    n_igt: int = 0
    n_itr: int = 0
    total_cost: float = 0.0
    n_mt: int = 0
    n_pt: int = 0
    n_ml: int = 0
    n_ignored_trajectories: int = 0
    tps: list = field(default_factory=list)
    itps: list = field(default_factory=list)
    fps: list = field(default_factory=list)
    fns: list = field(default_factory=list)
    ifns: list = field(default_factory=list)
    n_gts: list = field(default_factory=list)
    n_trs: list = field(default_factory=list)
    n_igts: list = field(default_factory=list)
    n_itrs: list = field(default_factory=list)
    seq_costs: list = field(default_factory=list)      # per sequence: sum of 1 - c over the matches
    seq_modp: list = field(default_factory=list)       # per sequence: sum of MODP_t
    seq_id_switches: list = field(default_factory=list)
    seq_fragments: list = field(default_factory=list)
    MODP_t: np.ndarray = None            # [frames]
    gt_tracker: np.ndarray = None        # per ground-truth object, sorted by (sequence, track ID, frame): matched ID or -1
    gt_ignored: np.ndarray = None        # the same order: ignored flag
    traj_key: np.ndarray = None          # [trajectories, 3]: sequence, track ID, objects

    def stats(self):
        """the 21 values of the devkit's stats_<cls>.txt line (:885-889)"""
        return (self.MOTA, self.MOTP, self.MOTAL, self.MODA, self.MODP, self.recall, self.precision, self.F1, self.FAR,
                self.MT, self.PT, self.ML, self.tp, self.fp, self.fn, self.id_switches, self.fragments, self.n_gt,
                self.n_gt_trajectories, self.n_tr, self.n_tr_trajectories)

    def stats_line(self):
        return '%.6f ' * 21 % self.stats()

    def summary(self):
        """the tuple the reference's ``evaluate`` returns"""
        return self.MOTA, self.MOTP, self.recall, self.precision, self.F1, self.fp, self.fn, self.id_switches


def pack(gt, tracker):
    """Labels of the ground truth and the tracker -> the tables of mmmot_clear_mot: a dict of numpy arrays plus the host
    side's bookkeeping.  Raises ValueError on frames beyond the kernel's limits, before anything reaches the device."""
    gt = concat(gt) if isinstance(gt, (list, tuple)) else gt
    tracker = concat(tracker) if isinstance(tracker, (list, tuple)) else tracker
    S = gt.n_sequences
    if tracker.n_sequences != S:
        raise ValueError('evaluate: %d ground-truth sequences, %d tracker sequences' % (S, tracker.n_sequences))
    if np.any(tracker.length < gt.length):
        raise ValueError('evaluate: the ground truth holds frames the tracker table does not reach')
    F = gt.length.astype(np.int64)
    foff = np.concatenate([[0], np.cumsum(F)])
    NF = int(foff[-1])

    def by_frame(rows, sel):
        """the rows ``sel`` (a mask) in frame order (stable: file order within a frame), their index in ``rows``,
        per-frame offset / count"""
        idx = np.flatnonzero(sel)
        fr = foff[rows[idx, SEQ].astype(np.int64)] + rows[idx, FRAME].astype(np.int64)
        order = np.argsort(fr, kind='stable')
        idx, fr = idx[order], fr[order]
        cnt = np.bincount(fr, minlength=NF).astype(np.int64)
        return rows[idx], idx, np.cumsum(cnt) - cnt, cnt

    g_rows, g_idx, g_off, g_cnt = by_frame(gt.rows, gt.rows[:, CLS] != DONTCARE)
    d_rows, _, d_off, d_cnt = by_frame(gt.rows, gt.rows[:, CLS] == DONTCARE)
    tr = tracker.rows
    t_rows, t_idx, t_off, t_cnt = by_frame(tr, tr[:, FRAME] < F[tr[:, SEQ].astype(np.int64)])
    if NF and (max(g_cnt.max(), t_cnt.max()) > CLEAR_MOT_MAX_BOXES or d_cnt.max() > CLEAR_MOT_MAX_DONTCARE):
        raise ValueError('evaluate: a frame holds more than %d boxes on a side or more than %d DontCare areas'
                         % (CLEAR_MOT_MAX_BOXES, CLEAR_MOT_MAX_DONTCARE))
    nG, nT, nD = len(g_rows), len(t_rows), len(d_rows)
    # trajectories: the ground-truth objects sorted by (sequence, track ID, frame)
    traj_obj = np.lexsort((g_rows[:, TID], g_rows[:, SEQ]))  # stable: frame order within a key
    key = g_rows[traj_obj][:, [SEQ, TID]].astype(np.int64)
    first = np.flatnonzero(np.r_[True, np.any(key[1:] != key[:-1], axis=1)]) if nG else np.zeros(0, np.int64)
    NTr = len(first)
    traj_off = np.r_[first, nG].astype(np.int64)
    traj_seq = key[first, 0] if NTr else np.zeros(0, np.int64)
    toff = np.searchsorted(traj_seq, np.arange(S + 1))
    frames = np.stack([g_off, g_cnt, t_off, t_cnt, d_off, d_cnt], axis=1) if NF else np.zeros((0, 6), np.int64)
    return {
        'sizes': [nG, nT, nD, NF, NTr, S],
        'boxes': np.concatenate([g_rows[:, X1:], t_rows[:, X1:], d_rows[:, X1:]]).astype(np.float64),
        'frames': frames, 'g_attr': g_rows[:, [TRUNC, OCC, CLS]], 't_attr': t_rows[:, [TID, CLS]],
        'traj_off': traj_off, 'traj_obj': traj_obj, 'seq_off': np.stack([foff, toff], axis=1),
        'g_cnt': g_cnt, 't_cnt': t_cnt, 'foff': foff, 'g_idx': g_idx, 't_idx': t_idx,
        'traj_key': np.stack([traj_seq, key[first, 1] if NTr else traj_seq, np.diff(traj_off)], axis=1),
        'n_frames': gt.n_frames, 'n_gt_trajectories': int(gt.n_traj.sum()),
        'n_tr_trajectories': int(tracker.n_traj.sum()), 'cls': gt.cls,
    }


def finish(p, out):
    """the packed tables and the device's output sections (numpy) -> ClearMot: per-sequence lists, totals and the
    ratios of evaluate_tracking.py:745-791"""
    nG, nT, nD, NF, NTr, S = p['sizes']
    seq_i = out['seq_i'].reshape(S + 1, CLEAR_MOT_SEQ_INTS).astype(np.int64)
    seq_d = out['seq_d'].reshape(S + 1, 2)
    frame_i = out['frame_i'].reshape(NF, 6)
    if NF and frame_i.min() < 0 or NTr and out['traj_i'].min() < -1:
        raise RuntimeError('mmmot_clear_mot: a frame or a trajectory outside the launch limits reached the kernel')
    foff = p['foff']
    per_seq = lambda cnt: [int(cnt[foff[s]:foff[s + 1]].sum()) for s in range(S)]
    m = ClearMot(cls=p['cls'])
    tp_all, m.itps, m.fns, m.ifns, m.fps, m.n_itrs = (seq_i[:S, q].tolist() for q in range(6))
    m.tps = [a - b for a, b in zip(tp_all, m.itps)]  # the per-sequence list leaves the ignored ones out, the total does not
    m.n_igts = [a + b for a, b in zip(m.ifns, m.itps)]
    m.n_gts, m.n_trs = per_seq(p['g_cnt']), per_seq(p['t_cnt'])
    m.seq_costs, m.seq_modp = seq_d[:S, 0].tolist(), seq_d[:S, 1].tolist()
    m.seq_id_switches, m.seq_fragments = seq_i[:S, 6].tolist(), seq_i[:S, 7].tolist()
    tot = [int(v) for v in seq_i[S]]
    m.tp, m.itp, m.fn, m.ifn, m.fp, m.n_itr, m.id_switches, m.fragments = tot[:8]
    m.n_mt, m.n_pt, m.n_ml, m.n_ignored_trajectories = tot[8:12]
    m.n_igt = m.ifn + m.itp
    m.n_gt = nG - m.n_igt
    m.n_tr = nT
    m.total_cost = float(seq_d[S, 0])
    m.n_gt_trajectories, m.n_tr_trajectories = p['n_gt_trajectories'], p['n_tr_trajectories']
    m.MODP_t = out['frame_d'].reshape(NF, 2)[:, 1].copy()
    gt_out = out['gt_out'].reshape(nG, 2)[p['traj_obj']]
    m.gt_tracker, m.gt_ignored = gt_out[:, 0].astype(np.int64), gt_out[:, 1].astype(bool)
    m.traj_key = p['traj_key']

    n_tracked = m.n_gt_trajectories - m.n_ignored_trajectories
    if n_tracked == 0:
        m.MT = m.PT = m.ML = 0.
    else:
        m.MT, m.PT, m.ML = m.n_mt / float(n_tracked), m.n_pt / float(n_tracked), m.n_ml / float(n_tracked)
    if (m.fp + m.tp) == 0 or (m.tp + m.fn) == 0:
        m.recall = m.precision = 0.
    else:
        m.recall = m.tp / float(m.tp + m.fn)
        m.precision = m.tp / float(m.fp + m.tp)
    m.F1 = 0. if (m.recall + m.precision) == 0 else 2. * (m.precision * m.recall) / (m.precision + m.recall)
    n_frames = int(np.sum(p['n_frames']))
    m.FAR = 'n/a' if n_frames == 0 else m.fp / float(n_frames)
    if m.n_gt == 0:
        m.MOTA = m.MODA = m.MOTAL = -float('inf')
    else:
        m.MOTA = 1 - (m.fn + m.fp + m.id_switches) / float(m.n_gt)
        m.MODA = 1 - (m.fn + m.fp) / float(m.n_gt)
        m.MOTAL = m.MOTA if m.id_switches == 0 else 1 - (m.fn + m.fp + math.log10(m.id_switches)) / float(m.n_gt)
    m.MOTP = float('inf') if m.tp == 0 else m.total_cost / float(m.tp)
    m.MODP = 'n/a' if n_frames == 0 else float(seq_d[S, 1]) / float(n_frames)
    return m


def upload(p, inp, n_in, device):
    """the tables ``p`` of an evaluator call as its one int32 block on ``device`` (``inp``, ``n_in``: the operator's
    input layout): one pinned block, the fp64 sections as their bit patterns, one asynchronous copy"""
    import torch
    host = torch.empty(n_in, dtype=torch.int32, pin_memory=device != 'meta')
    h = host.numpy()
    for name, (o, n) in inp.items():
        if name in FP64_SECTIONS:
            h[o:o + n].view(np.float64)[:] = np.asarray(p[name], np.float64).reshape(-1)
        else:
            h[o:o + n] = np.asarray(p[name]).reshape(-1)
    return host.to(device, non_blocking=True)


def read_back(res, outl):
    """an evaluator's result block -> its sections (``outl``: the operator's output layout) as numpy arrays"""
    return sections(res.cpu().numpy(), outl)


def evaluate_sequences(gt, tracker, cls='car', min_overlap=0.5, max_truncation=0, min_height=25, max_occlusion=2,
                       device='cuda'):
    """CLEAR-MOT statistics of tracker Labels against ground-truth Labels (one Labels of S sequences, or a list with
    one per sequence) on the device: one upload, the launches of mmmot_clear_mot, one read-back."""
    import torch
    p = pack(gt, tracker)
    p['cls'] = cls
    inp, outl, n_in, _ = clear_mot_layout(p['sizes'])
    res = torch.ops.mmmot.clear_mot(upload(p, inp, n_in, device), p['sizes'],
                                    [float(min_overlap), float(min_height), float(max_truncation), float(max_occlusion)])
    return finish(p, read_back(res, outl))


def sequences_of(part, gt_path):
    """(names, frame counts) of the sequences of ``part`` in the seqmap under ``gt_path`` (:106-123)"""
    ids = {'val': VALID_SEQ_ID, 'train': TRAIN_SEQ_ID, 'all': TRAINVAL_SEQ_ID}.get(part, [])
    names, n_frames = [], []
    with open(os.path.join(gt_path, 'evaluate_tracking.seqmap'), 'r') as fh:
        for line in fh:
            fields = line.split(' ')
            if len(fields) < 4:
                continue
            seq_id = '%04d' % int(fields[0])
            if seq_id in ids:
                names.append(seq_id)
                n_frames.append(int(fields[3]) - int(fields[2]) + 1)
    return names, n_frames


def evaluate(result_sha, root, part='all', gt_path='./data/tracking', cls=None, device='cuda'):
    """Drop-in for the reference's ``kitti_devkit.evaluate_tracking.evaluate(result_sha, root, part)``: evaluates
    ``root/result_sha/part/<sequence>.txt`` against ``gt_path/label_02`` for car, then pedestrian (``cls``: one class
    only), writes ``eval/<cls>/stats_<cls>.txt`` beside the results in the devkit's format and returns
    (MOTA, MOTP, recall, precision, F1, fp, fn, id_switches) of the last class evaluated, or False when the tracker
    holds neither class.  The pretty summary and the mail object are not built."""
    names, n_frames = sequences_of(part, gt_path)
    if not names:
        raise ValueError('evaluate: the seqmap under %s holds no sequence of part %r' % (gt_path, part))
    t_path = os.path.join(root, str(result_sha), part)
    last = None
    for c in (('car', 'pedestrian') if cls is None else (cls,)):
        try:
            tracker = concat([load_kitti(os.path.join(t_path, '%s.txt' % s), c, n, False)
                              for s, n in zip(names, n_frames)])
        except IOError:
            continue
        if tracker.n_traj.sum() == 0:  # no trajectory of the class: the class is skipped
            continue
        try:
            gt = concat([load_kitti(os.path.join(gt_path, 'label_02', '%s.txt' % s), c, n, True)
                         for s, n in zip(names, n_frames)])
        except IOError:
            raise ValueError('Ground truth not found.')
        m = evaluate_sequences(gt, tracker, cls=c, device=device)
        eval_dir = os.path.join(t_path, 'eval', c)
        os.makedirs(eval_dir, exist_ok=True)
        with open(os.path.join(eval_dir, 'stats_%s.txt' % c), 'w') as f:
            f.write(m.stats_line() + '\n')
        last = m
    return False if last is None else last.summary()


# ---- HOTA / IDF1 (csrc/hota.hip) -----------------------------------------------------------------------------------
HOTA_ALPHA = 0.05 * np.arange(1, HOTA_ALPHAS + 1)  # alpha_a = 0.05 (a + 1)
_PER_ALPHA = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')


@dataclass
class Hota:
    """HOTA and IDF1 of a set of sequences.  ``<name>_alpha``: the values at the 19 thresholds 0.05 .. 0.95; ``<name>``:
    their mean.  TP / FN / FP: int64 [19].  seq_*: one entry per sequence."""
    cls: str = 'car'
    alphas: np.ndarray = None
    TP: np.ndarray = None
    FN: np.ndarray = None
    FP: np.ndarray = None
    LocSum: np.ndarray = None
    HOTA_alpha: np.ndarray = None
    DetA_alpha: np.ndarray = None
    AssA_alpha: np.ndarray = None
    DetRe_alpha: np.ndarray = None
    DetPr_alpha: np.ndarray = None
    AssRe_alpha: np.ndarray = None
    AssPr_alpha: np.ndarray = None
    LocA_alpha: np.ndarray = None
    HOTA: float = 0.0
    DetA: float = 0.0
    AssA: float = 0.0
    DetRe: float = 0.0
    DetPr: float = 0.0
    AssRe: float = 0.0
    AssPr: float = 0.0
    LocA: float = 0.0
    IDTP: int = 0
    IDFN: int = 0
    IDFP: int = 0
    IDF1: float = 0.0
    IDR: float = 0.0
    IDP: float = 0.0
    n_gt: int = 0                                        # ground-truth boxes after the preparation
    n_tr: int = 0                                        # tracker boxes after the preparation
    seq_TP: list = field(default_factory=list)           # per sequence: int64 [19]
    seq_FN: list = field(default_factory=list)
    seq_FP: list = field(default_factory=list)
    seq_IDTP: list = field(default_factory=list)
    seq_IDFN: list = field(default_factory=list)
    seq_IDFP: list = field(default_factory=list)
    seq_n_gt: list = field(default_factory=list)
    seq_n_tr: list = field(default_factory=list)
    seq_AssA: list = field(default_factory=list)         # per sequence: float64 [19]
    seq_LocSum: list = field(default_factory=list)
    frame_values: np.ndarray = None   # debug, [frames, 2]: value of the preparation assignment, of the pass-2 assignment

    def summary(self):
        """(HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA, IDF1, IDR, IDP, IDTP, IDFN, IDFP)"""
        return (self.HOTA, self.DetA, self.AssA, self.DetRe, self.DetPr, self.AssRe, self.AssPr, self.LocA, self.IDF1,
                self.IDR, self.IDP, self.IDTP, self.IDFN, self.IDFP)

    def summary_line(self):
        return '%.6f ' * 11 % self.summary()[:11] + '%d %d %d' % self.summary()[11:]


def pack_hota(gt, tracker):
    """Labels of the ground truth and the tracker -> the tables of mmmot_hota: ``pack``'s frame tables plus the dense
    per-sequence IDs (ground truth: main class only) and the sequence table.  Raises ValueError on what the kernels do not
    take - frames beyond CLEAR-MOT's limits, an ID twice in a frame, more than HOTA_MAX_IDS IDs on a side or more than
    HOTA_MAX_CELLS (G * T) cells in a sequence - before anything reaches the device."""
    p = pack(gt, tracker)
    nG, nT, nD, NF, NTr, S = p['sizes']
    foff, g_cnt, t_cnt = p['foff'], p['g_cnt'], p['t_cnt']
    frame_seq = np.repeat(np.arange(S), np.diff(foff))
    g_fr, t_fr = np.repeat(np.arange(NF), g_cnt), np.repeat(np.arange(NF), t_cnt)
    g_tid = np.zeros(nG, np.int64)
    g_tid[p['traj_obj']] = np.repeat(p['traj_key'][:, 1], p['traj_key'][:, 2]) if NTr else 0
    t_tid = p['t_attr'][:, 0].astype(np.int64)
    main = p['g_attr'][:, 2] == MAIN

    def dense(fr, tid, use, what):
        """dense per-sequence IDs of the rows ``use`` (-1 elsewhere) and the ID count of every sequence"""
        out, n = np.full(len(tid), -1, np.int64), np.zeros(S, np.int64)
        seq = frame_seq[fr] if len(fr) else np.zeros(0, np.int64)
        for s in range(S):
            m = use & (seq == s)
            if len(np.unique(np.stack([fr[m], tid[m]], axis=1), axis=0)) != m.sum():
                raise ValueError('hota: %s track ids are not unique within a frame of sequence %d' % (what, s))
            ids, inv = np.unique(tid[m], return_inverse=True)
            out[m], n[s] = inv.reshape(-1), len(ids)
        return out, n

    g_id, Gs = dense(g_fr, g_tid, main, 'ground-truth')
    t_id, Ts = dense(t_fr, t_tid, np.ones(nT, bool), 'tracker')
    if S and (max(Gs.max(), Ts.max()) > HOTA_MAX_IDS or (Gs * Ts).max() > HOTA_MAX_CELLS):
        raise ValueError('hota: a sequence holds more than %d track ids on a side or more than %d (ground truth x '
                         'tracker) id pairs' % (HOTA_MAX_IDS, HOTA_MAX_CELLS))
    cum = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    cells, goff, toff = cum(Gs * Ts), cum(Gs), cum(Ts)
    seq_tab = np.stack([foff, np.r_[Gs, 0], np.r_[Ts, 0], cells, goff, toff], axis=1)
    d_cnt = p['frames'][:, 5] if NF else np.zeros(0, np.int64)
    big = lambda v: int(v.max()) if len(v) else 0
    return {
        'sizes': [nG, nT, nD, NF, S, int(cells[-1]), int(goff[-1]), int(toff[-1]), max(big(g_cnt), big(t_cnt)), big(d_cnt)],
        'boxes': p['boxes'], 'frames': p['frames'], 'frame_seq': frame_seq,
        'g_attr': np.concatenate([p['g_attr'], g_id[:, None]], axis=1), 't_id': t_id, 'seq_tab': seq_tab,
        'foff': foff, 'Gs': Gs, 'Ts': Ts, 'cls': p['cls'],
    }


def _hota_ratios(h, TP, FN, FP, LocSum, AssA, AssRe, AssPr):
    """steps 3 and 4: the ratios of every alpha from the counts, LocSum and the association values, and their means"""
    tp = TP.astype(np.float64)
    h.TP, h.FN, h.FP, h.LocSum = TP, FN, FP, LocSum
    h.AssA_alpha, h.AssRe_alpha, h.AssPr_alpha = AssA, AssRe, AssPr
    h.LocA_alpha = np.where(TP == 0, 1.0, LocSum / np.maximum(1e-10, tp))
    h.DetRe_alpha = tp / np.maximum(1, TP + FN)
    h.DetPr_alpha = tp / np.maximum(1, TP + FP)
    h.DetA_alpha = tp / np.maximum(1, TP + FN + FP)
    h.HOTA_alpha = np.sqrt(h.DetA_alpha * h.AssA_alpha)
    for k in _PER_ALPHA:
        setattr(h, k, float(np.mean(getattr(h, k + '_alpha'))))


def finish_hota(p, out):
    """the packed tables and the device's output sections (numpy) -> Hota"""
    NF, S = p['sizes'][3], p['sizes'][4]
    A = HOTA_ALPHAS
    seq_i = out['seq_i'].reshape(S + 1, HOTA_SEQ_I).astype(np.int64)
    seq_d = out['seq_d'].reshape(S + 1, HOTA_SEQ_D)
    if seq_i[:, A + 3].min() < 0:
        raise RuntimeError('mmmot_hota: a frame or a sequence outside the launch limits reached the kernel')
    h = Hota(cls=p['cls'], alphas=HOTA_ALPHA.copy())
    for s in range(S):
        tp, ng, nt, idtp = seq_i[s, :A], int(seq_i[s, A]), int(seq_i[s, A + 1]), int(seq_i[s, A + 2])
        h.seq_TP.append(tp.copy())
        h.seq_FN.append(ng - tp)
        h.seq_FP.append(nt - tp)
        h.seq_n_gt.append(ng)
        h.seq_n_tr.append(nt)
        h.seq_IDTP.append(idtp)
        h.seq_IDFN.append(ng - idtp)
        h.seq_IDFP.append(nt - idtp)
        h.seq_AssA.append(seq_d[s, A:2 * A] / np.maximum(1, tp))
        h.seq_LocSum.append(seq_d[s, :A].copy())
    TP, h.n_gt, h.n_tr, h.IDTP = seq_i[S, :A].copy(), int(seq_i[S, A]), int(seq_i[S, A + 1]), int(seq_i[S, A + 2])
    den = np.maximum(1, TP)
    _hota_ratios(h, TP, h.n_gt - TP, h.n_tr - TP, seq_d[S, :A].copy(), seq_d[S, A:2 * A] / den,
                 seq_d[S, 2 * A:3 * A] / den, seq_d[S, 3 * A:4 * A] / den)
    h.IDFN, h.IDFP = h.n_gt - h.IDTP, h.n_tr - h.IDTP
    h.IDF1 = h.IDTP / max(1.0, h.IDTP + 0.5 * h.IDFP + 0.5 * h.IDFN)
    h.IDR = h.IDTP / max(1.0, float(h.IDTP + h.IDFN))
    h.IDP = h.IDTP / max(1.0, float(h.IDTP + h.IDFP))
    h.frame_values = out['frame_d'].reshape(NF, HOTA_FRAME_D)[:, :2].copy()
    return h


def hota_sequences(gt, tracker, cls='car', prepare='kitti', max_truncation=0, min_height=25, max_occlusion=2,
                   device='cuda'):
    """HOTA and IDF1 of tracker Labels against ground-truth Labels (one Labels of S sequences, or a list with one per
    sequence) on the device: one upload, the launches of mmmot_hota, one read-back.  ``prepare``: 'kitti' (the
    preparation of DESIGN.md section 13 with the knobs of ``evaluate_sequences``) or None (every main-class ground-truth
    row and every tracker row)."""
    if prepare not in ('kitti', None):
        raise ValueError("hota: prepare must be 'kitti' or None, got %r" % (prepare,))
    p = pack_hota(gt, tracker)
    p['cls'] = cls
    return finish_hota(p, run_hota(p, [float(min_height), float(max_truncation), float(max_occlusion),
                                       1. if prepare == 'kitti' else 0.], device))


def run_hota(p, params, device='cuda'):
    """the tables of ``pack_hota`` through torch.ops.mmmot.hota -> the output sections as numpy arrays"""
    import torch
    inp, outl, n_in, _, _ = hota_layout(p['sizes'])
    return read_back(torch.ops.mmmot.hota(upload(p, inp, n_in, device), p['sizes'], params), outl)


def evaluate_hota(result_sha, root, part='all', gt_path='./data/tracking', cls=None, device='cuda'):
    """The file loading of ``evaluate`` with ``hota_sequences`` behind it: evaluates ``root/result_sha/part/<sequence>.txt``
    against ``gt_path/label_02`` for car, then pedestrian (``cls``: one class only) and returns the Hota record of the
    last class evaluated, or False when the tracker holds neither class.  No file is written."""
    names, n_frames = sequences_of(part, gt_path)
    if not names:
        raise ValueError('evaluate_hota: the seqmap under %s holds no sequence of part %r' % (gt_path, part))
    t_path = os.path.join(root, str(result_sha), part)
    last = None
    for c in (('car', 'pedestrian') if cls is None else (cls,)):
        try:
            tracker = concat([load_kitti(os.path.join(t_path, '%s.txt' % s), c, n, False)
                              for s, n in zip(names, n_frames)])
        except IOError:
            continue
        if tracker.n_traj.sum() == 0:
            continue
        try:
            gt = concat([load_kitti(os.path.join(gt_path, 'label_02', '%s.txt' % s), c, n, True)
                         for s, n in zip(names, n_frames)])
        except IOError:
            raise ValueError('Ground truth not found.')
        last = hota_sequences(gt, tracker, cls=c, device=device)
    return False if last is None else last


# ---- 3D / AMOTA (csrc/mot3d.hip) -------------------------------------------------------------------------------------
# columns of Labels.box3d
B3_H, B3_W, B3_L, B3_X, B3_Y, B3_Z, B3_RY, B3_SCORE = range(8)


def footprints(b3):
    """Labels.box3d rows -> float64 [n, 12]: the four footprint corners (x, z), y - h, y, w l, h w l (DESIGN.md section
    13 "3D / AMOTA"), in NumPy float64 - what the device and tests/mot3d_ref.py both start from."""
    b3 = np.asarray(b3, np.float64).reshape(-1, 8)
    h, w, l, x, y, z, ry = (b3[:, k] for k in range(7))
    c, s = np.cos(ry), np.sin(ry)
    out = np.empty((len(b3), MOT3D_BOX), np.float64)
    for k, (sx, sz) in enumerate(((1., 1.), (1., -1.), (-1., -1.), (-1., 1.))):
        dx, dz = sx * (l / 2), sz * (w / 2)
        out[:, 2 * k] = x + c * dx + s * dz
        out[:, 2 * k + 1] = z - s * dx + c * dz
    out[:, 8], out[:, 9], out[:, 10], out[:, 11] = y - h, y, w * l, h * w * l
    return out


def track_scores(rows, scores):
    """per row the score of its track: the mean, in fp64 and in row order, of the scores of the rows with the same
    (sequence, track ID)"""
    if not len(rows):
        return np.zeros(0, np.float64)
    _, inv = np.unique(rows[:, [SEQ, TID]].astype(np.int64), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    tot, cnt = np.zeros(inv.max() + 1, np.float64), np.bincount(inv)
    np.add.at(tot, inv, np.asarray(scores, np.float64))  # one element after the other, in row order
    return (tot / cnt)[inv]


def pack_3d(gt, tracker, need_3d=True):
    """``pack`` plus the tables of mmmot_mot3d: the packed 3D boxes (``footprints``), the track score of every evaluated
    tracker row (``track_scores`` over the evaluated rows, in file order) and the offsets of the per-frame overlap
    tables.  ``need_3d=False`` (the '2d' mode) takes Labels without box3d: zero boxes, zero scores.  Raises ValueError
    on what ``pack`` refuses, on Labels without box3d, on a non-positive or non-finite dimension and on an overlap table
    beyond 32-bit offsets - before anything reaches the device."""
    gt = concat(gt) if isinstance(gt, (list, tuple)) else gt
    tracker = concat(tracker) if isinstance(tracker, (list, tuple)) else tracker
    p = pack(gt, tracker)
    nG, nT = p['sizes'][0], p['sizes'][1]
    if gt.box3d is None or tracker.box3d is None:
        if need_3d:
            raise ValueError('evaluate_3d: the Labels hold no box3d (load_kitti / labels_from_tracks with box3d=True)')
        p['box3d'], p['sigma'] = np.zeros((nG + nT, MOT3D_BOX)), np.zeros(nT)
    else:
        if len(gt.box3d) != len(gt.rows) or len(tracker.box3d) != len(tracker.rows):
            raise ValueError('evaluate_3d: box3d and rows differ in length')
        b3 = np.concatenate([gt.box3d[p['g_idx']], tracker.box3d[p['t_idx']]]).reshape(-1, 8)
        if need_3d and not (np.all(np.isfinite(b3)) and np.all(b3[:, :3] > 0)):
            raise ValueError('evaluate_3d: a box has a non-positive or non-finite dimension')
        p['box3d'] = footprints(b3)
        file_order = np.sort(p['t_idx'])
        sig = np.zeros(len(tracker.rows))
        sig[file_order] = track_scores(tracker.rows[file_order], tracker.box3d[file_order, B3_SCORE])
        p['sigma'] = sig[p['t_idx']]
    cnt = p['g_cnt'] * p['t_cnt']
    p['cell_off'] = np.cumsum(cnt) - cnt
    p['cells'] = int(cnt.sum())
    if p['cells'] >= 2 ** 31:
        raise ValueError('evaluate_3d: the overlap tables hold %d cells, beyond 32-bit offsets' % p['cells'])
    return p


@dataclass
class Mot3D:
    """3D MOT evaluation.  Per-level arrays have one entry per level k = 1 .. levels (recall r_k = k / levels); an
    unreachable level holds 0 in the three metric arrays and +inf in ``thr``.  ``all``: the ClearMot of every track (pass
    A); ``best``: the ClearMot of the reachable level with the highest sMOTA (lowest k on ties), None when there is none."""
    cls: str = 'car'
    overlap: str = '3d'
    AMOTA: float = 0.0
    sAMOTA: float = 0.0
    AMOTP: float = 0.0
    levels: int = 0
    recall: np.ndarray = None         # r_k
    thr: np.ndarray = None
    reachable: np.ndarray = None      # bool
    MOTA_k: np.ndarray = None
    sMOTA_k: np.ndarray = None
    MOTP_k: np.ndarray = None
    counters: np.ndarray = None       # int64 [levels, 12]: the totals row of mmmot_clear_mot per level
    cost_k: np.ndarray = None         # sum of the overlaps of the matches
    n_gt_k: np.ndarray = None
    best_level: int = -1              # index into the per-level arrays
    all: ClearMot = None
    best: ClearMot = None

    def summary(self):
        """(AMOTA, sAMOTA, AMOTP, then MOTA, MOTP, recall, precision, fp, fn, id_switches of every track)"""
        a = self.all
        return (self.AMOTA, self.sAMOTA, self.AMOTP, a.MOTA, a.MOTP, a.recall, a.precision, a.fp, a.fn, a.id_switches)

    def summary_line(self):
        return '%.6f ' * 7 % self.summary()[:7] + '%d %d %d' % self.summary()[7:]


def sweep_metrics(tot_i, tot_d, n_obj, reach):
    """step 4 and 5 of the sweep from the levels' totals: tot_i int [L, 12] (the totals row of mmmot_clear_mot), tot_d
    float [L] (sum of the overlaps), n_obj = ground-truth objects, reach bool [L] ->
    (AMOTA, sAMOTA, AMOTP, MOTA_k, sMOTA_k, MOTP_k, n_gt_k)"""
    L = len(reach)
    mota, smota, motp, n_gts = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L, np.int64)
    for k in range(L):
        tp, itp, fn, ifn, fp, _, ids = (int(v) for v in tot_i[k][:7])
        n_gt = n_obj - ifn - itp
        n_gts[k] = n_gt
        if not reach[k] or n_gt <= 0:
            continue
        r = (k + 1) / float(L)
        mota[k] = 1 - (fn + fp + ids) / float(n_gt)
        smota[k] = max(0., 1 - (fp + fn + ids - (1 - r) * n_gt) / (r * n_gt))
        motp[k] = float(tot_d[k]) / float(tp) if tp else 0.
    mean = lambda v: sum(float(x) for x in v) / float(L) if L else 0.
    return mean(mota), mean(smota), mean(motp), mota, smota, motp, n_gts


def finish_3d(p, out, levels, overlap):
    """the packed tables and the device's output sections (numpy) -> Mot3D"""
    nG, nT, nD, NF, NTr, S = p['sizes']
    Lv = levels + 1
    lev = {'frame_d': out['frame_d'].reshape(Lv, -1), 'seq_d': out['seq_d'].reshape(Lv, -1),
           'frame_i': out['frame_i'].reshape(Lv, -1), 'gt_out': out['gt_out'].reshape(Lv, -1),
           'traj_i': out['traj_i'].reshape(Lv, -1), 'seq_i': out['seq_i'].reshape(Lv, -1)}
    thr = out['thr'].copy()
    reach = out['reach'].astype(bool)
    fseq = np.repeat(np.arange(S), np.diff(p['foff']))
    t_seq = np.repeat(fseq, p['t_cnt']) if nT else np.zeros(0, np.int64)
    t_frame = np.repeat(np.arange(NF), p['t_cnt'])
    t_key = np.stack([t_seq, p['t_attr'][:, 0].astype(np.int64)], axis=1) if nT else np.zeros((0, 2), np.int64)

    def one(k):
        """the ClearMot of level k (``levels``: pass A) over the tracker rows that level keeps"""
        q = dict(p)
        if k < levels:
            keep = p['sigma'] >= thr[k]
            q['sizes'] = [nG, int(keep.sum()), nD, NF, NTr, S]
            q['t_cnt'] = np.bincount(t_frame[keep], minlength=NF).astype(np.int64)
            q['n_tr_trajectories'] = len(np.unique(t_key[keep], axis=0))
        return finish(q, {name: v[k] for name, v in lev.items()})

    m = Mot3D(cls=p['cls'], overlap=overlap, levels=levels, all=one(levels))
    seq_i = lev['seq_i'].reshape(Lv, S + 1, CLEAR_MOT_SEQ_INTS).astype(np.int64)
    seq_d = lev['seq_d'].reshape(Lv, S + 1, 2)
    if levels and seq_i[:levels, S].min() < 0:
        raise RuntimeError('mmmot_mot3d: a frame or a trajectory outside the launch limits reached the kernel')
    m.recall = np.arange(1, levels + 1) / float(levels) if levels else np.zeros(0)
    m.thr, m.reachable = thr, reach
    m.counters, m.cost_k = seq_i[:levels, S].copy(), seq_d[:levels, S, 0].copy()
    m.AMOTA, m.sAMOTA, m.AMOTP, m.MOTA_k, m.sMOTA_k, m.MOTP_k, m.n_gt_k = sweep_metrics(m.counters, m.cost_k, nG, reach)
    if reach.any():
        m.best_level = int(np.argmax(np.where(reach, m.sMOTA_k, -1.)))  # the first of equal maxima
        m.best = one(m.best_level)
    return m


def upload_3d(p, sizes, device):
    """the tables of ``pack_3d`` as the one int32 block of mmmot::mot3d on ``device``"""
    inp, _, n_in, _ = mot3d_layout(sizes)
    return upload(p, inp, n_in, device)


def overlap_tables(gt, tracker, overlap='3d', device='cuda'):
    """c = 1 - overlap of every (ground truth, tracker) cell as the device forms it: per frame a float64 [G, T] array
    (the table the association reads; never read back by ``evaluate_3d_sequences``)"""
    from .torch_ops import mot3d_run
    if overlap not in MOT3D_MODES:
        raise ValueError("evaluate_3d: overlap must be '3d', 'bev' or '2d', got %r" % (overlap,))
    p = pack_3d(gt, tracker, need_3d=overlap != '2d')
    sizes = list(p['sizes']) + [p['cells'], 0, MOT3D_MODES[overlap]]
    tab = mot3d_run(upload_3d(p, sizes, device), sizes, [1.0, 25., 0., 2.])[1].cpu().numpy()
    return [tab[o:o + g * t].reshape(g, t) for o, g, t in zip(p['cell_off'], p['g_cnt'], p['t_cnt'])]


def evaluate_3d_sequences(gt, tracker, cls='car', overlap='3d', min_iou=0.25, levels=40, min_overlap=0.5,
                          max_truncation=0, min_height=25, max_occlusion=2, device='cuda'):
    """3D MOT statistics of tracker Labels against ground-truth Labels (one Labels of S sequences, or a list with one
    per sequence; both with ``box3d``) on the device: one upload, the launches of mmmot_mot3d, one read-back.
    ``overlap``: '3d' (IoU of the rotated boxes) or 'bev' (IoU of their footprints), both gated at ``min_iou``, or '2d'
    (the image-plane IoU of ``evaluate_sequences`` gated at ``min_overlap``; takes Labels without box3d).  ``levels``:
    the recall levels of the AMOTA sweep; 0 evaluates the one operating point with every track.  The rules are those
    of DESIGN.md section 13 "3D / AMOTA"; no agreement with any published 3D evaluator is claimed."""
    import torch
    if overlap not in MOT3D_MODES:
        raise ValueError("evaluate_3d: overlap must be '3d', 'bev' or '2d', got %r" % (overlap,))
    levels = int(levels)
    if levels < 0 or levels > MOT3D_MAX_LEVELS:
        raise ValueError('evaluate_3d: levels must lie in [0, %d], got %d' % (MOT3D_MAX_LEVELS, levels))
    p = pack_3d(gt, tracker, need_3d=overlap != '2d')
    p['cls'] = cls
    gate = float(min_overlap) if overlap == '2d' else 1.0 - float(min_iou)
    sizes = list(p['sizes']) + [p['cells'], levels, MOT3D_MODES[overlap]]
    res = torch.ops.mmmot.mot3d(upload_3d(p, sizes, device), sizes,
                                [gate, float(min_height), float(max_truncation), float(max_occlusion)])
    return finish_3d(p, read_back(res, mot3d_layout(sizes)[1]), levels, overlap)


def evaluate_3d(result_sha, root, part='all', gt_path='./data/tracking', cls=None, overlap='3d', min_iou=0.25,
                levels=40, device='cuda'):
    """The file loading of ``evaluate`` with ``evaluate_3d_sequences`` behind it: evaluates
    ``root/result_sha/part/<sequence>.txt`` (columns 10..17 included) against ``gt_path/label_02`` for car, then
    pedestrian (``cls``: one class only), writes ``eval/<cls>/stats3d_<cls>.txt`` (``Mot3D.summary_line``) beside the
    results and returns the Mot3D of the last class evaluated, or False when the tracker holds neither class."""
    names, n_frames = sequences_of(part, gt_path)
    if not names:
        raise ValueError('evaluate_3d: the seqmap under %s holds no sequence of part %r' % (gt_path, part))
    t_path = os.path.join(root, str(result_sha), part)
    last = None
    for c in (('car', 'pedestrian') if cls is None else (cls,)):
        try:
            tracker = concat([load_kitti(os.path.join(t_path, '%s.txt' % s), c, n, False, box3d=True)
                              for s, n in zip(names, n_frames)])
        except IOError:
            continue
        if tracker.n_traj.sum() == 0:
            continue
        try:
            gt = concat([load_kitti(os.path.join(gt_path, 'label_02', '%s.txt' % s), c, n, True, box3d=True)
                         for s, n in zip(names, n_frames)])
        except IOError:
            raise ValueError('Ground truth not found.')
        m = evaluate_3d_sequences(gt, tracker, cls=c, overlap=overlap, min_iou=min_iou, levels=levels, device=device)
        eval_dir = os.path.join(t_path, 'eval', c)
        os.makedirs(eval_dir, exist_ok=True)
        with open(os.path.join(eval_dir, 'stats3d_%s.txt' % c), 'w') as f:
            f.write(m.summary_line() + '\n')
        last = m
    return False if last is None else last
