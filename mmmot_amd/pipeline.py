"""One tracked sequence, frame by frame: the rows of SURVEY section 8 chained the way the reference's evaluation loop
chains them, with the next frame's upload and preparation running under the current pair's forward.

Reference chain per frame pair (t-1, t): ``TestSequence._generate_img_lidar`` (dataset/test_seq_dataset.py:176-246: per
frame ``get_pointcloud`` = ``read_and_prep_points`` and the crop / resize / normalise loop) -> ``input.cuda()``
(eval_seq.py:145-149) -> ``TrackingModule.predict`` (tracking_model.py:68-83: model forward, then ``ortools_solve`` on the
selected score rows).  The reference prepares BOTH frames of every pair on the host (each frame twice over a sequence)
and runs everything back to back.

Here, per frame t:   H2D (image, sweep)  ->  ``prep_points``  ->  ``crop_resize_u8``         [stage A: once per frame]
      per pair:      ``TrackingNet.forward`` on (A[t-1], A[t])  ->  ``scores_for_solver``    [stage B]
``overlap=True`` queues stage A of frame t+1 on a side stream BEFORE the host waits for the scores of pair (t-1, t), so
the upload, the gather and the resize run beside / under the forward.  Both orders launch the same kernels on the same
inputs: their outputs are bitwise equal (tests/test_pipeline_gpu.py).  No CPU fallback: every stage is a C-ABI kernel
sequence on the device.

Ego motion (``FrameFeed(..., pose=(pos, rad))``): the reference moves the points of a pair's SECOND
frame into the first frame's coordinates (``align_points``, dataset/test_seq_dataset.py:199-210) and leaves the first
frame's as they are, so a frame enters two pairs with two different point sets.  A prepared frame therefore keeps both:
``points``, the gather's rows, used when the frame is the first of a pair, and ``points_aligned``, the same rows aligned
to the previous frame (mmmot_amd.points.align_points_batched, one launch), used when it is the second.  The alignment of
frame t needs the pose of frame t-1 only - host data - so it is queued in stage A of frame t, once per frame, on the side
stream with ``overlap=True``; the sequence's first frame gets no aligned copy.  Either every frame of a sequence carries
a pose or none does.  ``FrameFeed(point_transform=...)`` is the older hook: one function applied to a frame's extracted
points in BOTH of its roles, which cannot express the reference's alignment; it stays for other uses.

Every frame of a sequence is the second frame of one pair and the first of the next, so the per-pair order runs each
frame's crops through the VGG trunk twice.  In eval mode a crop's appearance row does not depend on the crops beside it
(TrackingNet.encode_appearance), and two opt-in orders compute each frame's rows once:
  ``reuse_appearance=True`` (online): each pair runs the trunk on the new frame's crops only, beside the previous frame's
      rows (TrackingNet.forward_appearance), and keeps the new rows for the next pair;
  ``run_offline`` (the whole sequence known): the trunk over the crops of K frames per launch sequence, then the pairs B
      at a time on the rows (forward_batch with appearance rows).
Both return the scores of ``run`` bit for bit.  Rows are reused only while TrackingNet.appearance_is_current, which first
takes the range guard's verdict on the forward that made them: after each hand-off the rows of both frames are checked,
and rows from an out-of-range trunk, or from weights / an arithmetic that changed since, are encoded again with the pair.  ``stats`` counts the frames the trunk encoded.

``associate=True`` adds the association step of ``TrackingModule.predict`` (the ``ortools_solve`` drop-in of
mmmot_amd.association): each pair's solve is queued behind its forward (``run_offline``: one launch per batch of pairs),
and the hand-off copies scores and assignment to the host together.  The runs then return (scores, assignment) per pair
and call ``on_assign(t, assignment)`` beside ``on_scores(t, scores)``; the scores are those of ``associate=False``.

``track=True`` (with ``associate=True``) adds the last step of ``predict``, the ID bookkeeping (mmmot_amd.tracks): the ID
launch is queued behind each solve, the sequence's ID state stays on the device, and the IDs come back in the same copy.
Each run fills ``pipe.tracks`` - per frame an int64 array with one track ID per detection, -1 for a rejected one - and
calls ``on_tracks(t, ids)`` per emitted frame; the runs return what they return without it.

All orders and modes, pairs and windows, share their steps.  ``queue_hand_off`` queues what the mode asks for behind the
forward of one pair or window, or a batch of them, and returns a tracker_glue.HandOff; ``finish_hand_off`` is its host
copy - the one place the host waits - with one result (scores, assignment, ids) each, and ``_deliver`` turns a result
into the callbacks, ``stats`` and the returned shape.  ``run`` is one loop (``_run_online``) over
``tracks.window_starts`` - for ``window=2`` the list of pairs - and ``run_offline`` one loop over batches of them
(``_offline_frames`` and ``_offline_forwards``, which ``run_global`` shares: it keeps the batches' selected rows on the
device and decides the whole sequence with one min-cost flow, association.associate_sequence - with ``max_gap`` > 1
one with skip links, association.associate_sequence_gaps, over the pairs (f_t, f_{t+g}) as well).  A pair
differs from a window in three places: stage A aligns a frame to the one before it (a window aligns at launch;
``run_offline`` aligns K frames per launch in front of the trunk), the forward (``launch_pair`` with the stage events,
``launch_pair_cached`` on cached rows; ``launch_window`` otherwise), and the recompute check of ``reuse_appearance``.

Windows (``SequencePipeline(window=T)``, 3 <= T <= 8): the model scores T frames at once and the chain
solver (association.associate_chain) decides them together, so a weak detection that both neighbours support can
stay.  Windows start at frames 0, T-1, 2 (T-1), .. - neighbours share one frame - and the last one is shorter (at least
2 frames) when the sequence does not divide; the reference's dataset drops those trailing frames instead.  Per window:
one ``TrackingNet.forward`` over the T frames' crops and joined points, ``select_chain`` -> ``queue_solve_chains`` ->
``fetch``, with the frames of the next window prepared before the host blocks.  With poses frame k of a window is
aligned to the window's frame 0 by a k-step record (``ego.transform_record([R_1 .. R_k], [T_1 .. T_k], ..)``, the
accumulation of dataset/test_seq_dataset.py:200-210), all frames of a window in one launch; a frame keeps its raw rows
for its role as a window's frame 0.  The runs return one entry per window, the callbacks get the index of the window's
last frame, and ``pipe.tracks`` is filled through ``tracks.merge_chain_tracks``: as in the reference, a window whose
frame 0 continues the stored frame and whose frame 1 keeps no detection is not stored at all - its frames keep the IDs
they had (-1 if none) and the next window starts a new stretch of IDs.  ``window=2`` is the pair path above: the pair
solver, the pair ID entry point, a pair's ``ids`` tuple.

Frames without detections: the reference's dataset skips them (dataset/test_seq_dataset.py:82-102: a sample's second
frame is the next NON-EMPTY one) and the network is not defined on one, so the pair path (``run``, ``run_offline``, the
lockstep order) goes over the frames that hold a detection; callbacks and ``tracks`` keep the sequence's own frame
indices, an empty frame's ``tracks`` entry is the empty array, and ``stats['empty_frames']`` counts them.

Many sequences (``LockstepPipeline``): S live sequences step together in the ``reuse_appearance``
order - per step one stage A, one trunk launch sequence, one ``forward_batch``, one solve, one multi-state ID launch and
one hand-off copy for the pairs of all of them - and every sequence gets what ``SequencePipeline.run`` gives it alone.
"""
import time

import numpy as np
import torch

from .crops import crop_resize_u8, crop_resize_u8_multi
from . import ego
from .points import align_points_batched, prep_points_batched
from .association import (MotionGate, check_kept, check_status, gap_pairs, gap_sequences_table, launch_sequences,
                          pack_gate, queue_gate, select, select_chain, unpack_gaps)
from .tracker_glue import queue_scores, queue_solve, queue_solve_chains
from .torch_ops import FILL_MAX, SEQ_MAX_GAP
from .tracks import (TrackSmoother, TrackState, TrackStates, TrackStitcher, fill_gaps, merge_chain_tracks, merge_tracks,
                     smooth_tracks, stitch_tracks, window_starts)


class FrameFeed:
    """Host side of one frame: pinned staging copies of the image and the sweep (what a loader thread would hand over)."""

    def __init__(self, img, sweep, info, dets, point_transform=None, pose=None):
        if pose is not None:
            if point_transform is not None:
                raise ValueError('FrameFeed: give pose= (the ego-motion alignment of the second frame of a pair) or '
                                 'point_transform= (one function for both roles of the frame), not both')
            if 'calib/Tr_imu_to_velo' not in info:
                raise ValueError("FrameFeed: pose= needs info['calib/Tr_imu_to_velo']")
            pos, rad = (np.array(v, dtype=np.float64).reshape(-1) for v in pose)
            if pos.shape != (3,) or rad.shape != (3,):
                raise ValueError('FrameFeed: pose = (pos [3], rad [3]), got %s and %s' % (pos.shape, rad.shape))
            pose = (pos, rad)
        self.img = torch.from_numpy(np.ascontiguousarray(img)).pin_memory()
        self.sweep = torch.from_numpy(np.ascontiguousarray(sweep, dtype=np.float32)).pin_memory()
        self.info, self.dets = info, dets
        # optional: applied to the EXTRACTED points (device tensor [Q, 3|4]) of this frame - where the reference aligns the
        # second frame of a pair to the first one's coordinates (align_points, dataset/test_seq_dataset.py:199-210)
        self.point_transform = point_transform
        # optional: (pos, rad) of the frame as the reference's get_pos returns them.  With poses the pipeline aligns the
        # frame's points to the previous frame for its role as the SECOND frame of a pair (module docstring)
        self.pose = pose


def _check_poses(feeds):
    """every frame of a sequence carries a pose, or none does; True when they do"""
    n = sum(1 for f in feeds if f.pose is not None)
    if 0 < n < len(feeds):
        raise ValueError('SequencePipeline: %d of %d frames carry a pose; the ego-motion alignment needs the pose of '
                         'every frame (or of none)' % (n, len(feeds)))
    return n > 0


def _skip_empty(feeds, callbacks):
    """The pair path over the frames that hold a detection.  The reference's dataset never hands the tracker a frame
    without detections (dataset/test_seq_dataset.py:82-102, "skip the empty frame"): a sample starts at a non-empty
    frame and takes the NEXT NON-EMPTY frame as its second one, so the tracker sees the consecutive pairs of the
    sequence with its empty frames left out (the network is not defined on an empty frame).  Returns (the kept feeds,
    their indices in ``feeds``, the callbacks taking an index into the kept feeds and passing on the frame's own)."""
    idx = [t for t, f in enumerate(feeds) if len(f.dets['bbox']) > 0]
    if len(idx) == len(feeds):
        return feeds, idx, callbacks
    own = lambda f: None if f is None else (lambda t, x: f(idx[t], x))
    return [feeds[t] for t in idx], idx, tuple(own(f) for f in callbacks)


def _spread_tracks(tracks, idx, n_frames):
    """the tracks of the kept frames at their own indices; a frame without detections has the empty array"""
    out = [np.zeros(0, np.int64) for _ in range(n_frames)]
    for t, ids in zip(idx, tracks):
        out[t] = ids
    return out


def _pair_record(prev_feed, feed):
    """the transform record that aligns ``feed``'s points to ``prev_feed`` (one (R, T) step, ego.transform_record)"""
    R, T = ego.pair_motion(prev_feed.pose, feed.pose)
    return ego.transform_record([R], [T], feed.info['calib/Tr_imu_to_velo'])


def _window_records(feeds, steps):
    """per frame k = 1 .. len(feeds) - 1 of a window the record that aligns it to the window's frame 0: the k steps
    (R_1, T_1) .. (R_k, T_k) of the frames up to it, as the reference accumulates them, behind ``steps`` - k identity
    steps, which leave every coordinate as it is, so that one launch of ``steps`` steps serves all frames"""
    R, T, rec = [], [], []
    for k in range(1, len(feeds)):
        r, t = ego.pair_motion(feeds[k - 1].pose, feeds[k].pose)
        R.append(r)
        T.append(t)
        pad = steps - k
        rec.append(ego.transform_record([np.eye(3)] * pad + R, [np.zeros(3)] * pad + T,
                                        feeds[k].info['calib/Tr_imu_to_velo']))
    return np.stack(rec)


class SequencePipeline:
    def __init__(self, model, size=224, overlap=True, without_reflectivity=True, reuse_appearance=False, associate=False,
                 track=False, window=2):
        if not 2 <= int(window) <= 8:
            raise ValueError('SequencePipeline: window must lie in 2 .. 8 frames, got %s' % (window,))
        if track and not associate:
            raise ValueError('SequencePipeline: track=True needs associate=True (the IDs come from the assignments)')
        self.model, self.size, self.overlap = model, int(size), bool(overlap)
        self.wo_refl = without_reflectivity
        self.dev = next(model.parameters()).device
        self.side = torch.cuda.Stream(self.dev) if overlap else None
        self.stage_events = None   # set to [] to record HIP events per stage (serial order only)
        self.reuse_appearance = bool(reuse_appearance)
        self.associate = bool(associate)
        self.track = bool(track)
        self.window = int(window)  # frames scored and solved together; 2: the pair path
        self.track_state = TrackState(self.dev) if self.track else None
        self.tracks = None         # track=True: per frame the int64 track IDs of its detections (-1: rejected)
        # frames run through the trunk (a frame of a per-pair pair counts once per pair), pairs scored, pairs whose rows
        # were found stale after their hand-off and were computed again
        self.stats = {'encoded_frames': 0, 'pairs': 0, 'recomputed_pairs': 0}

    # ---- stage A: one frame onto the device and through the two preparation kernels ---------------------------
    def _prepare(self, feed, prev_feed=None):
        ev = self.stage_events
        marks = []

        def mark():
            if ev is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)
        mark()
        img = feed.img.to(self.dev, non_blocking=True)
        sweep = feed.sweep.to(self.dev, non_blocking=True)
        mark()
        # the image-frustum filter and the per-box gather in ONE launch sequence, one split read-back
        pc = prep_points_batched([sweep], [feed.info], [feed.dets], without_reflectivity=self.wo_refl)[0]
        pts = pc['points'] if feed.point_transform is None else feed.point_transform(pc['points']).contiguous()
        # with poses: the copy for the frame's role as the second frame of pair (prev_feed, feed)
        aligned = None
        if prev_feed is not None and feed.pose is not None:
            aligned = align_points_batched(pts, [0, int(pts.shape[0])], _pair_record(prev_feed, feed)[np.newaxis], 1)
        mark()
        crops = crop_resize_u8(img, feed.dets['bbox'], self.size)
        mark()
        if ev is not None:
            ev.append(('prep', marks))
        return {'crops': crops, 'points': pts, 'points_aligned': aligned,
                'split': np.asarray(pc['points_split'], dtype=np.int64), 'n': int(crops.shape[0]), 'ready': None}

    def prepare(self, feed, prev_feed=None):
        """stage A of ``feed``; ``prev_feed``: the frame before it in the sequence (None for the first one) - with poses
        the frame's points are aligned to it as well"""
        if not self.overlap:
            return self._prepare(feed, prev_feed)
        cur = torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(self.side):
            a = self._prepare(feed, prev_feed)
            a['ready'] = torch.cuda.Event()
            a['ready'].record(self.side)
        for t in (a['crops'], a['points'], a['points_aligned']):
            if t is not None:
                t.record_stream(cur)   # allocated on the side stream, consumed on the main one
        return a

    def _aligned_group(self, frames, feeds, t0, t1, gap=1):
        """the points of frames [t0, t1) (t0 >= gap), each aligned to the frame ``gap`` before it, in ONE launch"""
        self._wait(*frames[t0:t1])
        rows = np.concatenate([[0], np.cumsum([int(frames[t]['points'].shape[0]) for t in range(t0, t1)])])
        rec = np.stack([_pair_record(feeds[t - gap], feeds[t]) for t in range(t0, t1)])
        out = align_points_batched(torch.cat([frames[t]['points'] for t in range(t0, t1)]), rows, rec, 1)
        return [out[int(rows[i]):int(rows[i + 1])] for i in range(t1 - t0)]

    def _align_group(self, frames, feeds, t0, t1):
        """run_offline with poses: ``points_aligned`` of frames [t0, t1) (t0 >= 1) in ONE launch, each aligned to the
        frame before it"""
        for t, pts in zip(range(t0, t1), self._aligned_group(frames, feeds, t0, t1)):
            frames[t]['points_aligned'] = pts

    # ---- stage B: the pair forward + the packed hand-off -------------------------------------------------------
    def _wait(self, *frames):
        cur = torch.cuda.current_stream(self.dev)
        for x in frames:
            if x['ready'] is not None:
                cur.wait_event(x['ready'])

    @staticmethod
    def _second(b):
        """the points of frame b as the SECOND frame of a pair: aligned to the pair's first frame when the sequence has
        poses"""
        return b['points'] if b['points_aligned'] is None else b['points_aligned']

    @staticmethod
    def _pair_info(a, b):
        points = torch.cat([a['points'], SequencePipeline._second(b)]).unsqueeze(0)
        split = SequencePipeline._window_split([a, b])
        # the split is on the host already (prep_points read it back): hand it over as a CPU tensor - no D2H in forward
        return {'points': points, 'points_split': torch.from_numpy(split.astype(np.float32)).unsqueeze(0)}

    def launch_pair(self, a, b):
        """queue TrackingNet.forward on frames (a, b); returns the device outputs (nothing waits on the host)"""
        self._wait(a, b)
        crops = torch.cat([a['crops'], b['crops']])
        det_info = self._pair_info(a, b)
        self.stats['encoded_frames'] += 2
        ev = self.stage_events
        if ev is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        with torch.no_grad():
            out = self.model(crops, det_info, [torch.tensor([a['n']]), torch.tensor([b['n']])])
        if ev is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            ev.append(('forward', [e0, e1]))
        return out

    def queue_hand_off(self, outs, groups, stream_of=None):
        """Queue the hand-off of ``groups`` = [(first frame, frames)], pairs or windows, behind their forward outputs
        ``outs``; returns the pending HandOff.  associate=True: with the groups' solve in one launch (the pair solver for
        window = 2, the chain solver above); track=True: and the ID launch of these consecutive groups behind it.
        ``stream_of`` (LockstepPipeline): the pairs belong to several sequences, pair g to ``stream_of[g]``, and
        ``self.track_state`` is the table of their states."""
        tm = self.model.test_mode
        if not self.associate:
            return queue_scores(outs, tm)
        if self.window == 2:
            sel = [select(o[0], o[1], o[2], o[3], tm) for o in outs]
            track = self.track_state if stream_of is None else (self.track_state, list(stream_of))
            return queue_solve(sel, [(a['n'], b['n']) for _, (a, b) in groups], track=track,
                               frame_idx=[(s, s + 1) for s, _ in groups])
        sel = [select_chain(o[0], o[1], o[2], o[3], tm) for o in outs]
        return queue_solve_chains(sel, [[f['n'] for f in fr] for _, fr in groups], track=self.track_state,
                                  frame_idx=[list(range(s, s + len(fr))) for s, fr in groups])

    def finish_hand_off(self, pending):
        """the host copy, the one place the host waits for the pairs or windows: one result for each"""
        return pending.fetch()

    def _start_tracks(self, feeds):
        if self.track:
            self.track_state.reset()
            self.tracks = [np.full(len(f.dets['bbox']), -1, np.int64) for f in feeds]

    def _deliver(self, s, k, r, on_scores, on_assign, on_tracks, tracks=None):
        """the callbacks and the bookkeeping of the pair or window of k frames from frame s, a hand-off result; returns
        what the run returns for it.  ``tracks``: the per-frame list to fill (default ``self.tracks``)"""
        t = s + k - 1
        tracks = self.tracks if tracks is None else tracks
        if on_scores is not None:
            on_scores(t, r.scores)
        if on_assign is not None and r.assignment is not None:
            on_assign(t, r.assignment)
        if r.ids is not None:
            if self.window == 2:
                merge_tracks(tracks, t, r.ids[0], r.ids[1], r.ids[2], on_tracks)
            else:
                merge_chain_tracks(tracks, range(s, s + k), r.ids[0], r.ids[1], r.ids[3], on_tracks)
        key = 'pairs' if self.window == 2 else 'windows'
        self.stats[key] = self.stats.get(key, 0) + 1
        return (r.scores, r.assignment) if self.associate else r.scores

    def _stage_a(self, feeds, t):
        """stage A of frame t of the sequence; for pairs with its alignment to frame t-1 (windows align at launch)"""
        return self.prepare(feeds[t], feeds[t - 1] if self.window == 2 and t > 0 else None)

    def _launch(self, fr, feeds, moving):
        if self.window > 2:
            return self.launch_window(fr, feeds, moving)
        return (self.launch_pair_cached if self.reuse_appearance else self.launch_pair)(*fr)

    def _run_online(self, feeds, moving, on_scores, on_assign, on_tracks):
        """the pairs or windows one after the other, each frame prepared once; with ``reuse_appearance`` (pairs) on
        cached appearance rows (the trunk on the new frame only)"""
        reuse = self.reuse_appearance
        wins = window_starts(len(feeds), self.window)
        res, frames = [], {}
        for t in range(wins[0][1] if wins else len(feeds)):
            frames[t] = self._stage_a(feeds, t)
        if reuse and wins:
            self.encode([frames[0]])  # frame 0, once
        for w, (s, k) in enumerate(wins):
            fr = [frames[t] for t in range(s, s + k)]
            snap = self.track_state.snapshot() if reuse and self.track else None  # a recomputed pair starts from it again
            pending = self.queue_hand_off([self._launch(fr, feeds[s:s + k], moving)], [(s, fr)])
            # stage A of the next one's new frames is queued before the host blocks on this one's scores
            for t in range(s + k, sum(wins[w + 1]) if w + 1 < len(wins) else 0):
                frames[t] = self._stage_a(feeds, t)
            r = self.finish_hand_off(pending)[0]
            if reuse:
                r = self._checked_scores(fr[0], fr[1], r, s + 1, snap)
            res.append(self._deliver(s, k, r, on_scores, on_assign, on_tracks))
            for t in range(s, s + k - 1):
                del frames[t]
        return res

    def run(self, feeds, on_scores=None, on_assign=None, on_tracks=None):
        """All pairs (t-1, t) of the sequence.  Returns the list of host score tuples (det, [link], new, end) - what
        ``ortools_solve`` is called with; ``on_scores(t, scores)`` is where the host solver would run.  associate=True:
        the list of (scores, assignment), assignment as ``ortools_solve`` returns it; ``on_assign(t, assignment)``.
        track=True: ``self.tracks`` is filled as well, ``on_tracks(t, ids)`` per emitted frame.  window > 2: one entry
        per window, the callbacks with the index of the window's last frame."""
        moving = _check_poses(feeds)
        if self.window > 2:
            if self.reuse_appearance:
                raise ValueError('SequencePipeline.run: reuse_appearance=True runs the pair-shaped cached-rows forward; '
                                 'with window > 2 use run_offline, which encodes every frame once')
            self._check_window_poses(moving)
        n_frames, idx = len(feeds), None
        if self.window == 2:  # pairs: frames without detections are left out, as the reference's dataset leaves them out
            feeds, idx, (on_scores, on_assign, on_tracks) = _skip_empty(feeds, (on_scores, on_assign, on_tracks))
        self._start_tracks(feeds)
        res = self._run_online(feeds, moving, on_scores, on_assign, on_tracks)
        self.tracks = self._account_empty(self.tracks, idx, n_frames, self.reuse_appearance and len(feeds) >= 2)
        return res

    def _account_empty(self, tracks, idx, n_frames, once):
        """after a pair run over the kept frames ``idx``: returns ``tracks`` at the sequence's own frame indices, and the
        frames left out are counted.  ``once`` (the orders that encode every frame once): they count as encoded too, so that
        ``encoded_frames`` stays the sequence's frame count - a frame without crops has nothing left to encode"""
        if idx is None or len(idx) == n_frames:
            return tracks
        self.stats['empty_frames'] = self.stats.get('empty_frames', 0) + n_frames - len(idx)
        if once:
            self.stats['encoded_frames'] += n_frames - len(idx)
        return _spread_tracks(tracks, idx, n_frames) if self.track else tracks

    # ---- the forward of a window of 3 .. 8 frames --------------------------------------------------------------------
    def _check_window_poses(self, moving):
        if moving and self.window - 1 > ego.MAX_CHAIN:
            raise ValueError('SequencePipeline: window=%d with poses needs a chain of %d alignment steps; at most %d '
                             '(window <= %d)' % (self.window, self.window - 1, ego.MAX_CHAIN, ego.MAX_CHAIN + 1))

    def _window_points(self, frames, feeds, moving):
        """the point rows of a window's frames, joined: frame 0's as they are, frame k's aligned to frame 0 when the
        sequence has poses - all of them in ONE launch"""
        pts = [f['points'] for f in frames]
        if not moving:
            return torch.cat(pts)
        rows = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in pts[1:]])])
        out = torch.empty((int(pts[0].shape[0]) + int(rows[-1]), int(pts[0].shape[1])), dtype=pts[0].dtype,
                          device=pts[0].device)
        out[:pts[0].shape[0]] = pts[0]
        align_points_batched(torch.cat(pts[1:]), rows, _window_records(feeds, len(frames) - 1), len(frames) - 1,
                             out=out, out_row0=int(pts[0].shape[0]))
        return out

    @staticmethod
    def _window_split(frames):
        """the point split of the window's joined points: every frame's boundaries behind the frames before it"""
        split = frames[0]['split']
        for f in frames[1:]:
            split = np.concatenate([split, split[-1] + f['split'][1:]])
        return split

    def launch_window(self, frames, feeds, moving):
        """queue TrackingNet.forward on the T frames of one window; returns the device outputs (nothing waits)"""
        self._wait(*frames)
        crops = torch.cat([f['crops'] for f in frames])
        split = self._window_split(frames)
        det_info = {'points': self._window_points(frames, feeds, moving).unsqueeze(0),
                    'points_split': torch.from_numpy(split.astype(np.float32)).unsqueeze(0)}
        self.stats['encoded_frames'] += len(frames)
        with torch.no_grad():
            return self.model(crops, det_info, [torch.tensor([f['n']]) for f in frames])

    # ---- appearance rows computed once per frame -----------------------------------------------------------------
    def _current(self, a):
        return a.get('rows') is not None and self.model.appearance_is_current(a['rows'])

    def encode(self, frames):
        """one trunk launch sequence over the crops of `frames`; each frame keeps its AppearanceRows under 'rows'"""
        self._wait(*frames)
        crops = frames[0]['crops'] if len(frames) == 1 else torch.cat([a['crops'] for a in frames])
        with torch.no_grad():
            rows = self.model.encode_appearance(crops)
        for a, r in zip(frames, rows.split([a['n'] for a in frames])):
            a['rows'] = r
        self.stats['encoded_frames'] += len(frames)

    def launch_pair_cached(self, a, b):
        """queue the pair forward on frame a's rows and frame b's crops (TrackingNet.forward_appearance): the trunk runs
        on b's crops only, and b keeps its rows for the next pair.  a's rows are encoded again first when stale."""
        if not self._current(a):
            self.encode([a])
        self._wait(a, b)
        with torch.no_grad():
            out, b['rows'] = self.model.forward_appearance(a['rows'], b['crops'], self._pair_info(a, b),
                                                           [torch.tensor([a['n']]), torch.tensor([b['n']])],
                                                           return_rows=True)
        self.stats['encoded_frames'] += 1
        return out

    def _checked_scores(self, prev, cur, r, t, snap=None):
        """After the hand-off (the host has waited for the pair anyway): the range guard's verdict on the trunks that
        made both frames' rows (appearance_is_current takes it).  Rows it rejects - or that a lowered arithmetic made
        stale - are computed again and the pair with them; at most two rounds (the guard only lowers f16q8 -> f16x3 ->
        f32).  track=True: the pair's IDs are computed again too, from ``snap``, the ID state as it was before the pair."""
        for _ in range(3):
            if self._current(prev) and self._current(cur):
                return r
            self.stats['recomputed_pairs'] += 1
            if snap is not None:
                self.track_state.restore(snap)
            r = self.finish_hand_off(self.queue_hand_off([self.launch_pair_cached(prev, cur)], [(t - 1, [prev, cur])]))[0]
        raise RuntimeError('mmmot_amd: the appearance rows of a pair stayed stale after recomputing it three times')

    def _encode_all(self, frames, K):
        """rows for every frame: K consecutive frames per trunk launch sequence (fewer where their crops would pass the
        trunk's 32-bit offsets, Engine.appearance: L*S*S*16 < 2^31 - 64); stale groups again after the range verdict"""
        cap = (2 ** 31 - 65) // (self.size * self.size * 16)
        groups, i = [], 0
        while i < len(frames):
            j, n = i, 0
            while j < len(frames) and j - i < K and n + frames[j]['n'] <= cap:
                n += frames[j]['n']
                j += 1
            if j == i:
                raise ValueError('frame %d: %d crops of %d pixels exceed one trunk launch sequence' % (i, frames[i]['n'],
                                                                                                      self.size))
            groups.append(frames[i:j])
            i = j
        for _ in range(3):
            for g in groups:
                if not all(self._current(a) for a in g):
                    self.encode(g)
            if all(self._current(a) for a in frames):
                return
        raise RuntimeError('mmmot_amd: the appearance rows of the sequence stayed stale after encoding it three times')

    def run_offline(self, feeds, frames_per_encode=16, pairs_per_forward=8, on_scores=None, on_assign=None,
                    on_tracks=None, windows_per_forward=4):
        """The whole sequence at once (every frame known up front): stage A for every frame, the trunk over the crops of
        `frames_per_encode` frames per launch sequence (throughput-mode occupancy), then the pairs `pairs_per_forward` at
        a time on the rows (forward_batch with appearance rows: PointNet, fusion and the head batched).  Returns the list
        of ``run``; ``on_scores(t, scores)`` is called in pair order once each batch of pairs is on the host.
        associate=True: each batch of pairs is solved in one launch and copied back with its scores in one copy;
        track=True: one ID launch walks the batch's pairs behind that solve, and the IDs ride in the same copy.
        window > 2: the rows are encoded once per frame all the same, then ``windows_per_forward`` windows at a time
        run through forward_batch on plans of T-frame samples, with one chain solve and one ID launch per batch."""
        K, B = int(frames_per_encode), int(pairs_per_forward if self.window == 2 else windows_per_forward)
        if K < 1 or int(pairs_per_forward) < 1 or int(windows_per_forward) < 1:
            raise ValueError('frames_per_encode, pairs_per_forward and windows_per_forward must be >= 1')
        moving = _check_poses(feeds)
        if self.window > 2:
            self._check_window_poses(moving)
        n_frames, idx = len(feeds), None
        if self.window == 2:  # as in ``run``: the pairs of the frames that hold a detection
            feeds, idx, (on_scores, on_assign, on_tracks) = _skip_empty(feeds, (on_scores, on_assign, on_tracks))
        self._start_tracks(feeds)
        frames = self._offline_frames(feeds, K, moving)
        if len(frames) < 2:
            self.tracks = self._account_empty(self.tracks, idx, n_frames, False)
            return []
        res = []
        for grp, outs in self._offline_forwards(frames, feeds, moving, B):
            done = self.finish_hand_off(self.queue_hand_off(outs, grp))
            for (s, fr), r in zip(grp, done):
                res.append(self._deliver(s, len(fr), r, on_scores, on_assign, on_tracks))
        self.tracks = self._account_empty(self.tracks, idx, n_frames, True)
        return res

    def _offline_frames(self, feeds, K, moving):
        """the offline orders up to the rows: stage A of every frame, for pairs of a moving sequence one align launch per
        K frames in front of their trunk launches, then the trunk over K frames per launch sequence (with fewer than two
        frames: stage A only, nothing is scored)"""
        frames = [self.prepare(f) for f in feeds]
        if len(frames) < 2:
            return frames
        if moving and self.window == 2:
            for t0 in range(1, len(frames), K):
                self._align_group(frames, feeds, t0, min(t0 + K, len(frames)))
        self._encode_all(frames, K)  # waits for stage A of every frame
        return frames

    def _offline_forwards(self, frames, feeds, moving, B):
        """the offline orders' forwards: per batch of B pairs or windows (its groups [(first frame, frames)], the device
        outputs of one ``forward_batch`` on the rows)"""
        wins = window_starts(len(frames), self.window)
        for g0 in range(0, len(wins), B):
            grp = [(s, frames[s:s + k]) for s, k in wins[g0:g0 + B]]
            plan = self.model.make_plan([([f['n'] for f in fr], self._window_split(fr)) for _, fr in grp], self.size)
            if self.window == 2:  # aligned in front of the trunk launches
                points = [p for _, (a, b) in grp for p in (a['points'], self._second(b))]
            else:
                points = [self._window_points(fr, feeds[s:s + len(fr)], moving) for s, fr in grp]
            with torch.no_grad():
                outs = self.model.forward_batch(plan, None, torch.cat(points),
                                                appearance=torch.cat([f['rows'].rows for _, fr in grp for f in fr]))
            yield grp, outs

    def _gap_links(self, frames, feeds, moving, K, B, G, gap_penalty, skip=()):
        """run_global with skip links: the selected link block of every pair (f_t, f_{t+g}), g = 2 .. G, in layout order
        (gap by gap, each in frame order), flat, less ``gap_penalty * (g - 1)``.  The pairs run ``B`` at a time through
        ``forward_batch`` on the cached appearance rows; with poses the second frame of a pair is aligned to the pair's
        first frame, one launch per gap and group of ``K`` frames, and the copy is kept per gap (``points_aligned`` stays
        the alignment to the frame before).  A pair (t, g) in ``skip`` (the motion gate left it no link) is not
        forwarded: its block is all NaN."""
        tm, n = self.model.test_mode, len(frames)
        every = [(t, g) for g in range(2, G + 1) for t in range(n - g)]
        pairs = [p for p in every if p not in skip] if skip else every
        second = {}
        if moving:
            for g in range(2, G + 1):
                for t0 in range(g, n, K):
                    t1 = min(t0 + K, n)
                    second.update(zip(((t, g) for t in range(t0, t1)), self._aligned_group(frames, feeds, t0, t1, g)))
        links = {}
        for p0 in range(0, len(pairs), B):
            grp = [(frames[t], frames[t + g], second.get((t + g, g)), g) for t, g in pairs[p0:p0 + B]]
            plan = self.model.make_plan([([a['n'], b['n']], self._window_split([a, b])) for a, b, _, _ in grp], self.size)
            points = [p for a, b, sec, _ in grp for p in (a['points'], b['points'] if sec is None else sec)]
            with torch.no_grad():
                outs = self.model.forward_batch(plan, None, torch.cat(points),
                                                appearance=torch.cat([f['rows'].rows for a, b, _, _ in grp for f in (a, b)]))
            for o, (_, _, _, g), key in zip(outs, grp, pairs[p0:p0 + B]):
                blk = select(o[0], o[1], o[2], o[3], tm)[1][0].reshape(-1)
                links[key] = blk - gap_penalty * (g - 1) if gap_penalty != 0.0 else blk.clone()
        self.stats['pairs'] += len(pairs)
        self.stats['gap_pairs'] = self.stats.get('gap_pairs', 0) + len(pairs)
        if skip:
            self.stats['gated_pairs'] = self.stats.get('gated_pairs', 0) + len(every) - len(pairs)
            absent = lambda t, g: torch.full((frames[t]['n'] * frames[t + g]['n'],), float('nan'), dtype=torch.float32,
                                             device=self.dev)
            return [links[p] if p in links else absent(*p) for p in every]
        return [links[p] for p in every]

    def run_global(self, feeds, frames_per_encode=16, pairs_per_forward=8, max_gap=1, gap_penalty=0.0, fill=0,
                   gate=None, smooth=None, stitch=None):
        """The whole sequence decided at once: ``run_offline``'s stage A, alignment, trunk and batched pair forwards, then
        ONE min-cost flow over all frames (association.associate_sequence; DESIGN section 11, "Sequences") in place of a
        solve per pair and the ID walk - a unit of flow is a trajectory, its number the track ID.  Needs ``window == 2``.
        Per batch only the ``test_mode`` rows stay on the device; after the last batch the sequence's scores are
        assembled there - for the kept frames f_0 .. f_{K-1} and pair p = (f_p, f_{p+1}): det and new of frame 0 from
        pair 0's first half, of frame t >= 1 from pair t-1's second half; end of frame t <= K-2 from pair t's first half,
        of frame K-1 from pair K-2's second half; link_t = pair t's block (the layout a K-frame eval forward returns) -
        then one launch solves them and one copy brings everything back.  Returns a ``GlobalResult`` (``.scores`` and
        ``.assignment`` in ``ortools_solve`` order, ``.ids`` per kept frame, ``.n_tracks``, ``.objective``) and fills
        ``self.tracks`` at the sequence's own frame indices, whatever ``track`` is (``_account_empty`` spreads them only
        for ``track=True``, so the frames left out are counted here).  With fewer than two frames that
        hold a detection nothing is solved, as in ``run_offline``: returns None and the tracks stay -1.

        ``max_gap = G > 1`` ("skip links"): a trajectory may miss up to G - 1 of the kept frames.
        After the adjacent pairs the pairs (f_t, f_{t+g}), g = 2 .. G, are scored on the cached appearance rows - no crop
        is encoded again - and only their link blocks are kept, less ``gap_penalty * (g - 1)``; det / new / end stay those
        of the adjacent pairs.  One association.associate_sequence_gaps launch solves the program, one copy brings it
        back; the result carries the blocks of the gaps 2 .. G in ``.gap_scores`` / ``.gap_assignment``.  With fewer
        than G + 1 kept frames the largest gap that fits is used (``.max_gap``).  ``stats['gap_pairs']`` counts the pairs
        of the gaps above 1, ``stats['pairs']`` all pairs.  ``max_gap = 1`` is the path above, launch for launch.

        ``fill = F > 0``: behind the solve the frames a trajectory skipped get an interpolated box,
        ``tracks.fill_gaps(.., max_fill=F)`` over ALL frames of the sequence (the empty ones included; with the feeds'
        poses and the first feed's calibration when the camera moves) - one more upload, five small launches, one more
        copy, no forward.  The ``tracks.FilledTracks`` is stored as ``GlobalResult.filled``; ``self.tracks`` and
        everything else stay as they are.  ``fill = 0``: nothing of this runs and ``.filled`` is None.

        ``gate`` = an ``association.MotionGate`` ("motion gate"): a link whose two 3D boxes lie
        further apart than an object travels in the elapsed frames is absent from the program.  The frame numbers are
        the kept frames' own indices in the sequence; with poses the later box is moved into the earlier frame's
        coordinates (the feeds' poses and the first feed's calibration, as for ``fill``).  With G > 1, behind stage A one
        count-only launch (mmmot_gate_links) and one small copy tell which gap pairs (f_t, f_{t+g}) keep no link at
        all: those are not forwarded and their blocks are NaN; the adjacent pairs are always forwarded, det / new / end
        come from them.  One more launch gates the assembled link scores in place in front of the solve, and its kept
        counts ride in the solve's copy (``GlobalResult.gate_kept``, per block in layout order).  ``stats['gap_pairs']``
        then counts the gap pairs forwarded, ``stats['gated_pairs']`` those left out, ``stats['gated_links']`` the
        links absent from the program.  ``gate = None``: nothing of this runs.

        ``smooth`` = a ``tracks.TrackSmoother``: behind the solve (and the filling) the filled
        sequence - with ``fill = 0`` the solved one - goes through ``tracks.smooth_tracks``: a Kalman filter forwards
        and an RTS pass backwards along every track, the filled rows as unobserved ones, with the feeds' poses and the
        first feed's calibration when the camera moves - one more upload, five small launches, one more copy, no forward.
        The ``tracks.SmoothedTracks`` is stored as ``GlobalResult.smoothed``; ``self.tracks``, ``.filled``, the scores
        and the statistics stay as they are.  ``smooth = None``: nothing of this runs and ``.smoothed`` is None.

        ``stitch`` = a ``tracks.TrackStitcher``: behind the solve, the filling and the smoothing the
        smoothed sequence with its velocities - without ``smooth`` the filled or the solved one, without velocities -
        goes through ``tracks.stitch_tracks``, which rejoins tracks that an occlusion longer than ``max_gap`` broke -
        one more upload, eight small launches, one more copy, no forward.  When anything was stitched and ``fill`` > 0,
        one more ``fill_gaps`` over the relabelled (unsmoothed) sequence fills the new holes and, with ``smooth``, one
        more ``smooth_tracks`` follows, its mask the first one extended by the new rows.  The ``tracks.StitchedTracks``
        is stored as ``GlobalResult.stitched``, that second pass in its ``.filled`` / ``.smoothed`` (else None);
        ``self.tracks``, ``.filled``, ``.smoothed``, the scores and the statistics stay as they are.  ``stitch = None``:
        nothing of this runs and ``.stitched`` is None."""
        if self.window != 2:
            raise ValueError('SequencePipeline.run_global assembles the scores of frame pairs: window must be 2, got %d'
                             % self.window)
        K, B = int(frames_per_encode), int(pairs_per_forward)
        if K < 1 or B < 1:
            raise ValueError('frames_per_encode and pairs_per_forward must be >= 1')
        if not 1 <= int(max_gap) <= SEQ_MAX_GAP:
            raise ValueError('SequencePipeline.run_global: max_gap must lie in 1 .. %d, got %s' % (SEQ_MAX_GAP, max_gap))
        if not 0 <= int(fill) <= FILL_MAX:
            raise ValueError('SequencePipeline.run_global: fill must lie in 0 .. %d, got %s' % (FILL_MAX, fill))
        if gate is not None and not isinstance(gate, MotionGate):
            raise ValueError('SequencePipeline.run_global: gate must be an association.MotionGate or None, got %r' % (gate,))
        if smooth is not None and not isinstance(smooth, TrackSmoother):
            raise ValueError('SequencePipeline.run_global: smooth must be a tracks.TrackSmoother or None, got %r' % (smooth,))
        if stitch is not None and not isinstance(stitch, TrackStitcher):
            raise ValueError('SequencePipeline.run_global: stitch must be a tracks.TrackStitcher or None, got %r' % (stitch,))
        moving = _check_poses(feeds)
        n_frames, all_feeds = len(feeds), feeds
        feeds, idx, _ = _skip_empty(feeds, (None, None, None))
        tracks = [np.full(len(f.dets['bbox']), -1, np.int64) for f in feeds]
        frames = self._offline_frames(feeds, K, moving)
        res = None
        if len(frames) >= 2:
            tm, rows = self.model.test_mode, []
            G = min(int(max_gap), len(frames) - 1)  # the largest gap that fits
            gated, counted = None, None
            if gate is not None:
                tables = pack_gate([f.dets for f in feeds], idx, [f.pose for f in feeds] if moving else None,
                                   all_feeds[0].info if moving else None, gap_pairs(len(frames), G))
                gated = (tables, gate)
                if G > 1:  # which gap pairs keep a link at all: queued here, read behind the adjacent forwards
                    counted = queue_gate(tables, gate, None, self.dev)
            for grp, outs in self._offline_forwards(frames, feeds, moving, B):
                # the selected rows only: the batch's other rows go back to the allocator
                rows += [tuple(x.reshape(-1).clone() for x in (d, l[0], n, e))
                         for d, l, n, e in (select(o[0], o[1], o[2], o[3], tm) for o in outs)]
                self.stats['pairs'] += len(grp)
            skip = ()
            if counted is not None:
                kept = check_kept(counted.cpu().numpy(), tables)
                skip = frozenset((a, b - a) for (a, b), k in zip(gap_pairs(len(frames), G), kept) if b - a > 1 and k == 0)
            gap_links = self._gap_links(frames, feeds, moving, K, B, G, float(gap_penalty), skip) if G > 1 else ()
            res = solve_global(rows, [f['n'] for f in frames], gap_links, G, gated)
            if gate is not None:
                self.stats['gated_links'] = self.stats.get('gated_links', 0) + tables['n_link'] - int(res.gate_kept.sum())
                self.stats.setdefault('gated_pairs', 0)
            tracks = res.ids
        if len(idx) < n_frames:  # the frames left out: counted, and as encoded too once the trunk has run (``_account_empty``)
            self.stats['empty_frames'] = self.stats.get('empty_frames', 0) + n_frames - len(idx)
            if len(frames) >= 2:
                self.stats['encoded_frames'] += n_frames - len(idx)
        self.tracks = _spread_tracks(tracks, idx, n_frames)
        if res is not None and int(fill) > 0:
            res.filled = fill_gaps([f.dets for f in all_feeds], self.tracks,
                                   poses=[f.pose for f in all_feeds] if moving else None,
                                   calib=all_feeds[0].info if moving else None, max_fill=int(fill),
                                   device=self.dev)
        if res is not None and smooth is not None:
            ft = res.filled
            res.smoothed = smooth_tracks([f.dets for f in all_feeds] if ft is None else ft.frames,
                                         self.tracks if ft is None else ft.ids,
                                         observed=None if ft is None else [~m for m in ft.filled],
                                         poses=[f.pose for f in all_feeds] if moving else None,
                                         calib=all_feeds[0].info if moving else None, smoother=smooth, device=self.dev)
        if res is not None and stitch is not None:
            ft, sm = res.filled, res.smoothed
            ego = dict(poses=[f.pose for f in all_feeds] if moving else None, calib=all_feeds[0].info if moving else None)
            raw = [f.dets for f in all_feeds] if ft is None else ft.frames  # the rows of ``sm.frames``, unsmoothed
            sk = stitch_tracks(raw if sm is None else sm.frames, (self.tracks if ft is None else ft.ids) if sm is None
                               else sm.ids, velocity=None if sm is None else sm.velocity, stitcher=stitch,
                               device=self.dev, **ego)
            if sk.info['stitches'] > 0 and int(fill) > 0:
                sk.filled = fill_gaps(raw, sk.ids, max_fill=int(fill), device=self.dev, **ego)
                if smooth is not None:
                    seen = [np.ones(len(i), bool) for i in sk.ids] if ft is None else [~m for m in ft.filled]
                    sk.smoothed = smooth_tracks(sk.filled.frames, sk.filled.ids,
                                                observed=[np.concatenate([o, np.zeros(len(m) - len(o), bool)])
                                                          for o, m in zip(seen, sk.filled.filled)],
                                                smoother=smooth, device=self.dev, **ego)
            res.stitched = sk
        return res


class GlobalResult:
    """What ``SequencePipeline.run_global`` returns, on the host: ``scores`` = (det L, [link 1 x n_t x n_{t+1} ...],
    new L, end L) of the kept frames, ``assignment`` the 0 / 1 tensors of the same shapes (both in ``ortools_solve``
    order), ``ids`` per kept frame the int64 track IDs (-1: rejected), ``n_tracks``, ``objective`` (fp64), ``split``.
    With skip links (``max_gap`` > 1) ``gap_scores`` / ``gap_assignment`` hold, for g = 2 .. max_gap, the list of the
    blocks 1 x n_t x n_{t+g}; they are empty at ``max_gap`` = 1."""

    def __init__(self, scores, assignment, ids, n_tracks, objective, split, gap_scores=(), gap_assignment=(), max_gap=1):
        self.scores, self.assignment, self.ids = scores, assignment, ids
        self.n_tracks, self.objective, self.split = n_tracks, objective, split
        self.gap_scores, self.gap_assignment, self.max_gap = list(gap_scores), list(gap_assignment), max_gap
        self.filled = None  # run_global(fill=F > 0): the tracks.FilledTracks of the whole sequence
        self.smoothed = None  # run_global(smooth=): the tracks.SmoothedTracks of the filled (else the solved) sequence
        self.stitched = None  # run_global(stitch=): the tracks.StitchedTracks of the smoothed (else filled / solved) sequence
        self.gate_kept = None  # run_global(gate=): int64 [blocks], the links of every block the program holds


def assemble_rows(rows, counts):
    """The sequence's flat scores [det L | new L | end L | link_0 | ..] on the device from the selected rows of its
    consecutive pairs, ``rows[p]`` = (det, link, new, end) of pair (p, p + 1), flat; the convention of ``run_global``."""
    n = [int(c) for c in counts]
    last = len(n) - 2
    det = [rows[0][0][:n[0]]] + [r[0][n[p]:] for p, r in enumerate(rows)]
    new = [rows[0][2][:n[0]]] + [r[2][n[p]:] for p, r in enumerate(rows)]
    end = [r[3][:n[p]] for p, r in enumerate(rows)] + [rows[last][3][n[last]:]]
    return torch.cat(det + new + end + [r[1] for r in rows])


def solve_global(rows, counts, gap_links=(), max_gap=1, gate=None):
    """assemble, one ``association.launch_sequences`` launch, one copy; raises association.AssociationError on a status
    word.  ``max_gap`` > 1: ``gap_links`` = the flat link blocks of the gaps 2 .. max_gap in layout order, joined behind
    the adjacent pairs' blocks, and the launch is the one with skip links.  ``gate`` = (``pack_gate`` tables of the
    blocks in layout order, MotionGate): one mmmot_gate_links launch gates the assembled link scores in place in front
    of the solve, and the kept counts come back in the same copy (``GlobalResult.gate_kept``)."""
    split = [int(c) for c in counts]
    L = sum(split)
    flat = assemble_rows(rows, split)
    if max_gap > 1:
        flat = torch.cat([flat] + list(gap_links))
    flat = flat.to(torch.float32)
    scores = (flat[0:L], flat[L:2 * L], flat[2 * L:3 * L], flat[3 * L:])
    kept = None
    if gate is not None:
        if gate[0]['n_link'] != scores[3].numel():
            raise ValueError('solve_global: the gate tables hold %d links, the scores %d' % (gate[0]['n_link'], scores[3].numel()))
        kept = queue_gate(gate[0], gate[1], scores[3], flat.device)
    seqs, nts, _, _ = gap_sequences_table([split], max_gap)
    out, ids, obj, info = launch_sequences(scores, (seqs, nts), max_gap)
    # the fp64 objective first: every part then starts at a multiple of its element size, whatever L and the link count
    parts = [obj, flat, out, ids, info.reshape(-1)] + ([kept] if kept is not None else [])
    host = torch.cat([x.view(torch.uint8) for x in parts]).cpu()  # the one copy
    o, got = 0, []
    for x in parts:
        got.append(host[o:o + x.numel() * x.element_size()].view(x.dtype))
        o += x.numel() * x.element_size()
    if kept is not None:
        kept = check_kept(got.pop().numpy(), gate[0])
    got = got[1:] + got[:1]  # flat, out, ids, info, objective
    check_status(got[3].view(1, 4).numpy())
    like = got[0][0:L]
    tail = ([i.numpy() for i in got[2].to(torch.int64).split(split)], int(got[3][1]), float(got[4][0]), split)
    sizes = [[(1, split[t], split[t + g]) for t in range(len(split) - g)] for g in range(1, max_gap + 1)]
    sc, asg = (unpack_gaps(x, split, max_gap, like, sizes) for x in (got[0], got[1]))
    res = GlobalResult((sc[0], sc[1][0], sc[2], sc[3]), (asg[0], asg[1][0], asg[2], asg[3]), *tail,
                       gap_scores=sc[1][1:], gap_assignment=asg[1][1:], max_gap=max_gap)
    res.gate_kept = kept
    return res


def lockstep_steps(lens):
    """The lockstep schedule as a pure function: per step k the sequences (indices into ``lens``, their frame counts)
    that have a pair (k, k + 1).  A sequence of fewer than two frames is in no step; the steps end with the longest."""
    lens = [int(n) for n in lens]
    return [[s for s, n in enumerate(lens) if n >= k + 2] for k in range(max([n - 1 for n in lens if n >= 2], default=0))]


def lockstep_stage(lens, t):
    """the sequences whose frame t goes through stage A: those with a frame t that have a pair at all"""
    return [s for s, n in enumerate(lens) if int(n) >= 2 and int(n) > t]


class LockstepPipeline(SequencePipeline):
    """S live sequences frame by frame in lockstep: step k scores, solves and numbers pair (k, k+1) of EVERY sequence
    that still has one, in one batched launch sequence ("Many sequences").

    Per step: stage A of the live sequences' frames k+2 on the side stream (uploads, ONE ``prep_points_batched``, ONE
    alignment launch for the sequences that carry poses, ONE multi-image crop launch) -> ONE ``encode_appearance`` over
    the crops of the frames k+1 -> ONE ``forward_batch`` on the cached rows -> ONE solve, ONE multi-state ID launch
    (tracks.TrackStates) and ONE hand-off copy.  This is the ``reuse_appearance`` order of SequencePipeline - every
    frame goes through the trunk once - and its results are that pipeline's, sequence by sequence, bit for bit.

    Sequences end independently; one shorter than two frames contributes nothing.  A frame without detections is
    left out as SequencePipeline leaves it out (``_skip_empty``: step k scores a sequence's k-th pair of the frames that
    hold a detection; callbacks and ``tracks`` keep the sequence's own frame indices); the hand-off
    itself (tracker_glue.queue_solve with track=(states, stream_of)) answers a pair with an empty frame on the host
    without taking the step's other pairs there, and its IDs come from the same ID launch.  After the hand-off the rows of every sequence's two frames are checked
    (``appearance_is_current``): the sequences whose rows are stale get their states back from the step's snapshot,
    are encoded again and redo their pair - three rounds at most.  Per sequence either every frame carries a pose or
    none does; sequences may differ.  Pairs only: windows of 3 .. 8 frames run through SequencePipeline."""

    def __init__(self, model, size=224, overlap=True, without_reflectivity=True, associate=False, track=False, window=2):
        if int(window) != 2:
            raise ValueError('LockstepPipeline steps through pairs (window=2), got window=%s; windows of 3 .. 8 frames '
                             'run one sequence at a time: SequencePipeline(window=...)' % (window,))
        if track and not associate:
            raise ValueError('LockstepPipeline: track=True needs associate=True (the IDs come from the assignments)')
        super().__init__(model, size, overlap, without_reflectivity, reuse_appearance=True, associate=associate,
                         track=track)
        self.track_state = None    # track=True: the TrackStates table of the running sequences
        self.frames = None         # during a run: per sequence the prepared frames still in use
        self.stats['steps'] = 0

    # ---- stage A of one frame of each of several sequences ------------------------------------------------------------
    def _prepare_many(self, feeds, prevs):
        imgs = [f.img.to(self.dev, non_blocking=True) for f in feeds]
        sweeps = [f.sweep.to(self.dev, non_blocking=True) for f in feeds]
        pcs = prep_points_batched(sweeps, [f.info for f in feeds], [f.dets for f in feeds],
                                  without_reflectivity=self.wo_refl)
        pts = [pc['points'] if f.point_transform is None else f.point_transform(pc['points']).contiguous()
               for f, pc in zip(feeds, pcs)]
        aligned = [None] * len(feeds)
        mv = [i for i, (f, p) in enumerate(zip(feeds, prevs)) if p is not None and f.pose is not None]
        if mv:  # each aligned to the frame before it in its own sequence, all in one launch
            rows = np.concatenate([[0], np.cumsum([int(pts[i].shape[0]) for i in mv])])
            rec = np.stack([_pair_record(prevs[i], feeds[i]) for i in mv])
            out = align_points_batched(torch.cat([pts[i] for i in mv]), rows, rec, 1)
            for j, i in enumerate(mv):
                aligned[i] = out[int(rows[j]):int(rows[j + 1])]
        crops, counts = crop_resize_u8_multi(imgs, [f.dets['bbox'] for f in feeds], self.size)
        frames, o = [], 0
        for i, n in enumerate(counts):
            frames.append({'crops': crops[o:o + n], 'points': pts[i], 'points_aligned': aligned[i],
                           'split': np.asarray(pcs[i]['points_split'], dtype=np.int64), 'n': n, 'ready': None})
            o += n
        return frames

    def prepare_many(self, feeds, prevs):
        """stage A of ``feeds``, one frame of each of several sequences; ``prevs[i]``: the frame before ``feeds[i]`` in
        its sequence (None for a first frame)"""
        if not self.overlap:
            return self._prepare_many(feeds, prevs)
        cur = torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(self.side):
            frames = self._prepare_many(feeds, prevs)
            ready = torch.cuda.Event()
            ready.record(self.side)
        for a in frames:
            a['ready'] = ready
            for t in (a['crops'], a['points'], a['points_aligned']):
                if t is not None:
                    t.record_stream(cur)   # allocated on the side stream, consumed on the main one
        return frames

    # ---- one step: pair (k, k + 1) of the sequences ``live`` -----------------------------------------------------------
    def _launch_step(self, frames, live, k):
        """queue the encode of the frames that have no current rows, the forward of the pairs on the rows, and their
        hand-off; returns the pending HandOff"""
        prs = [(frames[s][k], frames[s][k + 1]) for s in live]
        if len(prs) == 1:  # one sequence left in the step: the pair forward of SequencePipeline, trunk and head in one op
            return self.queue_hand_off([self.launch_pair_cached(*prs[0])], [(k, list(prs[0]))], stream_of=live)
        both = [f for pr in prs for f in pr]
        self._wait(*both)
        new = [f for f in both if not self._current(f)]
        if new:
            self.encode(new)
        plan = self.model.make_plan([([a['n'], b['n']], self._window_split([a, b])) for a, b in prs], self.size)
        with torch.no_grad():
            outs = self.model.forward_batch(plan, None, torch.cat([p for a, b in prs for p in (a['points'], self._second(b))]),
                                            appearance=torch.cat([f['rows'].rows for f in both]))
        return self.queue_hand_off(outs, [(k, list(pr)) for pr in prs], stream_of=live)

    def _checked_step(self, frames, live, k, done, snap):
        """``_checked_scores`` for a step: the sequences whose rows the range guard rejected (or that went stale
        otherwise) get their ID states back from ``snap``, and their pairs are computed again - theirs only"""
        for _ in range(3):
            stale = [i for i, s in enumerate(live)
                     if not (self._current(frames[s][k]) and self._current(frames[s][k + 1]))]
            if not stale:
                return done
            self.stats['recomputed_pairs'] += len(stale)
            sub = [live[i] for i in stale]
            if snap is not None:
                self.track_state.restore(snap, sub)
            for i, r in zip(stale, self.finish_hand_off(self._launch_step(frames, sub, k))):
                done[i] = r
        raise RuntimeError('mmmot_amd: the appearance rows of a step stayed stale after recomputing it three times')

    def run(self, streams, on_scores=None, on_assign=None, on_tracks=None):
        """``streams``: S lists of FrameFeed, of any lengths.  Returns per sequence the list ``SequencePipeline.run``
        returns for it; the callbacks get (s, t, ..) with s the sequence; track=True: ``self.tracks[s]`` is that
        pipeline's ``tracks``.  Every call starts every sequence anew."""
        S = len(streams)
        if S < 1:
            raise ValueError('LockstepPipeline.run: no sequences')
        for feeds in streams:
            _check_poses(feeds)
        # per sequence the frames that hold a detection (``_skip_empty``): step k scores its k-th pair of THOSE, and a
        # frame index below is an index into them; the callbacks and ``tracks`` speak of the sequence's own indices
        n_frames, bind = [len(f) for f in streams], lambda f, s: None if f is None else (lambda t, x: f(s, t, x))
        kept = [_skip_empty(feeds, (bind(on_scores, s), bind(on_assign, s), bind(on_tracks, s)))
                for s, feeds in enumerate(streams)]
        streams, lens = [k[0] for k in kept], [len(k[0]) for k in kept]
        if self.track:
            self.track_state = TrackStates(S, self.dev)
            self.tracks = [[np.full(len(f.dets['bbox']), -1, np.int64) for f in feeds] for feeds in streams]
        res, frames = [[] for _ in range(S)], [{} for _ in range(S)]
        self.frames = frames   # per sequence {frame index: its prepared frame}, the frames still in use

        def stage_a(t):
            live = lockstep_stage(lens, t)
            if live:
                feeds = [streams[s][t] for s in live]
                for s, a in zip(live, self.prepare_many(feeds, [streams[s][t - 1] if t else None for s in live])):
                    frames[s][t] = a
        stage_a(0)
        stage_a(1)
        for k, live in enumerate(lockstep_steps(lens)):
            snap = self.track_state.snapshot() if self.track else None   # recomputed pairs start from it again
            pending = self._launch_step(frames, live, k)
            stage_a(k + 2)   # queued before the host blocks on this step's results
            done = self._checked_step(frames, live, k, self.finish_hand_off(pending), snap)
            for s, r in zip(live, done):
                res[s].append(self._deliver(k, 2, r, *kept[s][2], tracks=self.tracks[s] if self.track else None))
                del frames[s][k]
            self.stats['steps'] += 1
        for s, (_, idx, _) in enumerate(kept):   # the frames left out, per sequence
            tr = self._account_empty(self.tracks[s] if self.track else None, idx, n_frames[s], len(idx) >= 2)
            if self.track:
                self.tracks[s] = tr
        return res

    def run_offline(self, *args, **kwargs):
        raise NotImplementedError('LockstepPipeline steps through live sequences; a sequence known in full runs through '
                                  'SequencePipeline.run_offline')


def time_sequence(model, feeds, size=224, overlap=True, warm=3, associate=False, track=False):
    """frames/s of the chain over ``feeds`` (wall clock, synchronised on both sides; ``warm`` untimed leading pairs);
    ``associate``: with the device association of every pair (SequencePipeline(associate=True))."""
    pipe = SequencePipeline(model, size, overlap=overlap, associate=associate, track=track)
    pipe.run(feeds[:warm + 1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = pipe.run(feeds)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return (len(feeds) - 1) / dt, dt, res


def stage_times(model, feeds, size=224):
    """Device ms per stage of the SERIAL order (HIP events on the one stream): h2d, prep_points, crop_resize, forward;
    the hand-off copy is what is left of the wall time."""
    pipe = SequencePipeline(model, size, overlap=False)
    pipe.run(feeds[:3])
    pipe.stage_events = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipe.run(feeds)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    acc = {'h2d': 0.0, 'prep_points': 0.0, 'crop_resize': 0.0, 'forward': 0.0}
    nprep = nfwd = 0
    for kind, m in pipe.stage_events:
        if kind == 'prep':
            acc['h2d'] += m[0].elapsed_time(m[1])
            acc['prep_points'] += m[1].elapsed_time(m[2])
            acc['crop_resize'] += m[2].elapsed_time(m[3])
            nprep += 1
        else:
            acc['forward'] += m[0].elapsed_time(m[1])
            nfwd += 1
    out = {'h2d': acc['h2d'] / nprep, 'prep_points': acc['prep_points'] / nprep, 'crop_resize': acc['crop_resize'] / nprep,
           'forward': acc['forward'] / nfwd}
    out['sum_of_parts'] = sum(out.values())
    out['wall_per_frame_serial'] = wall / nfwd
    return {k: round(v, 4) for k, v in out.items()}
