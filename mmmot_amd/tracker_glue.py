"""Hand-off from the device forward to the reference's host-side tracker.

``TrackingModule.predict`` (reference tracking_model.py:68-83) indexes the network outputs by
``test_mode`` and passes them to ``ortools_solve``, which reads every score with ``.item()``
(solvers.py:32-45): O(N*M) device synchronisations once the scores live on the GPU.  ``scores_for_solver``
does the same selection and moves the selected rows to the host in ONE packed copy, returning CPU tensors
with exactly the shapes the solver indexes.  ``predict_assign`` also solves the association on the device
(mmmot_amd.association, the ``ortools_solve`` drop-in) and brings scores and assignment back in one copy;
``predict_assign_chain`` is the same for a model of ``seq_len > 2`` (every link block selected, the chain solver).

A sequence queues before it waits: ``queue_solve`` (pairs: the pair solver, and the track IDs with ``track=``),
``queue_solve_chains`` (WINDOWS of 2 .. 8 frames: one chain solve and one ID launch per batch of windows) and
``queue_scores`` (scores only) return a ``HandOff``, and ``HandOff.fetch()`` is the host copy, a list with one result
(scores, assignment, ids) per pair or window.  The copied buffer has one layout for both, a pair being a window of two
frames; ``unpack_chain_hand_off`` is its host-only reading and ``unpack_hand_off`` the same with a pair's ``ids`` tuple.
"""
from collections import namedtuple

import torch

from .association import (associate, chain_block_size, chain_of, chains_table, pairs_table, select, select_chain,
                          split_of, unpack_chain)
from .tracks import (queue_chain_ids, queue_chain_ids_multi, queue_ids, queue_ids_multi, split_chain_ids, split_ids,
                     split_ids_multi)

# one pair or window on the host: scores (det L, [link 1 x n_t x n_{t+1} ...], new L, end L) as ``scores_for_solver``
# returns them, assignment as ``ortools_solve`` does, ids = (ids0, ids1, frame_start, last_id) of ``tracks.split_ids``
# for a pair, (ids_per_frame, frame_start, last_id, stored) of ``tracks.split_chain_ids`` for a window; None where the
# stage was not asked for
PairResult = ChainResult = namedtuple('HandOffResult', 'scores assignment ids')


def scores_for_solver(det_score, link_scores, new_score, end_score, test_mode):
    """(det 3xL, [link 3xNxM ...], new 3xL, end 3xL) -> CPU (det L, [link 1xNxM ...], new L, end L)
    as consumed at reference tracking_model.py:72-75."""
    tm = int(test_mode)
    parts = [det_score[tm].reshape(-1), new_score[tm].reshape(-1), end_score[tm].reshape(-1)]
    parts += [l[tm:tm + 1].reshape(-1) for l in link_scores]
    flat = torch.cat(parts).to('cpu')  # one device-to-host transfer
    L = det_score.shape[1]
    det, new, end = flat[0:L], flat[L:2 * L], flat[2 * L:3 * L]
    links, o = [], 3 * L
    for l in link_scores:
        n = l.shape[1] * l.shape[2]
        links.append(flat[o:o + n].view(1, l.shape[1], l.shape[2]))
        o += n
    return det, links, new, end


def predict_scores(model, det_imgs, det_info, det_split):
    """Mirror of the first half of ``TrackingModule.predict``: forward + selection, ready for
    ``ortools_solve(det, links, new, end, det_split)``."""
    with torch.no_grad():
        det_score, link_score, new_score, end_score, _ = model(det_imgs, det_info, det_split)
    return scores_for_solver(det_score, link_score, new_score, end_score, model.test_mode)


class HandOff:
    """B frame pairs or windows queued behind their forward, one ``fetch()`` from the host.  ``flat``: the device buffer
    still to be copied (None: nothing is left on the device), read by ``unpack_chain_hand_off`` with ``layout`` =
    (splits, S, K, n_ids); ``pairs``: the entries are pairs, whose ``ids`` come back as ``tracks.split_ids`` gives them.
    ``done``: per pair the (scores, assignment) a pair with an empty frame was given on the host at queue time; ``flat``
    then holds the IDs alone.  In a hand-off over several sequences (``queue_solve`` with ``track=(states, stream_of)``)
    ``done`` holds None for the pairs the device solved, which ``flat`` then carries as usual.  ``outs`` (``queue_scores``): per entry the device outputs of a score-only hand-off."""

    def __init__(self, layout=None, flat=None, done=None, outs=None, test_mode=0, pairs=True, ids_reader=None):
        self.layout, self.flat, self.done, self.outs, self.test_mode = layout, flat, done, outs, test_mode
        # ``ids_reader``: the reading of a multi-state ID launch (``_hand_off``), in place of the single-state ones
        self.split_ids = ids_reader or (split_ids if pairs else split_chain_ids)

    def fetch(self):
        """the host copy -> per entry a result: ONE device-to-host copy of ``flat``; score-only: one per entry"""
        if self.outs is not None:
            return [PairResult(scores_for_solver(o[0], o[1], o[2], o[3], self.test_mode), None, None) for o in self.outs]
        flat = torch.zeros(0) if self.flat is None else self.flat.to('cpu')
        if self.done is None:
            return unpack_chain_hand_off(flat, *self.layout, split_ids=self.split_ids)
        # entries answered on the host stand in ``done``; the others (None there) are read from the buffer, in order
        splits, S, K, n_ids = self.layout
        solved = iter(unpack_chain_hand_off(flat, [s for s, d in zip(splits, self.done) if d is None], S, K))
        ids = unpack_ids(flat, splits, n_ids, self.split_ids)
        return [PairResult(*(next(solved)[:2] if d is None else d), i) for d, i in zip(self.done, ids)]


def unpack_ids(flat, splits, n_ids, split_ids=split_ids):
    """the last ``n_ids`` elements of the host buffer (int32 bits, ``tracks.queue_ids`` / ``queue_chain_ids``) -> per
    entry what ``split_ids`` (``tracks.split_ids`` or ``tracks.split_chain_ids``) gives; None per entry when no IDs
    were queued"""
    if not n_ids:
        return [None] * len(splits)
    return split_ids(flat[flat.numel() - n_ids:].view(torch.int32).numpy(), splits)


def unpack_chain_hand_off(flat, splits, S, K, n_ids=0, split_ids=split_chain_ids):
    """Host fp32 buffer [det S | new S | end S | links K of every entry | per entry the solver block [det L | new L |
    end L | link_0 | .. | link_{T-2}] | n_ids int32 bits] -> per entry a result (views of ``flat``); ``splits``: per
    entry [n_0 .. n_{T-1}], S = sum of the entries' L, K = sum of their link sizes.  A window without detections has
    empty scores and an empty assignment."""
    ids = unpack_ids(flat, splits, n_ids, split_ids)
    res, so, lo, oo = [], 0, 3 * S, 3 * S + K
    for split, i in zip(splits, ids):
        L = sum(split)
        scores = (flat[so:so + L], [], flat[S + so:S + so + L], flat[2 * S + so:2 * S + so + L])
        for a, b in zip(split[:-1], split[1:]):
            scores[1].append(flat[lo:lo + a * b].view(1, a, b))
            lo += a * b
        n = chain_block_size(split)
        res.append(ChainResult(scores, unpack_chain(flat[oo:oo + n], split), i))
        so += L
        oo += n
    return res


def unpack_hand_off(flat, splits, S, K, n_ids=0):
    """``unpack_chain_hand_off`` for pairs: ``splits`` per pair (N, M), ``ids`` as ``tracks.split_ids`` gives them"""
    return unpack_chain_hand_off(flat, splits, S, K, n_ids, split_ids)


def queue_scores(outs, test_mode):
    """The score-only hand-off of B pairs or windows: ``outs`` per entry the device outputs (det 3xL, [link 3 x n_t x
    n_{t+1} ...], new 3xL, end 3xL, ..) of the forward; ``fetch()`` runs ``scores_for_solver`` on each."""
    return HandOff(outs=outs, test_mode=test_mode)


def _hand_off(parts, out, splits, S, K, track, frame_idx, pairs, done=None, block_order=None):
    """the common tail of ``queue_solve`` and ``queue_solve_chains``: with ``track`` the ID launch behind the solver
    blocks ``out``, its int32 result appended to ``parts`` (bits, not values), and the pending ``HandOff``"""
    n_ids, reader = 0, None
    if isinstance(track, tuple):
        # (tracks.TrackStates, stream_of): ONE launch for the entries of several sequences.  ``block_order``: the
        # entries in the order their blocks lie in ``out``
        states, stream_of = track
        order = list(range(len(splits))) if block_order is None else list(block_order)
        o_splits, o_streams = [splits[i] for i in order], [int(stream_of[i]) for i in order]
        ids = (queue_ids_multi if pairs else queue_chain_ids_multi)(states, out, o_splits, [frame_idx[i] for i in order],
                                                                    o_streams)
        parts, n_ids = parts + [ids.view(torch.float32)], ids.numel()
        reader = lambda flat, _: multi_ids_reader(flat, o_splits, o_streams, order, 2 if pairs else 3)
    elif track is not None:
        ids = (queue_ids if pairs else queue_chain_ids)(track, out, splits, frame_idx)
        parts, n_ids = parts + [ids.view(torch.float32)], ids.numel()
    flat = None if not parts else parts[0] if len(parts) == 1 else torch.cat(parts)
    return HandOff((splits, S, K, n_ids), flat, done, pairs=pairs, ids_reader=reader)


def multi_ids_reader(flat, o_splits, o_streams, order, tail=2):
    """host int32 buffer of a multi-state ID launch whose entries were queued in the order ``order`` (entry order[k] of
    the hand-off at place k, of stream o_streams[k]) -> per entry of the hand-off, in ITS order, what
    ``tracks.split_ids_multi`` gives"""
    res = [None] * len(order)
    for i, r in zip(order, split_ids_multi(flat, o_splits, o_streams, tail=tail)):
        res[i] = r
    return res


def queue_solve(selected, splits, track=None, frame_idx=None):
    """Queue the association of B frame pairs behind their forward; nothing waits.  ``selected``: per pair the device
    rows (det L, [link 1 x N x M], new L, end L) of ``association.select``; ``splits``: per pair (N, M).  Returns the
    pending ``HandOff``: one device buffer [det | new | end | link of every pair | solver output].
    ``track`` (a tracks.TrackState; the pairs are then CONSECUTIVE pairs of its sequence, ``frame_idx`` their frame
    index pairs): the ID launch is queued behind the solve and its int32 result rides at the end of the same buffer.
    ``track`` = (tracks.TrackStates, stream_of): the pairs belong to several sequences, pair p to ``stream_of[p]``
    (``states`` may be None: no IDs); one multi-state ID launch serves all of them, and a pair with an empty frame is
    split off - answered on the host as above, while the others are solved in the one launch."""
    splits = [(int(N), int(M)) for N, M in splits]
    if isinstance(track, tuple):
        return _queue_solve_streams(selected, splits, track, frame_idx)
    if any(N == 0 or M == 0 for N, M in splits):  # an empty frame: nothing to link, answered on the host
        done = _host_pairs(selected, splits)
        blocks = None
        if track is not None:
            # the IDs still come from the kernel, so that the state stays on the device: the assignments are uploaded
            blocks = torch.cat([t.reshape(-1).to(torch.float32) for _, a in done for t in (a[0], a[2], a[3], a[1][0])])
            blocks = blocks.to(track.buf.device)
        return _hand_off([], blocks, splits, 0, 0, track, frame_idx, True, done)
    cat = lambda k: torch.cat([(s[k][0] if k == 1 else s[k]).reshape(-1) for s in selected])
    det, new, end, link = cat(0), cat(2), cat(3), cat(1)
    S, K = det.numel(), link.numel()
    buf = torch.cat([det, new, end, link])
    out, _ = torch.ops.mmmot.associate(buf[0:S], buf[S:2 * S], buf[2 * S:3 * S], buf[3 * S:], pairs_table(splits)[0])
    return _hand_off([buf, out], out, splits, S, K, track, frame_idx, True)


def _host_pairs(selected, splits):
    """pairs with an empty frame: their scores to the host and the assignment ``associate`` gives there"""
    host = [scores_for_solver(d.unsqueeze(0), l, n.unsqueeze(0), e.unsqueeze(0), 0) for d, l, n, e in selected]
    return [(sc, associate(sc[0], sc[1], sc[2], sc[3], split)) for sc, split in zip(host, splits)]


def _queue_solve_streams(selected, splits, track, frame_idx):
    """``queue_solve`` over the pairs of several sequences (``track`` = (TrackStates or None, stream_of)): the pairs
    with two non-empty frames in ONE solver launch, the others on the host; the IDs of all of them from ONE multi-state
    launch over [solver output | the uploaded assignments of the host pairs]"""
    states, stream_of = track
    if len(stream_of) != len(splits):
        raise ValueError('queue_solve: %d stream names for %d pairs' % (len(stream_of), len(splits)))
    full = [p for p, (N, M) in enumerate(splits) if N and M]
    host = [p for p, (N, M) in enumerate(splits) if not (N and M)]
    parts, out, S, K = [], None, 0, 0
    if full:
        cat = lambda k: torch.cat([(selected[p][k][0] if k == 1 else selected[p][k]).reshape(-1) for p in full])
        det, new, end, link = cat(0), cat(2), cat(3), cat(1)
        S, K = det.numel(), link.numel()
        buf = torch.cat([det, new, end, link])
        out, _ = torch.ops.mmmot.associate(buf[0:S], buf[S:2 * S], buf[2 * S:3 * S], buf[3 * S:],
                                           pairs_table([splits[p] for p in full])[0])
        parts = [buf, out]
    done = None
    if host:
        done = [None] * len(splits)
        for p, d in zip(host, _host_pairs([selected[p] for p in host], [splits[p] for p in host])):
            done[p] = d
        if states is not None:
            up = torch.cat([t.reshape(-1).to(torch.float32) for p in host for a in (done[p][1],)
                            for t in (a[0], a[2], a[3], a[1][0])]).to(states.buf.device)
            out = up if out is None else torch.cat([out, up])
    return _hand_off(parts, out, splits, S, K, None if states is None else (states, stream_of), frame_idx, True, done,
                     block_order=full + host)


def queue_solve_chains(selected, splits, track=None, frame_idx=None):
    """Queue the association of B windows of 2 .. 8 frames behind their forward; nothing waits.  ``selected``: per window
    the device rows (det L, [link 1 x n_t x n_{t+1} ...], new L, end L) of ``association.select_chain``; ``splits``: per
    window [n_0 .. n_{T-1}].  One ``associate_chains`` launch solves the windows that hold a detection (a frame without
    detections inside such a window goes to the device with it); a window with L = 0 has nothing to solve and is
    answered on the host with an empty assignment.  Returns the pending ``HandOff``.
    ``track`` (a tracks.TrackState; the windows are then CONSECUTIVE windows of its sequence, ``frame_idx`` per window
    its T frame indices): the ID launch walks ALL B windows behind the solve - the empty ones too, so that the state
    stays on the device - and its int32 result rides at the end of the same buffer."""
    splits = [chain_of(s) for s in splits]
    if not splits:
        raise ValueError('queue_solve_chains: no windows')
    full = [(s, sel) for s, sel in zip(splits, selected) if sum(s) > 0]
    if full:
        cat = lambda k: torch.cat([sel[k].reshape(-1) for _, sel in full])
        det, new, end = cat(0), cat(2), cat(3)
        links = [l.reshape(-1) for _, sel in full for l in sel[1]]
        S, K = det.numel(), sum(l.numel() for l in links)
        buf = torch.cat([det, new, end] + links)
        # the blocks of the solved windows one after the other: with the empty windows' blocks of size 0 between them
        # this is the layout of ALL windows, which the ID launch reads
        out, _ = torch.ops.mmmot.associate_chains(buf[0:S], buf[S:2 * S], buf[2 * S:3 * S], buf[3 * S:],
                                                  chains_table([s for s, _ in full])[0])
        parts = [buf, out]
    else:
        dev = track.buf.device if track is not None else None
        S, K, out, parts = 0, 0, torch.empty(0, dtype=torch.float32, device=dev), []
    return _hand_off(parts, out, splits, S, K, track, frame_idx, False)


def predict_assign(model, det_imgs, det_info, det_split):
    """``TrackingModule.predict`` up to the ID bookkeeping: forward, the ``test_mode`` selection and the association on
    the device, then ONE device-to-host copy.  Returns (scores, assignment): the host scores of ``predict_scores`` and
    what ``ortools_solve(*scores, det_split)`` returns."""
    with torch.no_grad():
        det_score, link_score, new_score, end_score, _ = model(det_imgs, det_info, det_split)
    sel = select(det_score, link_score, new_score, end_score, model.test_mode)
    return queue_solve([sel], [split_of(det_split)]).fetch()[0][:2]


def predict_assign_chain(model, det_imgs, det_info, det_split):
    """``predict_assign`` for a model of any ``seq_len >= 2``: forward, the ``test_mode`` rows of all T - 1 link blocks
    (``select_chain``) and the chain association on the device, then ONE device-to-host copy.  Returns (scores,
    assignment): host (det L, [link 1 x n_t x n_{t+1} ...], new L, end L) and what ``ortools_solve(*scores, det_split)``
    returns."""
    with torch.no_grad():
        det_score, link_score, new_score, end_score, _ = model(det_imgs, det_info, det_split)
    split = chain_of(det_split)
    if sum(split) == 0:
        raise ValueError('predict_assign_chain: no detections')
    sel = select_chain(det_score, link_score, new_score, end_score, model.test_mode)
    return queue_solve_chains([sel], [split]).fetch()[0][:2]
