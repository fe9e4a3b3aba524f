"""The frame-pair association of the tracker on the device: a drop-in for the reference's ``ortools_solve``.

``TrackingModule.predict`` (reference tracking_model.py:68-83) hands the selected score rows of a frame pair to
``ortools_solve`` (solvers.py:9-138), which builds a CBC mixed-integer program over every score with ``.item()`` per
value.  With two frames (``det_split = [N, M]``) that program is a maximum-weight bipartite matching (DESIGN.md,
"Frame-pair association"); ``associate`` solves it exactly on the device (csrc/assign.hip, one workgroup per pair) and
returns what ``ortools_solve`` returns: ``(assign_det, [assign_link 1 x N x M], assign_new, assign_end)`` with the
dtype and device of ``det_score``.  Ties go to the smallest index; the answer is the program's optimum.

    from mmmot_amd.association import associate
    assign_det, assign_link, assign_new, assign_end = associate(det, [link], new, end, det_split)

CPU scores go to the device in one copy and come back in one; device scores stay there (nothing waits on the host).
``associate_batch`` solves B pairs (e.g. the rows of one ``forward_batch``) in one launch.  ``associate`` itself refuses
chains of more than two frames and the ``gt`` loss-augmented objective.

Those are ``associate_chain``'s: ``ortools_solve`` for any ``len(det_split) >= 2`` (``sample_max_len > 2``), the program
as a min-cost flow on the layered network of the frames ("Chains"; csrc/assign_chain.hip, one workgroup per
chain), with ``gt=`` the loss-augmented objective of training-time inference:

    from mmmot_amd.association import associate_chain
    assign_det, assign_links, assign_new, assign_end = associate_chain(det, links, new, end, det_split, gt=None)

``associate_chain_batch`` solves B chains in one launch and ``select_chain`` picks the ``test_mode`` rows of every link
block of a ``TrackingNet(seq_len > 2)`` forward.

``associate_sequence`` is the same program at the length of a whole sequence (T up to 4096 frames, L up to 65536
detections; DESIGN.md, "Sequences"; csrc/assign_sequence.hip, one workgroup per sequence), and it can return the
trajectory number of every detection: a unit of flow is a trajectory and therefore an ID.

    from mmmot_amd.association import associate_sequence
    assign_det, assign_links, assign_new, assign_end, ids, n_tracks = associate_sequence(
        det, links, new, end, det_split, return_ids=True)

``associate_sequence_batch`` solves B sequences in one launch.

``associate_sequence_gaps`` adds skip links ("Sequences: skip links"; the same csrc/assign_sequence.hip):
``link_scores[g - 1][t]`` scores the links from frame t to frame t + g for every gap g = 1 .. G <= 8, so a trajectory
may miss up to G - 1 frames instead of ending at the first missed detection:

    from mmmot_amd.association import associate_sequence_gaps
    assign_det, assign_links, assign_new, assign_end, ids, n_tracks = associate_sequence_gaps(
        det, [links_gap1, links_gap2, links_gap3], new, end, det_split, return_ids=True)

``associate_sequence_gaps_batch`` solves B sequences with the same number of gaps in one launch.

The four families share one host path, ``_solve``: the refusals of a batch, the packing table (``_offsets``), one launch
through ``_launch``, the status check and the walk over every output block (``unpack_gaps``); a single-instance function
is its own checks and empty-case answer around that path at B = 1.

``MotionGate`` with ``gate_links`` / ``gate_sequence_links`` ("Sequences: motion gate"; csrc/gate_links.hip, one
launch for any number of link blocks) turns the links no object could have travelled - by the 3D boxes, the frame
numbers and, with poses, the ego motion - into NaN scores, which every solver above reads as absent edges:

    from mmmot_amd.association import MotionGate, gate_sequence_links
    gated, kept = gate_sequence_links([links_gap1, links_gap2, links_gap3], frames, MotionGate(max_speed=4.0, slack=2.0))
"""
from collections import namedtuple

import numpy as np
import torch

from . import torch_ops  # noqa: F401  (registers mmmot::associate, mmmot::associate_chains, mmmot::associate_sequences[_gap])


# ---- what the four families share: the launch seam, the packing offsets, the block walk, the solve path ------------------
DEVICE = 'cuda'  # where host scores are solved: they go there in one copy and the results come back in one


def _launch(op, det, new, end, link, tables, max_gap=None):
    """Every solver launch of this module: mmmot::``op`` over the four flat fp32 score tensors and the operator's CPU
    int32 ``tables``, with ``max_gap`` for the operator that takes it."""
    return getattr(torch.ops.mmmot, op)(det, new, end, link, *tables, *(() if max_gap is None else (max_gap,)))


def launch_sequences(scores, tables, max_gap):
    """The sequence operator for link blocks of the gaps 1 .. ``max_gap``, chosen here and nowhere else:
    mmmot::associate_sequences for next-frame links alone, else mmmot::associate_sequences_gap.  ``scores``: (det, new,
    end, link) flat on the device; ``tables``: (seqs, nts) of ``gap_sequences_table``.  -> (out, ids, objective, info)"""
    if max_gap == 1:
        return _launch('associate_sequences', *scores, tables)
    return _launch('associate_sequences_gap', *scores, tables, max_gap)


def gap_link_sizes(split, max_gap):
    """The (n_t, n_{t+g}) of every link block in layout order: all g = 1 blocks in frame order, then all g = 2 blocks,
    .. up to g = ``max_gap``."""
    return [(split[t], split[t + g]) for g in range(1, int(max_gap) + 1) for t in range(len(split) - g)]


def _offsets(splits, max_gap=1):
    """The score, link and output offsets of instances packed one after the other, each with the link blocks of the gaps
    1 .. ``max_gap``: three lists, each closed by its total.  The running sums every table is built on."""
    sos, los, oos, G = [0], [0], [0], int(max_gap)
    for split in splits:
        L, K = sum(split), sum(a * b for g in range(1, G + 1) for a, b in zip(split, split[g:]))
        sos.append(sos[-1] + L)
        los.append(los[-1] + K)
        oos.append(oos[-1] + 3 * L + K)
    return sos, los, oos


def gap_block_size(split, max_gap):
    return _offsets([split], max_gap)[2][1]


def unpack_gaps(block, split, max_gap, like=None, link_sizes=None):
    """One instance's output block [det L | new L | end L | g = 1 blocks | .. | g = max_gap blocks] -> (det, [[links of
    gap 1], [links of gap 2], ..], new, end), views of ``block``.  With ``like`` the results take its dtype, det / new /
    end its size and link (g, t) the size ``link_sizes[g - 1][t]``: one for every block.  The one walk over a block:
    ``unpack_chain`` and ``unpack`` are its one-gap case."""
    L, T, ab = sum(split), len(split), gap_link_sizes(split, max_gap)
    sizes = [L, L, L] + [a * b for a, b in ab]
    if block.numel() != sum(sizes):
        block = block[0:sum(sizes)]
    det, new, end, *flat = block.split_with_sizes(sizes)  # every view in one call
    if like is None:
        flat = [l.view(1, a, b) for l, (a, b) in zip(flat, ab)]
    else:
        size = like.size()
        if size != (L,):  # else they have it
            det, new, end = det.view(size), new.view(size), end.view(size)
        flat = [l.view(size) for l, size in zip(flat, [size for row in link_sizes for size in row])]
        if like.dtype != block.dtype:  # the same dtype: .to would hand back the tensor itself
            det, new, end, *flat = (t.to(like.dtype) for t in (det, new, end, *flat))
    starts = [0] + [g * T - g * (g + 1) // 2 for g in range(1, int(max_gap) + 1)]  # gap g holds T - g blocks
    return det, [flat[i:j] for i, j in zip(starts, starts[1:])], new, end


def _f32(t):
    t = t.detach().reshape(-1)
    return t if t.dtype == torch.float32 else t.to(torch.float32)  # as .to would: the tensor itself


# A family of solvers.  ``name`` (of its single-instance function), ``what`` it solves and what every one ``needs`` not
# to be ``empty`` word the refusals of a batch; ``table(splits, max_gap)`` and ``launch(scores, tables, max_gap)`` are
# looked up when called; ``ids``: two tables, and IDs and a status word come back too; ``nested``: links nested by gap.
_Family = namedtuple('_Family', 'name what needs empty table launch ids nested')
_PAIRS = _Family('associate', 'pair', 'detections in both frames (use associate for empty frames)', lambda s: 0 in s,
                 lambda splits, G: pairs_table(splits), lambda sc, tb, G: _launch('associate', *sc, tb), False, False)
_CHAINS = _Family('associate_chain', 'chain', 'a detection (use associate_chain for empty chains)', lambda s: sum(s) == 0,
                  lambda splits, G: chains_table(splits), lambda sc, tb, G: _launch('associate_chains', *sc, tb), False, False)
_SEQUENCES = _Family('associate_sequence', 'sequence', 'a detection (use associate_sequence for empty sequences)',
                     lambda s: sum(s) == 0, lambda splits, G: gap_sequences_table(splits, G), launch_sequences, True, False)
# associate_sequence_gaps keeps its own convention: the operator with skip links for every G, one gap included
_GAPS = _SEQUENCES._replace(name='associate_sequence_gaps', needs='a detection (use associate_sequence_gaps for empty sequences)',
                            launch=lambda sc, tb, G: _launch('associate_sequences_gap', *sc, tb, G), nested=True)


def _solve(fam, splits, flats, likes, links, max_gap=1, return_ids=False, single=False):
    """The one path from checked scores to results: B instances, one launch.  ``flats()``, called behind the refusals of
    the batch, gives per instance its flat fp32 scores [det | new | end | links], or their four parts in a list; ``likes``
    / ``links``: per instance the det scores and link blocks whose dtype and sizes the results take; ``single``: the call
    of a single-instance function, whose scores reach the operator as they are and, if on the host, by way of DEVICE.
    Returns (per instance (det, links, new, end[, per-frame IDs, track count]), the fp64 optima [B])."""
    if not splits:
        raise ValueError('%s_batch: no %ss' % (fam.name, fam.what))
    if not single and any(fam.empty(s) for s in splits):  # a single-instance function has answered the empty case
        raise ValueError('%s_batch: every %s needs %s' % (fam.name, fam.what, fam.needs))
    host = single and not likes[0].is_cuda
    parts = []
    for sc, s in zip(flats(), splits):
        sc = sc.to(DEVICE) if host else sc  # the one host-to-device copy
        parts.append(sc if isinstance(sc, list) else sc.split_with_sizes([sum(s)] * 3 + [sc.numel() - 3 * sum(s)]))
    # one sequence, or the instance of a single-instance function, goes as it is; a batch of one pair or chain is joined
    scores = parts[0] if len(parts) == 1 and (single or fam.ids) else [torch.cat([p[k] for p in parts]) for k in range(4)]
    if fam.ids:
        seqs, nts, offs, sos = fam.table(splits, max_gap)
        out, ids, obj, info = fam.launch(scores, (seqs, nts), max_gap)
        info = info.cpu().numpy()  # the one status read
        check_status(info)
    else:
        (table, offs), ids = fam.table(splits, max_gap), None
        out, obj = fam.launch(scores, (table,), max_gap)
    if host:
        out, ids = out.cpu(), ids.cpu() if fam.ids else None  # one device-to-host copy each
    one, res = len(splits) == 1, []
    blocks = [out] if one else out.split_with_sizes([b - a for a, b in zip(offs, offs[1:] + [out.numel()])])
    for i, (s, like, l) in enumerate(zip(splits, likes, links)):
        sizes = [[x.size() for x in row] for row in l] if fam.nested else [[x.size() for x in l]]
        r = unpack_gaps(blocks[i], s, max_gap, like, sizes)
        r = r if fam.nested else (r[0], r[1][0], r[2], r[3])
        if return_ids:
            r += (split_ids(ids if one else ids[sos[i]:sos[i] + sum(s)], s), int(info[i, 1]))
        res.append(r)
    return res, obj


def _batch_flats(check, flatten, det_scores, link_scores, new_scores, end_scores, splits, gts):
    """the ``flats`` of a batch: per instance its scores, checked and flattened when ``_solve`` calls for them"""
    def flats():
        out, gt = [], gts if gts is not None else [None] * len(splits)
        for d, l, n, e, s, g in zip(det_scores, link_scores, new_scores, end_scores, splits, gt):
            check(d, l, n, e, s)
            out.append(flatten(d, l, n, e, g))
        return out
    return flats


def _empty(det_score, link_scores, split=None):
    """no detection: zeros in the shapes of the scores and, with ``split``, no IDs per frame and no track; no launch"""
    zeros = lambda l: [zeros(x) for x in l] if isinstance(l, (list, tuple)) else det_score.new_zeros(l.size())
    z = zeros(det_score)
    ids = () if split is None else ([torch.zeros(0, dtype=torch.int64, device=det_score.device) for _ in split], 0)
    return (z, zeros(link_scores), z.clone(), z.clone()) + ids


# ---- frame pairs ----------------------------------------------------------------------------------------------------------
def split_of(det_split):
    """(N, M) of a two-frame ``det_split`` (ints or 1-element tensors, as eval_seq passes them)."""
    if len(det_split) != 2:
        raise ValueError('associate solves frame pairs: det_split must have 2 entries, got %d (chains of more frames '
                         'are a min-cost flow, not supported)' % len(det_split))
    return int(det_split[0]), int(det_split[1])


def select(det_score, link_scores, new_score, end_score, test_mode):
    """The rows ``TrackingModule.predict`` passes to the solver (tracking_model.py:72-75), as device views:
    (det L, [link 1 x N x M], new L, end L)."""
    tm = int(test_mode)
    return det_score[tm], [link_scores[0][tm:tm + 1]], new_score[tm], end_score[tm]


def pairs_table(splits):
    """CPU int32 [B, 4] (N, M, score offset, link offset) of pairs packed one after the other, and the output offsets."""
    sos, los, oos = _offsets(splits)
    return torch.tensor([(N, M, so, lo) for (N, M), so, lo in zip(splits, sos, los)], dtype=torch.int32), oos[:-1]


def unpack(block, N, M, like=None, link_size=None):
    """One pair's output block [det L | new L | end L | link N*M] -> the ortools_solve tuple (views of ``block``): the
    two-frame case of ``unpack_chain``."""
    return unpack_chain(block, [N, M], like, None if like is None else [link_size])


def _host_unmatched(det_score, link_score, new_score, end_score, N, M):
    """N == 0 or M == 0: no link exists, every detection takes det = new = end = [its score sum > 0]; no launch."""
    d, n, e = (np.asarray(t.detach().reshape(-1).cpu(), dtype=np.float64) for t in (det_score, new_score, end_score))
    x = np.concatenate([(d[:N] + n[:N] + e[:N]) > 0, (d[N:] + e[N:] + n[N:]) > 0]).astype(np.float32)
    xt = torch.from_numpy(x).to(det_score.device).to(det_score.dtype).view(det_score.size())
    return xt.clone(), [det_score.new_zeros(link_score.size())], xt.clone(), xt.clone()


def associate(det_score, link_score, new_score, end_score, det_split, gt=None):
    """Drop-in for reference ``ortools_solve(det_score, link_score, new_score, end_score, det_split)`` with two frames:
    det / new / end [L], link_score = [link 1 x N x M]."""
    if gt is not None:
        raise NotImplementedError('associate: the gt (loss-augmented) objective is not supported')
    N, M = split_of(det_split)
    link = link_score[0]
    L = N + M
    if det_score.numel() != L or new_score.numel() != L or end_score.numel() != L or link.numel() != N * M:
        raise ValueError('associate: scores do not match det_split [%d, %d]' % (N, M))
    if N == 0 or M == 0:
        return _host_unmatched(det_score, link, new_score, end_score, N, M)
    parts = [_f32(t) for t in (det_score, new_score, end_score, link)]
    # device scores go to the operator as they are; host scores travel as one tensor
    scores = [p.contiguous() for p in parts] if det_score.is_cuda else torch.cat(parts)
    return _solve(_PAIRS, [(N, M)], lambda: [scores], [det_score], [link_score], single=True)[0][0]


def associate_batch(det_scores, link_scores, new_scores, end_scores, det_splits, return_objective=False):
    """B frame pairs in one launch.  Per pair p: det_scores[p] / new_scores[p] / end_scores[p] [L_p],
    link_scores[p] = [link 1 x N_p x M_p] (the ``select`` rows of a ``forward_batch`` result), all on one device.
    Returns the list of ortools_solve tuples (on that device), and the fp64 optima [B] when ``return_objective``."""
    flats = lambda: [[_f32(t) for t in (d, n, e, l[0])] for d, l, n, e in zip(det_scores, link_scores, new_scores, end_scores)]
    res, obj = _solve(_PAIRS, [split_of(s) for s in det_splits], flats, det_scores, link_scores)
    return (res, obj) if return_objective else res


# ---- chains of T >= 2 frames -------------------------------------------------------------------------------------------
def chain_of(det_split):
    """[n_0 .. n_{T-1}] of a ``det_split`` of T >= 2 frames (ints or 1-element tensors)."""
    split = [int(n) for n in det_split]
    if len(split) < 2:
        raise ValueError('associate_chain: det_split must have at least 2 entries, got %d' % len(split))
    return split


def select_chain(det_score, link_scores, new_score, end_score, test_mode):
    """The ``test_mode`` rows of a forward over T frames, every one of the T - 1 link blocks included (the reference's
    ``predict`` slices ``link_score[0]`` only): (det L, [link 1 x n_t x n_{t+1} ...], new L, end L), device views."""
    tm = int(test_mode)
    return det_score[tm], [l[tm:tm + 1] for l in link_scores], new_score[tm], end_score[tm]


def chains_table(splits):
    """CPU int32 [B, 11] (T, score offset, link offset, n_0 .. n_7) of chains packed one after the other, and the
    output offsets."""
    for split in splits:
        if len(split) > torch_ops.CHAIN_MAX_T:
            raise ValueError('associate_chain: at most %d frames, got %d' % (torch_ops.CHAIN_MAX_T, len(split)))
    sos, los, oos = _offsets(splits)
    rows = [[len(s), so, lo] + list(s) + [0] * (torch_ops.CHAIN_MAX_T - len(s)) for s, so, lo in zip(splits, sos, los)]
    return torch.tensor(rows, dtype=torch.int32), oos[:-1]


def chain_block_size(split):
    return gap_block_size(split, 1)


def unpack_chain(block, split, like=None, link_sizes=None):
    """One chain's output block [det L | new L | end L | link_0 | .. | link_{T-2}] -> the ortools_solve tuple (views)."""
    det, links, new, end = unpack_gaps(block, split, 1, like, [link_sizes])
    return det, links[0], new, end


def _check_chain(det_score, link_scores, new_score, end_score, split):
    L = sum(split)
    if len(link_scores) != len(split) - 1 or any(t.numel() != L for t in (det_score, new_score, end_score)) or \
            any(l.numel() != a * b for l, a, b in zip(link_scores, split[:-1], split[1:])):
        raise ValueError('associate_chain: scores do not match det_split %s' % (split,))


def _flat_scores(det_score, link_scores, new_score, end_score, gt):
    """[det | new | end | link_0 | ..] fp32 on the scores' device; with ``gt`` the loss-augmented scores of
    solvers.py:50-81: the objective gains gt - y * gt_eff per variable, gt_eff = gt + (gt == 0) * -1, so every score
    drops by gt_eff (the constant sum of gt does not move the arg-max) - one fused expression."""
    flat = torch.cat([_f32(t) for t in (det_score, new_score, end_score, *link_scores)])
    if gt is None:
        return flat
    g = torch.cat([_f32(t) for t in (gt[0], gt[1], gt[2], *gt[3])]).to(flat.device)
    if g.numel() != flat.numel():
        raise ValueError('associate_chain: gt does not match the scores')
    return flat - (g + g.eq(0).float().mul(-1))


def associate_chain(det_score, link_scores, new_score, end_score, det_split, gt=None):
    """Drop-in for reference ``ortools_solve(det_score, link_score, new_score, end_score, det_split, gt)`` with any
    ``len(det_split) >= 2``: det / new / end [L], link_scores = [link 1 x n_t x n_{t+1} ...]; ``gt`` = (gt_det, gt_new,
    gt_end, [gt_link ...]) selects the loss-augmented objective.  Returns (assign_det, [assign_link ...], assign_new,
    assign_end) with the dtype, device and shapes of the scores."""
    split = chain_of(det_split)
    _check_chain(det_score, link_scores, new_score, end_score, split)
    if sum(split) == 0:
        return _empty(det_score, link_scores)
    flat = _flat_scores(det_score, link_scores, new_score, end_score, gt)
    return _solve(_CHAINS, [split], lambda: [flat], [det_score], [link_scores], single=True)[0][0]


def associate_chain_batch(det_scores, link_scores, new_scores, end_scores, det_splits, gts=None,
                          return_objective=False):
    """B chains in one launch.  Per chain c: det_scores[c] / new_scores[c] / end_scores[c] [L_c], link_scores[c] = [link
    1 x n_t x n_{t+1} ...] (the ``select_chain`` rows), all on one device; ``gts``: None or per chain a ``gt`` tuple (or
    None).  Returns the list of ortools_solve tuples (on that device), and the fp64 optima [B] of the solved scores when
    ``return_objective``."""
    splits = [chain_of(s) for s in det_splits]
    flats = _batch_flats(_check_chain, _flat_scores, det_scores, link_scores, new_scores, end_scores, splits, gts)
    res, obj = _solve(_CHAINS, splits, flats, det_scores, link_scores)
    return (res, obj) if return_objective else res


# ---- whole sequences: one min-cost flow each ---------------------------------------------------------------------------
class AssociationError(RuntimeError):
    """The sequence solver ended a sequence at one of its loop bounds, or found it outside the launch contract: its
    status word is in ``.status`` (include/mmmot_hip.h, MMMOT_SEQ_*), the sequence's place in the batch in ``.index``."""

    def __init__(self, index, status):
        names = {1: 'outside the launch contract', 2: 'augmentation bound hit', 3: 'pass bound hit',
                 4: 'path walk bound hit'}
        super().__init__('associate_sequence: sequence %d not solved: %s (status %d)'
                         % (index, names.get(status, 'unknown status'), status))
        self.index, self.status = index, status


SEQ_MAX_N = torch_ops.MAX_ASSOC


def sequence_of(det_split):
    """[n_0 .. n_{T-1}] of a ``det_split`` of 2 <= T <= 4096 frames of at most 512 detections, L <= 65536."""
    split = [int(n) for n in det_split]
    if len(split) < 2:
        raise ValueError('associate_sequence: det_split must have at least 2 entries, got %d' % len(split))
    if len(split) > torch_ops.SEQ_MAX_T:
        raise ValueError('associate_sequence: at most %d frames, got %d' % (torch_ops.SEQ_MAX_T, len(split)))
    if min(split) < 0 or max(split) > SEQ_MAX_N:
        raise ValueError('associate_sequence: every frame needs 0 <= n_t <= %d detections' % SEQ_MAX_N)
    if sum(split) > torch_ops.SEQ_MAX_L:
        raise ValueError('associate_sequence: at most %d detections, got %d' % (torch_ops.SEQ_MAX_L, sum(split)))
    return split


def sequences_table(splits):
    """``gap_sequences_table`` of next-frame links alone."""
    return gap_sequences_table(splits, 1)


def check_status(info):
    """``info``: host int32 [B, 4]; raises AssociationError for the first sequence whose status word is set"""
    bad = np.nonzero(info[:, 0])[0]
    if bad.size:
        raise AssociationError(int(bad[0]), int(info[bad[0], 0]))


_raise_status = check_status


def split_ids(ids, split):
    """flat per-detection IDs -> per frame an int64 array (views of one int64 copy)"""
    ids = ids.to(torch.int64)
    return list(ids.split(split))


def associate_sequence(det_score, link_scores, new_score, end_score, det_split, gt=None, return_ids=False):
    """``ortools_solve(det_score, link_score, new_score, end_score, det_split, gt)`` at the length of a whole sequence
    (2 <= T <= 4096 frames of at most 512 detections, L <= 65536): the arguments, the results, the shapes, dtypes and the
    host / device rules of ``associate_chain``.  With ``return_ids`` also the per-frame int64 trajectory numbers (-1: not
    kept; trajectories numbered in the order of first frame, then detection index) and the trajectory count.  Raises
    AssociationError when the solver reports a status (one host read of four words per call)."""
    split = sequence_of(det_split)
    _check_chain(det_score, link_scores, new_score, end_score, split)
    if sum(split) == 0:
        return _empty(det_score, link_scores, split if return_ids else None)
    flat = _flat_scores(det_score, link_scores, new_score, end_score, gt)
    return _solve(_SEQUENCES, [split], lambda: [flat], [det_score], [link_scores], 1, return_ids, single=True)[0][0]


def associate_sequence_batch(det_scores, link_scores, new_scores, end_scores, det_splits, gts=None,
                             return_objective=False, return_ids=False):
    """B sequences in one launch, one workgroup each.  Per sequence s: det_scores[s] / new_scores[s] / end_scores[s]
    [L_s], link_scores[s] = [link 1 x n_t x n_{t+1} ...], all on one device; ``gts``: None or per sequence a ``gt`` tuple
    (or None).  Returns the list of ortools_solve tuples (on that device) - each followed by its per-frame IDs and its
    trajectory count with ``return_ids`` - and the fp64 optima [B] when ``return_objective``."""
    splits = [sequence_of(s) for s in det_splits]
    flats = _batch_flats(_check_chain, _flat_scores, det_scores, link_scores, new_scores, end_scores, splits, gts)
    res, obj = _solve(_SEQUENCES, splits, flats, det_scores, link_scores, 1, return_ids)
    return (res, obj) if return_objective else res


# ---- whole sequences with skip links: a trajectory may miss up to max_gap - 1 frames ---------------------------------------
SEQ_MAX_GAP = torch_ops.SEQ_MAX_GAP


def gap_sequences_table(splits, max_gap):
    """(seqs CPU int32 [B, 4] = (T, score offset, link offset, offset of n_0 in nts), nts CPU int32 flat, output
    offsets, score offsets) of sequences packed one after the other, with link blocks of every gap 1 .. ``max_gap``."""
    sos, los, oos = _offsets(splits, max_gap)
    if los[-1] >= 2 ** 31 - 1 or oos[-1] >= 2 ** 31 - 1:
        raise ValueError('associate_sequence_gaps: the link scores of one launch must number fewer than 2^31')
    rows, nts = [], []
    for split, so, lo in zip(splits, sos, los):
        rows.append([len(split), so, lo, len(nts)])
        nts.extend(split)
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(nts, dtype=torch.int32), oos[:-1], sos[:-1]


def _check_gaps(det_score, link_scores, new_score, end_score, split):
    """refuses, naming the fault, what ``associate_sequence_gaps`` cannot solve; returns max_gap"""
    G, T, L = len(link_scores), len(split), sum(split)
    if G < 1 or G > SEQ_MAX_GAP:
        raise ValueError('associate_sequence_gaps: link_scores must hold the blocks of 1 .. %d gaps, got %d' % (SEQ_MAX_GAP, G))
    if G >= T:
        raise ValueError('associate_sequence_gaps: max_gap = %d needs more than %d frames, got %d' % (G, G, T))
    if any(t.numel() != L for t in (det_score, new_score, end_score)):
        raise ValueError('associate_sequence_gaps: det / new / end scores do not match det_split %s' % (split,))
    for g, row in enumerate(link_scores, 1):
        if len(row) != T - g:
            raise ValueError('associate_sequence_gaps: gap %d needs %d link blocks, got %d' % (g, T - g, len(row)))
        for t, l in enumerate(row):
            if tuple(l.shape) not in ((split[t], split[t + g]), (1, split[t], split[t + g])):
                raise ValueError('associate_sequence_gaps: link block (gap %d, frame %d) must be %d x %d, got %s'
                                 % (g, t, split[t], split[t + g], tuple(l.shape)))
    return G


def _flat_gaps(det_score, link_scores, new_score, end_score, gt):
    if gt is not None:
        if len(gt) != 4 or len(gt[3]) != len(link_scores) or any(len(a) != len(b) for a, b in zip(gt[3], link_scores)):
            raise ValueError('associate_sequence_gaps: gt does not match the scores')
        gt = (gt[0], gt[1], gt[2], [g for row in gt[3] for g in row])
    return _flat_scores(det_score, [l for row in link_scores for l in row], new_score, end_score, gt)


def associate_sequence_gaps(det_score, link_scores, new_score, end_score, det_split, gt=None, return_ids=False):
    """``associate_sequence`` with skip links: ``link_scores[g - 1][t]`` is the n_t x n_{t+g} (or 1 x n_t x n_{t+g})
    block of the links from frame t to frame t + g, ``G = len(link_scores)`` <= 8 the largest gap, G < T.  A kept
    detection continues into one detection of the next G frames or ends; a trajectory may miss up to G - 1 frames and may
    cross an empty frame.  Returns (det, [[links of gap 1], [links of gap 2], ..], new, end) with the dtype, device and
    shapes of the scores, and with ``return_ids`` the per-frame int64 trajectory numbers and the trajectory count.  ``gt``
    = (gt_det, gt_new, gt_end, [[gt_link of gap 1 ..], ..]) selects the loss-augmented objective.  Host or device inputs,
    as ``associate_sequence``; with one gap the results are those of ``associate_sequence``.  Refuses before any launch,
    with a ValueError, scores that do not match; raises AssociationError when the solver reports a status."""
    split = sequence_of(det_split)
    G = _check_gaps(det_score, link_scores, new_score, end_score, split)
    if sum(split) == 0:
        return _empty(det_score, link_scores, split if return_ids else None)
    flat = _flat_gaps(det_score, link_scores, new_score, end_score, gt)
    return _solve(_GAPS, [split], lambda: [flat], [det_score], [link_scores], G, return_ids, single=True)[0][0]


def associate_sequence_gaps_batch(det_scores, link_scores, new_scores, end_scores, det_splits, gts=None,
                                  return_objective=False, return_ids=False):
    """B sequences with skip links in one launch, all with the same number of gaps; per sequence the arguments of
    ``associate_sequence_gaps``, all on one device.  Returns what ``associate_sequence_batch`` returns, the links nested
    by gap."""
    splits = [sequence_of(s) for s in det_splits]
    G = len(link_scores[0]) if len(link_scores) else 0  # no link blocks: the refusals of the batch come first

    def check(d, l, n, e, s):
        if _check_gaps(d, l, n, e, s) != G:
            raise ValueError('associate_sequence_gaps_batch: every sequence needs the blocks of the same %d gaps' % G)
    flats = _batch_flats(check, _flat_gaps, det_scores, link_scores, new_scores, end_scores, splits, gts)
    res, obj = _solve(_GAPS, splits, flats, det_scores, link_scores, G, return_ids)
    return (res, obj) if return_objective else res


# ---- motion gate: links no object could have travelled become absent edges (csrc/gate_links.hip) -------------------------
GATE_MAX_DT = torch_ops.GATE_MAX_DT


class GateError(AssociationError):
    """The motion gate found a block outside its launch contract (``kept`` = -1): the block's place in the call in
    ``.index``, its frames in ``.frames``."""

    def __init__(self, index, frames):
        RuntimeError.__init__(self, 'gate_links: block %d (frames %d -> %d) lies outside the launch contract: frame '
                                    'indices, increasing frame numbers, the records\' reach or the link range'
                                    % (index, frames[0], frames[1]))
        self.index, self.status, self.frames = index, -1, frames


class MotionGate:
    """The parameters of the motion gate ("Sequences: motion gate") and its two fp64 tables: a link
    between two detections ``dt`` frame numbers apart passes iff ``1 <= dt <= max_dt`` and the squared distance of the
    two box centres - ``mode`` 'ground': in the camera's x / z plane, '3d': with y - is at most ``r2[dt] = (max_speed *
    dt + slack) ** 2``; with ``max_size_ratio`` > 0 also each of the three dimensions may differ by at most that factor.
    ``weight`` > 0 lowers a passing score by ``weight * d2 / r2[dt]``; 0 leaves it bit for bit.  ``max_speed`` is in
    metres per frame number (4.0: 40 m/s at KITTI's 10 Hz), ``slack`` in metres (the detector's localisation noise)."""

    def __init__(self, max_speed=4.0, slack=2.0, max_dt=8, mode='ground', max_size_ratio=0.0, weight=0.0):
        fin = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        if not (fin(max_speed) and fin(slack) and max_speed >= 0 and slack >= 0 and max_speed + slack > 0):
            raise ValueError('MotionGate: max_speed and slack must be finite and >= 0, and not both 0, got %r, %r'
                             % (max_speed, slack))
        if not isinstance(max_dt, (int, np.integer)) or not 1 <= int(max_dt) <= GATE_MAX_DT:
            raise ValueError('MotionGate: max_dt must be an integer in 1 .. %d, got %r' % (GATE_MAX_DT, max_dt))
        if mode not in torch_ops.GATE_MODES:
            raise ValueError('MotionGate: mode must be one of %s, got %r' % (sorted(torch_ops.GATE_MODES), mode))
        if not (fin(max_size_ratio) and (max_size_ratio == 0 or max_size_ratio >= 1)):
            raise ValueError('MotionGate: max_size_ratio must be 0 (off) or a finite factor >= 1, got %r' % (max_size_ratio,))
        if not (fin(weight) and weight >= 0):
            raise ValueError('MotionGate: weight must be finite and >= 0, got %r' % (weight,))
        self.max_speed, self.slack, self.max_dt, self.mode = float(max_speed), float(slack), int(max_dt), mode
        self.max_size_ratio, self.weight = float(max_size_ratio), float(weight)
        r = np.float64(self.max_speed) * np.arange(self.max_dt + 1, dtype=np.float64) + np.float64(self.slack)
        self.r2 = r * r
        self.inv_r2 = np.zeros_like(self.r2)  # entry 0 is never read: dt >= 1
        self.inv_r2[1:] = np.float64(1.0) / self.r2[1:]

    def block(self, p):
        """(the int32 block of torch_ops.gate_layout, sizes) of a ``pack_gate`` result under this gate"""
        sizes = [len(p['det']), len(p['frame_no']), len(p['blocks']), p['rec_gaps'], self.max_dt,
                 torch_ops.GATE_MODES[self.mode], p['n_link']]
        lay, n = torch_ops.gate_layout(sizes)
        tab = dict(p, r2=self.r2, inv_r2=self.inv_r2)
        packed = np.zeros(n, np.int32)
        for name, (o, m) in lay.items():
            if m:
                packed[o:o + m] = np.ascontiguousarray(tab[name]).reshape(-1).view(np.int32)
        return packed, sizes


def gap_pairs(n_frames, max_gap):
    """the (t, t + g) of every link block of a sequence in layout order, as ``gap_link_sizes``"""
    return [(t, t + g) for g in range(1, int(max_gap) + 1) for t in range(int(n_frames) - g)]


def pack_gate(frames, frame_idx=None, poses=None, calib=None, pairs=None):
    """The host side of ``gate_links`` before the launch.  ``frames``: per frame the detection dict (``dimensions``,
    ``location``, .. as ``tracks.pack_fill`` reads them; the frames of several sequences may follow each other);
    ``frame_idx``: their frame numbers (default 0, 1, ..); ``pairs``: the (a, b) frame positions of every link block, a <
    b, in the order of the blocks (default: the consecutive pairs) - ``gap_pairs(T, G)`` for a sequence with skip links.
    ``poses``: per frame (pos, rad), for all frames or none, with ``calib`` as ``tracks.fill_gaps`` takes them; every
    listed pair then gets the record ``ego.box_motion`` of its two frames.  Returns a dict of the tables of
    mmmot_gate_links: ``det`` fp32 [L, 12], ``frame_start``, ``frame_no``, ``blocks`` int32 [NB, 4], ``xf`` fp64 [F,
    rec_gaps, 33] (or None, ``rec_gaps`` 0), ``sizes`` the (n_a, n_b) per block and ``n_link``."""
    from . import ego
    from .tracks import box_rows
    F = len(frames)
    pairs = [(t, t + 1) for t in range(F - 1)] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    no = np.arange(F, dtype=np.int64) if frame_idx is None else np.asarray(frame_idx, dtype=np.int64).reshape(-1)
    if len(no) != F:
        raise ValueError('gate_links: %d frames but %d frame numbers' % (F, len(no)))
    if np.abs(no).max(initial=0) >= 2 ** 31:
        raise ValueError('gate_links: frame numbers must fit 32 bits')
    if poses is not None and (len(poses) != F or any(q is None for q in poses)):
        raise ValueError('gate_links: poses are given for all frames or none')
    if poses is not None and calib is None:
        raise ValueError('gate_links: poses need calib (R0_rect, Tr_velo_to_cam, Tr_imu_to_velo)')
    counts = [len(np.asarray(d['location'], dtype=np.float64).reshape(-1, 3)) for d in frames]
    det = [box_rows(d, m) for d, m in zip(frames, counts)]
    blocks, sizes, off = [], [], 0
    for i, (a, b) in enumerate(pairs):
        if not 0 <= a < b < F:
            raise ValueError('gate_links: pair %d joins frames %d -> %d; it needs 0 <= a < b < %d' % (i, a, b, F))
        if no[b] <= no[a]:
            raise ValueError('gate_links: pair %d: the frame numbers must increase, got %d -> %d' % (i, no[a], no[b]))
        blocks.append((a, b, off, 0))
        sizes.append((counts[a], counts[b]))
        off += counts[a] * counts[b]
    if off >= 2 ** 31 - 1:
        raise ValueError('gate_links: the links of one launch must number fewer than 2^31')
    xf, rec_gaps = None, 0
    if poses is not None and pairs:
        rec_gaps = max(b - a for a, b in pairs)
        xf = np.zeros((F, rec_gaps, torch_ops.FILL_REC), np.float64)
        xf[:, :, 0:16] = xf[:, :, 16:32] = np.eye(4).reshape(-1)
        for a, b in set(pairs):
            C, Ci, dyaw = ego.box_motion(poses[a], poses[b], calib)
            rec = xf[a, b - a - 1]
            rec[0:16], rec[16:32], rec[32] = C.reshape(-1), Ci.reshape(-1), dyaw
    return {'det': np.concatenate(det + [np.zeros((0, 12), np.float32)]),
            'frame_start': np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32),
            'frame_no': no.astype(np.int32), 'blocks': np.asarray(blocks, np.int32).reshape(-1, 4), 'xf': xf,
            'rec_gaps': rec_gaps, 'sizes': sizes, 'n_link': off}


def queue_gate(p, gate, link, device):
    """ONE upload of the call's tables and ONE launch: ``link`` (flat fp32 on ``device``, or None to count only) is
    gated in place; returns the device kept counts [NB].  Nothing waits on the host."""
    packed, sizes = gate.block(p)
    dev = torch_ops._upload(device, packed)[0]
    return torch.ops.mmmot.gate_links(dev, link, sizes, gate.max_size_ratio, gate.weight)


def check_kept(kept, p):
    """host kept counts -> int64 array; raises ``GateError`` naming the first block outside the contract"""
    kept = np.asarray(kept, dtype=np.int64)
    bad = np.nonzero(kept < 0)[0]
    if bad.size:
        raise GateError(int(bad[0]), tuple(int(v) for v in p['blocks'][bad[0], 0:2]))
    return kept


def gate_links(link_blocks, frames, gate, frame_idx=None, poses=None, calib=None, pairs=None):
    """The motion gate over the link blocks of a pair, a window or any list of frame pairs: ``link_blocks[i]`` scores
    the links of ``pairs[i]`` = (a, b), n_a x n_b values in any shape (1 x n_a x n_b as the solvers take them), host or
    device.  Returns (the gated blocks in the shapes, dtype and device given - a gated link is NaN, which ``associate``,
    ``associate_chain`` and ``associate_sequence[_gaps]`` read as an absent edge; a passing fp32 score is unchanged bit
    for bit at ``gate.weight`` 0 - and the int64 kept counts per block).  The inputs are not modified.  One upload, one
    launch, one copy back; raises ``GateError`` for a block outside the contract."""
    if not isinstance(gate, MotionGate):
        raise ValueError('gate_links: gate must be a MotionGate, got %r' % (gate,))
    p = pack_gate(frames, frame_idx, poses, calib, pairs)
    if len(link_blocks) != len(p['sizes']):
        raise ValueError('gate_links: %d link blocks for %d pairs' % (len(link_blocks), len(p['sizes'])))
    for i, (l, (a, b)) in enumerate(zip(link_blocks, p['sizes'])):
        if l.numel() != a * b:
            raise ValueError('gate_links: link block %d must hold %d x %d scores, got %s' % (i, a, b, tuple(l.shape)))
    if not link_blocks:
        return [], np.zeros(0, np.int64)
    on_host = not link_blocks[0].is_cuda
    flat = torch.cat([l.detach().reshape(-1).to(torch.float32) for l in link_blocks] + [link_blocks[0].new_zeros(0, dtype=torch.float32)])
    if on_host:
        flat = flat.to(DEVICE)
    kept = queue_gate(p, gate, flat, flat.device)
    if on_host:
        flat = flat.cpu()
    kept = check_kept(kept.cpu().numpy(), p)
    out, o = [], 0
    for l, (a, b) in zip(link_blocks, p['sizes']):
        out.append(flat[o:o + a * b].view(l.size()).to(l.dtype))
        o += a * b
    return out, kept


def gate_sequence_links(link_scores, frames, gate, frame_idx=None, poses=None, calib=None):
    """``gate_links`` in the nested layout of ``associate_sequence_gaps``: ``link_scores[g - 1][t]`` scores the links
    from frame t to frame t + g.  Returns (the gated blocks nested alike, the kept counts nested alike)."""
    G, T = len(link_scores), len(frames)
    for g, row in enumerate(link_scores, 1):
        if len(row) != T - g:
            raise ValueError('gate_sequence_links: gap %d needs %d link blocks, got %d' % (g, T - g, len(row)))
    out, kept = gate_links([l for row in link_scores for l in row], frames, gate, frame_idx, poses, calib,
                           gap_pairs(T, G))
    nested, counts, o = [], [], 0
    for row in link_scores:
        nested.append(out[o:o + len(row)])
        counts.append(kept[o:o + len(row)])
        o += len(row)
    return nested, counts
