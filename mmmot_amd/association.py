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
``associate_batch`` solves B pairs (e.g. the rows of one ``forward_batch``) in one launch.  Chains of more than two
frames (a min-cost flow) and the ``gt`` loss-augmented objective are not supported.
"""
import numpy as np
import torch

from . import torch_ops  # noqa: F401  (registers mmmot::associate)


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
    rows, so, lo, oo, offs = [], 0, 0, 0, []
    for N, M in splits:
        rows.append((N, M, so, lo))
        offs.append(oo)
        so += N + M
        lo += N * M
        oo += 3 * (N + M) + N * M
    return torch.tensor(rows, dtype=torch.int32), offs


def unpack(block, N, M, like=None, link_size=None):
    """One pair's output block [det L | new L | end L | link N*M] -> the ortools_solve tuple (views of ``block``)."""
    L = N + M
    det, new, end = block[0:L], block[L:2 * L], block[2 * L:3 * L]
    link = block[3 * L:3 * L + N * M].view(1, N, M)
    if like is not None:
        det, new, end = (t.view(like.size()).to(like.dtype) for t in (det, new, end))
        link = link.view(link_size).to(like.dtype)
    return det, [link], new, end


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
    parts = [t.detach().reshape(-1).to(torch.float32) for t in (det_score, new_score, end_score, link)]
    on_host = not det_score.is_cuda
    if on_host:
        flat = torch.cat(parts).to('cuda')  # one host-to-device copy
        parts = [flat[0:L], flat[L:2 * L], flat[2 * L:3 * L], flat[3 * L:]]
    else:
        parts = [p.contiguous() for p in parts]
    pairs, _ = pairs_table([(N, M)])
    out, _ = torch.ops.mmmot.associate(parts[0], parts[1], parts[2], parts[3], pairs)
    if on_host:
        out = out.cpu()  # one device-to-host copy
    return unpack(out, N, M, det_score, link.size())


def associate_batch(det_scores, link_scores, new_scores, end_scores, det_splits, return_objective=False):
    """B frame pairs in one launch.  Per pair p: det_scores[p] / new_scores[p] / end_scores[p] [L_p],
    link_scores[p] = [link 1 x N_p x M_p] (the ``select`` rows of a ``forward_batch`` result), all on one device.
    Returns the list of ortools_solve tuples (on that device), and the fp64 optima [B] when ``return_objective``."""
    splits = [split_of(s) for s in det_splits]
    if not splits:
        raise ValueError('associate_batch: no pairs')
    if any(N == 0 or M == 0 for N, M in splits):
        raise ValueError('associate_batch: every pair needs detections in both frames (use associate for empty frames)')
    cat = lambda ts: torch.cat([t.detach().reshape(-1).to(torch.float32) for t in ts])
    det, new, end = cat(det_scores), cat(new_scores), cat(end_scores)
    link = cat([l[0] for l in link_scores])
    pairs, offs = pairs_table(splits)
    out, obj = torch.ops.mmmot.associate(det, new, end, link, pairs)
    res = []
    for (N, M), o, d, l in zip(splits, offs, det_scores, link_scores):
        res.append(unpack(out[o:o + 3 * (N + M) + N * M], N, M, d, l[0].size()))
    return (res, obj) if return_objective else res
