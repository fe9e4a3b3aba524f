"""PyTorch-ROCm custom operators of the HIP path (``torch.ops.mmmot.*``).

``TrackingNet.forward`` reaches libmmmot_hip.so through ONE registered operator per fused group, dispatched on the
CUDA (= HIP on ROCm) key only:

    mmmot::forward_batch(Tensor? crops, Tensor? points, int engine, int plan) -> Tensor[]
        the whole eval-mode frame-pair forward of reference modules/tracking_net.py:165-193 for a batch of
        samples: VGG trunk + SkipPool, PointNet, fusion, w_det, affinity + new/end, softmax.
        Returns [det (nR, Lt), link (flat), new (nR, Lt), end (nR, Lt)].
    mmmot::appearance(Tensor crops, int engine, int plan) -> Tensor      L x 512 image features (appear_net.py:178-190)
    mmmot::pointnet(Tensor points, int engine, int plan) -> Tensor       L x 512 LiDAR features (point_net.py:25-44)

Appearance rows computed once per frame (TrackingNet.encode_appearance) and reused across the pairs of a sequence:
    mmmot::encode_appearance(Tensor crops, int engine, int plan) -> Tensor
        L x 512 image features of one frame's crops under the engine's range guard (plan: a CropPlan).
    mmmot::forward_batch_appearance(Tensor appearance, Tensor? points, int engine, int plan) -> Tensor[]
        forward_batch with every detection's appearance row given [Lt, 512]: no trunk, no SkipPool heads.
    mmmot::forward_pair_appearance(Tensor appearance, Tensor crops, Tensor? points, int engine, int plan) -> Tensor[]
        one frame pair (B = 1) with the first frame's N rows given and the second frame's M crops: the trunk runs on the
        M crops.  Returns forward_batch's four outputs and the second frame's rows [M, 512] (for the next pair).

``engine`` / ``plan`` are handles into this module's registries: the packed weights + workspace arena (an
``Engine``) and the integer tile / segment tables of one batch shape (a ``BatchPlan``) are host objects that hold
device memory; they are not tensors and do not belong in an operator signature.  There is no CPU kernel: CPU tensors
raise ``NotImplementedError`` from the dispatcher (no fallback).  Every operator has a Meta kernel (output shapes
from the plan), so the path can be traced with FakeTensors / ``torch.compile`` graphs can carry it as an opaque node.
The launches go to torch's current HIP stream; nothing synchronises.

Contract the schema cannot express (the handles hide mutable state):
  * every returned tensor is freshly allocated and no two outputs share storage (the engine's new / end scores live in
    one buffer: ``end`` is copied out) - what the functional custom-op contract and the Meta kernels promise;
  * the engine's workspace arena is scratch shared by all calls on that engine.  ``Engine.forward`` refuses a second
    thread while a forward is being issued and orders a forward behind the previous one when the stream changed, so
    eager use from any stream is safe; what is NOT supported is two calls on the SAME engine issued concurrently or
    re-ordered as if independent (a compiler that treats the op as pure may do the latter only for calls whose
    results are unused) - use one TrackingNet per concurrent stream.
"""
import itertools
import weakref

import numpy as np
import torch

_LIB = torch.library.Library('mmmot', 'DEF')
_ENGINES = weakref.WeakValueDictionary()
_PLANS = weakref.WeakValueDictionary()
_ids = itertools.count(1)


def handle(obj, registry):
    """Stable integer handle of an Engine / BatchPlan (kept on the object; the registry holds a weak reference)."""
    h = getattr(obj, '_mmmot_handle', None)
    if h is None:
        h = next(_ids)
        obj._mmmot_handle = h
    registry[h] = obj
    return h


def engine_handle(engine):
    return handle(engine, _ENGINES)


def plan_handle(plan):
    return handle(plan, _PLANS)


def _lookup(engine, plan):
    try:
        return _ENGINES[engine], _PLANS[plan]
    except KeyError:
        raise RuntimeError('mmmot: stale engine / plan handle (the owning TrackingNet or BatchPlan was released)')


_OPS = []


def _ops():
    """the launchers of the operators below, made at the first call (importing this module loads no library)"""
    if not _OPS:
        from .ops import HipOps
        _OPS.append(HipOps())
    return _OPS[0]


def _upload(device, *parts):
    """Host tables (tensors or arrays, each flattened to int32) -> one device slice per part.  ONE pinned block and ONE
    asynchronous copy (a pageable one would wait for the stream); nothing synchronises.  The first slice starts the
    block."""
    flat = [torch.as_tensor(p).reshape(-1) for p in parts]
    ends = list(itertools.accumulate(int(t.numel()) for t in flat))
    host = torch.empty(ends[-1], dtype=torch.int32, pin_memory=True)
    for t, a, b in zip(flat, [0] + ends, ends):
        host[a:b] = t
    dev = host.to(device, non_blocking=True)
    return [dev[a:b] for a, b in zip([0] + ends, ends)]


FP64_SECTIONS = frozenset(('boxes', 'box3d', 'sigma', 'frame_d', 'seq_d', 'thr',  # of the packed evaluator blocks
                           'xf', 'wtab',                                           # of the gap-filling block
                           'r2', 'inv_r2',                                         # of the motion-gate block
                           'xf0',                                                  # of the smoothing block
                           'objective'))                                           # of the stitching block


def _sections_layout(op, parts):
    """({name: (offset, int32 count)}, total ints) of the sections (name, count) laid out one after the other"""
    out, o = {}, 0
    for name, n in parts:
        out[name] = (o, n)
        o += n
    if o >= 2 ** 31:
        raise ValueError('mmmot::%s: block exceeds 32-bit offsets' % op)
    return out, o


def sections(block, lay):
    """{name: its slice} of an int32 block (a tensor or a numpy array) under a layout; fp64 sections as float64"""
    f64 = torch.float64 if isinstance(block, torch.Tensor) else np.float64
    return {name: block[o:o + n].view(f64) if name in FP64_SECTIONS else block[o:o + n] for name, (o, n) in lay.items()}


def _forward_batch(crops, points, engine, plan):
    eng, pl = _lookup(engine, plan)
    out = eng.forward(pl, crops, points)
    return [out['det'], out['link'], out['new'], out['end'].clone()]  # new / end share one buffer in the engine


def _forward_batch_meta(crops, points, engine, plan):
    _, pl = _lookup(engine, plan)
    ref = crops if crops is not None else points
    n_link = pl.pair_tiles.R
    mk = lambda *s: ref.new_empty(s, dtype=torch.float32)
    return [mk(pl.nR, pl.Lt), mk(n_link), mk(pl.nR, pl.Lt), mk(pl.nR, pl.Lt)]


def _appearance(crops, engine, plan):
    eng, pl = _lookup(engine, plan)
    eng.dev = crops.device
    cat = eng.buf('cat', pl.Lt, 1024)
    eng.appearance(pl, crops, cat)
    return cat[:, :512].clone()


def _pointnet(points, engine, plan):
    eng, pl = _lookup(engine, plan)
    eng.dev = points.device
    cat = eng.buf('cat', pl.Lt, 1024)
    eng.pointnet(pl, points, cat)
    return cat[:, 512:].clone()


def _encode_appearance(crops, engine, plan):
    eng, pl = _lookup(engine, plan)
    return eng.encode(pl, crops)[0]


def _forward_batch_appearance(appearance, points, engine, plan):
    eng, pl = _lookup(engine, plan)
    out = eng.forward(pl, None, points, appearance=appearance)
    return [out['det'], out['link'], out['new'], out['end'].clone()]


def _forward_batch_appearance_meta(appearance, points, engine, plan):
    return _forward_batch_meta(appearance, points, engine, plan)


def _forward_pair_appearance(appearance, crops, points, engine, plan):
    eng, pl = _lookup(engine, plan)
    out = eng.forward(pl, crops, points, appearance=appearance)
    n = int(appearance.shape[0])
    return [out['det'], out['link'], out['new'], out['end'].clone(), out['cat'][n:, 0:512].clone()]


def _forward_pair_appearance_meta(appearance, crops, points, engine, plan):
    _, pl = _lookup(engine, plan)
    rows = appearance.new_empty((pl.Lt - int(appearance.shape[0]), 512), dtype=torch.float32)
    return _forward_batch_meta(appearance, points, engine, plan) + [rows]


def _feat_meta(x, engine, plan):
    _, pl = _lookup(engine, plan)
    return x.new_empty((pl.Lt, 512), dtype=torch.float32)


_LIB.define('forward_batch(Tensor? crops, Tensor? points, int engine, int plan) -> Tensor[]')
_LIB.impl('forward_batch', _forward_batch, 'CUDA')
_LIB.impl('forward_batch', _forward_batch_meta, 'Meta')
_LIB.define('appearance(Tensor crops, int engine, int plan) -> Tensor')
_LIB.impl('appearance', _appearance, 'CUDA')
_LIB.impl('appearance', _feat_meta, 'Meta')
_LIB.define('pointnet(Tensor points, int engine, int plan) -> Tensor')
_LIB.impl('pointnet', _pointnet, 'CUDA')
_LIB.impl('pointnet', _feat_meta, 'Meta')
_LIB.define('encode_appearance(Tensor crops, int engine, int plan) -> Tensor')
_LIB.impl('encode_appearance', _encode_appearance, 'CUDA')
_LIB.impl('encode_appearance', _feat_meta, 'Meta')
_LIB.define('forward_batch_appearance(Tensor appearance, Tensor? points, int engine, int plan) -> Tensor[]')
_LIB.impl('forward_batch_appearance', _forward_batch_appearance, 'CUDA')
_LIB.impl('forward_batch_appearance', _forward_batch_appearance_meta, 'Meta')
_LIB.define('forward_pair_appearance(Tensor appearance, Tensor crops, Tensor? points, int engine, int plan) -> Tensor[]')
_LIB.impl('forward_pair_appearance', _forward_pair_appearance, 'CUDA')
_LIB.impl('forward_pair_appearance', _forward_pair_appearance_meta, 'Meta')


# ---- frame-pair association (mmmot_amd/association.py; csrc/assign.hip) --------------------------------------------
#   mmmot::associate(Tensor det, Tensor new, Tensor end, Tensor link, Tensor pairs) -> Tensor[]
#       B frame pairs solved exactly in one launch (mmmot_associate_pairs).  det / new / end / link: flat fp32 device
#       tensors; pairs: a CPU int32 [B, 4] table (N, M, score offset, link offset) - host data, so that the output sizes
#       are known without a device read (and the Meta kernel can give them).  Returns [out, objective]: out fp32, pair
#       p's [det L | new L | end L | link N*M] at offset sum over q < p of 3 (N_q + M_q) + N_q M_q; objective fp64 [B].
MAX_ASSOC = 512


def associate_layout(pairs, n_scores=None, n_link=None):
    """(total output floats, int64 [B] output offsets, max(N, M)) of a pair table; checks the table against the sizes of
    the score / link buffers when given (the kernel reads what the table says)."""
    if pairs.device.type != 'cpu' or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 4:
        raise ValueError('mmmot::associate: pairs must be a CPU int32 [B, 4] table (N, M, score offset, link offset)')
    if pairs.shape[0] < 1:
        raise ValueError('mmmot::associate: no pairs')
    t = pairs.numpy().astype(np.int64)  # host arithmetic in numpy: a few microseconds, not one torch op per line
    N, M, so, lo = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    if np.minimum(N, M).min() < 1 or np.maximum(N, M).max() > MAX_ASSOC:
        raise ValueError('mmmot::associate: every pair needs 1 <= N, M <= %d' % MAX_ASSOC)
    if np.minimum(so, lo).min() < 0:
        raise ValueError('mmmot::associate: negative offset in the pair table')
    if n_scores is not None and (so + N + M).max() > n_scores:
        raise ValueError('mmmot::associate: a pair reads past the end of the score buffers')
    if n_link is not None and (lo + N * M).max() > n_link:
        raise ValueError('mmmot::associate: a pair reads past the end of the link buffer')
    sizes = 3 * (N + M) + N * M
    off = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    if total >= 2 ** 31:
        raise ValueError('mmmot::associate: output block exceeds 32-bit offsets')
    return total, torch.from_numpy(off), int(np.maximum(N, M).max())


def _associate(det, new, end, link, pairs):
    n_scores = min(int(det.numel()), int(new.numel()), int(end.numel()))
    total, off, max_nm = associate_layout(pairs, n_scores, int(link.numel()))
    B = int(pairs.shape[0])
    table, off = _upload(det.device, pairs, off)
    out = torch.empty(total, dtype=torch.float32, device=det.device)
    obj = torch.empty(B, dtype=torch.float64, device=det.device)
    _ops().associate_pairs(det, new, end, link, table, B, max_nm, out, off, obj)
    return [out, obj]


def _associate_meta(det, new, end, link, pairs):
    total, _, _ = associate_layout(pairs)
    return [det.new_empty((total,), dtype=torch.float32), det.new_empty((int(pairs.shape[0]),), dtype=torch.float64)]


_LIB.define('associate(Tensor det, Tensor new, Tensor end, Tensor link, Tensor pairs) -> Tensor[]')
_LIB.impl('associate', _associate, 'CUDA')
_LIB.impl('associate', _associate_meta, 'Meta')


# ---- chain association (mmmot_amd/association.py; csrc/assign_chain.hip) --------------------------------------------
#   mmmot::associate_chains(Tensor det, Tensor new, Tensor end, Tensor link, Tensor chains) -> Tensor[]
#       B chains of 2 .. 8 frames solved exactly in one launch (mmmot_associate_chains).  det / new / end / link: flat
#       fp32 device tensors; chains: a CPU int32 [B, 11] table (T, score offset, link offset, n_0 .. n_7) - host data,
#       like the pair table of mmmot::associate.  Returns [out, objective]: out fp32, chain c's [det L | new L | end L |
#       link_0 | .. | link_{T-2}] one after the other; objective fp64 [B].
CHAIN_MAX_T = 8
CHAIN_ROW = 3 + CHAIN_MAX_T
CHAIN_MAX_L = 1024


def chain_layout(chains, n_scores=None, n_link=None, op='associate_chains'):
    """(total output floats, int64 [B] output offsets, max n_t, max L) of a chain table; checks the table, and against
    the sizes of the score / link buffers when given (the kernel reads what the table says).  ``op``: the operator the
    table is for (mmmot::associate_chains and mmmot::generate_gt share it), named in the refusals."""
    if chains.device.type != 'cpu' or chains.dtype != torch.int32 or chains.dim() != 2 or chains.shape[1] != CHAIN_ROW:
        raise ValueError('mmmot::%s: chains must be a CPU int32 [B, %d] table (T, score offset, link offset, '
                         'n_0 .. n_7)' % (op, CHAIN_ROW))
    if chains.shape[0] < 1:
        raise ValueError('mmmot::%s: no chains' % op)
    t = chains.numpy().astype(np.int64)
    T, so, lo = t[:, 0], t[:, 1], t[:, 2]
    if T.min() < 2 or T.max() > CHAIN_MAX_T:
        raise ValueError('mmmot::%s: every chain needs 2 <= T <= %d frames' % (op, CHAIN_MAX_T))
    n = np.where(np.arange(CHAIN_MAX_T)[None, :] < T[:, None], t[:, 3:], 0)  # entries past n_{T-1} are ignored
    if n.min() < 0 or n.max() > MAX_ASSOC:
        raise ValueError('mmmot::%s: every frame needs 0 <= n_t <= %d' % (op, MAX_ASSOC))
    L = n.sum(1)
    if L.min() < 1 or L.max() > CHAIN_MAX_L:
        raise ValueError('mmmot::%s: every chain needs 1 <= L <= %d detections' % (op, CHAIN_MAX_L))
    if np.minimum(so, lo).min() < 0:
        raise ValueError('mmmot::%s: negative offset in the chain table' % op)
    K = (n[:, :-1] * n[:, 1:]).sum(1)
    if n_scores is not None and (so + L).max() > n_scores:
        raise ValueError('mmmot::%s: a chain reads past the end of the score buffers' % op)
    if n_link is not None and (lo + K).max() > n_link:
        raise ValueError('mmmot::%s: a chain reads past the end of the link buffer' % op)
    sizes = 3 * L + K
    off = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    if total >= 2 ** 31:
        raise ValueError('mmmot::%s: output block exceeds 32-bit offsets' % op)
    return total, torch.from_numpy(off), int(n.max()), int(L.max())


def _associate_chains(det, new, end, link, chains):
    n_scores = min(int(det.numel()), int(new.numel()), int(end.numel()))
    total, off, max_n, max_L = chain_layout(chains, n_scores, int(link.numel()))
    B = int(chains.shape[0])
    if link.numel() == 0:  # no chain has a link (an empty frame between the others): never read, but not a null pointer
        link = det
    table, off = _upload(det.device, chains, off)
    out = torch.empty(total, dtype=torch.float32, device=det.device)
    obj = torch.empty(B, dtype=torch.float64, device=det.device)
    _ops().associate_chains(det, new, end, link, table, B, max_n, max_L, out, off, obj)
    return [out, obj]


def _associate_chains_meta(det, new, end, link, chains):
    total, _, _, _ = chain_layout(chains)
    return [det.new_empty((total,), dtype=torch.float32), det.new_empty((int(chains.shape[0]),), dtype=torch.float64)]


_LIB.define('associate_chains(Tensor det, Tensor new, Tensor end, Tensor link, Tensor chains) -> Tensor[]')
_LIB.impl('associate_chains', _associate_chains, 'CUDA')
_LIB.impl('associate_chains', _associate_chains_meta, 'Meta')


# ---- whole-sequence association (mmmot_amd/association.py; csrc/assign_sequence.hip) --------------------------------
#   mmmot::associate_sequences(Tensor det, Tensor new, Tensor end, Tensor link, Tensor seqs, Tensor nts) -> Tensor[]
#       B sequences of 2 .. 4096 frames solved exactly in one launch (mmmot_associate_sequences).  det / new / end /
#       link: flat fp32 device tensors; seqs: a CPU int32 [B, 4] table (T, score offset, link offset, offset of n_0 in
#       nts); nts: a CPU int32 flat array of the n_t - host data, like the chain table.  Returns [out, ids, objective,
#       info]: out fp32, sequence s's [det L | new L | end L | link_0 | .. | link_{T-2}] one after the other; ids int32
#       with the layout of det (-1: not kept, else the trajectory's number); objective fp64 [B]; info int32 [B, 4]
#       (status, trajectories, augmentations, passes).  The search state lives in a workspace allocated here.
SEQ_MAX_T = 4096
SEQ_MAX_L = 65536
SEQ_ROW = 6
SEQ_STATE_BYTES = 53


def _sequence_layout(op, seqs, nts, max_gap, n_scores, n_link):
    """``sequence_layout`` (max_gap = 0: links to the next frame only, no offset table in the workspace) and
    ``sequence_gap_layout`` (link blocks of every gap 1 .. max_gap)"""
    if seqs.device.type != 'cpu' or seqs.dtype != torch.int32 or seqs.dim() != 2 or seqs.shape[1] != 4:
        raise ValueError('%s: seqs must be a CPU int32 [B, 4] table (T, score offset, link '
                         'offset, offset of n_0 in nts)' % op)
    if nts.device.type != 'cpu' or nts.dtype != torch.int32 or nts.dim() != 1:
        raise ValueError('%s: nts must be a CPU int32 flat array of the n_t' % op)
    if seqs.shape[0] < 1:
        raise ValueError('%s: no sequences' % op)
    G = max(int(max_gap), 1)
    t = seqs.numpy().astype(np.int64)
    n = nts.numpy().astype(np.int64)
    T, so, lo, no = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    if T.min() < 2 or T.max() > SEQ_MAX_T:
        raise ValueError('%s: every sequence needs 2 <= T <= %d frames' % (op, SEQ_MAX_T))
    if T.min() <= G:
        raise ValueError('%s: every sequence needs more than max_gap = %d frames' % (op, G))
    if min(so.min(), lo.min(), no.min()) < 0:
        raise ValueError('%s: negative offset in the sequence table' % op)
    if (no + T).max() > n.size:
        raise ValueError('%s: a sequence reads past the end of nts' % op)
    if n.size and (n.min() < 0 or n.max() > MAX_ASSOC):
        raise ValueError('%s: every frame needs 0 <= n_t <= %d' % (op, MAX_ASSOC))
    L = np.empty(len(T), np.int64)
    K = np.empty(len(T), np.int64)
    max_n = 0
    for s in range(len(T)):
        ns = n[no[s]:no[s] + T[s]]
        L[s], max_n = ns.sum(), max(max_n, int(ns.max()))
        K[s] = sum(int((ns[:-g] * ns[g:]).sum()) for g in range(1, G + 1))
    if L.min() < 1 or L.max() > SEQ_MAX_L:
        raise ValueError('%s: every sequence needs 1 <= L <= %d detections' % (op, SEQ_MAX_L))
    if n_scores is not None and (so + L).max() > n_scores:
        raise ValueError('%s: a sequence reads past the end of the score buffers' % op)
    if n_link is not None and (lo + K).max() > n_link:
        raise ValueError('%s: a sequence reads past the end of the link buffer' % op)
    sizes = 3 * L + K
    total = int(sizes.sum())
    if total >= 2 ** 31 - 1 or int((lo + K).max()) >= 2 ** 31 - 1:
        raise ValueError('%s: link scores or output block exceed 32-bit offsets' % op)
    units = (SEQ_STATE_BYTES * L + 7) // 8
    if max_gap:  # the G x T table of block offsets in front of the state
        units = units + (G * T + 1) // 2
    return (total, torch.from_numpy(np.cumsum(sizes) - sizes), torch.from_numpy(np.cumsum(units) - units),
            int(units.sum()), max_n, int(L.max()), int(T.max()))


def sequence_layout(seqs, nts, n_scores=None, n_link=None):
    """(total output floats, int64 [B] output offsets, int64 [B] workspace offsets in 8-byte units, workspace units,
    max n_t, max L, max T) of a sequence table; checks the table, and against the sizes of the score / link buffers when given
    (the kernel reads what the table says)."""
    return _sequence_layout('mmmot::associate_sequences', seqs, nts, 0, n_scores, n_link)


def _launch_sequences(det, new, end, link, seqs, nts, max_gap):
    """the launch of mmmot::associate_sequences (max_gap = 0) and mmmot::associate_sequences_gap"""
    n_scores = min(int(det.numel()), int(new.numel()), int(end.numel()))
    if max_gap:
        lay = sequence_gap_layout(seqs, nts, max_gap, n_scores, int(link.numel()))
    else:
        lay = sequence_layout(seqs, nts, n_scores, int(link.numel()))
    total, off, woff, units, max_n, max_L, max_T = lay
    B = int(seqs.shape[0])
    if link.numel() == 0:  # no sequence has a link: never read, but not a null pointer
        link = det
    # rows of SEQ_ROW ints: the sequence's table row, its output offset, its workspace offset
    table, nts = _upload(det.device, np.column_stack([seqs.numpy(), off.numpy(), woff.numpy()]), nts)
    out = torch.empty(total, dtype=torch.float32, device=det.device)
    ids = torch.empty(n_scores, dtype=torch.int32, device=det.device)
    obj = torch.empty(B, dtype=torch.float64, device=det.device)
    info = torch.empty((B, 4), dtype=torch.int32, device=det.device)
    ws = torch.empty(units, dtype=torch.float64, device=det.device)
    args = (det.contiguous(), new.contiguous(), end.contiguous(), link.contiguous(), table, nts, B, max_T, max_n, max_L)
    if max_gap:
        _ops().associate_sequences_gap(*args, int(max_gap), out, ids, obj, info, ws)
    else:
        _ops().associate_sequences(*args, out, ids, obj, info, ws)
    return [out, ids, obj, info]


def _sequences_meta(det, total, B):
    n_scores = int(det.numel())
    return [det.new_empty((total,), dtype=torch.float32), det.new_empty((n_scores,), dtype=torch.int32),
            det.new_empty((B,), dtype=torch.float64), det.new_empty((B, 4), dtype=torch.int32)]


def _associate_sequences(det, new, end, link, seqs, nts):
    return _launch_sequences(det, new, end, link, seqs, nts, 0)


def _associate_sequences_meta(det, new, end, link, seqs, nts):
    n = min((det, new, end), key=lambda t: int(t.numel()))
    return _sequences_meta(n, sequence_layout(seqs, nts)[0], int(seqs.shape[0]))


_LIB.define('associate_sequences(Tensor det, Tensor new, Tensor end, Tensor link, Tensor seqs, Tensor nts) -> Tensor[]')
_LIB.impl('associate_sequences', _associate_sequences, 'CUDA')
_LIB.impl('associate_sequences', _associate_sequences_meta, 'Meta')


# ---- whole-sequence association with skip links (mmmot_amd/association.py; csrc/assign_sequence.hip, GAPS) ----------
#   mmmot::associate_sequences_gap(Tensor det, Tensor new, Tensor end, Tensor link, Tensor seqs, Tensor nts,
#                                  int max_gap) -> Tensor[]
#       mmmot::associate_sequences with link blocks for every gap g = 1 .. max_gap <= 8 (mmmot_associate_sequences_gap):
#       a trajectory may miss up to max_gap - 1 frames.  link, and the link part of every output block: the blocks gap
#       by gap - all g = 1 blocks in frame order, then all g = 2 blocks, ..  Every sequence needs T > max_gap.  The same
#       tables and the same four results; the workspace also holds each sequence's max_gap x T table of block offsets.
SEQ_MAX_GAP = 8


def sequence_gap_layout(seqs, nts, max_gap, n_scores=None, n_link=None):
    """``sequence_layout`` for link blocks of every gap 1 .. ``max_gap``: the same tuple, the workspace of a sequence
    being its offset table ((max_gap T + 1) // 2 units) followed by its search state."""
    if not 1 <= int(max_gap) <= SEQ_MAX_GAP:
        raise ValueError('mmmot::associate_sequences_gap: max_gap must be in 1 .. %d, got %d' % (SEQ_MAX_GAP, max_gap))
    return _sequence_layout('mmmot::associate_sequences_gap', seqs, nts, int(max_gap), n_scores, n_link)


def _associate_sequences_gap(det, new, end, link, seqs, nts, max_gap):
    return _launch_sequences(det, new, end, link, seqs, nts, int(max_gap))


def _associate_sequences_gap_meta(det, new, end, link, seqs, nts, max_gap):
    n = min((det, new, end), key=lambda t: int(t.numel()))
    return _sequences_meta(n, sequence_gap_layout(seqs, nts, max_gap)[0], int(seqs.shape[0]))


_LIB.define('associate_sequences_gap(Tensor det, Tensor new, Tensor end, Tensor link, Tensor seqs, Tensor nts, '
            'int max_gap) -> Tensor[]')
_LIB.impl('associate_sequences_gap', _associate_sequences_gap, 'CUDA')
_LIB.impl('associate_sequences_gap', _associate_sequences_gap_meta, 'Meta')


# ---- track IDs (mmmot_amd/tracks.py; csrc/track_ids.hip) -------------------------------------------------------------
#   mmmot::track_ids(Tensor blocks, Tensor pairs, Tensor frame_idx, Tensor(a!) state, int max_nm) -> Tensor
#       Track IDs of B consecutive pairs of ONE sequence (mmmot_track_ids) from the solver's output blocks: blocks = the
#       `out` of mmmot::associate for the same pairs table (a CPU int32 [B, 4]; N or M may be 0 here); frame_idx: CPU
#       int32 [B, 2]; state: the sequence's device int32 [TRACK_STATE_INTS] block, updated in place; max_nm: 0 = from
#       the table, else >= every N and M (above 128 the four-wave kernel runs).  Returns int32
#       [sum (N + M + 2)]: per pair [ids frame 0 | ids frame 1 | frame_start | last_id].
#   mmmot::track_chain_ids(Tensor blocks, Tensor chains, Tensor frame_idx, Tensor(a!) state, int max_n) -> Tensor
#       The same for B consecutive WINDOWS of 2 .. 8 frames (mmmot_track_chain_ids): blocks = the `out` of
#       mmmot::associate_chains for the same chains table (a CPU int32 [B, 11]; any n_t may be 0 here); frame_idx: CPU
#       int32 [B, 8], the first T of a row are read; max_n: 0 = from the table, else >= every n_t.  Returns int32
#       [sum (L + 3)]: per window [ids of its L detections | frame_start | last_id | stored].
#   Both layouts reduce their table to per entry the counts and frame indices ([B, T] with zeros behind an entry's
#   frames); _track_sizes and _track_launch are the rest, once.
TRACK_STATE_HEAD = 4
TRACK_STATE_INTS = TRACK_STATE_HEAD + 512


def _track_sizes(op, what, n, frames, tail, n_blocks):
    """(total ids_out ints, int64 [B] block offsets, max count) from int64 [B, T] counts and frame indices"""
    if frames.min() < 0:
        raise ValueError('mmmot::%s: frame indices must be >= 0' % op)
    if n.min() < 0 or n.max() > MAX_ASSOC:
        raise ValueError('mmmot::%s: every frame of a %s needs 0 <= n_t <= %d' % (op, what, MAX_ASSOC))
    L = n.sum(1)
    sizes = 3 * L + (n[:, :-1] * n[:, 1:]).sum(1)
    off = np.cumsum(sizes) - sizes
    if int(sizes.sum()) >= 2 ** 31:
        raise ValueError('mmmot::%s: the solver blocks exceed 32-bit offsets' % op)
    if n_blocks is not None and int(sizes.sum()) > n_blocks:
        raise ValueError('mmmot::%s: a %s reads past the end of the solver blocks' % (op, what))
    return int((L + tail).sum()), torch.from_numpy(off), int(n.max())


def track_layout(pairs, frame_idx, n_blocks=None):
    """(total ids_out ints, int64 [B] block offsets, max(N, M)) of a pair table for mmmot::track_ids; checks the table."""
    if pairs.device.type != 'cpu' or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 4 or \
            pairs.shape[0] < 1:
        raise ValueError('mmmot::track_ids: pairs must be a CPU int32 [B, 4] table (N, M, score offset, link offset)')
    if frame_idx.device.type != 'cpu' or frame_idx.dtype != torch.int32 or tuple(frame_idx.shape) != (pairs.shape[0], 2):
        raise ValueError('mmmot::track_ids: frame_idx must be a CPU int32 [B, 2] table')
    return _track_sizes('track_ids', 'pair', pairs.numpy()[:, :2].astype(np.int64), frame_idx.numpy(), 2, n_blocks)


def track_chain_layout(chains, frame_idx, n_blocks=None):
    """(total ids_out ints, int64 [B] block offsets, max n_t) of a chain table for mmmot::track_chain_ids; checks it."""
    if chains.device.type != 'cpu' or chains.dtype != torch.int32 or chains.dim() != 2 or \
            chains.shape[1] != CHAIN_ROW or chains.shape[0] < 1:
        raise ValueError('mmmot::track_chain_ids: chains must be a CPU int32 [B, %d] table (T, score offset, link offset, '
                         'n_0 .. n_7)' % CHAIN_ROW)
    if frame_idx.device.type != 'cpu' or frame_idx.dtype != torch.int32 or \
            tuple(frame_idx.shape) != (chains.shape[0], CHAIN_MAX_T):
        raise ValueError('mmmot::track_chain_ids: frame_idx must be a CPU int32 [B, %d] table' % CHAIN_MAX_T)
    t = chains.numpy().astype(np.int64)
    T = t[:, 0]
    if T.min() < 2 or T.max() > CHAIN_MAX_T:
        raise ValueError('mmmot::track_chain_ids: every window needs 2 <= T <= %d frames' % CHAIN_MAX_T)
    used = np.arange(CHAIN_MAX_T)[None, :] < T[:, None]  # entries past frame T-1 are ignored
    return _track_sizes('track_chain_ids', 'window', np.where(used, t[:, 3:], 0), np.where(used, frame_idx.numpy(), 0), 3,
                        n_blocks)


def _track_launch(op, layout, blocks, table, frame_idx, state, max_n):
    """the op behind both schemas: the layout's checks, the tensors', one pinned block [table | block offsets |
    frame_idx] in one asynchronous copy, and the launch"""
    total, off, need = layout(table, frame_idx, int(blocks.numel()))
    if blocks.dtype != torch.float32 or not blocks.is_contiguous():
        raise ValueError('mmmot::%s: blocks must be a contiguous fp32 device tensor' % op)
    if state.dtype != torch.int32 or state.numel() != TRACK_STATE_INTS or not state.is_contiguous() or \
            state.device != blocks.device:
        raise ValueError('mmmot::%s: state must be a contiguous int32 [%d] block on the blocks\' device'
                         % (op, TRACK_STATE_INTS))
    if max_n and (max_n < need or max_n > MAX_ASSOC):
        raise ValueError('mmmot::%s: max_n %d does not cover the table (%d)' % (op, max_n, need))
    tab, off, fidx = _upload(blocks.device, table, off, frame_idx)
    ids = torch.empty(total, dtype=torch.int32, device=blocks.device)
    if blocks.numel() == 0:  # entries without a detection: never read, but not a null pointer
        blocks = tab.view(torch.float32)
    getattr(_ops(), op)(blocks, tab, off, fidx, int(table.shape[0]), max_n or need, state, ids)
    return ids


def _track_ids(blocks, pairs, frame_idx, state, max_nm):
    return _track_launch('track_ids', track_layout, blocks, pairs, frame_idx, state, max_nm)


def _track_ids_meta(blocks, pairs, frame_idx, state, max_nm):
    total, _, _ = track_layout(pairs, frame_idx)
    return blocks.new_empty((total,), dtype=torch.int32)


def _track_chain_ids(blocks, chains, frame_idx, state, max_n):
    return _track_launch('track_chain_ids', track_chain_layout, blocks, chains, frame_idx, state, max_n)


def _track_chain_ids_meta(blocks, chains, frame_idx, state, max_n):
    total, _, _ = track_chain_layout(chains, frame_idx)
    return blocks.new_empty((total,), dtype=torch.int32)


_LIB.define('track_ids(Tensor blocks, Tensor pairs, Tensor frame_idx, Tensor(a!) state, int max_nm) -> Tensor')
_LIB.impl('track_ids', _track_ids, 'CUDA')
_LIB.impl('track_ids', _track_ids_meta, 'Meta')
_LIB.define('track_chain_ids(Tensor blocks, Tensor chains, Tensor frame_idx, Tensor(a!) state, int max_n) -> Tensor')
_LIB.impl('track_chain_ids', _track_chain_ids, 'CUDA')
_LIB.impl('track_chain_ids', _track_chain_ids_meta, 'Meta')


#   mmmot::track_ids_multi(Tensor blocks, Tensor pairs, Tensor frame_idx, Tensor seq_start, Tensor(a!) states,
#                          int max_nm) -> Tensor
#   mmmot::track_chain_ids_multi(Tensor blocks, Tensor chains, Tensor frame_idx, Tensor seq_start, Tensor(a!) states,
#                                int max_n) -> Tensor
#       The ID step of S sequences in ONE launch (mmmot_track_ids_multi / mmmot_track_chain_ids_multi): states = the
#       device int32 [S, TRACK_STATE_INTS] table; seq_start = CPU int32 [S + 1], entries [seq_start[s], seq_start[s+1])
#       of the table are the consecutive pairs (windows) of sequence s.  seq_start is NOT checked here - a range that is
#       decreasing or leaves [0, B] is answered by the kernel with ECONTRACT in that sequence's state.  The words of
#       such a sequence in the returned buffer (and only those) are unwritten memory.  Same layout as the single forms.
def _seq_start_checked(op, seq_start, states):
    if states.dtype != torch.int32 or states.dim() != 2 or states.shape[1] != TRACK_STATE_INTS or states.shape[0] < 1 \
            or not states.is_contiguous():
        raise ValueError('mmmot::%s: states must be a contiguous int32 [S, %d] table' % (op, TRACK_STATE_INTS))
    if seq_start.device.type != 'cpu' or seq_start.dtype != torch.int32 or \
            tuple(seq_start.shape) != (states.shape[0] + 1,):
        raise ValueError('mmmot::%s: seq_start must be a CPU int32 [S + 1] table' % op)


def _track_launch_multi(op, layout, blocks, table, frame_idx, seq_start, states, max_n, chains):
    """``_track_launch`` with the state table and seq_start behind the same pinned block"""
    total, off, need = layout(table, frame_idx, int(blocks.numel()))
    _seq_start_checked(op, seq_start, states)
    if blocks.dtype != torch.float32 or not blocks.is_contiguous() or states.device != blocks.device:
        raise ValueError('mmmot::%s: blocks must be a contiguous fp32 tensor on the states\' device' % op)
    if max_n and (max_n < need or max_n > MAX_ASSOC):
        raise ValueError('mmmot::%s: max_n %d does not cover the table (%d)' % (op, max_n, need))
    B, S = int(table.shape[0]), int(states.shape[0])
    tab, off, fidx, start = _upload(blocks.device, table, off, frame_idx, seq_start)
    ids = torch.empty(total, dtype=torch.int32, device=blocks.device)
    if blocks.numel() == 0:  # entries without a detection: never read, but not a null pointer
        blocks = tab.view(torch.float32)
    _ops().track_ids_multi(blocks, tab, off, fidx, start, S, B, max_n or need, states, ids, chains=chains)
    return ids


def _track_ids_multi(blocks, pairs, frame_idx, seq_start, states, max_nm):
    return _track_launch_multi('track_ids_multi', track_layout, blocks, pairs, frame_idx, seq_start, states, max_nm, False)


def _track_ids_multi_meta(blocks, pairs, frame_idx, seq_start, states, max_nm):
    total, _, _ = track_layout(pairs, frame_idx)
    return blocks.new_empty((total,), dtype=torch.int32)


def _track_chain_ids_multi(blocks, chains, frame_idx, seq_start, states, max_n):
    return _track_launch_multi('track_chain_ids_multi', track_chain_layout, blocks, chains, frame_idx, seq_start, states,
                               max_n, True)


def _track_chain_ids_multi_meta(blocks, chains, frame_idx, seq_start, states, max_n):
    total, _, _ = track_chain_layout(chains, frame_idx)
    return blocks.new_empty((total,), dtype=torch.int32)


_LIB.define('track_ids_multi(Tensor blocks, Tensor pairs, Tensor frame_idx, Tensor seq_start, Tensor(a!) states, '
            'int max_nm) -> Tensor')
_LIB.impl('track_ids_multi', _track_ids_multi, 'CUDA')
_LIB.impl('track_ids_multi', _track_ids_multi_meta, 'Meta')
_LIB.define('track_chain_ids_multi(Tensor blocks, Tensor chains, Tensor frame_idx, Tensor seq_start, Tensor(a!) states, '
            'int max_n) -> Tensor')
_LIB.impl('track_chain_ids_multi', _track_chain_ids_multi, 'CUDA')
_LIB.impl('track_chain_ids_multi', _track_chain_ids_multi_meta, 'Meta')


# ---- CLEAR-MOT evaluation (mmmot_amd/evaluate.py; csrc/clear_mot.hip) ----------------------------------------------
#   mmmot::clear_mot(Tensor packed, int[] sizes, float[] params) -> Tensor
#       Evaluates S sequences (mmmot_clear_mot: frame, trajectory, sequence and total launches).  packed: ONE device
#       int32 block holding the call's tables in the order of clear_mot_layout()[0] (the fp64 boxes first, as their bit
#       patterns), so that a call is one upload; sizes = [nG, nT, nD, NF, NTr, S]; params = [min_overlap, min_height,
#       max_truncation, max_occlusion].  Returns ONE int32 block in the order of clear_mot_layout()[1] (the fp64 sums
#       first), so that a call is one read-back.  The frame limits (128 boxes a side, 64 DontCare areas) are the
#       caller's to check on the host (evaluate.pack); the kernel marks a frame outside them instead of reading it.
CLEAR_MOT_SEQ_INTS = 12
CLEAR_MOT_MAX_BOXES, CLEAR_MOT_MAX_DONTCARE = 128, 64


def clear_mot_layout(sizes):
    """({input section: (offset, int32 count)}, {output section: (offset, int32 count)}, input ints, output ints) of a
    call with sizes = [nG, nT, nD, NF, NTr, S]; fp64 sections come first in both blocks (8-byte aligned)."""
    if len(sizes) != 6 or min(sizes) < 0 or sizes[5] < 1:
        raise ValueError('mmmot::clear_mot: sizes must be [nG, nT, nD, NF, NTr, S] with S >= 1, got %s' % (list(sizes),))
    nG, nT, nD, NF, NTr, S = (int(v) for v in sizes)
    lay = lambda parts: _sections_layout('clear_mot', parts)

    inp, n_in = lay([('boxes', 8 * (nG + nT + nD)), ('frames', 6 * NF), ('g_attr', 3 * nG), ('t_attr', 2 * nT),
                     ('traj_off', NTr + 1), ('traj_obj', nG), ('seq_off', 2 * (S + 1))])
    out, n_out = lay([('frame_d', 4 * NF), ('seq_d', 4 * (S + 1)), ('frame_i', 6 * NF), ('gt_out', 2 * nG),
                      ('traj_i', 4 * NTr), ('seq_i', CLEAR_MOT_SEQ_INTS * (S + 1))])
    return inp, out, n_in, n_out


def _clear_mot(packed, sizes, params):
    inp, outl, n_in, n_out = clear_mot_layout(sizes)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::clear_mot: packed must be a contiguous int32 [%d] block for sizes %s' % (n_in, list(sizes)))
    if len(params) != 4:
        raise ValueError('mmmot::clear_mot: params = [min_overlap, min_height, max_truncation, max_occlusion]')
    nG, nT, nD, NF, NTr, S = (int(v) for v in sizes)
    res = torch.empty(n_out, dtype=torch.int32, device=packed.device)
    i, o = sections(packed, inp), sections(res, outl)
    _ops().clear_mot(i['boxes'], nG, nT, nD, i['frames'], NF, i['g_attr'], i['t_attr'], i['traj_off'], i['traj_obj'], NTr,
                     i['seq_off'], S, params, o['frame_d'], o['frame_i'], o['gt_out'], o['traj_i'], o['seq_d'], o['seq_i'])
    return res


def _clear_mot_meta(packed, sizes, params):
    return packed.new_empty((clear_mot_layout(sizes)[3],), dtype=torch.int32)


_LIB.define('clear_mot(Tensor packed, int[] sizes, float[] params) -> Tensor')
_LIB.impl('clear_mot', _clear_mot, 'CUDA')
_LIB.impl('clear_mot', _clear_mot_meta, 'Meta')


# ---- HOTA / IDF1 evaluation (mmmot_amd/evaluate.py; csrc/hota.hip) -------------------------------------------------
#   mmmot::hota(Tensor packed, int[] sizes, float[] params) -> Tensor
#       Evaluates S sequences (mmmot_hota: a fixed number of launches).  packed: ONE device int32 block holding the
#       call's tables in the order of hota_layout()[0] (the fp64 boxes first, as their bit patterns); sizes = [nG, nT,
#       nD, NF, S, cells, sumG, sumT, max_boxes, max_dontcare]; params = [min_height, max_truncation, max_occlusion,
#       prepare (1 = KITTI preparation, 0 = none)].  Returns ONE int32 block in the order of hota_layout()[1] (the fp64
#       sections first).  The work tables (pot, mc, pm, counts, keep flags) are allocated here and never read back.  The
#       frame and table limits are the caller's to check on the host (evaluate.pack_hota): beyond them this raises.
HOTA_ALPHAS = 19
HOTA_FRAME_D, HOTA_FRAME_I, HOTA_SEQ_D, HOTA_SEQ_I, HOTA_SEQ_TAB = 21, 21, 76, 24, 6
HOTA_MAX_CELLS, HOTA_MAX_IDS = 1 << 18, 2048  # per sequence: G * T, and G or T


def hota_layout(sizes):
    """({input section: (offset, int32 count)}, {output section: (offset, int32 count)}, input ints, output ints, work
    ints) of a call with sizes = [nG, nT, nD, NF, S, cells, sumG, sumT, max_boxes, max_dontcare]; fp64 sections come
    first in every block (8-byte aligned).  Raises ValueError beyond the limits of mmmot_hota."""
    if len(sizes) != 10 or min(sizes) < 0 or sizes[4] < 1:
        raise ValueError('mmmot::hota: sizes must be [nG, nT, nD, NF, S, cells, sumG, sumT, max_boxes, max_dontcare] '
                         'with S >= 1, got %s' % (list(sizes),))
    nG, nT, nD, NF, S, cells, sumG, sumT, max_boxes, max_dontcare = (int(v) for v in sizes)
    if max_boxes > CLEAR_MOT_MAX_BOXES or max_dontcare > CLEAR_MOT_MAX_DONTCARE:
        raise ValueError('mmmot::hota: a frame holds more than %d boxes on a side or more than %d DontCare areas'
                         % (CLEAR_MOT_MAX_BOXES, CLEAR_MOT_MAX_DONTCARE))
    if cells > S * HOTA_MAX_CELLS or max(sumG, sumT) > S * HOTA_MAX_IDS:
        raise ValueError('mmmot::hota: the ID tables exceed %d cells or %d IDs per sequence' % (HOTA_MAX_CELLS, HOTA_MAX_IDS))
    lay = lambda parts: _sections_layout('hota', parts)

    inp, n_in = lay([('boxes', 8 * (nG + nT + nD)), ('frames', 6 * NF), ('frame_seq', NF), ('g_attr', 4 * nG),
                     ('t_id', nT), ('seq_tab', HOTA_SEQ_TAB * (S + 1))])
    out, n_out = lay([('frame_d', 2 * HOTA_FRAME_D * NF), ('seq_d', 2 * HOTA_SEQ_D * (S + 1)),
                      ('frame_i', HOTA_FRAME_I * NF), ('seq_i', HOTA_SEQ_I * (S + 1))])
    _, n_work = lay([('work', max(2, 2 * cells + (HOTA_ALPHAS + 1) * cells + sumG + sumT + nG + nT))])
    return inp, out, n_in, n_out, n_work


def _hota(packed, sizes, params):
    inp, outl, n_in, n_out, n_work = hota_layout(sizes)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::hota: packed must be a contiguous int32 [%d] block for sizes %s' % (n_in, list(sizes)))
    if len(params) != 4 or params[3] not in (0., 1.):
        raise ValueError('mmmot::hota: params = [min_height, max_truncation, max_occlusion, prepare (0 or 1)]')
    nG, nT, nD, NF, S, cells, sumG, sumT, max_boxes, max_dontcare = (int(v) for v in sizes)
    res = torch.empty(n_out, dtype=torch.int32, device=packed.device)
    work = torch.empty(n_work, dtype=torch.int32, device=packed.device)
    i, o = sections(packed, inp), sections(res, outl)
    _ops().hota(i['boxes'], nG, nT, nD, i['frames'], NF, i['frame_seq'], i['g_attr'], i['t_id'], i['seq_tab'], S, cells,
                sumG, sumT, max_boxes, max_dontcare, params[:3], int(params[3]), work, o['frame_d'], o['frame_i'],
                o['seq_d'], o['seq_i'])
    return res


def _hota_meta(packed, sizes, params):
    return packed.new_empty((hota_layout(sizes)[3],), dtype=torch.int32)


_LIB.define('hota(Tensor packed, int[] sizes, float[] params) -> Tensor')
_LIB.impl('hota', _hota, 'CUDA')
_LIB.impl('hota', _hota_meta, 'Meta')


# ---- 3D MOT evaluation (mmmot_amd/evaluate.py; csrc/mot3d.hip) ------------------------------------------------------
#   mmmot::mot3d(Tensor packed, int[] sizes, float[] params) -> Tensor
#       Evaluates S sequences at levels + 1 operating points (mmmot_mot3d: the overlap table and pass A, a sort of the
#       matched track scores, the thresholds and the sweep - a launch count that depends on neither NF nor S nor levels).
#       packed: ONE device int32 block in the order of mot3d_layout()[0] (the fp64 sections first, as their bit patterns);
#       sizes = [nG, nT, nD, NF, NTr, S, cells, levels, mode (0 '3d', 1 'bev', 2 '2d')]; params = [gate, min_height,
#       max_truncation, max_occlusion].  Returns ONE int32 block in the order of mot3d_layout()[1]: the sections of
#       mmmot::clear_mot with a leading level axis [levels + 1] (the last level is pass A), thr and reach.  The overlap
#       table and the matched scores are allocated here and never read back.  The frame limits are the caller's to check
#       on the host (evaluate.pack_3d); the kernel marks a frame outside them instead of reading it.
MOT3D_BOX = 12          # doubles per packed 3D box: four footprint corners (x, z), y - h, y, w l, h w l
MOT3D_MAX_LEVELS = 1024
MOT3D_MODES = {'3d': 0, 'bev': 1, '2d': 2}


def mot3d_layout(sizes):
    """({input section: (offset, int32 count)}, {output section: (offset, int32 count)}, input ints, output ints) of a
    call with sizes = [nG, nT, nD, NF, NTr, S, cells, levels, mode]; fp64 sections come first in both blocks (8-byte
    aligned).  Raises ValueError beyond the limits of mmmot_mot3d."""
    if len(sizes) != 9 or min(sizes) < 0 or sizes[5] < 1 or sizes[7] > MOT3D_MAX_LEVELS or sizes[8] > 2:
        raise ValueError('mmmot::mot3d: sizes must be [nG, nT, nD, NF, NTr, S, cells, levels, mode] with S >= 1, levels '
                         '<= %d and mode in 0..2, got %s' % (MOT3D_MAX_LEVELS, list(sizes)))
    nG, nT, nD, NF, NTr, S, cells, levels, mode = (int(v) for v in sizes)
    if cells >= 2 ** 31:
        raise ValueError('mmmot::mot3d: the overlap table exceeds 32-bit offsets')
    Lv = levels + 1
    lay = lambda parts: _sections_layout('mot3d', parts)

    inp, n_in = lay([('boxes', 8 * (nG + nT + nD)), ('box3d', 2 * MOT3D_BOX * (nG + nT)), ('sigma', 2 * nT),
                     ('frames', 6 * NF), ('cell_off', NF), ('g_attr', 3 * nG), ('t_attr', 2 * nT),
                     ('traj_off', NTr + 1), ('traj_obj', nG), ('seq_off', 2 * (S + 1))])
    out, n_out = lay([('frame_d', 4 * NF * Lv), ('seq_d', 4 * (S + 1) * Lv), ('thr', 2 * levels),
                      ('frame_i', 6 * NF * Lv), ('gt_out', 2 * nG * Lv), ('traj_i', 4 * NTr * Lv),
                      ('seq_i', CLEAR_MOT_SEQ_INTS * (S + 1) * Lv), ('reach', levels)])
    return inp, out, n_in, n_out


def mot3d_run(packed, sizes, params):
    """mmmot::mot3d's launches -> (the result block, the overlap table fp64 [cells]); the table is what
    evaluate.overlap_tables shows, the operator returns the block alone"""
    inp, outl, n_in, n_out = mot3d_layout(sizes)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::mot3d: packed must be a contiguous int32 [%d] block for sizes %s' % (n_in, list(sizes)))
    if len(params) != 4:
        raise ValueError('mmmot::mot3d: params = [gate, min_height, max_truncation, max_occlusion]')
    nG, nT, nD, NF, NTr, S, cells, levels, mode = (int(v) for v in sizes)
    res = torch.empty(n_out, dtype=torch.int32, device=packed.device)
    table = torch.empty(cells, dtype=torch.float64, device=packed.device)
    msig = torch.full((nG,), float('-inf'), dtype=torch.float64, device=packed.device)
    i, o = sections(packed, inp), sections(res, outl)

    def phase(k, m):
        _ops().mot3d(i['boxes'], i['box3d'], i['sigma'], nG, nT, nD, i['frames'], i['cell_off'], NF, i['g_attr'],
                     i['t_attr'], i['traj_off'], i['traj_obj'], NTr, i['seq_off'], S, mode, levels, k, params, table,
                     cells, m, o['frame_d'], o['frame_i'], o['gt_out'], o['traj_i'], o['seq_d'], o['seq_i'], o['thr'],
                     o['reach'])

    phase(0, msig)
    if levels:
        phase(1, torch.sort(msig, descending=True).values)
    return res, table


def _mot3d(packed, sizes, params):
    return mot3d_run(packed, sizes, params)[0]


def _mot3d_meta(packed, sizes, params):
    return packed.new_empty((mot3d_layout(sizes)[3],), dtype=torch.int32)


_LIB.define('mot3d(Tensor packed, int[] sizes, float[] params) -> Tensor')
_LIB.impl('mot3d', _mot3d, 'CUDA')
_LIB.impl('mot3d', _mot3d_meta, 'Meta')


# ---- training labels (mmmot_amd/labels.py; csrc/labels.hip) ---------------------------------------------------------
#   mmmot::generate_gt(Tensor ids, Tensor cls, Tensor chains) -> Tensor
#       The targets of B chains in one launch (mmmot_generate_gt).  ids / cls: flat int32 device tensors, chain c's L
#       values at its score offset; chains: the CPU int32 [B, 11] table of mmmot::associate_chains (the link offset is not
#       read).  Returns out fp32: chain c's [gt_det L | gt_new L | gt_end L | link_0 | .. | link_{T-2}] one after the
#       other, at the offsets of chain_layout - the block of association.unpack_chain.
def _generate_gt(ids, cls, chains):
    if ids.dtype != torch.int32 or cls.dtype != torch.int32 or ids.dim() != 1 or cls.dim() != 1:
        raise ValueError('mmmot::generate_gt: ids and cls must be flat int32 tensors')
    total, off, max_n, max_L = chain_layout(chains, min(int(ids.numel()), int(cls.numel())), op='generate_gt')
    B = int(chains.shape[0])
    table, off = _upload(ids.device, chains, off)
    out = torch.empty(total, dtype=torch.float32, device=ids.device)
    _ops().generate_gt(ids.contiguous(), cls.contiguous(), table, B, max_n, max_L, out, off)
    return out


def _generate_gt_meta(ids, cls, chains):
    return ids.new_empty((chain_layout(chains, op='generate_gt')[0],), dtype=torch.float32)


_LIB.define('generate_gt(Tensor ids, Tensor cls, Tensor chains) -> Tensor')
_LIB.impl('generate_gt', _generate_gt, 'CUDA')
_LIB.impl('generate_gt', _generate_gt_meta, 'Meta')


#   mmmot::match_dets(Tensor det_xywh, Tensor gt_xywh, Tensor gt_id, Tensor gt_name, Tensor frames, int car, int dontcare,
#                     float max_iou) -> Tensor
#       generate_det_id_matrix for NF frames in one launch (mmmot_match_dets).  det_xywh / gt_xywh: fp64 device [.][4]
#       boxes (x, y, w, h); gt_id / gt_name: int32 device, one per gt box; frames: a CPU int32 [NF, 4] table (det offset,
#       n_det, gt offset, n_gt).  Returns int32 [2, number of det boxes]: row 0 the ids, row 1 the classes (a detection
#       that no frame of the table covers keeps -1 / 0).
def match_layout(frames, n_det=None, n_gt=None):
    """max(n_det, n_gt, 1) of a frame table; checks the table, and against the box counts when given (the kernel reads
    and writes what the table says)."""
    if frames.device.type != 'cpu' or frames.dtype != torch.int32 or frames.dim() != 2 or frames.shape[1] != 4:
        raise ValueError('mmmot::match_dets: frames must be a CPU int32 [NF, 4] table (det offset, n_det, gt offset, n_gt)')
    if frames.shape[0] < 1:
        raise ValueError('mmmot::match_dets: no frames')
    t = frames.numpy().astype(np.int64)
    do, nd, go, ng = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    if t.min() < 0:
        raise ValueError('mmmot::match_dets: negative entry in the frame table')
    if max(nd.max(), ng.max()) > MAX_ASSOC:
        raise ValueError('mmmot::match_dets: every frame needs n_det, n_gt <= %d' % MAX_ASSOC)
    if n_det is not None and (do + nd).max() > n_det:
        raise ValueError('mmmot::match_dets: a frame reaches past the end of the detection boxes')
    if n_gt is not None and (go + ng).max() > n_gt:
        raise ValueError('mmmot::match_dets: a frame reads past the end of the ground-truth boxes')
    order = np.argsort(do, kind='stable')  # two frames must not write the same detections
    if ((do + nd)[order][:-1] > do[order][1:]).any():
        raise ValueError('mmmot::match_dets: the detection ranges of two frames overlap')
    return int(max(nd.max(), ng.max(), 1))


def _match_dets(det_xywh, gt_xywh, gt_id, gt_name, frames, car, dontcare, max_iou):
    f64 = lambda t: t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 4
    if not f64(det_xywh) or not f64(gt_xywh):
        raise ValueError('mmmot::match_dets: boxes must be fp64 [n, 4] tensors')
    if gt_id.dtype != torch.int32 or gt_name.dtype != torch.int32:
        raise ValueError('mmmot::match_dets: gt_id and gt_name must be int32 tensors')
    n_det = int(det_xywh.shape[0])
    n_gt = min(int(gt_xywh.shape[0]), int(gt_id.numel()), int(gt_name.numel()))
    max_n = match_layout(frames, n_det, n_gt)
    res = torch.empty((2, n_det), dtype=torch.int32, device=det_xywh.device)
    res[0].fill_(-1)
    res[1].zero_()
    if n_det == 0:
        return res
    NF = int(frames.shape[0])
    table, = _upload(det_xywh.device, frames)
    if n_gt == 0:  # never read (every n_gt is 0), but not a null pointer
        gt_xywh, gt_id, gt_name = det_xywh, res[0], res[0]
    _ops().match_dets(det_xywh.contiguous(), gt_xywh.contiguous(), gt_id.contiguous(), gt_name.contiguous(), table, NF,
                      car, dontcare, max_iou, max_n, res[0], res[1])
    return res


def _match_dets_meta(det_xywh, gt_xywh, gt_id, gt_name, frames, car, dontcare, max_iou):
    match_layout(frames)
    return det_xywh.new_empty((2, int(det_xywh.shape[0])), dtype=torch.int32)


_LIB.define('match_dets(Tensor det_xywh, Tensor gt_xywh, Tensor gt_id, Tensor gt_name, Tensor frames, int car, '
            'int dontcare, float max_iou) -> Tensor')
_LIB.impl('match_dets', _match_dets, 'CUDA')
_LIB.impl('match_dets', _match_dets_meta, 'Meta')


# ---- gap filling of tracked sequences (mmmot_amd/tracks.py; csrc/fill_tracks.hip) -----------------------------------
#   mmmot::fill_tracks(Tensor packed, int[] sizes) -> Tensor
#       One interpolated box per listed frame a track skipped, for S sequences (mmmot_fill_tracks: five launches).
#       packed: ONE device int32 block holding the call's tables in the order of fill_layout()[0] (the fp64 records and
#       weights first, as their bit patterns; the fp32 detections as theirs), so that a call is one upload; sizes = [L, F,
#       S, max_fill, capacity, moving (1: the block holds ego-motion records, 0: a standing camera)].  Returns ONE int32
#       block in the order of fill_layout()[1] (the fp32 rows as their bit patterns), so that a call is one read-back.
#       The scratch of the entry is allocated here and never read back.
FILL_MAX = 30   # MMMOT_FILL_MAX
FILL_REC = 33   # MMMOT_FILL_REC: doubles per ego-motion record (C 16, inv C 16, dyaw)
FILL_WT = FILL_MAX + 2
FILL_EDUP, FILL_ECAPACITY, FILL_ECONTRACT = 1, 2, 4


def fill_layout(sizes):
    """({input section: (offset, int32 count)}, {output section: (offset, int32 count)}, input ints, output ints) of a
    call with sizes = [L, F, S, max_fill, capacity, moving]; the fp64 sections come first (8-byte aligned)."""
    if len(sizes) != 6 or min(sizes) < 0 or sizes[2] < 1 or sizes[5] > 1:
        raise ValueError('mmmot::fill_tracks: sizes must be [L, F, S, max_fill, capacity, moving] with S >= 1, got %s'
                         % (list(sizes),))
    L, F, S, max_fill, capacity, moving = (int(v) for v in sizes)
    if not 1 <= max_fill <= FILL_MAX:
        raise ValueError('mmmot::fill_tracks: max_fill must be in 1 .. %d, got %d' % (FILL_MAX, max_fill))
    lay = lambda parts: _sections_layout('fill_tracks', parts)
    inp, n_in = lay([('xf', 2 * FILL_REC * F * (max_fill + 1) * moving), ('wtab', 2 * FILL_WT * FILL_WT),
                     ('det', 12 * L), ('ids', L), ('frame_start', F + 1), ('frame_no', F), ('seq_start', S + 1)])
    out, n_out = lay([('out', 12 * capacity), ('out_id', capacity), ('out_src', 2 * capacity), ('fill_start', F + 1),
                      ('info', 4 * S)])
    return inp, out, n_in, n_out


def _fill_tracks(packed, sizes):
    inp, outl, n_in, n_out = fill_layout(sizes)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::fill_tracks: packed must be a contiguous int32 [%d] block for sizes %s'
                         % (n_in, list(sizes)))
    L, F, S, max_fill, capacity, moving = (int(v) for v in sizes)
    res = torch.zeros(n_out, dtype=torch.int32, device=packed.device)  # L = 0 or F = 0: nothing is launched
    work = torch.empty(3 * L + 1, dtype=torch.int32, device=packed.device)
    i, o = sections(packed, inp), sections(res, outl)
    st = _ops().fill_tracks(i['det'].view(torch.float32), i['ids'], i['frame_start'], i['frame_no'], i['seq_start'],
                            i['xf'] if moving else None, i['wtab'], L, F, S, max_fill, capacity, work, o['fill_start'],
                            o['out'].view(torch.float32), o['out_id'], o['out_src'], o['info'])
    from . import _lib
    _lib.check(st, 'mmmot_fill_tracks')
    return res


def _fill_tracks_meta(packed, sizes):
    return packed.new_empty((fill_layout(sizes)[3],), dtype=torch.int32)


_LIB.define('fill_tracks(Tensor packed, int[] sizes) -> Tensor')
_LIB.impl('fill_tracks', _fill_tracks, 'CUDA')
_LIB.impl('fill_tracks', _fill_tracks_meta, 'Meta')


# ---- smoothing of tracked sequences (mmmot_amd/tracks.py; csrc/smooth_tracks.hip) -----------------------------------
#   mmmot::smooth_tracks(Tensor packed, int[] sizes) -> Tensor
#       A Kalman filter forwards and an RTS pass backwards along every track of S sequences (mmmot_smooth_tracks: five
#       launches).  packed: ONE device int32 block holding the call's tables in the order of smooth_layout()[0] (the fp64
#       records first, as their bit patterns); sizes = [L, F, S, moving (1: the block holds the per-frame ego-motion
#       records xf0), masked (1: the block holds `observed`), yaw_flip] followed by the 8 fp64 parameters q_loc, r_loc,
#       v0_loc, q_yaw, r_yaw, v0_yaw, q_dim, r_dim as their int64 bit patterns (smooth_param_bits): they are host
#       arguments of the entry, which refuses bad ones before any launch.  Returns ONE int32 block in the order of
#       smooth_layout()[1]: out [L, 12] and vel [L, 4] (fp32 as bit patterns), info [S, 4].
SMOOTH_PARAMS = 8


def smooth_param_bits(params):
    """the 8 fp64 parameters as int64 bit patterns, for the tail of ``sizes``"""
    return [int(v) for v in np.asarray(list(params), np.float64).view(np.int64)]


def smooth_layout(sizes):
    """({input section: (offset, int32 count)}, {output section: (offset, int32 count)}, input ints, output ints) of a
    call with sizes = [L, F, S, moving, masked, yaw_flip, ...]; the fp64 section comes first (8-byte aligned)."""
    head = [int(v) for v in sizes[:6]]
    if len(sizes) not in (6, 6 + SMOOTH_PARAMS) or min(head) < 0 or head[2] < 1 or max(head[3:]) > 1:
        raise ValueError('mmmot::smooth_tracks: sizes must be [L, F, S, moving, masked, yaw_flip] (+ %d parameter bit '
                         'patterns) with S >= 1 and flags 0 / 1, got %s' % (SMOOTH_PARAMS, list(sizes),))
    L, F, S, moving, masked, _ = head
    lay = lambda parts: _sections_layout('smooth_tracks', parts)
    inp, n_in = lay([('xf0', 2 * FILL_REC * F * moving), ('det', 12 * L), ('ids', L), ('observed', L * masked),
                     ('frame_start', F + 1), ('frame_no', F), ('seq_start', S + 1)])
    out, n_out = lay([('out', 12 * L), ('vel', 4 * L), ('info', 4 * S)])
    return inp, out, n_in, n_out


def _smooth_tracks(packed, sizes):
    inp, outl, n_in, n_out = smooth_layout(sizes)
    if len(sizes) != 6 + SMOOTH_PARAMS:
        raise ValueError('mmmot::smooth_tracks: sizes must end in the %d parameter bit patterns' % SMOOTH_PARAMS)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::smooth_tracks: packed must be a contiguous int32 [%d] block for sizes %s'
                         % (n_in, list(sizes[:6])))
    L, F, S, moving, masked, yaw_flip = (int(v) for v in sizes[:6])
    params = [float(v) for v in np.asarray([int(v) for v in sizes[6:]], np.int64).view(np.float64)]
    res = torch.zeros(n_out, dtype=torch.int32, device=packed.device)  # L = 0 or F = 0: nothing is launched
    work = torch.empty((75 * L + 2 + 1) // 2, dtype=torch.int64, device=packed.device).view(torch.int32)  # 8-byte aligned
    i, o = sections(packed, inp), sections(res, outl)
    st = _ops().smooth_tracks(i['det'].view(torch.float32), i['ids'], i['frame_start'], i['frame_no'], i['seq_start'],
                              i['observed'] if masked else None, i['xf0'] if moving else None, L, F, S, params, yaw_flip,
                              work, o['out'].view(torch.float32), o['vel'].view(torch.float32), o['info'])
    from . import _lib
    _lib.check(st, 'mmmot_smooth_tracks')
    return res


def _smooth_tracks_meta(packed, sizes):
    return packed.new_empty((smooth_layout(sizes)[3],), dtype=torch.int32)


_LIB.define('smooth_tracks(Tensor packed, int[] sizes) -> Tensor')
_LIB.impl('smooth_tracks', _smooth_tracks, 'CUDA')
_LIB.impl('smooth_tracks', _smooth_tracks_meta, 'Meta')


# ---- tracklet stitching of tracked sequences (mmmot_amd/tracks.py; csrc/stitch_tracks.hip) --------------------------
#   mmmot::stitch_tracks(Tensor packed, int[] sizes) -> Tensor
#       Tails of tracks joined to the heads of later ones, one to one, for S sequences (mmmot_stitch_tracks: seven
#       launches and the pair solver's).  packed: ONE device int32 block holding the call's tables in the order of
#       stitch_layout()[0] (the fp64 records and radius tables first, as their bit patterns); sizes = [L, F, S, n_tracks,
#       n_link, max_k, moving (1: the block holds xf0), has_vel (1: the block holds vel), min_dt, max_dt, min_rows, mode]
#       followed by max_size_ratio and gap_penalty as their int64 bit patterns (stitch_param_bits): host arguments of
#       the entry, which refuses bad ones before any launch.  Returns ONE int32 block in the order of stitch_layout()[1]:
#       objective [S] (fp64), out_ids [L], next [L], links [n_link] (fp32 as bit patterns), info [S, 4].
STITCH_MAXK, STITCH_MAX_DT, STITCH_ETOOMANY = 512, 256, 8  # MMMOT_STITCH_MAXK, MMMOT_STITCH_MAX_DT, MMMOT_STITCH_ETOOMANY
STITCH_SIZES, STITCH_PARAMS = 12, 2
STITCH_MODES = {'ground': 0, '3d': 1}


def stitch_param_bits(max_size_ratio, gap_penalty):
    """the 2 fp64 parameters as int64 bit patterns, for the tail of ``sizes``"""
    return [int(v) for v in np.asarray([max_size_ratio, gap_penalty], np.float64).view(np.int64)]


def stitch_work(L, F, S, T, n_link):
    """MMMOT_STITCH_WORK: the ints of scratch of a call"""
    return 4 * L + F + 5 * S + 39 * T + n_link + 2


def stitch_layout(sizes):
    """({input section: (offset, int32 count)}, {output section: (offset, int32 count)}, input ints, output ints) of a
    call with sizes = [L, F, S, n_tracks, n_link, max_k, moving, has_vel, min_dt, max_dt, min_rows, mode, ...]; the
    fp64 sections come first (8-byte aligned)."""
    head = [int(v) for v in sizes[:STITCH_SIZES]]
    if len(sizes) not in (STITCH_SIZES, STITCH_SIZES + STITCH_PARAMS) or min(head) < 0 or head[2] < 1 or \
            max(head[6:8]) > 1:
        raise ValueError('mmmot::stitch_tracks: sizes must be [L, F, S, n_tracks, n_link, max_k, moving, has_vel, min_dt, '
                         'max_dt, min_rows, mode] (+ %d parameter bit patterns) with S >= 1 and flags 0 / 1, got %s'
                         % (STITCH_PARAMS, list(sizes),))
    L, F, S, T, n_link, _, moving, has_vel, min_dt, max_dt, _, mode = head
    if not 1 <= min_dt <= max_dt <= STITCH_MAX_DT:
        raise ValueError('mmmot::stitch_tracks: 1 <= min_dt <= max_dt <= %d, got %d, %d' % (STITCH_MAX_DT, min_dt, max_dt))
    if mode not in (0, 1):
        raise ValueError('mmmot::stitch_tracks: mode must be 0 (ground plane) or 1 (3d), got %d' % mode)
    lay = lambda parts: _sections_layout('stitch_tracks', parts)
    inp, n_in = lay([('xf0', 2 * FILL_REC * F * moving), ('r2', 4 * (max_dt + 1)), ('inv_r2', 4 * (max_dt + 1)),
                     ('det', 12 * L), ('vel', 4 * L * has_vel), ('ids', L), ('frame_start', F + 1), ('frame_no', F),
                     ('seq_start', S + 1), ('k_start', S + 1), ('pairs', 4 * S)])
    out, n_out = lay([('objective', 2 * S), ('out_ids', L), ('next', L), ('links', n_link), ('info', 4 * S)])
    return inp, out, n_in, n_out


def _stitch_tracks(packed, sizes):
    inp, outl, n_in, n_out = stitch_layout(sizes)
    if len(sizes) != STITCH_SIZES + STITCH_PARAMS:
        raise ValueError('mmmot::stitch_tracks: sizes must end in the %d parameter bit patterns' % STITCH_PARAMS)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::stitch_tracks: packed must be a contiguous int32 [%d] block for sizes %s'
                         % (n_in, list(sizes[:STITCH_SIZES])))
    L, F, S, T, n_link, max_k, moving, has_vel, min_dt, max_dt, min_rows, mode = (int(v) for v in sizes[:STITCH_SIZES])
    ratio, penalty = (float(v) for v in np.asarray([int(v) for v in sizes[STITCH_SIZES:]], np.int64).view(np.float64))
    res = torch.zeros(n_out, dtype=torch.int32, device=packed.device)
    work = torch.empty((stitch_work(L, F, S, T, n_link) + 1) // 2, dtype=torch.int64,
                       device=packed.device).view(torch.int32)  # 8-byte aligned
    i, o = sections(packed, inp), sections(res, outl)
    if L == 0 or F == 0:  # nothing is launched: no tracks, no links, objectives of sequences without tracks
        o['objective'].fill_(float('nan'))
    st = _ops().stitch_tracks(i['det'].view(torch.float32), i['ids'], i['frame_start'], i['frame_no'], i['seq_start'],
                              i['vel'].view(torch.float32) if has_vel else None, i['xf0'] if moving else None,
                              i['k_start'], i['pairs'], i['r2'], i['inv_r2'], L, F, S, T, n_link, max_k, min_dt, max_dt,
                              min_rows, mode, ratio, penalty, work, o['out_ids'], o['next'], o['links'].view(torch.float32),
                              o['objective'], o['info'])
    from . import _lib
    _lib.check(st, 'mmmot_stitch_tracks')
    return res


def _stitch_tracks_meta(packed, sizes):
    return packed.new_empty((stitch_layout(sizes)[3],), dtype=torch.int32)


_LIB.define('stitch_tracks(Tensor packed, int[] sizes) -> Tensor')
_LIB.impl('stitch_tracks', _stitch_tracks, 'CUDA')
_LIB.impl('stitch_tracks', _stitch_tracks_meta, 'Meta')


# ---- motion gate of links (mmmot_amd/association.py; csrc/gate_links.hip) -------------------------------------------
#   mmmot::gate_links(Tensor packed, Tensor(a!)? link, int[] sizes, float max_size_ratio, float weight) -> Tensor
#       Links whose two 3D boxes lie too far apart for the elapsed frames become absent edges (NaN), for NB link blocks
#       in ONE launch (mmmot_gate_links).  packed: ONE device int32 block holding the call's tables in the order of
#       gate_layout() (the fp64 records and radius tables first, as their bit patterns), so that a call is one upload;
#       sizes = [L, F, NB, rec_gaps (0: a standing camera, no records), max_dt, mode, n_link].  link: the flat fp32
#       scores [n_link], gated IN PLACE, or None: count only.  Returns kept int32 [NB] (-1: a block outside the contract).
GATE_MAX_DT = 64  # MMMOT_GATE_MAX_DT
GATE_MODES = {'ground': 0, '3d': 1}


def gate_layout(sizes):
    """({section: (offset, int32 count)}, ints) of the packed block of a call with sizes = [L, F, NB, rec_gaps, max_dt,
    mode, n_link]; the fp64 sections come first (8-byte aligned)."""
    if len(sizes) != 7 or min(sizes) < 0:
        raise ValueError('mmmot::gate_links: sizes must be [L, F, NB, rec_gaps, max_dt, mode, n_link], all >= 0, got %s'
                         % (list(sizes),))
    L, F, NB, rec_gaps, max_dt, mode, n_link = (int(v) for v in sizes)
    if not 1 <= max_dt <= GATE_MAX_DT:
        raise ValueError('mmmot::gate_links: max_dt must be in 1 .. %d, got %d' % (GATE_MAX_DT, max_dt))
    if mode not in (0, 1):
        raise ValueError('mmmot::gate_links: mode must be 0 (ground plane) or 1 (3d), got %d' % mode)
    return _sections_layout('gate_links', [('xf', 2 * FILL_REC * F * rec_gaps), ('r2', 2 * (max_dt + 1)),
                                           ('inv_r2', 2 * (max_dt + 1)), ('det', 12 * L), ('frame_start', F + 1),
                                           ('frame_no', F), ('blocks', 4 * NB)])


def _gate_links(packed, link, sizes, max_size_ratio, weight):
    lay, n_in = gate_layout(sizes)
    if packed.dtype != torch.int32 or packed.dim() != 1 or packed.numel() != n_in or not packed.is_contiguous():
        raise ValueError('mmmot::gate_links: packed must be a contiguous int32 [%d] block for sizes %s'
                         % (n_in, list(sizes)))
    L, F, NB, rec_gaps, max_dt, mode, n_link = (int(v) for v in sizes)
    if link is not None and (link.dtype != torch.float32 or link.dim() != 1 or link.numel() != n_link
                             or not link.is_contiguous()):
        raise ValueError('mmmot::gate_links: link must be a contiguous float32 [%d] tensor' % n_link)
    kept = torch.zeros(NB, dtype=torch.int32, device=packed.device)
    i = sections(packed, lay)
    st = _ops().gate_links(i['det'].view(torch.float32), i['frame_start'], i['frame_no'], i['blocks'],
                           i['xf'] if rec_gaps else None, i['r2'], i['inv_r2'], link, link, kept, L, F, NB, rec_gaps,
                           n_link, mode, max_dt, max_size_ratio, weight)
    from . import _lib
    _lib.check(st, 'mmmot_gate_links')
    return kept


def _gate_links_meta(packed, link, sizes, max_size_ratio, weight):
    gate_layout(sizes)
    return packed.new_empty((int(sizes[2]),), dtype=torch.int32)


_LIB.define('gate_links(Tensor packed, Tensor(a!)? link, int[] sizes, float max_size_ratio, float weight) -> Tensor')
_LIB.impl('gate_links', _gate_links, 'CUDA')
_LIB.impl('gate_links', _gate_links_meta, 'Meta')

# ---- optimizer step (mmmot_amd/optim.py; csrc/adam_step.hip) --------------------------------------------------------
#   mmmot::adam_step(Tensor chunks, Tensor ptrs, Tensor scal, float beta1, float beta2, float eps) -> ()
#       One Adam step of T tensors in one launch (mmmot_adam_step).  chunks: the device int32 [n, 2] chunk table
#       (tensor index, chunk index) of mmmot_adam_chunks - it depends on the sizes only and is uploaded once by its
#       owner; ptrs: a CPU int64 [T, 6] table (p, g, m, v addresses, numel, flags); scal: a CPU float64 [T, 4] table
#       (step_size, bc2_sqrt, decay, l2) - host data of THIS step, packed here into the 64-byte rows of mmmot_adam_row
#       (the doubles are rounded to fp32 once) and uploaded by one pinned asynchronous copy.  Returns nothing: the
#       tensors behind the addresses are updated in place, which the schema cannot say - the caller (optim.Adam) owns
#       them, keeps them alive and advances the version counters of the parameters it had written.
ADAM_ROW = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('numel', '<i8'), ('step_size', '<f4'),
                     ('bc2_sqrt', '<f4'), ('decay', '<f4'), ('l2', '<f4'), ('flags', '<i4'), ('reserved', '<i4')])
ADAM_HAS_GRAD = 1


def adam_tables(chunks, ptrs, scal, beta1, beta2, eps):
    """T of an adam_step call; checks what the host can see of its tables (the kernel follows the addresses)."""
    if chunks.dtype != torch.int32 or chunks.dim() != 2 or chunks.shape[1] != 2 or chunks.shape[0] < 1 or \
            not chunks.is_contiguous():
        raise ValueError('mmmot::adam_step: chunks must be a contiguous int32 [n, 2] table with n >= 1')
    if ptrs.device.type != 'cpu' or ptrs.dtype != torch.int64 or ptrs.dim() != 2 or ptrs.shape[1] != 6 or ptrs.shape[0] < 1:
        raise ValueError('mmmot::adam_step: ptrs must be a CPU int64 [T, 6] table (p, g, m, v, numel, flags), T >= 1')
    T = int(ptrs.shape[0])
    if scal.device.type != 'cpu' or scal.dtype != torch.float64 or tuple(scal.shape) != (T, 4):
        raise ValueError('mmmot::adam_step: scal must be a CPU float64 [%d, 4] table (step_size, bc2_sqrt, decay, l2)' % T)
    t = ptrs.numpy()
    if t[:, 4].min() < 1:
        raise ValueError('mmmot::adam_step: every tensor needs numel >= 1')
    has = (t[:, 5] & ADAM_HAS_GRAD) != 0
    if (t[:, 0] == 0).any() or (t[has, 1:4] == 0).any():
        raise ValueError('mmmot::adam_step: null address in the tensor table')
    if (t[:, 0] & 3).any() or (t[has, 1:4] & 3).any():
        raise ValueError('mmmot::adam_step: an address that is not 4-byte aligned')
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError('mmmot::adam_step: betas must lie in [0, 1), got (%r, %r)' % (beta1, beta2))
    if not eps >= 0.0:
        raise ValueError('mmmot::adam_step: eps must be >= 0, got %r' % (eps,))
    return T


def adam_pack(ptrs, scal, device):
    """The step's rows (mmmot_adam_row) in one pinned block, on their way to ``device`` by an asynchronous copy (a
    pageable one would wait for the stream)."""
    T = int(ptrs.shape[0])
    host = torch.empty(T * ADAM_ROW.itemsize, dtype=torch.uint8, pin_memory=True)
    rows = host.numpy().view(ADAM_ROW)
    t, s = ptrs.numpy(), scal.numpy()
    for j, k in enumerate(('p', 'g', 'm', 'v', 'numel')):
        rows[k] = t[:, j]
    for j, k in enumerate(('step_size', 'bc2_sqrt', 'decay', 'l2')):
        rows[k] = s[:, j]  # rounded to fp32 here, once
    rows['flags'] = t[:, 5]
    rows['reserved'] = 0
    return host.to(device, non_blocking=True)


def _adam_step(chunks, ptrs, scal, beta1, beta2, eps):
    _ops().adam_step(chunks, ptrs, scal, beta1, beta2, eps)  # checks the tables, packs, uploads, launches


def _adam_step_meta(chunks, ptrs, scal, beta1, beta2, eps):
    return None


_LIB.define('adam_step(Tensor chunks, Tensor ptrs, Tensor scal, float beta1, float beta2, float eps) -> ()')
_LIB.impl('adam_step', _adam_step, 'CUDA')
_LIB.impl('adam_step', _adam_step_meta, 'Meta')
