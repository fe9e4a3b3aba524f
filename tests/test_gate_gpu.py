"""The motion gate on the device (csrc/gate_links.hip through HipOps.gate_links, mmmot::gate_links and
mmmot_amd.association.gate_links / gate_sequence_links) against the NumPy restatement tests/gate_ref.py: BIT FOR BIT on
out_link (the NaN pattern and every value) and on kept, between guard words that must survive, every case twice for bit
equality of two calls.  Then gated scores through the three solvers against the references of their own suites with
the gated links at -1e6, and the scene in which only the gate keeps two similar objects from swapping their IDs."""
import numpy as np
import pytest
import torch

import association_chain_ref as chain_ref
import association_ref as pair_ref
import gate_cases
import gate_ref
import sequence_gap_ref as gap_ref
from mmmot_amd import association as A
from mmmot_amd import torch_ops

pytestmark = pytest.mark.gpu

GUARD = 7
SENTINEL = -77
GUARD_SCORE = 12345.5
EINVAL = -1
ABSENT = -1e6  # a link is never forced, so no optimum of the references uses one at this score: it stands for "absent"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_gate(t, blocks, link, xf=None, r2=None, inv_r2=None, mode=0, max_dt=8, ratio=0.0, weight=0.0, inplace=False,
                count_only=False, nulls=(), n_link=None, NB=None, rec_gaps=None):
    """one call of the entry on fresh buffers, the link and kept buffers between guard words: (status, out_link or
    None, kept, the input buffer after the call), host arrays with the guards checked here"""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt)).reshape(-1)).cuda()
    blocks = np.asarray(blocks, np.int32).reshape(-1, 4)
    n = len(link) if n_link is None else n_link
    NB = len(blocks) if NB is None else NB
    guarded = lambda body: np.concatenate([np.full(GUARD, GUARD_SCORE, np.float32), body, np.full(GUARD, GUARD_SCORE, np.float32)])
    a = dict(det=dev(t['det'], np.float32), frame_start=dev(t['frame_start'], np.int32), frame_no=dev(t['frame_no'], np.int32),
             blocks=dev(blocks, np.int32), xf=None if xf is None else dev(xf, np.float64), r2=dev(r2, np.float64),
             inv_r2=dev(inv_r2, np.float64), kept=torch.full((len(blocks) + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda'))
    buf_in = None if count_only else torch.from_numpy(guarded(np.asarray(link, np.float32))).cuda()
    buf_out = buf_in if inplace or count_only else torch.from_numpy(guarded(np.full(len(link), GUARD_SCORE, np.float32))).cuda()
    a['link'] = None if count_only else buf_in[GUARD:GUARD + len(link)]
    a['out_link'] = None if count_only else buf_out[GUARD:GUARD + len(link)]
    a['kept_body'] = a['kept'][GUARD:GUARD + len(blocks)]
    for k in nulls:
        a['kept_body' if k == 'kept' else k] = None
    st = torch_ops._ops().gate_links(a['det'], a['frame_start'], a['frame_no'], a['blocks'], a['xf'], a['r2'], a['inv_r2'],
                                     a['link'], a['out_link'], a['kept_body'], len(t['det']),
                                     len(t['frame_no']), NB, (0 if xf is None else xf.shape[1]) if rec_gaps is None else rec_gaps,
                                     n, mode, max_dt, ratio, weight)
    torch.cuda.synchronize()
    kept = a['kept'].cpu().numpy()
    assert (kept[:GUARD] == SENTINEL).all() and (kept[GUARD + len(blocks):] == SENTINEL).all()
    out = src = None
    if not count_only:
        out, src = buf_out.cpu().numpy(), buf_in.cpu().numpy()
        for b in (out, src):
            assert (b[:GUARD] == GUARD_SCORE).all() and (b[GUARD + len(link):] == GUARD_SCORE).all()
        out, src = out[GUARD:GUARD + len(link)], src[GUARD:GUARD + len(link)]
    return st, out, kept[GUARD:GUARD + len(blocks)], src


def check(t, blocks, link, xf=None, speed=1.5, slack=2.0, want_mix=True, **kw):
    """the device against the restatement, bit for bit, twice, out of place and in place, and count-only against the
    counts of the full call; returns the restatement's (out, kept)"""
    max_dt = kw.get('max_dt', 8)
    r2, inv = gate_ref.tables(speed, slack, max_dt)
    want, wkept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, xf, r2, inv, link, kw.get('mode', 0),
                                max_dt, kw.get('ratio', 0.0), kw.get('weight', 0.0))
    runs = [device_gate(t, blocks, link, xf, r2, inv, inplace=ip, **kw) for ip in (False, False, True)]
    for st, out, kept, src in runs:
        assert st == 0
        assert np.array_equal(bits(out), bits(want)), (np.isnan(out) != np.isnan(want)).sum()
        assert np.array_equal(kept, wkept)
    for st, out, kept, src in runs[:2]:  # out of place: the input is as it was
        assert np.array_equal(bits(src), bits(link))
    st, _, counted, _ = device_gate(t, blocks, link, xf, r2, inv, count_only=True, **kw)
    _, ckept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, xf, r2, inv, None, kw.get('mode', 0), max_dt,
                             kw.get('ratio', 0.0), n_link=len(link))
    assert st == 0 and np.array_equal(counted, ckept)
    if not np.isnan(link).any():
        assert np.array_equal(counted, wkept)
    if want_mix:  # the case gates some links and passes others
        assert 0 < np.isnan(want).sum() < len(want)
    return want, wkept


def single(seed, na, nb, **kw):
    rng = np.random.default_rng(seed)
    t = gate_cases.tables(rng, [na, nb])
    return check(t, [(0, 1, 0, 0)], gate_cases.random_links(rng, na * nb), **kw)


@pytest.mark.parametrize('na,nb', [(1, 1), (70, 3), (3, 600), (600, 1), (5, 1030)])
def test_one_block(na, nb):
    # 1 x 1; rows that span more than a wave; across the 512-wide tile, two and three tiles; one column
    want, kept = single(na * 1000 + nb, na, nb, speed=100.0 if na == nb == 1 else 1.5, want_mix=(na, nb) != (1, 1))
    assert kept[0] == (~np.isnan(want)).sum()
    if (na, nb) == (1, 1):  # the one link once passed, once gated
        assert kept[0] == 1 and single(1001, 1, 1, speed=0.01, slack=0.01, want_mix=False)[1][0] == 0


def records_of(kind, n_frames, pairs, rec_gaps, seed=0):
    if kind == 'none':
        return None
    if kind == 'identity':
        return gate_cases.identity_records(n_frames, rec_gaps)
    return gate_cases.records(gate_cases.drive(n_frames, seed), pairs, n_frames, rec_gaps)


def sequence(seed, T, G, holes=True):
    rng = np.random.default_rng(seed)
    counts = [int(n) for n in rng.integers(1, 8, T)]
    t = gate_cases.tables(rng, counts, gate_cases.holey_numbers(rng, T) if holes else None)
    blocks, n = gate_cases.gap_blocks(counts, G)
    return t, counts, blocks, gate_cases.random_links(rng, n)


@pytest.mark.parametrize('kind', ['none', 'identity', 'drive'])
@pytest.mark.parametrize('G,T', [(1, 2), (1, 12), (3, 4), (3, 12), (8, 9), (8, 12)])
def test_sequences_against_the_restatement(G, T, kind):
    t, counts, blocks, link = sequence(100 * G + T, T, G)
    xf = records_of(kind, T, [(b[0], b[1]) for b in blocks], G, seed=G)
    want, kept = check(t, blocks, link, xf, want_mix=T > 2)
    if G == 8:  # frame numbers up to 3 apart per step: some blocks lie beyond max_dt and are gated whole
        dt = np.asarray([t['frame_no'][b[1]] - t['frame_no'][b[0]] for b in blocks])
        assert (dt > 8).any() and (kept[dt > 8] == 0).all() and (kept[dt <= 8] > 0).any()


def test_identity_records_equal_no_records_and_a_drive_does_not():
    t, counts, blocks, link = sequence(7, 12, 3)
    pairs = [(b[0], b[1]) for b in blocks]
    res = {k: check(t, blocks, link, records_of(k, 12, pairs, 3, seed=2), mode=1, weight=0.5) for k in ('none', 'identity', 'drive')}
    assert np.array_equal(bits(res['none'][0]), bits(res['identity'][0])) and np.array_equal(res['none'][1], res['identity'][1])
    assert not np.array_equal(bits(res['none'][0]), bits(res['drive'][0]))


@pytest.mark.parametrize('weight', [0.0, 0.5])
@pytest.mark.parametrize('ratio', [0.0, 1.5])
@pytest.mark.parametrize('mode', [0, 1])
def test_modes_size_ratio_and_weight(mode, ratio, weight):
    t, counts, blocks, link = sequence(11, 12, 3)
    link[::7] = np.float32('nan')          # NaN inputs stay, uncounted
    link[1::7] = np.float32('-inf')
    link[2::7] = np.float32(-0.0)
    xf = records_of('drive', 12, [(b[0], b[1]) for b in blocks], 3, seed=5)
    want, kept = check(t, blocks, link, xf, mode=mode, ratio=ratio, weight=weight)
    base, bkept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, xf, *gate_ref.tables(1.5, 2.0, 8), link)
    if mode or ratio:  # the stricter rule gates more
        assert kept.sum() < bkept.sum()
    if not weight:  # what passes is the input, bit for bit
        assert np.array_equal(bits(want[~np.isnan(want)]), bits(link[~np.isnan(want)]))


def test_three_sequences_in_one_launch_equal_three_calls():
    rng = np.random.default_rng(21)
    G = 3
    seqs = [[int(n) for n in rng.integers(1, 8, T)] for T in (5, 9, 4)]
    counts = [n for s in seqs for n in s]
    t = gate_cases.tables(rng, counts, np.concatenate([gate_cases.holey_numbers(rng, len(s)) for s in seqs]))
    blocks, off, first, spans = [], 0, 0, []
    for s in seqs:
        rows, end = gate_cases.gap_blocks(s, G, first, off)
        spans.append((first, len(s), len(blocks), len(rows), off, end))
        blocks, off, first = blocks + rows, end, first + len(s)
    link = gate_cases.random_links(rng, off)
    poses = [p for k, s in enumerate(seqs) for p in gate_cases.drive(len(s), k)]
    xf = gate_cases.records(poses, [(b[0], b[1]) for b in blocks], len(counts), G)
    want, kept = check(t, blocks, link, xf, weight=0.25)
    for f0, nf, b0, nb, l0, l1 in spans:  # the sequence alone: its own frames, records, blocks and links
        d0, d1 = t['frame_start'][f0], t['frame_start'][f0 + nf]
        alone = dict(det=t['det'][d0:d1], frame_start=t['frame_start'][f0:f0 + nf + 1] - d0, frame_no=t['frame_no'][f0:f0 + nf])
        rows = [(a - f0, b - f0, o - l0, 0) for a, b, o, _ in blocks[b0:b0 + nb]]
        r2, inv = gate_ref.tables(1.5, 2.0, 8)
        st, out, k, _ = device_gate(alone, rows, link[l0:l1], xf[f0:f0 + nf], r2, inv, weight=0.25)
        assert st == 0 and np.array_equal(bits(out), bits(want[l0:l1])) and np.array_equal(k, kept[b0:b0 + nb])


def test_broken_blocks_get_minus_one_and_nothing_else():
    t, counts, blocks, link = sequence(31, 6, 2, holes=False)
    F, n = 6, len(link)
    xf = gate_cases.identity_records(F, 2)
    sizes = [counts[a] * counts[b] for a, b, _, _ in blocks]
    r2, inv = gate_ref.tables(1.5, 2.0, 8)
    swapped = dict(t, frame_no=np.asarray([0, 1, 5, 3, 4, 6], np.int32))   # frame 2 carries a number behind frame 3's
    past = dict(t, frame_start=np.concatenate([t['frame_start'][:3], t['frame_start'][3:] + 1000]).astype(np.int32))
    cases = {
        'a == b': (t, {1: (1, 1, blocks[1][2], 0)}), 'a > b': (t, {1: (2, 1, blocks[1][2], 0)}),
        'a < 0': (t, {0: (-1, 1, 0, 0)}), 'b >= F': (t, {4: (4, F, blocks[4][2], 0)}), 'b far': (t, {4: (4, 2 ** 30, blocks[4][2], 0)}),
        'frame numbers': (swapped, {}), 'reach of the records': (t, {0: (0, 3, 0, 0)}),
        'past n_link': (t, {len(blocks) - 1: blocks[-1][:2] + (n - sizes[-1] + 1, 0)}), 'negative offset': (t, {0: (0, 1, -4, 0)}),
        'frame_start past L': (past, {}),
    }
    for name, (tab, edits) in cases.items():
        rows = [edits.get(i, b) for i, b in enumerate(blocks)]
        want, wkept = gate_ref.gate(tab['det'], tab['frame_start'], tab['frame_no'], rows, xf, r2, inv, link)
        assert (wkept == -1).any() and (wkept >= 0).any(), name
        for i in edits:
            assert wkept[i] == -1, name
        for ip in (False, True):
            st, out, kept, _ = device_gate(tab, rows, link, xf, r2, inv, inplace=ip)
            assert st == 0 and np.array_equal(kept, wkept), name
            if ip:
                assert np.array_equal(bits(out), bits(want)), name
            else:  # out of place: the words of a broken block are the buffer's own, the others the restatement's
                own = np.ones(n, bool)
                for (a, b, o, _), k, sz in zip(blocks, wkept, sizes):
                    if k >= 0:
                        own[o:o + sz] = False
                        assert np.array_equal(bits(out[o:o + sz]), bits(want[o:o + sz])), name
                assert (out[own] == GUARD_SCORE).all(), name
        st, _, counted, _ = device_gate(tab, rows, link, xf, r2, inv, count_only=True)
        assert st == 0 and np.array_equal(counted == -1, wkept == -1), name
    # without records the reach is not a condition
    _, wkept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], [(0, 3, 0, 0)], None, r2, inv, link)
    st, _, kept, _ = device_gate(t, [(0, 3, 0, 0)], link, None, r2, inv)
    assert st == 0 and kept[0] == wkept[0] >= 0


def test_refusals_before_any_launch_and_the_empty_call():
    t, counts, blocks, link = sequence(41, 4, 2, holes=False)
    r2, inv = gate_ref.tables(1.5, 2.0, 8)
    xf = gate_cases.identity_records(4, 2)
    untouched = lambda r: r[0] == EINVAL and (r[2] == SENTINEL).all() and (r[1] is None or (r[1] == GUARD_SCORE).all())
    for k in ('det', 'frame_start', 'frame_no', 'blocks', 'r2', 'inv_r2', 'kept', 'link', 'out_link'):
        assert untouched(device_gate(t, blocks, link, xf, r2, inv, nulls=(k,))), k
    for kw in (dict(NB=-1), dict(max_dt=0), dict(max_dt=65), dict(mode=2), dict(mode=-1), dict(n_link=-1), dict(ratio=-1.0),
               dict(ratio=float('nan')), dict(weight=-0.5), dict(weight=float('nan')), dict(rec_gaps=0)):
        tabs = gate_ref.tables(1.5, 2.0, 64) if kw.get('max_dt') == 65 else (r2, inv)
        assert untouched(device_gate(t, blocks, link, xf, *tabs, **kw)), kw
    # NB = 0: a no-op that returns 0, whatever else is null
    st, out, kept, _ = device_gate(t, blocks, link, xf, r2, inv, NB=0, nulls=('det', 'blocks', 'kept'))
    assert st == 0 and (kept == SENTINEL).all() and (out == GUARD_SCORE).all()
    # the operator: one block in, kept out, the link gated in place; what it refuses
    p = A.pack_gate(gate_cases.frame_dicts(t), pairs=[(b[0], b[1]) for b in blocks])
    gate = A.MotionGate(max_speed=1.5, slack=2.0)
    packed, sizes = gate.block(p)
    dev_link = torch.from_numpy(link.copy()).cuda()
    kept = torch.ops.mmmot.gate_links(torch.from_numpy(packed).cuda(), dev_link, sizes, 0.0, 0.0)
    want, wkept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, None, r2, inv, link)
    assert np.array_equal(bits(dev_link.cpu().numpy()), bits(want)) and np.array_equal(kept.cpu().numpy(), wkept)
    with pytest.raises(ValueError, match='packed must be a contiguous int32'):
        torch.ops.mmmot.gate_links(torch.from_numpy(packed[:-1]).cuda(), dev_link, sizes, 0.0, 0.0)
    with pytest.raises(ValueError, match='link must be a contiguous float32'):
        torch.ops.mmmot.gate_links(torch.from_numpy(packed).cuda(), dev_link[:-1], sizes, 0.0, 0.0)
    with pytest.raises(RuntimeError, match='MMMOT_EINVAL'):
        torch.ops.mmmot.gate_links(torch.from_numpy(packed).cuda(), dev_link, sizes, -1.0, 0.0)


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def test_gate_links_shapes_dtypes_devices_and_the_block_it_names():
    t, counts, blocks, link = sequence(51, 5, 2)
    frames, pairs = gate_cases.frame_dicts(t), [(b[0], b[1]) for b in blocks]
    poses = gate_cases.drive(5, 9)
    gate = A.MotionGate(max_speed=1.5, slack=2.0, mode='3d', max_size_ratio=1.5, weight=0.5)
    xf = gate_cases.records(poses, pairs, 5, 2)
    want, wkept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, xf, gate.r2, gate.inv_r2, link, 1, 8, 1.5, 0.5)
    split = lambda flat: [flat[o:o + counts[a] * counts[b]].reshape(1, counts[a], counts[b]) for a, b, o, _ in blocks]
    given = [torch.from_numpy(x.copy()) for x in split(link)]
    for dev in ('cpu', 'cuda'):
        out, kept = A.gate_links([g.to(dev) for g in given], frames, gate, t['frame_no'], poses, gate_cases.fill_cases.CALIB, pairs)
        assert kept.dtype == np.int64 and np.array_equal(kept, wkept)
        for o, g, w in zip(out, given, split(want)):
            assert o.shape == g.shape and o.dtype == torch.float32 and o.device.type == dev
            assert np.array_equal(bits(o.cpu().numpy()), bits(w))
    assert all(np.array_equal(bits(g.numpy()), bits(x)) for g, x in zip(given, split(link)))  # the inputs are as they were
    # fp64 blocks come back as fp64 (the values those of the fp32 path)
    out, _ = A.gate_links([g.double() for g in given], frames, gate, t['frame_no'], poses, gate_cases.fill_cases.CALIB, pairs)
    assert all(o.dtype == torch.float64 and np.array_equal(o.numpy().astype(np.float32), w, equal_nan=True) for o, w in zip(out, split(want)))
    # the nested layout
    nested = [given[:4], given[4:]]
    out, kept = A.gate_sequence_links(nested, frames, gate, t['frame_no'], poses, gate_cases.fill_cases.CALIB)
    assert [len(r) for r in out] == [4, 3] and np.array_equal(np.concatenate(kept), wkept)
    assert all(np.array_equal(bits(o.numpy()), bits(w)) for o, w in zip([x for r in out for x in r], split(want)))
    # a block outside the contract is named: the tables of a call whose records reach one frame only
    p = A.pack_gate(frames, t['frame_no'], poses, gate_cases.fill_cases.CALIB, pairs)
    p['xf'], p['rec_gaps'] = p['xf'][:, :1].copy(), 1
    kept = A.queue_gate(p, gate, torch.from_numpy(link.copy()).cuda(), 'cuda').cpu().numpy()
    with pytest.raises(A.GateError, match=r'block 4 \(frames 0 -> 2\)') as e:
        A.check_kept(kept, p)
    assert isinstance(e.value, A.AssociationError) and e.value.index == 4 and e.value.frames == (0, 2)


# ---- gated scores through the solvers -----------------------------------------------------------------------------------------
def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


def absent(x):
    return np.where(np.isnan(x), np.float32(ABSENT), x).astype(np.float32)


def test_gated_pair_through_associate():
    rng = np.random.default_rng(61)
    gate = A.MotionGate(max_speed=4.0, slack=4.0)
    for N, M in ((1, 1), (5, 4), (7, 7), (3, 6)):
        t = gate_cases.tables(rng, [N, M])
        det, new, end, link = pair_ref.random_instance(rng, N, M, 1.0, 'normal')
        (gated,), kept = A.gate_links([torch.from_numpy(link)[None]], gate_cases.frame_dicts(t), gate)
        g = gated.numpy()[0]
        assert kept[0] == (~np.isnan(g)).sum() and (N * M == 1 or 0 < kept[0] < N * M)
        got = A.associate(torch.from_numpy(det), [gated], torch.from_numpy(new), torch.from_numpy(end), [N, M])
        got = (got[0].numpy(), got[1][0].numpy()[0], got[2].numpy(), got[3].numpy())
        want, wobj = pair_ref.lsa_route(det, new, end, absent(g), N, M)
        assert pair_ref.feasible(got, N, M)
        for x, w, name in zip(got, want, ('det', 'link', 'new', 'end')):
            assert np.array_equal(x.reshape(-1), w.reshape(-1)), (N, M, name)
        assert close(pair_ref.objective(got, det, new, end, absent(g)), wobj)
        assert (got[1][np.isnan(g)] == 0).all()


def test_gated_chain_through_associate_chain():
    rng = np.random.default_rng(62)
    gate = A.MotionGate(max_speed=4.0, slack=4.0)
    for split in ([3, 4, 2], [5, 5, 5], [1, 6, 3]):
        t = gate_cases.tables(rng, split)
        det, new, end, links = chain_ref.random_chain(rng, split, 1.0, 'normal')
        gated, kept = A.gate_links([torch.from_numpy(np.asarray(l, np.float32))[None] for l in links], gate_cases.frame_dicts(t), gate)
        g = [x.numpy()[0] for x in gated]
        assert 0 < kept.sum() < sum(x.size for x in g)
        got = A.associate_chain(torch.from_numpy(det), gated, torch.from_numpy(new), torch.from_numpy(end), split)
        got = (got[0].numpy(), [l.numpy()[0] for l in got[1]], got[2].numpy(), got[3].numpy())
        ref_links = [absent(x) for x in g]
        want, wobj = chain_ref.lp_route(det, new, end, ref_links, split)
        other, oobj = chain_ref.milp_route(det, new, end, ref_links, split)
        assert chain_ref.same_assignment(want, other) and close(oobj, wobj)  # no tied optimum
        assert chain_ref.feasible(got, split) and chain_ref.same_assignment(got, want), split
        assert close(chain_ref.objective(got, det, new, end, ref_links), wobj)
        assert all((a[np.isnan(x)] == 0).all() for a, x in zip(got[1], g))


def test_gated_sequence_through_associate_sequence_gaps():
    G, T = 3, 6
    gate = A.MotionGate(max_speed=4.0, slack=4.0)
    for seed in range(4):
        rng = np.random.default_rng(630 + seed)
        split = [int(n) for n in rng.integers(1, 6, T)]
        t = gate_cases.tables(rng, split, gate_cases.holey_numbers(rng, T))
        det, new, end, links = gap_ref.random_gap_sequence(rng, split, G, 'normal')
        nested = [[torch.from_numpy(np.asarray(l, np.float32))[None] for l in row] for row in links]
        gated, kept = A.gate_sequence_links(nested, gate_cases.frame_dicts(t), gate, t['frame_no'])
        g = [[x.numpy()[0] for x in row] for row in gated]
        n_nan = sum(int(np.isnan(x).sum()) for row in g for x in row)
        assert 0 < n_nan < sum(x.size for row in g for x in row) and sum(int(k.sum()) for k in kept) + n_nan == sum(x.size for row in g for x in row)
        got = A.associate_sequence_gaps(torch.from_numpy(det), gated, torch.from_numpy(new), torch.from_numpy(end), split,
                                        return_ids=True)
        asg = (got[0].numpy(), [[l.numpy()[0] for l in row] for row in got[1]], got[2].numpy(), got[3].numpy())
        ref_links = [[absent(x) for x in row] for row in g]
        want, wobj, info = gap_ref.ssp_gap_route(det, new, end, ref_links, split)
        other, oobj = gap_ref.milp_gap_route(det, new, end, ref_links, split)
        assert info['status'] == 0 and close(oobj, wobj)
        assert gap_ref.gap_feasible(asg, split) and gap_ref.same_gap_assignment(asg, want), split
        assert close(gap_ref.gap_objective(asg, det, new, end, ref_links), wobj)
        assert all((a[np.isnan(x)] == 0).all() for ra, rx in zip(asg[1], g) for a, x in zip(ra, rx))
        assert all(np.array_equal(i.numpy(), w) for i, w in zip(got[4], gap_ref.ids_of_gaps(asg, split)))


def test_only_the_gate_keeps_two_similar_objects_from_swapping():
    frames, objs, split, (det, links, new, end) = gate_cases.swap_scene()
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    nested = [[t_(l)[None] for l in row] for row in links]

    def ids_by_object(link_scores):
        got = A.associate_sequence_gaps(t_(det), link_scores, t_(new), t_(end), split, return_ids=True)
        assert got[5] >= 1
        return [dict(zip(o, i.tolist())) for o, i in zip(objs, got[4])], got[5]

    first, last = gate_cases.SWAP_HOLE[0] - 1, gate_cases.SWAP_HOLE[1] + 1
    # appearance alone: behind the hole object 0 carries object 1's ID and the reverse - asserted, so the case stays a case
    plain, n = ids_by_object(nested)
    assert n == 6 and plain[last][0] == plain[first][1] and plain[last][1] == plain[first][0] and plain[first][0] != plain[first][1]
    # with the gate every object keeps one ID through all of its frames, the scene's
    gated, kept = A.gate_sequence_links(nested, frames, A.MotionGate(max_speed=1.0, slack=1.0))
    assert all(bool(torch.isnan(g).any()) for row in gated for g in row)
    ids, n = ids_by_object(gated)
    assert n == 6 and all(per[o] == ids[0][o] for per in ids for o in per) and len(set(ids[0].values())) == 6
