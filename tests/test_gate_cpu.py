"""The motion gate ("Sequences: motion gate") without a GPU: the properties of the NumPy restatement
tests/gate_ref.py at the boundaries the specification names, the composed record against ``ego.align_pos``, the host
side ``association.pack_gate`` / ``MotionGate``, the Meta kernel of mmmot::gate_links, and ``tracks.pack_fill`` on the
rows of the helper it now shares with ``pack_gate``."""
import numpy as np
import pytest
import torch

import fill_cases
import gate_cases
import gate_ref
from mmmot_amd import association as A
from mmmot_amd import ego, synth, torch_ops, tracks


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def two_frames(loc_a, loc_b, dims_a=(1.5, 1.75, 4.0), dims_b=(1.5, 1.75, 4.0), frame_no=(0, 1)):
    """one detection per frame: the tables and the block of their one link"""
    det = np.zeros((2, 12), np.float32)
    det[0, 4:7], det[1, 4:7], det[0, 7:10], det[1, 7:10] = dims_a, dims_b, loc_a, loc_b
    return dict(det=det, frame_start=np.asarray([0, 1, 2], np.int32), frame_no=np.asarray(frame_no, np.int32)), [(0, 1, 0, 0)]


def one(t, blocks, score=1.0, max_speed=1.0, slack=0.5, max_dt=8, **kw):
    r2, inv = gate_ref.tables(max_speed, slack, max_dt)
    out, kept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, kw.pop('xf', None), r2, inv,
                              np.asarray([score], np.float32), max_dt=max_dt, **kw)
    return out[0], int(kept[0])


def test_a_link_on_the_radius_passes_and_the_next_location_is_gated():
    # max_speed 1, slack 0.5: r2[1] = 2.25, r2[2] = 6.25; locations on multiples of 0.25, so d2 is exact
    for loc_b, no in (((1.5, 0.75, 0.0), (0, 1)), ((0.0, -3.0, 1.5), (4, 5)), ((1.5, 0.25, 2.0), (0, 2)), ((-2.0, 9.0, -1.5), (7, 9))):
        t, blk = two_frames((0.0, 0.0, 0.0), loc_b, frame_no=no)
        assert one(t, blk) == (np.float32(1.0), 1)
        for axis in (0, 2):
            if loc_b[axis] == 0:
                continue
            beyond = np.asarray(loc_b, np.float32)
            beyond[axis] = np.nextafter(beyond[axis], np.float32(np.sign(beyond[axis]) * np.inf))
            s, k = one(*two_frames((0.0, 0.0, 0.0), beyond, frame_no=no))
            assert np.isnan(s) and k == 0 and bits(s) == 0x7fc00000
    # '3d' adds dy * dy last: the same links with y on the sphere pass, y beyond it is gated
    t, blk = two_frames((0.25, 1.0, 0.5), (1.25, 2.0, 1.0), frame_no=(0, 1))  # 1 + 0.25 + 1 = 2.25
    assert one(t, blk, mode=1) == (np.float32(1.0), 1) and one(t, blk, mode=0)[1] == 1
    t, blk = two_frames((0.25, 1.0, 0.5), (1.25, np.nextafter(np.float32(2.0), np.float32(3)), 1.0))
    assert one(t, blk, mode=1)[1] == 0 and one(t, blk, mode=0)[1] == 1


def test_dt_boundary_and_frame_numbers_with_holes():
    for max_dt in (1, 3, 8):
        t, blk = two_frames((0, 0, 0), (0, 0, 0), frame_no=(10, 10 + max_dt))
        assert one(t, blk, max_dt=max_dt)[1] == 1
        t, blk = two_frames((0, 0, 0), (0, 0, 0), frame_no=(10, 11 + max_dt))
        s, k = one(t, blk, max_dt=max_dt)
        assert np.isnan(s) and k == 0
    # the radius follows the frame NUMBERS, not the positions: 3 m apart passes at dt = 3 (r = 3.5) and not at dt = 2
    assert one(*two_frames((0, 0, 0), (3.0, 0, 0), frame_no=(5, 8)))[1] == 1
    assert one(*two_frames((0, 0, 0), (3.0, 0, 0), frame_no=(5, 7)))[1] == 0
    # frame numbers that do not increase: a broken block, nothing written
    for no in ((5, 5), (5, 4)):
        s, k = one(*two_frames((0, 0, 0), (0, 0, 0), frame_no=no), score=7.0)
        assert s == 7.0 and k == -1


def test_nan_inputs():
    nan = float('nan')
    for loc in ((nan, 0, 0), (0, 0, nan)):
        for t, blk in (two_frames(loc, (0, 0, 0)), two_frames((0, 0, 0), loc)):
            s, k = one(t, blk)
            assert np.isnan(s) and k == 0
    # y is not read in 'ground' mode
    t, blk = two_frames((0, nan, 0), (0, 0, 0))
    assert one(t, blk, mode=0)[1] == 1 and one(t, blk, mode=1)[1] == 0
    # a NaN dimension gates only when the size ratio is on, on either side
    for t, blk in (two_frames((0, 0, 0), (0, 0, 0), dims_a=(nan, 1, 1)), two_frames((0, 0, 0), (0, 0, 0), dims_b=(1, 1, nan))):
        assert one(t, blk)[1] == 1 and one(t, blk, max_size_ratio=2.0)[1] == 0
    # a NaN score stays as it is, payload included, is not counted, and is not touched by the weight
    payload = np.frombuffer(np.uint32(0x7fc12345).tobytes(), np.float32)[0]
    for w in (0.0, 0.5):
        s, k = one(*two_frames((0, 0, 0), (0, 0, 0)), score=payload, weight=w)
        assert bits(s) == 0x7fc12345 and k == 0


def test_size_ratio():
    f = lambda a, b, r: one(*two_frames((0, 0, 0), (0, 0, 0), dims_a=a, dims_b=b), max_size_ratio=r)[1]
    assert f((1.5, 2, 4), (3, 1, 2), 2.0) == 1      # every ratio exactly 2
    assert f((1.5, 2, 4), (3.25, 1, 2), 2.0) == 0 and f((1.5, 2, 4), (3, 1, 1.75), 2.0) == 0
    assert f((1.5, 2, 4), (30, 1, 1), 0.0) == 1     # off


def test_weight_zero_keeps_every_bit_pattern_and_the_weight_formula():
    rng = np.random.default_rng(0)
    t = gate_cases.tables(rng, [6, 7])
    r2, inv = gate_ref.tables(100.0, 1.0, 8)  # everything passes
    raw = rng.integers(0, 2 ** 32, 42, dtype=np.uint64).astype(np.uint32)
    raw[:6] = [0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x7fc00001, 0xffc00000]
    link = raw.view(np.float32)
    out, kept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], [(0, 1, 0, 0)], None, r2, inv, link)
    assert np.array_equal(bits(out), raw) and kept[0] == 42 - np.isnan(link).sum()
    link = gate_cases.random_links(rng, 42)
    out, kept = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], [(0, 1, 0, 0)], None, r2, inv, link, weight=0.5)
    a, b = t['det'][:6, None, 7:10].astype(np.float64), t['det'][None, 6:, 7:10].astype(np.float64)
    d2 = ((a - b)[..., 0] ** 2 + (a - b)[..., 2] ** 2).reshape(-1)
    assert kept[0] == 42 and np.array_equal(out, (link.astype(np.float64) - 0.5 * (d2 * inv[1])).astype(np.float32))
    assert (out < link).all()


def sequence_case(seed, counts, G, holes=True):
    rng = np.random.default_rng(seed)
    t = gate_cases.tables(rng, counts, gate_cases.holey_numbers(rng, len(counts)) if holes else None)
    blocks, n = gate_cases.gap_blocks(counts, G)
    return t, blocks, gate_cases.random_links(rng, n)


def test_identity_records_give_the_standing_camera_bits():
    t, blocks, link = sequence_case(3, [3, 5, 1, 4, 6, 2], 3)
    r2, inv = gate_ref.tables(1.5, 2.0, 8)
    for kw in (dict(), dict(mode=1, weight=0.5, max_size_ratio=2.5)):
        still = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, None, r2, inv, link, **kw)
        ident = gate_ref.gate(t['det'], t['frame_start'], t['frame_no'], blocks, gate_cases.identity_records(6, 3), r2,
                              inv, link, **kw)
        assert np.array_equal(bits(still[0]), bits(ident[0])) and np.array_equal(still[1], ident[1])
        assert 0 < np.isnan(still[0]).sum() < len(link) and (still[1] >= 0).all()


def test_composed_record_moves_a_centre_like_align_pos():
    """the words 0..15 ``pack_gate`` stores for a pair, applied by the restatement, against ``ego.align_pos`` with the
    pair's (R, T): 1e-11 m, the bound of tests/test_fill_cpu.py for the same composed matrix (five 4x4 products of
    entries up to 70 m; 5.7e-14 m was measured there)"""
    rng = np.random.default_rng(5)
    counts = [4, 3, 5, 2, 4, 3]
    t = gate_cases.tables(rng, counts)
    poses = gate_cases.drive(6, 3)
    pairs = A.gap_pairs(6, 3)
    p = A.pack_gate(gate_cases.frame_dicts(t), None, poses, fill_cases.CALIB, pairs)
    assert p['rec_gaps'] == 3 and p['xf'].shape == (6, 3, gate_ref.REC)
    assert np.array_equal(p['xf'], gate_cases.records(poses, pairs, 6, 3))
    for a, b in pairs:
        loc = t['det'][t['frame_start'][b]:t['frame_start'][b + 1], 7:10]
        R, T = ego.pair_motion(poses[a], poses[b])
        want, _ = ego.align_pos([R], [T], synth.KITTI_TR, synth.KITTI_IMU2VELO, synth.KITTI_R0,
                                [poses[b][1] - poses[a][1]], loc.astype(np.float64), np.zeros(len(loc)))
        assert np.abs(gate_ref.moved(loc, p['xf'][a, b - a - 1, 0:16]) - want).max() < 1e-11


def test_pack_gate_pair_window_and_batched_gap_layout():
    rng = np.random.default_rng(6)
    # a pair: one block
    t = gate_cases.tables(rng, [3, 4])
    p = A.pack_gate(gate_cases.frame_dicts(t))
    assert p['blocks'].tolist() == [[0, 1, 0, 0]] and p['n_link'] == 12 and p['sizes'] == [(3, 4)] and p['xf'] is None
    assert np.array_equal(bits(p['det'][:, :11]), bits(t['det'][:, :11])) and (p['det'][:, 11] == np.float32(0.9)).all()
    assert np.array_equal(p['frame_start'], t['frame_start'])
    assert p['det'].dtype == np.float32 and p['frame_start'].dtype == p['frame_no'].dtype == p['blocks'].dtype == np.int32
    # a window: the consecutive pairs, in the order of ``chains_table``'s link blocks; an empty frame is a 0-link block
    counts = [2, 0, 3, 1]
    t = gate_cases.tables(rng, counts)
    p = A.pack_gate(gate_cases.frame_dicts(t), frame_idx=[4, 6, 7, 9])
    assert p['blocks'].tolist() == [[0, 1, 0, 0], [1, 2, 0, 0], [2, 3, 0, 0]] and p['n_link'] == 3
    assert p['frame_no'].tolist() == [4, 6, 7, 9]
    # two sequences with skip links in one call, the frames numbered across them: gap_sequences_table's link layout
    splits, G = [[2, 3, 1, 4], [1, 2, 2]], 2
    t = gate_cases.tables(rng, splits[0] + splits[1])
    pairs = A.gap_pairs(4, G) + [(4 + a, 4 + b) for a, b in A.gap_pairs(3, G)]
    p = A.pack_gate(gate_cases.frame_dicts(t), pairs=pairs)
    seqs, _, _, _ = A.gap_sequences_table(splits, G)
    want, off = [], 0
    for s, first in zip(splits, (0, 4)):
        rows, off = gate_cases.gap_blocks(s, G, first, off)
        want += rows
    assert p['blocks'].tolist() == [list(r) for r in want] and p['n_link'] == off
    assert [int(p['blocks'][i, 2]) for i in (0, len(A.gap_pairs(4, G)))] == seqs[:, 2].tolist()
    assert p['sizes'] == A.gap_link_sizes(splits[0], G) + A.gap_link_sizes(splits[1], G)
    # the block the operator takes: every table at its place, the fp64 tables as their bits
    gate = A.MotionGate(max_speed=2.0, slack=1.0, max_dt=5, mode='3d')
    packed, sizes = gate.block(p)
    assert sizes == [len(t['det']), 7, len(pairs), 0, 5, 1, off]
    lay, n = torch_ops.gate_layout(sizes)
    got = torch_ops.sections(packed, lay)
    r2, inv = gate_ref.tables(2.0, 1.0, 5)
    assert len(packed) == n and np.array_equal(got['r2'], r2) and np.array_equal(got['inv_r2'], inv)
    assert np.array_equal(got['det'].view(np.float32).reshape(-1, 12), p['det']) and got['xf'].size == 0
    assert np.array_equal(got['blocks'].reshape(-1, 4), p['blocks']) and np.array_equal(got['frame_no'], p['frame_no'])
    # what the host refuses
    frames = gate_cases.frame_dicts(t)
    for bad in ([(1, 1)], [(2, 1)], [(-1, 2)], [(0, 7)]):
        with pytest.raises(ValueError, match='pair 0'):
            A.pack_gate(frames, pairs=bad)
    with pytest.raises(ValueError, match='frame numbers must increase'):
        A.pack_gate(frames, frame_idx=[0, 1, 2, 2, 4, 5, 6])
    with pytest.raises(ValueError, match='poses'):
        A.pack_gate(frames, poses=gate_cases.drive(7, 0)[:3] + [None] * 4, calib=fill_cases.CALIB)
    with pytest.raises(ValueError, match='calib'):
        A.pack_gate(frames, poses=gate_cases.drive(7, 0))


def test_motion_gate_defaults_tables_and_refusals():
    g = A.MotionGate()
    assert (g.max_speed, g.slack, g.max_dt, g.mode, g.max_size_ratio, g.weight) == (4.0, 2.0, 8, 'ground', 0.0, 0.0)
    r2, inv = gate_ref.tables(4.0, 2.0, 8)
    assert np.array_equal(g.r2, r2) and np.array_equal(g.inv_r2, inv) and g.r2.dtype == np.float64
    assert g.r2.tolist() == [(4.0 * dt + 2.0) ** 2 for dt in range(9)]
    assert A.MotionGate(max_dt=64).r2.shape == (65,)
    for kw in (dict(max_speed=-1.0), dict(max_speed=float('nan')), dict(slack=-0.1), dict(slack=float('inf')),
               dict(max_speed=0.0, slack=0.0), dict(max_dt=0), dict(max_dt=65), dict(max_dt=2.5), dict(mode='bev'),
               dict(max_size_ratio=-1.0), dict(max_size_ratio=0.5), dict(max_size_ratio=float('nan')), dict(weight=-0.5),
               dict(weight=float('inf'))):
        with pytest.raises(ValueError, match='MotionGate'):
            A.MotionGate(**kw)


def test_run_global_and_gate_links_refuse_what_is_no_gate():
    from mmmot_amd.pipeline import SequencePipeline
    pipe = SequencePipeline(torch.nn.Linear(1, 1), overlap=False)
    for bad in (4.0, 'ground', dict(max_speed=4.0)):
        with pytest.raises(ValueError, match='gate must be an association.MotionGate'):
            pipe.run_global([], max_gap=3, gate=bad)
    with pytest.raises(ValueError, match='gate must be a MotionGate'):
        A.gate_links([], [], 4.0)
    t = gate_cases.tables(np.random.default_rng(1), [2, 3])
    with pytest.raises(ValueError, match='link block 0 must hold 2 x 3'):
        A.gate_links([torch.zeros(1, 2, 2)], gate_cases.frame_dicts(t), A.MotionGate())
    with pytest.raises(ValueError, match='1 link blocks for 0 pairs'):
        A.gate_links([torch.zeros(1, 2, 3)], gate_cases.frame_dicts(t)[:1], A.MotionGate())
    with pytest.raises(ValueError, match='gap 2 needs 0 link blocks'):
        A.gate_sequence_links([[torch.zeros(2, 3)], [torch.zeros(2, 3)]], gate_cases.frame_dicts(t), A.MotionGate())


def test_meta_kernel_shapes_and_layout_refusals():
    sizes = [9, 4, 5, 2, 8, 0, 37]
    lay, n = torch_ops.gate_layout(sizes)
    assert lay['xf'] == (0, 2 * 33 * 4 * 2) and lay['r2'][1] == lay['inv_r2'][1] == 18 and lay['blocks'][1] == 20
    assert all(lay[k][0] % 2 == 0 for k in ('xf', 'r2', 'inv_r2'))  # 8-byte aligned
    packed = torch.empty(n, dtype=torch.int32, device='meta')
    kept = torch.ops.mmmot.gate_links(packed, torch.empty(37, device='meta'), sizes, 0.0, 0.0)
    assert kept.shape == (5,) and kept.dtype == torch.int32 and kept.device.type == 'meta'
    assert torch.ops.mmmot.gate_links(packed, None, sizes, 2.0, 0.5).shape == (5,)
    for bad in ([9, 4, 5, 2, 0, 0, 37], [9, 4, 5, 2, 65, 0, 37], [9, 4, 5, 2, 8, 2, 37], [9, 4, 5, 2, 8, 0], [9, -4, 5, 2, 8, 0, 37]):
        with pytest.raises(ValueError, match='gate_links'):
            torch_ops.gate_layout(bad)
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel
        torch.ops.mmmot.gate_links(torch.zeros(n, dtype=torch.int32), None, sizes, 0.0, 0.0)


def stated_rows(d, m, scores):
    """the [m, 12] rows of mmmot_fill_tracks as the header states them, written out once more"""
    row = np.empty((m, 12), np.float32)
    lhw = np.asarray(d['dimensions'], np.float64).reshape(m, 3)
    row[:, 0:4] = np.asarray(d['bbox'], np.float64).reshape(m, 4)
    row[:, 4], row[:, 5], row[:, 6] = lhw[:, 1], lhw[:, 2], lhw[:, 0]
    row[:, 7:10] = np.asarray(d['location'], np.float64).reshape(m, 3)
    row[:, 10] = np.asarray(d['rotation_y'], np.float64).reshape(m)
    row[:, 11] = 0.9 if scores is None else np.asarray(scores, np.float64).reshape(m)
    return row


def test_pack_fill_is_unchanged_on_the_shared_rows():
    from test_fill_cpu import moving_sequence
    frames, ids, frame_idx, scores, poses = moving_sequence()
    for seq, sc in (((frames, ids, frame_idx, scores, poses, fill_cases.CALIB), scores), (fill_cases.scene(True), None),
                    (fill_cases.scene(False), None)):
        p = tracks.pack_fill([seq])
        want = np.concatenate([stated_rows(d, len(i), None if sc is None else sc[t])
                               for t, (d, i) in enumerate(zip(seq[0], seq[1]))])
        assert p['det'].dtype == np.float32 and np.array_equal(bits(p['det']), bits(want)) and len(want) > 100
        # and both packers read the same rows
        g = A.pack_gate(seq[0], seq[2] if len(seq) > 2 else None)
        assert np.array_equal(bits(g['det'][:, :11]), bits(p['det'][:, :11])) and np.array_equal(g['frame_start'], p['frame_start'])


def test_the_swap_scene_needs_the_gate():
    """the scene of the GPU test, on the host: the gate (1 m per frame + 1 m) removes exactly the links between
    different objects, the two 6.0 links across the hole among them"""
    frames, objs, split, (det, links, new, end) = gate_cases.swap_scene()
    p = A.pack_gate(frames, pairs=A.gap_pairs(gate_cases.SWAP_FRAMES, gate_cases.SWAP_GAP))
    gate = A.MotionGate(max_speed=1.0, slack=1.0)
    flat = np.concatenate([l.reshape(-1) for row in links for l in row])
    out, kept = gate_ref.gate(p['det'], p['frame_start'], p['frame_no'], p['blocks'], None, gate.r2, gate.inv_r2, flat)
    assert (flat == 6.0).sum() == 2 and np.array_equal(np.isnan(out), flat != 5.5) and kept.sum() == (flat == 5.5).sum()
