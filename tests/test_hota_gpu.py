"""HOTA / IDF1 on the device (mmmot_amd.evaluate.hota_sequences, csrc/hota.hip) against the NumPy restatement
tests/hota_ref.py on the seeded inputs of tests/hota_cases.py.

Tolerances.  With u = 2^-53, a sum of n non-negative fp64 terms taken in any order lies within n u (relative) of the
exact sum, so two orders differ by at most 2 n u; the tests assert at 4 n u with
  LocSum, LocA:       n = TP of the lowest alpha (the pairs summed) + 1 (the quotient)
  AssA, AssRe, AssPr: n = the largest G T of a sequence (the cells summed; a cell's own term is formed by the same
                      operations on both sides) + S (the TP-weighted sum) + 3 (quotients and the weight)
  HOTA:               the same n + 2 (product and root)
  scalar means:       + 19
  frame value 0:      n = B, the largest box count a side (the gated IoUs of the preparation assignment)
  frame value 1:      n = 2 (F + 2 B + 3) + B + 3: pot is a sum over at most F frames of s / d with d from row and column
                      sums of at most B terms each, align = pot / (counts - pot) (the denominator is at least pot, so its
                      relative error is no larger), and the value sums at most B products align s.
Integer fields are compared exactly."""
import os

import numpy as np
import pytest

import hota_cases
import hota_ref
from mmmot_amd import evaluate as E

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
INT_FIELDS = ('TP', 'FN', 'FP', 'IDTP', 'IDFN', 'IDFP', 'n_gt', 'n_tr')
RATIOS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA')


@pytest.fixture(scope='module')
def cases():
    """name -> (gt, tracker, prepare, matchings checked, the restatement's answer), computed once"""
    out = {}
    for name in hota_cases.specs():
        gts, trs, prepare, matchings, _, _ = hota_cases.build(name)
        out[name] = (gts, trs, prepare, matchings, hota_ref.hota(gts, trs, prepare=prepare))
    return out


def within(got, want, n, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    print('%-24s n = %6d  worst |diff| / |want| = %.3e  (bound %.3e)' % (
        what, n, float(np.max(err / np.maximum(np.abs(want), 1e-300), initial=0.0)), 4 * n * U))
    assert got.shape == want.shape and np.all(err <= 4 * n * U * np.abs(want)), what


def sizes_of(gts, trs):
    p = E.pack_hota(gts, trs)
    return p, int(p['sizes'][8]), int(np.diff(p['foff']).max()), int((p['Gs'] * p['Ts']).max())


def check_values(h, want, gts, trs):
    """the per-frame assignment totals and the integer IDF1 fields: independent of which optimal matching is taken"""
    _, B, F, _ = sizes_of(gts, trs)
    assert h.frame_values.shape == want['frame_values'].shape
    within(h.frame_values[:, 0], want['frame_values'][:, 0], B, 'preparation value')
    within(h.frame_values[:, 1], want['frame_values'][:, 1], 2 * (F + 2 * B + 3) + B + 3, 'pass-2 value')
    for k in ('IDTP', 'IDFN', 'IDFP', 'n_gt', 'n_tr'):
        assert getattr(h, k) == want[k], k
    assert h.seq_IDTP == [s['IDTP'] for s in want['seq']] and h.seq_IDFN == [s['IDFN'] for s in want['seq']]
    assert h.seq_IDFP == [s['IDFP'] for s in want['seq']]


def check_record(h, want, gts, trs):
    check_values(h, want, gts, trs)
    p, _, _, cells = sizes_of(gts, trs)
    S = len(want['seq'])
    for k in ('TP', 'FN', 'FP'):
        assert np.array_equal(getattr(h, k), want[k]), k
        for s in range(S):
            assert np.array_equal(getattr(h, 'seq_' + k)[s], want['seq'][s][k]), (k, s)
    n_loc, n_ass = int(want['TP'][0]) + 1, cells + S + 3
    within(h.LocSum, want['LocSum'], n_loc, 'LocSum')
    within(h.LocA_alpha, want['LocA_alpha'], n_loc, 'LocA')
    for k in ('AssA', 'AssRe', 'AssPr'):
        within(getattr(h, k + '_alpha'), want[k + '_alpha'], n_ass, k)
    within(h.HOTA_alpha, want['HOTA_alpha'], n_ass + 2, 'HOTA')
    for k in ('DetA', 'DetRe', 'DetPr'):  # integers through the same quotient
        assert np.array_equal(getattr(h, k + '_alpha'), want[k + '_alpha']), k
    for k in RATIOS:
        within(getattr(h, k), want[k], max(n_loc, n_ass) + 2 + 19, 'mean ' + k)
    for s in range(S):
        within(h.seq_AssA[s], want['seq'][s]['AssA_alpha'], n_ass, 'AssA of sequence %d' % s)
        within(h.seq_LocSum[s], want['seq'][s]['LocSum'], n_loc, 'LocSum of sequence %d' % s)
    for k in ('IDF1', 'IDR', 'IDP'):
        assert getattr(h, k) == want[k], k
    assert len(h.summary()) == 14 and h.summary()[0] == h.HOTA and h.summary()[8] == h.IDF1


@pytest.mark.parametrize('name', ['small_kitti', 'small_plain'])
def test_small_frames_equal_the_restatement(cases, name):
    """3 sequences (1, 2 and 37 frames; 0, 1, 5 and 6 boxes a side) in one call: every field"""
    gts, trs, prepare, matchings, want = cases[name]
    assert matchings and len(gts) == 3
    h = E.hota_sequences(gts, trs, prepare=prepare)
    check_record(h, want, gts, trs)
    assert h.TP[0] > 0 and h.FP[0] > 0 and h.FN[0] > 0 and 0 < h.IDTP < h.n_gt
    # a sequence's values do not depend on what else the call holds
    alone = E.hota_sequences(gts[2], trs[2], prepare=prepare)
    assert np.array_equal(alone.TP, h.seq_TP[2]) and alone.IDTP == h.seq_IDTP[2]
    assert np.array_equal(alone.seq_AssA[0], h.seq_AssA[2]) and np.array_equal(alone.LocSum, h.seq_LocSum[2])


def test_small_frames_with_the_other_preparation(cases):
    """the kitti inputs (DontCare and neighbour-class rows) without preparation"""
    gts, trs, _, _, _ = cases['small_kitti']
    if not all(hota_cases.conditions_met(g, t, None, True) for g, t in zip(gts, trs)):
        pytest.fail('the small_kitti inputs break the generator conditions without preparation')
    check_record(E.hota_sequences(gts, trs, prepare=None), hota_ref.hota(gts, trs, prepare=None), gts, trs)


@pytest.mark.parametrize('name', ['mid_kitti', 'full_frame', 'wide_ids'])
def test_larger_frames_and_many_ids(cases, name):
    """12 boxes a side; a frame at exactly CLEAR_MOT_MAX_BOXES; G = 70 and T = 90 IDs: the quantities that do not depend
    on the choice among optimal matchings"""
    gts, trs, prepare, matchings, want = cases[name]
    h = E.hota_sequences(gts, trs, prepare=prepare)
    check_values(h, want, gts, trs)
    assert h.IDTP > 0 and h.IDFN > 0 and h.IDFP > 0


def test_transposed_rows_equal_columns_and_an_empty_side(cases):
    """hota_cases.twin_sequence: every field - each twin's ID occurs once, so the record is the same whichever is taken"""
    gts, trs, prepare, _, want = cases['transposed_twins']
    h = E.hota_sequences(gts, trs, prepare=prepare)
    check_record(h, want, gts, trs)
    assert h.TP[0] == 6 and h.IDTP == 6 and h.n_gt == 73 and h.n_tr == 75


def test_two_calls_are_bit_equal(cases):
    for name in ('small_kitti', 'full_frame', 'wide_ids'):
        gts, trs, prepare, _, _ = cases[name]
        p = E.pack_hota(gts, trs)
        params = [25., 0., 2., 1. if prepare else 0.]
        a, b = E.run_hota(p, params), E.run_hota(p, params)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_evaluate_hota_reads_what_write_kitti_tracks_wrote(cases, tmp_path):
    from mmmot_amd.tracks import write_kitti_tracks
    gts, trs, _, _, _ = cases['small_kitti']
    names = {E.MAIN: 'Car', E.NEIGHBOUR: 'Van'}

    def frames_of(lab):
        rows = lab.rows[lab.rows[:, E.CLS] != E.DONTCARE]  # an ID of -1 is not written
        dets, ids = [], []
        for f in range(int(lab.n_frames[0])):
            r = rows[rows[:, E.FRAME] == f]
            n = len(r)
            dets.append({'bbox': r[:, E.X1:], 'name': [names[int(c)] for c in r[:, E.CLS]], 'truncated': r[:, E.TRUNC],
                         'occluded': r[:, E.OCC].astype(np.int64), 'dimensions': np.zeros((n, 3)),
                         'location': np.zeros((n, 3)), 'rotation_y': np.zeros(n)})
            ids.append(r[:, E.TID].astype(np.int64))
        return dets, ids

    os.makedirs(str(tmp_path / 'gt' / 'label_02'))
    os.makedirs(str(tmp_path / 'res' / 'sha' / 'all'))
    tab_g, tab_t, seqmap = [], [], []
    for s, (g, t) in enumerate(zip(gts[1:], trs[1:])):  # 2 and 37 frames
        n = int(g.n_frames[0])
        seqmap.append('%04d empty %06d %06d' % (s, 0, n - 1))
        for lab, path, tabs, is_gt in ((g, tmp_path / 'gt' / 'label_02', tab_g, True),
                                       (t, tmp_path / 'res' / 'sha' / 'all', tab_t, False)):
            dets, ids = frames_of(lab)
            write_kitti_tracks(str(path / ('%04d.txt' % s)), dets, ids)
            tabs.append(E.labels_from_tracks(dets, ids, n_frames=n, ground_truth=is_gt))
    with open(str(tmp_path / 'gt' / 'evaluate_tracking.seqmap'), 'w') as f:
        f.write('\n'.join(seqmap) + '\n')
    got = E.evaluate_hota('sha', str(tmp_path / 'res'), 'all', gt_path=str(tmp_path / 'gt'), cls='car')
    want = E.hota_sequences(tab_g, tab_t)
    assert isinstance(got, E.Hota) and got.TP[0] > 0
    for k in INT_FIELDS + ('LocSum',) + tuple(r + '_alpha' for r in RATIOS):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert got.summary() == want.summary() and got.summary_line() == want.summary_line()
    assert E.evaluate_hota('sha', str(tmp_path / 'res'), 'all', gt_path=str(tmp_path / 'gt'), cls='pedestrian') is False


def test_limits_are_refused():
    import torch
    from mmmot_amd import _lib
    gts, trs, _, _, _, _ = hota_cases.build('small_plain')
    p = E.pack_hota(gts, trs)
    nG, nT, nD, NF, S, cells, sumG, sumT, max_boxes, max_dc = p['sizes']
    # the launcher: a frame or table limit beyond the kernel's returns -1 without a launch
    dev = torch.zeros(4096, dtype=torch.int32, device='cuda')
    ptr = dev.data_ptr()
    call = lambda **kw: _lib.load().mmmot_hota(*[kw.get(k, v) for k, v in (
        ('boxes', ptr), ('nG', 1), ('nT', 1), ('nD', 0), ('frames', ptr), ('NF', 1), ('frame_seq', ptr), ('g_attr', ptr),
        ('t_id', ptr), ('seq_tab', ptr), ('S', 1), ('cells', 1), ('sumG', 1), ('sumT', 1), ('max_boxes', 1),
        ('max_dontcare', 0), ('min_height', 25.), ('max_truncation', 0.), ('max_occlusion', 2.), ('prepare', 1),
        ('work', ptr), ('work_bytes', 4 * 4096), ('frame_d', ptr), ('frame_i', ptr), ('seq_d', ptr), ('seq_i', ptr),
        ('stream', None))])
    assert call(max_boxes=E.CLEAR_MOT_MAX_BOXES + 1) == -1 and call(max_dontcare=E.CLEAR_MOT_MAX_DONTCARE + 1) == -1
    assert call(cells=E.HOTA_MAX_CELLS + 1) == -1 and call(sumG=E.HOTA_MAX_IDS + 1) == -1
    assert call(sumT=E.HOTA_MAX_IDS + 1) == -1 and call(work_bytes=8) == -1
    torch.cuda.synchronize()
    assert not dev.any()  # nothing was launched
    # the operator: the same limits raise on the host
    with pytest.raises(ValueError, match='more than 128 boxes'):
        torch.ops.mmmot.hota(dev[:8], [nG, nT, nD, NF, S, cells, sumG, sumT, 129, max_dc], [25., 0., 2., 1.])
    with pytest.raises(ValueError, match='ID tables'):
        torch.ops.mmmot.hota(dev[:8], [nG, nT, nD, NF, S, S * E.HOTA_MAX_CELLS + 1, sumG, sumT, max_boxes, max_dc],
                             [25., 0., 2., 1.])
    with pytest.raises(ValueError, match='packed must be'):
        torch.ops.mmmot.hota(dev[:8], p['sizes'], [25., 0., 2., 1.])
    # a frame row beyond the limit that a caller let through: the kernel marks it and reads nothing of it
    p['frames'] = p['frames'].copy()
    p['frames'][NF - 1, 1] = E.CLEAR_MOT_MAX_BOXES + 1
    out = E.run_hota(p, [25., 0., 2., 1.])
    assert np.all(out['frame_i'].reshape(NF, -1)[NF - 1] == -1) and np.all(out['frame_i'].reshape(NF, -1)[:NF - 1] >= 0)
    with pytest.raises(RuntimeError, match='outside the launch limits'):
        E.finish_hota(p, out)
    # the meta kernel gives the output's shape without a device
    meta = torch.ops.mmmot.hota(torch.empty(E.hota_layout(p['sizes'])[2], dtype=torch.int32, device='meta'), p['sizes'],
                                [25., 0., 2., 1.])
    assert meta.shape == (E.hota_layout(p['sizes'])[3],) and meta.dtype == torch.int32
