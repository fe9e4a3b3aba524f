"""HOTA / IDF1 without a GPU: the NumPy restatement (tests/hota_ref.py) on cases with closed forms, the host side of
mmmot_amd.evaluate.hota_sequences (packing, limits, refusals), the launcher's argument checks and the conditions of the
random inputs the device test uses."""
import numpy as np
import pytest

import hota_cases
import hota_ref
from hota_cases import labels
from mmmot_amd import _lib
from mmmot_amd import evaluate as E
from mmmot_amd.evaluate import Hota, evaluate_hota, hota_sequences  # noqa: F401  (the public names)

M, N, D = E.MAIN, E.NEIGHBOUR, E.DONTCARE
BOX = [100., 100., 200., 180.]


def row(frame, tid, box, cls=M, trunc=0, occ=0):
    return [0, frame, tid, cls, trunc, occ] + list(box)


def shifted(box, dx):
    return [box[0] + dx, box[1], box[2] + dx, box[3]]


def test_tracker_equal_to_ground_truth():
    g = [row(f, k, shifted(BOX, 150 * k + 3 * f)) for f in range(6) for k in range(3)]
    r = hota_ref.hota(labels(g, 6, True), labels(g, 6, False))
    for k in ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA'):
        assert np.all(r[k + '_alpha'] == 1.0) and r[k] == 1.0, k
    assert np.all(r['TP'] == 18) and not r['FN'].any() and not r['FP'].any()
    assert (r['IDTP'], r['IDFN'], r['IDFP'], r['IDF1'], r['IDR'], r['IDP']) == (18, 0, 0, 1.0, 1.0, 1.0)


@pytest.mark.parametrize('n', [1, 4])
def test_id_change_half_way(n):
    g = [row(f, 7, shifted(BOX, f)) for f in range(2 * n)]
    t = [row(f, 1 if f < n else 2, shifted(BOX, f)) for f in range(2 * n)]
    r = hota_ref.hota(labels(g, 2 * n, True), labels(t, 2 * n, False))
    assert np.all(r['TP'] == 2 * n) and np.all(r['DetA_alpha'] == 1.0) and np.all(r['AssA_alpha'] == 0.5)
    assert np.all(r['HOTA_alpha'] == np.sqrt(0.5)) and np.all(r['LocA_alpha'] == 1.0)
    assert np.all(r['AssRe_alpha'] == 0.5) and np.all(r['AssPr_alpha'] == 1.0)
    assert (r['IDTP'], r['IDFN'], r['IDFP'], r['IDF1']) == (n, n, n, 0.5)


def test_empty_tracker_and_empty_ground_truth():
    g = [row(f, 0, BOX) for f in range(3)] + [row(1, 1, shifted(BOX, 300))]
    none = np.zeros((0, 10))
    r = hota_ref.hota(labels(g, 3, True), labels(none, 3, False))
    assert not r['TP'].any() and np.all(r['FN'] == 4) and not r['FP'].any()
    assert r['HOTA'] == 0.0 and np.all(r['LocA_alpha'] == 1.0) and r['IDF1'] == 0.0 and r['IDFN'] == 4
    r = hota_ref.hota(labels(none, 3, True), labels(g, 3, False))
    assert not r['TP'].any() and not r['FN'].any() and np.all(r['FP'] == 4)
    assert r['HOTA'] == 0.0 and (r['IDTP'], r['IDFN'], r['IDFP']) == (0, 0, 4)


def test_iou_two_thirds_counts_up_to_alpha_065():
    # boxes 100 wide shifted by 20: intersection 80, union 120
    g, t = [row(0, 0, BOX)], [row(0, 0, shifted(BOX, 20))]
    r = hota_ref.hota(labels(g, 1, True), labels(t, 1, False))
    assert hota_ref.iou_matrix(BOX, shifted(BOX, 20))[0, 0] == pytest.approx(2 / 3, abs=1e-15)
    want = (hota_ref.ALPHAS < 0.66).astype(np.int64)
    assert want.sum() == 13 and np.array_equal(r['TP'], want)
    assert np.array_equal(r['FN'], 1 - want) and np.array_equal(r['FP'], 1 - want)
    assert np.allclose(r['LocA_alpha'], np.where(want == 1, 2 / 3, 1.0), rtol=0, atol=1e-15)
    assert (r['IDTP'], r['IDFN'], r['IDFP']) == (1, 0, 0)  # 2 / 3 >= 0.5


def test_two_sequences_combine_by_tp_weight():
    # sequence A: the ID change over 2 x 2 frames (TP 4, AssA 0.5); sequence B: a perfect track of 6 frames plus 2
    # frames of a tracker box on nothing (TP 6, FP 2, AssA 1)
    ga = [row(f, 7, BOX) for f in range(4)]
    ta = [row(f, 1 if f < 2 else 2, BOX) for f in range(4)]
    gb = [row(f, 0, BOX) for f in range(6)]
    tb = gb + [row(f, 9, shifted(BOX, 500)) for f in range(2)]
    r = hota_ref.hota([labels(ga, 4, True), labels(gb, 6, True)], [labels(ta, 4, False), labels(tb, 6, False)])
    assert np.all(r['TP'] == 10) and np.all(r['FP'] == 2) and not r['FN'].any()
    ass = (0.5 * 4 + 1.0 * 6) / 10
    det = 10 / 12
    assert np.allclose(r['AssA_alpha'], ass, rtol=0, atol=1e-15) and np.allclose(r['DetA_alpha'], det, rtol=0, atol=1e-15)
    assert r['HOTA'] == pytest.approx(np.sqrt(ass * det), abs=1e-15)
    assert [s['AssA'] for s in r['seq']] == [0.5, 1.0]
    assert (r['IDTP'], r['IDFN'], r['IDFP']) == (2 + 6, 2, 2 + 2)
    assert r['IDF1'] == 8 / (8 + 0.5 * 4 + 0.5 * 2)


def kept(g, t, **kw):
    """(kept gt count, kept tracker count) of a one-frame sequence"""
    r = hota_ref.hota(labels(g, 1, True), labels(t, 1, False), **kw)
    return r['n_gt'], r['n_tr']


def test_preparation_rules():
    far = shifted(BOX, 400)
    # a tracker box matched to a neighbour-class / occluded / truncated gt row leaves with it; the other pair stays
    for bad in (dict(cls=N), dict(occ=3), dict(trunc=1)):
        assert kept([row(0, 0, BOX, **bad), row(0, 1, far)], [row(0, 0, BOX), row(0, 1, far)]) == (1, 1)
    assert kept([row(0, 0, BOX, occ=2), row(0, 1, far)], [row(0, 0, BOX), row(0, 1, far)]) == (2, 2)
    # ... unmatched (IoU 1 / 3 < 0.5) it stays
    assert kept([row(0, 0, BOX, cls=N), row(0, 1, far)], [row(0, 0, shifted(BOX, 50)), row(0, 1, far)]) == (1, 2)
    # an unmatched box of height exactly 25 leaves, one of 25.5 stays; matched, height does not matter
    low = lambda h: [600., 100., 700., 100. + h]
    assert kept([row(0, 0, BOX)], [row(0, 0, BOX), row(0, 1, low(25.0))]) == (1, 1)
    assert kept([row(0, 0, BOX)], [row(0, 0, BOX), row(0, 1, low(25.5))]) == (1, 2)
    assert kept([row(0, 0, low(25.0))], [row(0, 0, low(25.0)), row(0, 1, far)]) == (1, 2)
    # an unmatched box covered by a DontCare area to exactly 0.5 stays, to 0.51 leaves
    dc = lambda c: row(0, -1, [600., 0., 600. + 100 * c, 300.], cls=D, trunc=-1, occ=-1)
    tall = [600., 100., 700., 200.]
    assert kept([row(0, 0, BOX), dc(0.5)], [row(0, 0, BOX), row(0, 1, tall)]) == (1, 2)
    assert kept([row(0, 0, BOX), dc(0.51)], [row(0, 0, BOX), row(0, 1, tall)]) == (1, 1)
    # without preparation: every main-class gt row, every tracker row
    assert kept([row(0, 0, BOX, occ=3), row(0, 1, far, cls=N), dc(1.0)], [row(0, 0, BOX), row(0, 1, low(5.0)), row(0, 2, tall)],
                prepare=None) == (1, 3)


def test_pack_hota_tables():
    g = [row(0, 40, BOX), row(0, 10, shifted(BOX, 300), cls=N), row(1, 40, BOX), row(1, 70, shifted(BOX, 300)),
         row(1, -1, BOX, cls=D, trunc=-1, occ=-1)]
    t = [row(0, 5, BOX), row(1, 3, BOX), row(1, 5, shifted(BOX, 300)), row(2, 8, BOX)]
    g2, t2 = [row(0, 1, BOX)], [row(0, 1, BOX), row(0, 2, shifted(BOX, 300))]
    p = E.pack_hota([labels(g, 3, True), labels(g2, 1, True)], [labels(t, 3, False), labels(t2, 1, False)])
    assert p['sizes'] == [5, 6, 1, 4, 2, 2 * 3 + 1 * 2, 3, 5, 2, 1]
    assert p['frame_seq'].tolist() == [0, 0, 0, 1]
    assert p['g_attr'][:, 3].tolist() == [0, -1, 0, 1, 0]           # dense IDs, main class only
    assert p['t_id'].tolist() == [1, 0, 1, 2, 0, 1]
    assert p['seq_tab'].tolist() == [[0, 2, 3, 0, 0, 0], [3, 1, 2, 6, 2, 3], [4, 0, 0, 8, 3, 5]]
    inp, out, n_in, n_out, n_work = E.hota_layout(p['sizes'])
    assert n_in == 8 * 12 + 6 * 4 + 4 + 4 * 5 + 6 + 6 * 3 and inp['boxes'][0] == 0
    assert n_out == 2 * 21 * 4 + 2 * 76 * 3 + 21 * 4 + 24 * 3 and out['seq_d'][0] % 2 == 0
    assert n_work == 2 * 8 + 20 * 8 + 3 + 5 + 5 + 6


def test_host_refusals():
    one = labels([row(0, 0, BOX)], 1, True)
    with pytest.raises(ValueError, match='prepare'):
        hota_sequences(one, one, prepare='mot17', device='cpu')
    many = [row(0, k, shifted(BOX, k)) for k in range(E.CLEAR_MOT_MAX_BOXES + 1)]
    with pytest.raises(ValueError, match='more than 128 boxes'):
        E.pack_hota(labels(many, 1, True), one)
    with pytest.raises(ValueError, match='not unique'):
        E.pack_hota(labels([row(0, 3, BOX), row(0, 3, shifted(BOX, 300))], 1, True), one)
    with pytest.raises(ValueError, match='not unique'):
        E.pack_hota(one, labels([row(0, 3, BOX), row(0, 3, shifted(BOX, 300))], 1, True))
    with pytest.raises(ValueError, match='sequences'):
        E.pack_hota([one, one], one)
    # ID limits: 2049 IDs on a side; 600 x 600 = 360 000 > 2^18 id pairs
    ids = lambda n, frames: labels([row(k // 100, k, BOX) for k in range(n)], frames, True)
    assert E.HOTA_MAX_IDS == 2048 and E.HOTA_MAX_CELLS == 2 ** 18
    with pytest.raises(ValueError, match='track ids on a side'):
        E.pack_hota(ids(2049, 21), ids(1, 21))
    with pytest.raises(ValueError, match='id pairs'):
        E.pack_hota(ids(600, 6), ids(600, 6))
    assert E.pack_hota(ids(512, 6), ids(512, 6))['sizes'][5] == 2 ** 18
    for sizes in ([1, 1, 0, 1, 1, 1, 1, 1, 129, 0], [1, 1, 0, 1, 1, 1, 1, 1, 1, 65], [1, 1, 0, 1, 1, 2 ** 18 + 1, 1, 1, 1, 0],
                  [1, 1, 0, 1, 1, 1, 2049, 1, 1, 0], [1, 1, 0, 1, 0, 1, 1, 1, 1, 0], [1, 1, 0, 1, 1, 1, 1, 1, 1]):
        with pytest.raises(ValueError):
            E.hota_layout(sizes)


def test_launcher_refuses_without_a_launch():
    lib = _lib.load()
    assert lib.mmmot_abi_version() == 10
    d = 4096  # never dereferenced: the argument checks come before any launch
    good = [d, 1, 1, 0, d, 1, d, d, d, d, 1, 1, 1, 1, 1, 0, 25., 0., 2., 1, d, 1 << 20, d, d, d, d, None]
    names = ['boxes', 'nG', 'nT', 'nD', 'frames', 'NF', 'frame_seq', 'g_attr', 't_id', 'seq_tab', 'S', 'cells', 'sumG',
             'sumT', 'max_boxes', 'max_dontcare', 'min_height', 'max_truncation', 'max_occlusion', 'prepare', 'work',
             'work_bytes', 'frame_d', 'frame_i', 'seq_d', 'seq_i', 'stream']
    assert len(good) == len(names) == len(_lib.SIGNATURES['mmmot_hota'])
    bad = {'boxes': [None, d + 4], 'frames': [None], 'frame_seq': [None], 'g_attr': [None], 't_id': [None],
           'seq_tab': [None], 'work': [None, d + 4], 'frame_d': [None, d + 4], 'frame_i': [None], 'seq_d': [None, d + 4],
           'seq_i': [None], 'nG': [-1], 'nT': [-1], 'nD': [-1], 'NF': [-1], 'S': [0, -1], 'cells': [-1, 2 ** 18 + 1],
           'sumG': [-1, 2049], 'sumT': [-1, 2049], 'max_boxes': [-1, 129], 'max_dontcare': [-1, 65], 'prepare': [2, -1],
           'work_bytes': [0, 8 * 1 + 4 * (20 + 1 + 1 + 1 + 1) - 1]}
    for name, values in bad.items():
        for v in values:
            args = list(good)
            args[names.index(name)] = v
            assert lib.mmmot_hota(*args) == -1, (name, v)


def test_committed_seeds_meet_the_generator_conditions():
    drawn = replaced = 0
    for name in hota_cases.specs():
        gts, trs, prepare, matchings, d, r = hota_cases.build(name)
        drawn, replaced = drawn + d, replaced + r
        p = E.pack_hota(gts, trs)
        if name == 'wide_ids':
            assert p['Gs'].tolist() == [70] and p['Ts'].tolist() == [90]
        if name == 'full_frame':
            assert p['frames'][0, 1] == p['frames'][0, 3] == E.CLEAR_MOT_MAX_BOXES
        if matchings:
            assert p['sizes'][8] <= 6
    assert drawn >= 9 and replaced <= 0.1 * drawn, (drawn, replaced)
    # the brute force itself: two optimal matchings that differ in a non-zero cell are told apart ...
    assert hota_cases.distinct_totals(np.array([[1., 1.], [1., 1.]]))[:2] == [2.0, 2.0]
    # ... and matchings that differ only in zero-valued cells are one
    assert hota_cases.distinct_totals(np.array([[1., 0., 0.], [0., 0., 0.]])) == [1.0, 0.0]
