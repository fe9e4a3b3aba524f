"""SequencePipeline.run_global(max_gap=3, gate=MotionGate(..)) on synthetic sequences of 6 frames, with a standing and
with a moving camera: a gate that passes everything changes no bit of the result; a tight gate leaves out exactly the
gap pairs the restatement tests/gate_ref.py finds without a surviving link, and the whole result is ``solve_global`` by
hand on the ungated run's scores after ``association.gate_links`` by hand; ``fill=`` runs behind it unchanged."""
import numpy as np
import pytest
import torch

import gate_ref
from test_lockstep_gpu import shaped
from test_pipeline_gap_gpu import S, model, nested, same_arrays
from mmmot_amd import association as A
from mmmot_amd.pipeline import FrameFeed, SequencePipeline, solve_global
from mmmot_amd.synth import make_sequence

pytestmark = pytest.mark.gpu

N, G = 6, 3
# 1 m per frame + 1 m.  The synthetic frames hold unrelated random boxes, so this radius - chosen with gate_ref on the
# host - leaves some gap pairs without any link and some with a few (asserted below), for both cameras
TIGHT = dict(max_speed=1.0, slack=1.0)
_FEEDS, _PLAIN = {}, {}


def feeds_of(poses):
    if poses not in _FEEDS:
        frames = make_sequence(N, seed=21, n_pts=4000, det_range=(2, 5), hw=(120, 400), ego=0 if poses else None)
        _FEEDS[poses] = [FrameFeed(img, sweep, info, shaped(dets), pose=(info['pos'], info['rad']) if poses else None)
                         for img, sweep, info, dets in frames]
    return _FEEDS[poses]


def run(poses, **kw):
    pipe = SequencePipeline(model(), S)
    return pipe, pipe.run_global(feeds_of(poses), frames_per_encode=4, pairs_per_forward=3, max_gap=G, **kw)


def plain(poses):
    """the run without a gate, once per camera"""
    if poses not in _PLAIN:
        _PLAIN[poses] = run(poses)
    return _PLAIN[poses]


def same_result(a, b):
    """two GlobalResults: the same bits, NaN scores at the same places"""
    fl = lambda r: [r[0], r[2], r[3]] + [l for row in r[1] for l in row]
    (sa, aa), (sb, ab) = nested(a), nested(b)
    assert len(fl(sa)) == len(fl(sb))
    for x, y in zip(fl(sa), fl(sb)):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
    assert same_arrays(aa, ab)
    assert all(np.array_equal(x, y) for x, y in zip(a.ids, b.ids)) and a.n_tracks == b.n_tracks
    assert a.objective == b.objective and a.split == b.split and a.max_gap == b.max_gap


@pytest.mark.parametrize('poses', [False, True], ids=['still', 'poses'])
def test_a_gate_that_passes_everything_changes_nothing(poses):
    a_pipe, a = plain(poses)
    b_pipe, b = run(poses, gate=A.MotionGate(max_speed=1e6))
    same_result(a, b)
    assert not any(bool(torch.isnan(l).any()) for row in [b.scores[1]] + b.gap_scores for l in row)
    assert a.gate_kept is None and np.array_equal(b.gate_kept, [x * y for x, y in A.gap_link_sizes(b.split, G)])
    assert b_pipe.stats['gated_pairs'] == 0 and b_pipe.stats['gated_links'] == 0
    assert b_pipe.stats['gap_pairs'] == a_pipe.stats['gap_pairs'] == (N - 2) + (N - 3)
    assert b_pipe.stats['pairs'] == a_pipe.stats['pairs'] and 'gated_pairs' not in a_pipe.stats
    assert all(np.array_equal(x, y) for x, y in zip(a_pipe.tracks, b_pipe.tracks))


@pytest.mark.parametrize('poses', [False, True], ids=['still', 'poses'])
def test_a_tight_gate_skips_the_pairs_without_a_link(poses):
    feeds, gate = feeds_of(poses), A.MotionGate(**TIGHT)
    pairs = A.gap_pairs(N, G)
    dets = [f.dets for f in feeds]
    geometry = dict(frame_idx=list(range(N)), poses=[f.pose for f in feeds] if poses else None,
                    calib=feeds[0].info if poses else None)
    p = A.pack_gate(dets, pairs=pairs, **geometry)
    _, counted = gate_ref.gate(p['det'], p['frame_start'], p['frame_no'], p['blocks'], p['xf'], gate.r2, gate.inv_r2, None,
                               n_link=p['n_link'])
    gaps = np.asarray([b - a > 1 for a, b in pairs])
    empty = gaps & (counted == 0)
    # what the test rests on: some gap pairs keep no link, some keep a few
    assert empty.sum() >= 1 and (gaps & (counted > 0)).sum() >= 1
    pipe, got = run(poses, gate=gate)
    assert pipe.stats['gated_pairs'] == empty.sum()
    assert pipe.stats['gap_pairs'] == (N - 2) + (N - 3) - empty.sum()
    assert pipe.stats['pairs'] == (N - 1) + pipe.stats['gap_pairs']
    assert np.array_equal(got.gate_kept, counted) and pipe.stats['gated_links'] == p['n_link'] - counted.sum()
    blocks = [l for row in [got.scores[1]] + got.gap_scores for l in row]
    assert len(blocks) == len(pairs)
    for l, k, skipped in zip(blocks, counted, empty):
        assert int((~torch.isnan(l)).sum()) == k
        assert not skipped or bool(torch.isnan(l).all())
    # by hand: the ungated run's scores, gated by association.gate_links, solved by solve_global
    _, ungated = plain(poses)
    det, links1, new, end = ungated.scores
    given = list(links1) + [l for row in ungated.gap_scores for l in row]
    gated, kept = A.gate_links([l.cuda() for l in given], dets, gate, pairs=pairs, **geometry)
    assert np.array_equal(kept, counted)
    for l, g in zip(blocks, gated):  # the pipeline's blocks: a surviving score is the ungated run's, bit for bit
        assert l.shape == g.shape and np.array_equal(l.numpy(), g.cpu().numpy(), equal_nan=True)
    split = ungated.split
    o = np.concatenate([[0], np.cumsum(split)])
    part = lambda x, t: x.reshape(-1)[o[t]:o[t + 2]].cuda()
    rows = [(part(det, t), gated[t].reshape(-1), part(new, t), part(end, t)) for t in range(N - 1)]
    by_hand = solve_global(rows, split, [g.reshape(-1) for g in gated[N - 1:]], G)
    same_result(got, by_hand)


def test_fill_runs_behind_the_gate_unchanged():
    gate = A.MotionGate(**TIGHT)
    a_pipe, a = run(True, gate=gate)
    b_pipe, b = run(True, gate=gate, fill=3)
    same_result(a, b)
    assert a_pipe.stats == b_pipe.stats and a.filled is None and b.filled is not None
    assert all(np.array_equal(x, y) for x, y in zip(a_pipe.tracks, b_pipe.tracks))
    assert len(b.filled.frames) == N and all(len(i) >= len(t) for i, t in zip(b.filled.ids, b_pipe.tracks))
    with pytest.raises(ValueError, match='gate must be an association.MotionGate'):
        a_pipe.run_global(feeds_of(True), max_gap=G, gate=4.0)
