"""SequencePipeline.run_global - a whole sequence decided by one min-cost flow - on a synthetic sequence with one frame
emptied of detections: its scores are ``sequence_ref.assemble`` of what ``run_offline`` returns, bit for bit; its
assignment is the host oracle's optimum of those scores; ``pipe.tracks`` are ``sequence_ref.ids_of`` of that assignment at
the sequence's own frame indices; a sequence with poses runs the same way; ``window=3`` is refused.  The frames hold
[3, 2, 4, 2, 5, 2] detections: emptying frame 2 leaves an even number of them (14), emptying frame 4 an odd one (13) - the
hand-off packs 4-byte and 8-byte values into one copy, whose offsets depend on that."""
import numpy as np
import pytest
import torch

from association_chain_ref import feasible, lp_route, milp_route, same_assignment
from sequence_ref import assemble, ids_of
from test_lockstep_gpu import KW, shaped
from mmmot_amd import TrackingNet
from mmmot_amd.pipeline import FrameFeed, GlobalResult, SequencePipeline
from mmmot_amd.synth import make_sequence
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu

S = 32        # the smallest crop side the trunk accepts
N, EMPTY = 6, 2
COUNTS = [3, 2, 4, 2, 5, 2]
_MODEL, _FEEDS = [], {}


def model():
    if not _MODEL:
        m = TrackingNet(**KW)
        init_module(m, seed=0)
        _MODEL.append(m.eval().cuda())
    return _MODEL[0]


def feeds_of(poses, empty=EMPTY):
    if (poses, empty) not in _FEEDS:
        frames = make_sequence(N, seed=21, n_pts=4000, det_range=(2, 5), hw=(120, 400), ego=0 if poses else None)
        assert [len(shaped(d)['bbox']) for *_, d in frames] == COUNTS
        _FEEDS[poses, empty] = [FrameFeed(img, sweep, info, shaped(dets, 0 if t == empty else None),
                                          pose=(info['pos'], info['rad']) if poses else None)
                                for t, (img, sweep, info, dets) in enumerate(frames)]
    return _FEEDS[poses, empty]


def run_both(poses, empty):
    feeds = feeds_of(poses, empty)
    kept = [t for t, f in enumerate(feeds) if len(f.dets['bbox'])]
    counts = [len(feeds[t].dets['bbox']) for t in kept]
    assert kept == [t for t in range(N) if t != empty] and sum(counts) == sum(COUNTS) - COUNTS[empty]
    pairs = SequencePipeline(model(), S).run_offline(feeds, frames_per_encode=4, pairs_per_forward=3)
    assert len(pairs) == len(kept) - 1
    pipe = SequencePipeline(model(), S)
    got = pipe.run_global(feeds, frames_per_encode=4, pairs_per_forward=3)
    return feeds, kept, counts, assemble(pairs, counts), pipe, got


def numpy_of(t):
    return (t[0].numpy(), [l[0].numpy() for l in t[1]], t[2].numpy(), t[3].numpy())


@pytest.mark.parametrize('poses,empty', [(False, 2), (True, 2), (False, 4), (True, 4)],
                         ids=['still-even', 'poses-even', 'still-odd', 'poses-odd'])
def test_run_global(poses, empty):
    feeds, kept, counts, want, pipe, got = run_both(poses, empty)
    assert sum(counts) % 2 == (empty == 4)
    assert isinstance(got, GlobalResult) and got.split == counts
    L = sum(counts)
    # the scores: the assembly convention over run_offline's pairs, bit for bit
    sc = numpy_of(got.scores)
    assert sc[0].dtype == np.float32 and sc[0].shape == (L,) and len(sc[1]) == len(counts) - 1
    assert np.array_equal(sc[0], want[0]) and np.array_equal(sc[2], want[2]) and np.array_equal(sc[3], want[3])
    assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(sc[1], want[1]))
    assert all(l.shape == (1, a, b) for l, a, b in zip(got.scores[1], counts[:-1], counts[1:]))
    # the assignment: the optimum of those scores
    a, oa = lp_route(want[0], want[2], want[3], want[1], counts)
    assert same_assignment(a, milp_route(want[0], want[2], want[3], want[1], counts)[0]), 'a tied instance: another seed'
    asg = numpy_of(got.assignment)
    assert feasible(asg, counts) and same_assignment(asg, a)
    assert abs(got.objective - oa) <= 1e-9 * max(1.0, abs(oa))
    # the tracks: trajectory numbers at the sequence's own frame indices, the emptied frame an empty array
    ids = ids_of(asg, counts)
    assert got.n_tracks == int(asg[2].sum()) and len(got.ids) == len(kept)
    assert len(pipe.tracks) == N and pipe.tracks[empty].shape == (0,) and pipe.tracks[empty].dtype == np.int64
    for t, w, g in zip(kept, ids, got.ids):
        assert pipe.tracks[t].dtype == np.int64 and np.array_equal(pipe.tracks[t], w) and np.array_equal(g, w)
    assert pipe.stats['pairs'] == len(kept) - 1 and pipe.stats['encoded_frames'] == N
    assert pipe.stats['empty_frames'] == 1


def test_short_sequences_and_refusals():
    feeds = feeds_of(False)
    with pytest.raises(ValueError, match='window must be 2'):
        SequencePipeline(model(), S, window=3).run_global(feeds)
    with pytest.raises(ValueError, match='>= 1'):
        SequencePipeline(model(), S).run_global(feeds, pairs_per_forward=0)
    pipe = SequencePipeline(model(), S)
    assert pipe.run_global(feeds[EMPTY - 1:EMPTY + 1]) is None  # one frame that holds a detection: nothing is solved
    assert len(pipe.tracks) == 2 and (pipe.tracks[0] == -1).all() and pipe.tracks[1].shape == (0,)
    assert pipe.tracks[0].shape == (len(feeds[EMPTY - 1].dets['bbox']),)
