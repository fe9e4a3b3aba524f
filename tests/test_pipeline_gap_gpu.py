"""SequencePipeline.run_global(max_gap=G) - the whole sequence decided by one min-cost flow with skip links - on a
synthetic sequence of 12 frames with detections removed from middle frames: ``max_gap=1`` is ``run_global()`` bit for
bit; with ``max_gap=3`` the assembled scores are those built on the host from one ``forward_batch`` call per pair (with
poses: the second frame of a gap pair aligned to the pair's first frame by ``points.align_points``), the assignment and
the IDs are ``associate_sequence_gaps`` of those scores, no crop is encoded again; ``gap_penalty`` shifts the gap blocks
only; an emptied frame is left out and the trajectories go on across it; a short sequence takes the largest gap that
fits."""
import numpy as np
import pytest
import torch

from sequence_gap_ref import gap_feasible, ids_of_gaps
from sequence_ref import assemble
from test_lockstep_gpu import KW, shaped
from mmmot_amd import TrackingNet, ego
from mmmot_amd.association import associate_sequence_gaps, select
from mmmot_amd.pipeline import FrameFeed, GlobalResult, SequencePipeline
from mmmot_amd.points import align_points
from mmmot_amd.synth import make_sequence
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu

S = 32                 # the smallest crop side the trunk accepts
N = 12
MISSES = (3, 5, 6, 8)  # these frames lose their last detection
_MODEL, _FEEDS, _HOST = [], {}, {}


def model():
    if not _MODEL:
        m = TrackingNet(**KW)
        init_module(m, seed=0)
        _MODEL.append(m.eval().cuda())
    return _MODEL[0]


def feeds_of(poses, empty=None):
    if (poses, empty) not in _FEEDS:
        frames = make_sequence(N, seed=21, n_pts=4000, det_range=(2, 5), hw=(120, 400), ego=0 if poses else None)
        keep = lambda t, d: 0 if t == empty else len(d['rotation_y']) - 1 if t in MISSES else None
        _FEEDS[poses, empty] = [FrameFeed(img, sweep, info, shaped(dets, keep(t, dets)),
                                          pose=(info['pos'], info['rad']) if poses else None)
                                for t, (img, sweep, info, dets) in enumerate(frames)]
        assert all(len(f.dets['bbox']) >= 1 or t == empty for t, f in enumerate(_FEEDS[poses, empty]))
    return _FEEDS[poses, empty]


def host_scores(poses, G):
    """(counts, (det, links nested by gap numpy, new, end)) from ONE forward_batch call per pair (f_t, f_{t+g}) on the
    rows of the pipeline's own stage A and trunk; the adjacent pairs assembled by ``sequence_ref.assemble``"""
    if (poses, G) in _HOST:
        return _HOST[poses, G]
    feeds, m = feeds_of(poses), model()
    pipe = SequencePipeline(m, S)
    frames = pipe._offline_frames(feeds, 4, poses)
    counts = [f['n'] for f in frames]

    def pair(t, g):
        a, b = frames[t], frames[t + g]
        second = b['points']
        if poses:
            R, T = ego.pair_motion(feeds[t].pose, feeds[t + g].pose)
            second = align_points([R], [T], feeds[t + g].info['calib/Tr_imu_to_velo'], b['points'])
        plan = m.make_plan([([a['n'], b['n']], pipe._window_split([a, b]))], S)
        with torch.no_grad():
            o = m.forward_batch(plan, None, torch.cat([a['points'], second]),
                                appearance=torch.cat([a['rows'].rows, b['rows'].rows]))[0]
        d, l, n, e = select(o[0], o[1], o[2], o[3], m.test_mode)
        return d.cpu(), [l[0].cpu()], n.cpu(), e.cpu()

    adjacent = [pair(t, 1) for t in range(N - 1)]
    det, links1, new, end = assemble(adjacent, counts)
    links = [links1] + [[pair(t, g)[1][0][0].numpy() for t in range(N - g)] for g in range(2, G + 1)]
    _HOST[poses, G] = counts, (det, links, new, end)
    return _HOST[poses, G]


def nested(res):
    """the (det, [[links] per gap], new, end) numpy of a GlobalResult's scores and assignment"""
    f = lambda t, gaps: (t[0].numpy(), [[l[0].numpy() for l in row] for row in [t[1]] + list(gaps)], t[2].numpy(), t[3].numpy())
    return f(res.scores, res.gap_scores), f(res.assignment, res.gap_assignment)


def same_arrays(a, b):
    fl = lambda r: [r[0], r[2], r[3]] + [l for row in r[1] for l in row]
    return len(fl(a)) == len(fl(b)) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(fl(a), fl(b)))


def test_max_gap_1_is_run_global_bit_for_bit():
    feeds = feeds_of(False)
    a_pipe, b_pipe = SequencePipeline(model(), S), SequencePipeline(model(), S)
    a = a_pipe.run_global(feeds, frames_per_encode=4, pairs_per_forward=3)
    b = b_pipe.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=1, gap_penalty=2.0)
    assert isinstance(b, GlobalResult) and b.max_gap == a.max_gap == 1 and b.gap_scores == [] and b.gap_assignment == []
    assert same_arrays(nested(a)[0], nested(b)[0]) and same_arrays(nested(a)[1], nested(b)[1])
    assert all(np.array_equal(x, y) for x, y in zip(a.ids, b.ids)) and a.n_tracks == b.n_tracks
    assert a.objective == b.objective and a.split == b.split and a_pipe.stats['pairs'] == b_pipe.stats['pairs'] == N - 1
    assert 'gap_pairs' not in b_pipe.stats


@pytest.mark.parametrize('poses', [False, True], ids=['still', 'poses'])
def test_run_global_with_skip_links(poses):
    G = 3
    feeds = feeds_of(poses)
    counts, want = host_scores(poses, G)
    pipe = SequencePipeline(model(), S)
    got = pipe.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=G)
    assert got.max_gap == G and got.split == counts and len(got.gap_scores) == len(got.gap_assignment) == G - 1
    sc, asg = nested(got)
    # the scores: one forward_batch call per pair, bit for bit; the blocks keep the 1 x n_t x n_{t+g} shape
    assert sc[0].dtype == np.float32 and same_arrays(sc, want)
    assert all(l.shape == (1, counts[t], counts[t + g]) for g in (2, 3) for t, l in enumerate(got.gap_scores[g - 2]))
    # the assignment, the IDs and the trajectory count: associate_sequence_gaps of those scores
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    ref = associate_sequence_gaps(t(want[0]), [[t(l) for l in row] for row in want[1]], t(want[2]), t(want[3]), counts,
                                  return_ids=True)
    ref_asg = (ref[0].numpy(), [[l.numpy() for l in row] for row in ref[1]], ref[2].numpy(), ref[3].numpy())
    assert gap_feasible(asg, counts) and same_arrays(asg, ref_asg)
    assert got.n_tracks == ref[5] == int(asg[2].sum())
    for g, r, w, own in zip(got.ids, ref[4], ids_of_gaps(asg, counts), pipe.tracks):
        assert np.array_equal(g, r.numpy()) and np.array_equal(g, w) and np.array_equal(own, g) and own.dtype == np.int64
    # no crop is encoded again: the trunk ran once per frame, as without gaps
    one = SequencePipeline(model(), S)
    one.run_global(feeds, frames_per_encode=4, pairs_per_forward=3)
    assert pipe.stats['encoded_frames'] == one.stats['encoded_frames'] == N
    assert pipe.stats['gap_pairs'] == (N - 2) + (N - 3) and pipe.stats['pairs'] == (N - 1) + pipe.stats['gap_pairs']
    assert one.stats['pairs'] == N - 1


def test_gap_penalty_shifts_the_gap_blocks_only():
    feeds = feeds_of(False)
    counts, want = host_scores(False, 3)
    got = SequencePipeline(model(), S).run_global(feeds, frames_per_encode=5, pairs_per_forward=8, max_gap=3, gap_penalty=0.5)
    sc, _ = nested(got)
    shifted = (want[0], [want[1][0]] + [[l - np.float32(0.5 * (g - 1)) for l in want[1][g - 1]] for g in (2, 3)],
               want[2], want[3])
    assert same_arrays(sc, shifted)
    assert any(l.size for l in sc[1][1]) and not same_arrays(sc, want)


def test_an_emptied_frame_is_left_out_and_crossed():
    empty = 4
    feeds = feeds_of(False, empty)
    pipe = SequencePipeline(model(), S)
    got = pipe.run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=2)
    kept = [t for t in range(N) if t != empty]
    counts = [len(feeds[t].dets['bbox']) for t in kept]
    assert got.split == counts and got.max_gap == 2 and len(got.gap_scores[0]) == len(kept) - 2
    assert pipe.stats['gap_pairs'] == len(kept) - 2 and pipe.stats['empty_frames'] == 1
    sc, asg = nested(got)
    assert gap_feasible(asg, counts)
    # the frames beside the emptied one are neighbours: link block 3 joins the sequence's frames 3 and 5
    assert sc[1][0][empty - 1].shape == (counts[empty - 1], counts[empty]) and sc[1][1][empty - 1].shape == (counts[empty - 1], counts[empty + 1])
    assert len(pipe.tracks) == N and pipe.tracks[empty].shape == (0,) and pipe.tracks[empty].dtype == np.int64
    for t, w in zip(kept, ids_of_gaps(asg, counts)):
        assert np.array_equal(pipe.tracks[t], w)
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    ref = associate_sequence_gaps(t_(sc[0]), [[t_(l) for l in row] for row in sc[1]], t_(sc[2]), t_(sc[3]), counts)
    assert same_arrays(asg, (ref[0].numpy(), [[l.numpy() for l in row] for row in ref[1]], ref[2].numpy(), ref[3].numpy()))


def test_short_sequences_take_the_largest_gap_that_fits_and_refusals():
    feeds = feeds_of(False)
    pipe = SequencePipeline(model(), S)
    got = pipe.run_global(feeds[:3], max_gap=8)
    assert got.max_gap == 2 and len(got.gap_scores) == 1 and len(got.gap_scores[0]) == 1 and pipe.stats['gap_pairs'] == 1
    two = SequencePipeline(model(), S)
    got = two.run_global(feeds[:2], max_gap=3)
    assert got.max_gap == 1 and got.gap_scores == [] and 'gap_pairs' not in two.stats
    for bad in (0, 9):
        with pytest.raises(ValueError, match='max_gap must lie in 1 .. 8'):
            SequencePipeline(model(), S).run_global(feeds, max_gap=bad)
