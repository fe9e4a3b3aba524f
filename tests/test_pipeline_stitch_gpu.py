"""``SequencePipeline.run_global(stitch=)``: the stitcher runs behind the solve, the filling and
the smoothing, on the smoothed sequence with its velocities, and is the calls by hand; ``stitch=None`` is the run without
the argument.  The test model's random weights link little, so this covers the hand-off; the stitching behind it is
covered by tests/test_stitch_gpu.py."""
import numpy as np
import pytest

from mmmot_amd import tracks
from mmmot_amd.pipeline import FrameFeed, SequencePipeline
from mmmot_amd.synth import make_sequence

pytestmark = pytest.mark.gpu


def feeds_of():
    from test_lockstep_gpu import shaped
    frames = make_sequence(8, seed=23, n_pts=4000, det_range=(2, 5), hw=(120, 400), ego=1)
    return [FrameFeed(img, sweep, info, shaped(dets, 0 if t == 5 else None), pose=(info['pos'], info['rad']))
            for t, (img, sweep, info, dets) in enumerate(frames)]


def test_run_global_stitch():
    from test_fill_gpu import same_filled
    from test_pipeline_gap_gpu import S, model
    from test_smooth_cpu import same_smoothed
    from test_stitch_gpu import same_stitched
    feeds = feeds_of()
    kw = dict(frames_per_encode=4, pairs_per_forward=3, max_gap=3, fill=7)
    sm = tracks.TrackSmoother()
    # a wide stitcher, so that some of the one-row tracks the random weights leave are joined: any two boxes up to 30 m
    # apart are candidates (one-row tracks have no velocity: the static radius)
    sk = tracks.TrackStitcher(max_dt=7, max_speed=0.0, slack=30.0, min_rows=2)
    plain, none, stitched = (SequencePipeline(model(), S) for _ in range(3))
    a = plain.run_global(feeds, smooth=sm, **kw)
    b = none.run_global(feeds, smooth=sm, stitch=None, **kw)
    c = stitched.run_global(feeds, smooth=sm, stitch=sk, **kw)
    # stitch=None is the run without the argument, and the stitcher changes nothing of what came before it
    for r, pipe in ((b, none), (c, stitched)):
        assert pipe.stats == plain.stats and r.objective == a.objective and r.n_tracks == a.n_tracks
        assert all(np.array_equal(x, y) for x, y in zip(plain.tracks, pipe.tracks))
        assert all(np.array_equal(x, y) for x, y in zip(a.ids, r.ids))
        for x, y in zip(a.scores, r.scores):
            x, y = (list(v) if isinstance(v, (list, tuple)) else [v] for v in (x, y))
            assert all(np.array_equal(np.asarray(p), np.asarray(q), equal_nan=True) for p, q in zip(x, y))
        same_filled(a.filled, r.filled)
        same_smoothed(a.smoothed, r.smoothed)
    assert a.stitched is None and b.stitched is None and c.stitched is not None
    # the calls by hand
    poses = [f.pose for f in feeds]
    ego = dict(poses=poses, calib=feeds[0].info)
    st = tracks.stitch_tracks(c.smoothed.frames, c.smoothed.ids, velocity=c.smoothed.velocity, stitcher=sk, **ego)
    same_stitched(c.stitched, st)
    n_rows = sum(len(i) for i in c.smoothed.ids)
    assert sum(len(i) for i in st.ids) == n_rows and st.info['tracks'] >= 2
    print('tracks %d, stitches %d, rows changed %d' % (st.info['tracks'], st.info['stitches'], st.info['rows_changed']))
    if st.info['stitches'] > 0:
        filled = tracks.fill_gaps(c.filled.frames, st.ids, max_fill=7, **ego)
        same_filled(c.stitched.filled, filled)
        seen = [np.concatenate([~m, np.zeros(len(m2) - len(m), bool)]) for m, m2 in zip(c.filled.filled, filled.filled)]
        same_smoothed(c.stitched.smoothed, tracks.smooth_tracks(filled.frames, filled.ids, observed=seen, smoother=sm, **ego))
    else:
        assert c.stitched.filled is None and c.stitched.smoothed is None
    # without smooth the filled sequence is stitched, without velocities; without fill the solved one
    d = SequencePipeline(model(), S).run_global(feeds, stitch=sk, **kw)
    same_stitched(d.stitched, tracks.stitch_tracks(d.filled.frames, d.filled.ids, stitcher=sk, **ego))
    assert d.smoothed is None and d.stitched.smoothed is None
    e = SequencePipeline(model(), S).run_global(feeds, frames_per_encode=4, pairs_per_forward=3, max_gap=3, stitch=sk)
    same_stitched(e.stitched, tracks.stitch_tracks([f.dets for f in feeds], stitched.tracks, stitcher=sk, **ego))
    assert e.filled is None and e.stitched.filled is None
    with pytest.raises(ValueError, match='TrackStitcher'):
        plain.run_global(feeds, stitch=dict(max_dt=5))
