"""The ID bookkeeping without a GPU: the index restatement of tests/tracking_ref.py against the fixtures the reference
itself produced (tests/golden/track_ids_*.npz, tools/gen_golden_tracks.py), the host writer of the KITTI result file
against the reference writer's text, and the new entry point in the cross-compiled library and the header."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from tracking_ref import Tracker, check_pair, load_fixture, tracks_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'track_ids_*.npz')))
NAMES = [os.path.basename(f)[len('track_ids_'):-4] for f in FIXTURES]


def test_fixture_set():
    assert set(NAMES) == {'kitti', 'start', 'n64', 'n12x100', 'n300'}
    for f in FIXTURES + [os.path.join(GOLDEN, 'tracks_kitti_0001.txt')]:
        assert os.path.getsize(f) < 1 << 20


@pytest.mark.parametrize('path', FIXTURES, ids=NAMES)
def test_restatement_reproduces_reference(path):
    pairs, z = load_fixture(path)
    tr = Tracker()
    for p in pairs:
        ids0, ids1, start = tr.pair(p['det'], p['link'], p['new'], p['N'], p['M'], p['f0'], p['f1'])
        check_pair(p, ids0, ids1, start, tr.last_id)


def test_fixtures_cover_the_cases():
    """what the fixtures must contain, read off the reference's own results"""
    pairs, z = load_fixture(os.path.join(GOLDEN, 'track_ids_kitti.npz'))
    assert len(pairs) == 38 and all(10 <= p['N'] <= 12 and 10 <= p['M'] <= 12 for p in pairs)
    assert len(set(z['frame_idx'].reshape(-1).tolist())) == 40
    # a frame-index gap: a pair after the first that starts again with both frames (case b) although pairs before it stored
    gaps = [i for i in range(1, len(pairs)) if pairs[i]['f0'] != pairs[i - 1]['f1']]
    assert gaps and all(pairs[i]['frame_start'] == 0 for i in gaps)
    # the quirk: a case-c pair whose second frame keeps nothing, followed by a case-b pair on consecutive frames
    quirk = [i for i, p in enumerate(pairs) if p['frame_start'] == 1 and not (p['det'][p['N']:] == 1).any()]
    assert quirk and all(pairs[i + 1]['frame_start'] == 0 and pairs[i + 1]['f0'] == pairs[i]['f1'] for i in quirk)
    # rejected by one pair and kept by the next: a fresh ID for a first-frame detection, and holes in the ID sequence
    holes = 0
    for a, b in zip(pairs[:-1], pairs[1:]):
        if b['frame_start'] == 1:
            holes += int(((a['det'][a['N']:] != 1) & (b['det'][:b['N']] == 1)).sum())
    assert holes > 0
    used = set(z['frames_id'].tolist())
    assert len(used) < int(z['last_id'][-1]) + 1
    start, _ = load_fixture(os.path.join(GOLDEN, 'track_ids_start.npz'))
    assert not (start[0]['det'][:start[0]['N']] == 1).any() and start[0]['frame_start'] == 0
    assert any(p['M'] == 0 for p in start) and any(p['N'] == 0 for p in start)
    assert all((p['N'], p['M']) == (64, 64) for p in load_fixture(os.path.join(GOLDEN, 'track_ids_n64.npz'))[0])
    assert {(p['N'], p['M']) for p in load_fixture(os.path.join(GOLDEN, 'track_ids_n12x100.npz'))[0]} == {(12, 100), (100, 12)}


def test_tracks_of_matches_reference_frames_id():
    """the per-frame list (last emission stands) against the reference's final frames_id, on the gapless sequences"""
    for name in ('start', 'n64', 'n12x100', 'n300'):
        pairs, z = load_fixture(os.path.join(GOLDEN, 'track_ids_%s.npz' % name))
        counts = [pairs[0]['N']] + [p['M'] for p in pairs]
        tracks = tracks_of([(p['det'], p['link'], p['new']) for p in pairs], counts)
        o = 0
        for f, n in zip(z['frames_id_frame'], z['frames_id_len']):
            assert np.array_equal(tracks[f][tracks[f] >= 0], z['frames_id'][o:o + n]), (name, f)
            o += n


def test_restatement_rejects_infeasible():
    det = np.array([1, 1, 1], np.float32)
    with pytest.raises(ValueError):  # the kept second-frame detection is neither new nor linked
        Tracker().pair(det, np.zeros((2, 1)), np.array([1, 1, 0], np.float32), 2, 1, 0, 1)


def kitti_dets():
    pairs, z = load_fixture(os.path.join(GOLDEN, 'track_ids_kitti.npz'))
    frames = sorted(set(z['frame_idx'].reshape(-1).tolist()))
    keys = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y')
    dets = [{k: z['dets_%d_%s' % (f, k)] for k in keys} for f in frames]
    return pairs, frames, dets


def test_write_kitti_tracks_matches_reference_text(tmp_path):
    from mmmot_amd.tracks import write_kitti_tracks
    pairs, frames, dets = kitti_dets()
    slot = {f: i for i, f in enumerate(frames)}
    tr = Tracker()
    ids = [np.full(len(d['bbox']), -1, np.int64) for d in dets]
    for p in pairs:
        ids0, ids1, start = tr.pair(p['det'], p['link'], p['new'], p['N'], p['M'], p['f0'], p['f1'])
        if not start:
            ids[slot[p['f0']]] = ids0
        ids[slot[p['f1']]] = ids1
    out = tmp_path / '0001.txt'
    write_kitti_tracks(str(out), dets, ids, frame_idx=frames)
    with open(os.path.join(GOLDEN, 'tracks_kitti_0001.txt'), 'rb') as f:
        want = f.read()
    assert out.read_bytes() == want and len(want) > 10000


def test_write_kitti_tracks_pipeline_dets(tmp_path):
    """the dicts the pipeline holds carry boxes only: the format's "unknown" values fill the rest"""
    from mmmot_amd.tracks import write_kitti_tracks
    d = {'bbox': np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float64), 'dimensions': np.array([[1, 2, 3], [4, 5, 6]]),
         'location': np.zeros((2, 3)), 'rotation_y': np.array([0.5, -0.5])}
    out = tmp_path / 't.txt'
    write_kitti_tracks(str(out), [d], [np.array([-1, 7])])
    assert out.read_text() == ('0 7 Car -1 -1 -10 5.0000 6.0000 7.0000 8.0000 5.0000 6.0000 4.0000 0.0000 0.0000 0.0000 '
                               '-0.5000 0.9000')


def test_library_exports_track_ids_and_header_declares_it():
    from mmmot_amd import _lib
    path = _lib.build()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', path]).decode()
    assert re.search(r'\bT mmmot_track_ids\b', syms)
    with open(os.path.join(ROOT, 'include', 'mmmot_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint mmmot_track_ids\(const float\* blocks, const int\* pairs,', header)
    assert len(_lib.SIGNATURES['mmmot_track_ids']) == 9 and 'track_ids.hip' in _lib.SOURCES


def test_abi_version_and_argument_checks():
    from mmmot_amd import _lib
    _lib.build()
    lib = _lib.load()
    assert lib.mmmot_abi_version() == 10
    # rejected before any launch: null pointers, no pairs, max_nm out of range
    assert lib.mmmot_track_ids(None, None, None, None, 1, 12, None, None, None) == -1
    assert lib.mmmot_track_ids(8, 8, 8, 8, 0, 12, 8, 8, None) == -1
    assert lib.mmmot_track_ids(8, 8, 8, 8, 1, 513, 8, 8, None) == -1
    assert lib.mmmot_track_ids(8, 8, 8, 8, 1, -1, 8, 8, None) == -1


def test_track_needs_associate():
    import torch
    from mmmot_amd.pipeline import SequencePipeline
    with pytest.raises(ValueError, match='associate'):
        SequencePipeline(torch.nn.Linear(1, 1), track=True, associate=False)


def test_meta_kernel_gives_the_output_size():
    import torch
    import mmmot_amd.torch_ops  # noqa: F401
    from mmmot_amd.torch_ops import TRACK_STATE_INTS
    pairs = torch.tensor([[3, 4, 0, 0], [4, 0, 7, 12]], dtype=torch.int32)
    fidx = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)
    blocks = torch.empty(3 * 7 + 12 + 3 * 4, dtype=torch.float32, device='meta')
    state = torch.empty(TRACK_STATE_INTS, dtype=torch.int32, device='meta')
    ids = torch.ops.mmmot.track_ids(blocks, pairs, fidx, state, 0)
    assert ids.shape == (3 + 4 + 2 + 4 + 0 + 2,) and ids.dtype == torch.int32 and ids.device.type == 'meta'


@pytest.mark.parametrize('frame_start', [0, 1])
def test_merge_tracks_is_the_stored_two_frame_merge_of_windows(frame_start):
    from mmmot_amd.tracks import merge_chain_tracks, merge_tracks
    ids0, ids1 = np.array([3, -1, 4]), np.array([-1, -1])   # a second frame that keeps nothing is written all the same
    got, want = [[None] * 4, []], [[None] * 4, []]
    merge_tracks(got[0], 2, ids0, ids1, frame_start, on_tracks=lambda t, i: got[1].append((t, i.tolist())))
    merge_chain_tracks(want[0], [1, 2], [ids0, ids1], frame_start, stored=1,
                       on_tracks=lambda t, i: want[1].append((t, i.tolist())))
    assert got[1] == want[1] == ([(2, [-1, -1])] if frame_start else [(1, [3, -1, 4]), (2, [-1, -1])])
    assert len(got[0]) == len(want[0]) == 4
    for a, b in zip(got[0], want[0]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert got[0][0] is None and got[0][3] is None and (got[0][1] is None) == bool(frame_start) and got[0][2] is ids1
    merge_tracks(got[0], 2, ids0, ids1, frame_start)   # without a callback
