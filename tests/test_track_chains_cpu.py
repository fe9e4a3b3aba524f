"""The ID bookkeeping of windows of 2 .. 8 frames without a GPU: the index restatement of tests/tracking_chain_ref.py
against the fixtures the reference itself produced (tests/golden/track_chain_ids_*.npz,
tools/gen_golden_track_chains.py) and, on two-frame windows, against tests/tracking_ref.py on the pair fixtures; the host
helpers of mmmot_amd.tracks; the window schedule; the operator's table refusals; the new entry point in the library."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import tracking_ref
from tracking_chain_ref import ChainTracker, check_final, check_window, load_fixture, tracks_of_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'track_chain_ids_*.npz')))
NAMES = [os.path.basename(f)[len('track_chain_ids_'):-4] for f in FIXTURES]
PAIR_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'track_ids_*.npz')))


def fixture(name):
    return load_fixture(os.path.join(GOLDEN, 'track_chain_ids_%s.npz' % name))


def test_fixture_set():
    assert set(NAMES) == {'kitti3', 't8', 'roles5', 'roles3', 'waves', 'n300'}
    limit = max(os.path.getsize(f) for f in PAIR_FIXTURES)
    for f in FIXTURES:
        assert os.path.getsize(f) <= limit
        assert set(np.load(f).files) == {'chains', 'frame_idx', 'blocks', 'emit_len', 'emit_ids', 'frame_start',
                                         'last_id', 'frames_id_len', 'frames_id', 'frames_id_frame'}  # data only


@pytest.mark.parametrize('path', FIXTURES, ids=NAMES)
def test_restatement_reproduces_reference(path):
    wins, z = load_fixture(path)
    tr, tracks = ChainTracker(), {}
    for w in wins:
        ids, start, stored = tr.window(w['det'], w['links'], w['new'], w['split'], w['frames'])
        check_window(w, ids, start, tr.last_id)
        if stored:
            tracks.update(list(zip(w['frames'], ids))[start:])
    check_final(z, tracks)


def quirk(w):
    return w['frame_start'] == 1 and not (w['det'][w['split'][0]:w['split'][0] + w['split'][1]] == 1).any()


def test_fixtures_cover_the_cases():
    """what the fixtures must contain, read off the reference's own results"""
    k, z = fixture('kitti3')
    assert len(k) == 19 and all(w['T'] == 3 and all(10 <= n <= 12 for n in w['split']) for w in k)
    assert len(set(f for w in k for f in w['frames'])) == 40
    gaps = [i for i in range(1, len(k)) if k[i]['frames'][0] != k[i - 1]['frames'][-1]]
    assert gaps and all(k[i]['frame_start'] == 0 for i in gaps)
    for name in ('kitti3', 'roles5', 'roles3'):
        wins, z = fixture(name)
        # the quirk: frames >= 2 keep detections that never reach frames_id, and the next window starts anew
        q = [i for i, w in enumerate(wins[:-1]) if quirk(w) and (w['det'][sum(w['split'][:2]):] == 1).any()]
        assert q, name
        for i in q:
            assert wins[i + 1]['frame_start'] == 0 and wins[i + 1]['frames'][0] == wins[i]['frames'][-1]
    t8, _ = fixture('t8')
    assert [w['T'] for w in t8] == [8, 8, 8] and all(2 <= n <= 6 for w in t8 for n in w['split'])
    for w in t8:  # linked (new == 0) kept detections in the last frame of a T = 8 window
        last = slice(sum(w['split'][:-1]), None)
        assert ((w['det'][last] == 1) & (w['new'][last] == 0)).any()
    r5, _ = fixture('roles5')
    r3, _ = fixture('roles3')
    assert [w['T'] for w in r5] == [5, 5, 5, 5, 2] and all(w['T'] == 3 for w in r3)
    assert not (r5[0]['det'][:r5[0]['split'][0]] == 1).any() and r5[0]['frame_start'] == 0
    roles = {(t == 0, t == w['T'] - 1) for w in r5 + r3 for t, n in enumerate(w['split']) if n == 0}
    assert roles == {(True, False), (False, False), (False, True)}  # an empty frame first, in the middle, last
    assert any(not (w['det'][sum(w['split'][:-1]):] == 1).any() and w['split'][-1] > 0 for w in r5 + r3)
    wv, _ = fixture('waves')
    assert {n for w in wv for n in w['split']} == {1, 63, 64, 65, 128, 129} and wv[0]['T'] == 4
    n3, _ = fixture('n300')
    assert [w['split'] for w in n3] == [[300, 257, 300], [300, 131, 260]]
    assert all((w['det'][256:w['split'][0]] == 1).any() for w in n3)


@pytest.mark.parametrize('path', PAIR_FIXTURES, ids=[os.path.basename(f)[:-4] for f in PAIR_FIXTURES])
def test_two_frame_windows_equal_the_pair_restatement(path):
    pairs, _ = tracking_ref.load_fixture(path)
    a, b = tracking_ref.Tracker(), ChainTracker()
    for p in pairs:
        ids0, ids1, start = a.pair(p['det'], p['link'], p['new'], p['N'], p['M'], p['f0'], p['f1'])
        ids, s, stored = b.window(p['det'], [p['link']], p['new'], [p['N'], p['M']], [p['f0'], p['f1']])
        assert np.array_equal(ids[0], ids0) and np.array_equal(ids[1], ids1) and s == start
        assert (a.last_id, a.stored) == (b.last_id, b.stored) and np.array_equal(a.stored_ids, b.stored_ids)
        assert stored == int(not start or (ids1 >= 0).any())


def test_restatement_rejects_infeasible():
    det = np.ones(4, np.float32)
    new = np.array([1, 1, 1, 0], np.float32)
    links = [np.array([[1.]]), np.zeros((1, 2))]
    links[1][0, 0] = 1
    with pytest.raises(ValueError):  # the kept last-frame detection 1 is neither new nor linked
        ChainTracker().window(det, links, np.array([1, 0, 0, 0], np.float32), [1, 1, 2], [0, 1, 2])
    ChainTracker().window(det, links, np.array([1, 0, 0, 1], np.float32), [1, 1, 2], [0, 1, 2])


def test_tracks_of_windows_on_a_fixture():
    wins, z = fixture('roles3')
    frames = sorted({f for w in wins for f in w['frames']})
    assert frames == list(range(len(frames)))
    counts = {f: n for w in wins for f, n in zip(w['frames'], w['split'])}
    tracks = tracks_of_windows([(w['det'], w['links'], w['new']) for w in wins], [w['frames'] for w in wins],
                               [counts[f] for f in frames])
    check_final(z, dict(enumerate(tracks)))


def test_split_and_merge_on_hand_made_buffers():
    from mmmot_amd.tracks import TrackingError, merge_chain_tracks, split_chain_ids
    splits = [[2, 0, 1], [1, 2]]
    flat = np.array([5, -1, 6, 0, 6, 1,   6, -1, -1, 1, 6, 0,   0], np.int32)
    a, b = split_chain_ids(flat, splits)
    assert [x.tolist() for x in a[0]] == [[5, -1], [], [6]] and a[1:] == (0, 6, 1)
    assert [x.tolist() for x in b[0]] == [[6], [-1, -1]] and b[1:] == (1, 6, 0)
    assert all(x.dtype == np.int64 for x in a[0] + b[0])
    tracks, seen = [None] * 4, []
    merge_chain_tracks(tracks, [0, 1, 2], *a[:2], a[3], on_tracks=lambda t, i: seen.append(t))
    assert [None if x is None else x.tolist() for x in tracks] == [[5, -1], [], [6], None] and seen == [0, 1, 2]
    merge_chain_tracks(tracks, [2, 3], *b[:2], b[3], on_tracks=lambda t, i: seen.append(t))   # stored = 0: nothing
    assert tracks[2].tolist() == [6] and tracks[3] is None and seen == [0, 1, 2]
    merge_chain_tracks(tracks, [2, 3], b[0], 1, 1)   # frame_start = 1: frame 0 of the window is not written again
    assert tracks[2].tolist() == [6] and tracks[3].tolist() == [-1, -1]
    for flags in (1, 2, 3):
        flat[-1] = flags
        with pytest.raises(TrackingError):
            split_chain_ids(flat, splits)


def test_window_schedule():
    from mmmot_amd.tracks import window_starts
    want3 = {1: [], 2: [(0, 2)], 3: [(0, 3)], 7: [(0, 3), (2, 3), (4, 3)], 8: [(0, 3), (2, 3), (4, 3), (6, 2)]}
    want8 = {1: [], 2: [(0, 2)], 3: [(0, 3)], 7: [(0, 7)], 8: [(0, 8)]}
    for n in (1, 2, 3, 7, 8):
        assert window_starts(n, 3) == want3[n] and window_starts(n, 8) == want8[n]
    assert window_starts(16, 8) == [(0, 8), (7, 8), (14, 2)]
    assert window_starts(5, 2) == [(0, 2), (1, 2), (2, 2), (3, 2)]
    for n in range(2, 30):  # every frame is covered, neighbours share exactly one frame, no window has fewer than 2
        for T in range(2, 9):
            w = window_starts(n, T)
            assert w[0][0] == 0 and w[-1][0] + w[-1][1] == n and all(2 <= k <= T for _, k in w)
            assert all(a + k - 1 == b for (a, k), (b, _) in zip(w[:-1], w[1:]))
    for bad in (1, 9):
        with pytest.raises(ValueError):
            window_starts(5, bad)


def tables(rows, fidx):
    import torch
    return (torch.tensor([r + [0] * (11 - len(r)) for r in rows], dtype=torch.int32),
            torch.tensor([f + [0] * (8 - len(f)) for f in fidx], dtype=torch.int32))


def test_meta_kernel_gives_the_output_size_and_refuses_bad_tables():
    import torch
    import mmmot_amd.torch_ops  # noqa: F401
    from mmmot_amd.torch_ops import TRACK_STATE_INTS, track_chain_layout
    chains, fidx = tables([[3, 0, 0, 3, 0, 4], [2, 7, 0, 4, 2]], [[0, 1, 2], [2, 3]])
    blocks = torch.empty(3 * 7 + 3 * 6 + 8, dtype=torch.float32, device='meta')
    state = torch.empty(TRACK_STATE_INTS, dtype=torch.int32, device='meta')
    ids = torch.ops.mmmot.track_chain_ids(blocks, chains, fidx, state, 0)
    assert ids.shape == (7 + 3 + 6 + 3,) and ids.dtype == torch.int32 and ids.device.type == 'meta'
    total, off, need = track_chain_layout(chains, fidx, 3 * 7 + 3 * 6 + 8)
    assert (total, off.tolist(), need) == (19, [0, 21], 4)

    def refused(rows, f, n_blocks=None, chains=None, fidx=None):
        c, x = tables(rows, f)
        with pytest.raises(ValueError):
            track_chain_layout(c if chains is None else chains, x if fidx is None else fidx, n_blocks)
        with pytest.raises(ValueError):
            torch.ops.mmmot.track_chain_ids(blocks, c if chains is None else chains, x if fidx is None else fidx, state, 0)
    refused([[1, 0, 0, 3]], [[0]])                               # T outside 2 .. 8
    refused([[9, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]], [[0] * 8])
    refused([[2, 0, 0, 3, 513]], [[0, 1]])                       # n_t outside 0 .. 512
    refused([[2, 0, 0, -1, 3]], [[0, 1]])
    refused([[3, 0, 0, 3, 2, 2]], [[0, 1, -1]])                  # a negative frame index
    refused([[2, 0, 0, 3, 2]], [[0, 1]], chains=chains.to(torch.int64)[:1])      # dtype
    refused([[2, 0, 0, 3, 2]], [[0, 1]], chains=chains[:1, :10])                 # shape
    refused([[2, 0, 0, 3, 2]], [[0, 1]], fidx=fidx)                              # frame rows for another B
    refused([[2, 0, 0, 3, 2]], [[0, 1]], fidx=fidx[:1, :2].contiguous())
    with pytest.raises(ValueError):                                              # blocks shorter than the table reads
        track_chain_layout(chains, fidx, 3 * 7 + 3 * 6 + 7)
    # entries behind frame T-1 are ignored
    c, x = tables([[2, 0, 0, 3, 2, 999]], [[0, 1, -5]])
    assert track_chain_layout(c, x)[0] == 8


def test_library_exports_track_chain_ids_and_header_declares_it():
    from mmmot_amd import _lib
    path = _lib.build()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', path]).decode()
    assert re.search(r'\bT mmmot_track_chain_ids\b', syms)
    with open(os.path.join(ROOT, 'include', 'mmmot_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint mmmot_track_chain_ids\(const float\* blocks, const int\* chains,', header)
    assert len(_lib.SIGNATURES['mmmot_track_chain_ids']) == 9 and 'track_ids.hip' in _lib.SOURCES


def test_abi_version_and_argument_checks():
    from mmmot_amd import _lib
    _lib.build()
    lib = _lib.load()
    assert lib.mmmot_abi_version() == 10
    # rejected before any launch: null pointers, no windows, max_n out of range
    assert lib.mmmot_track_chain_ids(None, None, None, None, 1, 12, None, None, None) == -1
    for k in range(6):
        args = [8, 8, 8, 8, 1, 12, 8, 8, None]
        args[k if k < 4 else k + 2] = None
        assert lib.mmmot_track_chain_ids(*args) == -1
    assert lib.mmmot_track_chain_ids(8, 8, 8, 8, 0, 12, 8, 8, None) == -1
    assert lib.mmmot_track_chain_ids(8, 8, 8, 8, 1, 513, 8, 8, None) == -1
    assert lib.mmmot_track_chain_ids(8, 8, 8, 8, 1, -1, 8, 8, None) == -1


def test_pipeline_window_argument_checks():
    import torch
    from mmmot_amd.pipeline import SequencePipeline
    lin = torch.nn.Linear(1, 1)
    for bad in (1, 9):
        with pytest.raises(ValueError, match='window'):
            SequencePipeline(lin, overlap=False, window=bad)
    assert SequencePipeline(lin, overlap=False).window == 2
    assert SequencePipeline(lin, overlap=False, window=5).window == 5
