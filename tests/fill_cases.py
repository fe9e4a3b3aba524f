"""Inputs shared by tests/test_fill_cpu.py and tests/test_fill_gpu.py: small tables for mmmot_fill_tracks and the
"recall comes back" scene."""
import numpy as np

from mmmot_amd import ego, synth

import fill_ref

CALIB = {'calib/R0_rect': synth.KITTI_R0, 'calib/Tr_velo_to_cam': synth.KITTI_TR,
         'calib/Tr_imu_to_velo': synth.KITTI_IMU2VELO}


def random_dets(rng, n):
    """[n, 12] fp32 rows: 2D box, h w l, x y z, rotation_y in [-pi, pi), score"""
    d = np.empty((n, 12), np.float64)
    d[:, 0:2] = rng.uniform(0, 1000, (n, 2))
    d[:, 2:4] = d[:, 0:2] + rng.uniform(20, 200, (n, 2))
    d[:, 4:7] = rng.uniform(1.2, 5.0, (n, 3))
    d[:, 7] = rng.uniform(-30, 30, n)
    d[:, 8] = rng.uniform(-2, 3, n)
    d[:, 9] = rng.uniform(3, 70, n)
    d[:, 10] = rng.uniform(-np.pi, np.pi, n)
    d[:, 11] = rng.uniform(0, 1, n)
    return d.astype(np.float32)


def tables(seqs):
    """seqs: per sequence a list of (frame number, ids of the frame's detections) -> det (random), ids, frame_start,
    frame_no, seq_start as the entry takes them"""
    rng = np.random.default_rng(len(seqs))
    ids = np.asarray([i for s in seqs for _, f in s for i in f], np.int32)
    counts = [len(f) for s in seqs for _, f in s]
    return dict(det=random_dets(rng, len(ids)), ids=ids,
                frame_start=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                frame_no=np.asarray([no for s in seqs for no, _ in s], np.int32),
                seq_start=np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32))


def random_sequence(rng, n_frames, n_tracks, p_miss=0.25, p_unlisted=0.15, p_empty=0.05):
    """a sequence whose tracks miss frames, with rejected detections (-1), frames without detections and frame numbers
    that are not listed; the IDs of a frame are distinct and in random order"""
    seq, no = [], int(rng.integers(0, 5))
    for _ in range(n_frames):
        no += 1 + int(rng.random() < p_unlisted) * int(rng.integers(1, 3))
        if rng.random() < p_empty:
            seq.append((no, []))
            continue
        seen = [t for t in range(n_tracks) if rng.random() >= p_miss]
        row = seen + [-1] * int(rng.integers(0, 3))
        rng.shuffle(row)
        seq.append((no, row))
    return seq


def motion_records(n_frames, max_fill, seed, seq_start=None):
    """xf [F, max_fill + 1, REC] of ``synth.ego_poses``: every record (p, k - 1) whose two frames lie in one sequence"""
    poses = synth.ego_poses(n_frames, seed)
    bounds = [0, n_frames] if seq_start is None else list(seq_start)
    xf = np.zeros((n_frames, max_fill + 1, fill_ref.REC), np.float64)
    for b, e in zip(bounds[:-1], bounds[1:]):
        for p in range(b, e):
            for q in range(p + 1, min(p + max_fill + 2, e)):
                C, Ci, dyaw = ego.box_motion(poses[p], poses[q], CALIB)
                xf[p, q - p - 1, 0:16], xf[p, q - p - 1, 16:32], xf[p, q - p - 1, 32] = C.reshape(-1), Ci.reshape(-1), dyaw
    return xf


def identity_records(n_frames, max_fill):
    xf = np.zeros((n_frames, max_fill + 1, fill_ref.REC), np.float64)
    xf[:, :, 0:16] = xf[:, :, 16:32] = np.eye(4).reshape(-1)
    return xf


# ---- the recall scene: 6 objects over 40 frames, a standing camera, every value linear in the frame number -----------
N_OBJ, N_FRAMES = 6, 40


def scene_row(o, t):
    x1, y1 = 60.0 + 190.0 * o + 1.5 * t, 120.0 + 4.0 * o + 0.5 * t
    return dict(bbox=[x1, y1, x1 + 90.0 + 0.25 * t, y1 + 70.0 + 0.125 * t], dimensions=[4.0 + 0.1 * o, 1.5, 1.75],
                location=[-14.0 + 5.5 * o + 0.0625 * t, 1.5 + 0.015625 * t, 12.0 + 2.0 * o + 0.125 * t],
                rotation_y=0.25 * o - 0.5 + 0.0078125 * t)


def scene_holes(o):
    """the frames object o is missed in: two holes of 1 .. 3 frames, never at its first or last frame"""
    a, b = 4 + 2 * o, 21 + 2 * o
    return set(range(a, a + 1 + o % 3)) | set(range(b, b + 1 + (o + 1) % 3))


def scene(with_holes):
    """(frames, ids): the ground truth (``with_holes`` False) or the tracker's detections with the missed ones dropped;
    ``truncated`` / ``occluded`` 0 so that, read as ground truth, every object counts"""
    frames, ids = [], []
    for t in range(N_FRAMES):
        objs = [o for o in range(N_OBJ) if not (with_holes and t in scene_holes(o))]
        rows = [scene_row(o, t) for o in objs]
        d = {k: np.asarray([r[k] for r in rows], np.float64).reshape((len(rows),) + s)
             for k, s in (('bbox', (4,)), ('dimensions', (3,)), ('location', (3,)), ('rotation_y', ()))}
        d['truncated'], d['occluded'] = np.zeros(len(rows)), np.zeros(len(rows), np.int64)
        frames.append(d)
        ids.append(np.asarray(objs, np.int64))
    return frames, ids


def host_fill(sequences, max_fill=7):
    """``tracks.fill_gaps_batch`` with the restatement standing in for the launches"""
    from mmmot_amd import tracks
    p = tracks.pack_fill(sequences, max_fill)
    res = fill_ref.fill(p['det'], p['ids'], p['frame_start'], p['frame_no'], p['seq_start'], p['xf'], p['wtab'],
                        max_fill, p['sizes'][4])
    return p, res, tracks.unpack_fill(p, fill_ref.block_of(res, p['sizes']))
