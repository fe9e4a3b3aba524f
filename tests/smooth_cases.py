"""Inputs shared by tests/test_smooth_cpu.py and tests/test_smooth_gpu.py: tables for mmmot_smooth_tracks on top of
tests/fill_cases.py, per-frame ego-motion records, single tracks with chosen measurements, and the noisy scene."""
import numpy as np

from mmmot_amd import ego, synth, tracks

import fill_cases
import fill_ref
import smooth_ref

PARAMS = dict(smooth_ref.DEFAULT)  # the defaults of tracks.TrackSmoother, restated


def frame_records(n_frames, seed, seq_start=None):
    """xf0 [F, REC] of ``synth.ego_poses``: the record of frame p is ``ego.box_motion(pose_a, pose_p)``, a the first
    frame of p's sequence (the identity for a itself)"""
    poses = synth.ego_poses(n_frames, seed)
    bounds = [0, n_frames] if seq_start is None else [int(v) for v in seq_start]
    xf0 = identity_records(n_frames)
    for b, e in zip(bounds[:-1], bounds[1:]):
        for p in range(b + 1, e):
            C, Ci, dyaw = ego.box_motion(poses[b], poses[p], fill_cases.CALIB)
            xf0[p, 0:16], xf0[p, 16:32], xf0[p, 32] = C.reshape(-1), Ci.reshape(-1), dyaw
    return xf0


def identity_records(n_frames):
    xf0 = np.zeros((n_frames, fill_ref.REC), np.float64)
    xf0[:, 0:16] = xf0[:, 16:32] = np.eye(4).reshape(-1)
    return xf0


def single_track(no, loc=None, yaw=None, dims=None):
    """the tables of ONE track, one detection per listed frame: frame numbers ``no``, location [m, 3], yaw [m],
    dimensions h w l [m, 3] (defaults: zeros / ones)"""
    m = len(no)
    det = np.zeros((m, 12), np.float64)
    det[:, 2:4] = 50.0
    det[:, 4:7] = 1.0 if dims is None else np.asarray(dims, np.float64).reshape(m, 3)
    det[:, 7:10] = 0.0 if loc is None else np.asarray(loc, np.float64).reshape(m, 3)
    det[:, 10] = 0.0 if yaw is None else np.asarray(yaw, np.float64).reshape(m)
    det[:, 11] = 0.5
    return dict(det=det.astype(np.float32), ids=np.full(m, 3, np.int32), frame_start=np.arange(m + 1, dtype=np.int32),
                frame_no=np.asarray(no, np.int32), seq_start=np.asarray([0, m], np.int32))


def ref(t, observed=None, xf0=None, **prm):
    return smooth_ref.smooth(t['det'], t['ids'], t['frame_start'], t['frame_no'], t['seq_start'], observed, xf0, **prm)


def random_mask(t, seed, p=0.3):
    return (np.random.default_rng(seed).random(len(t['ids'])) >= p).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the noisy scene: fill_cases.scene with seeded Gaussian noise on location, size and yaw ---------------------------
NOISE_SEED, SIGMA_LOC, SIGMA_DIM, SIGMA_YAW = 7, 0.2, 0.1, 0.1


def noisy_scene(with_holes=True, seed=NOISE_SEED):
    """(frames, ids) of ``fill_cases.scene`` with N(0, sigma) noise on every location, dimension and yaw; the noise of an
    object in a frame does not depend on ``with_holes``"""
    frames, ids = fill_cases.scene(with_holes)
    rng = np.random.default_rng(seed)
    noise = rng.normal(size=(fill_cases.N_FRAMES, fill_cases.N_OBJ, 7))
    out = []
    for t, (d, fid) in enumerate(zip(frames, ids)):
        d = dict(d)
        n = noise[t, fid]
        d['location'] = d['location'] + SIGMA_LOC * n[:, 0:3]
        d['dimensions'] = d['dimensions'] + SIGMA_DIM * n[:, 3:6]
        d['rotation_y'] = d['rotation_y'] + SIGMA_YAW * n[:, 6]
        out.append(d)
    return out, ids


def host_smooth(sequences, smoother=None):
    """``tracks.smooth_tracks_batch`` with the restatement standing in for the launches"""
    p = tracks.pack_smooth(sequences, smoother)
    prm = dict(zip(smooth_ref.PARAMS, p['smoother'].params()), yaw_flip=p['smoother'].yaw_flip)
    res = smooth_ref.smooth(p['det'], p['ids'], p['frame_start'], p['frame_no'], p['seq_start'], p['observed'], p['xf0'],
                            **prm)
    return p, res, tracks.unpack_smooth(p, smooth_ref.block_of(res, p['sizes']))


def location_error(frames, ids, rows=None):
    """mean Euclidean distance of the boxes' locations to the noise-free scene, over the rows ``rows[t]`` selects
    (default: every row with an ID)"""
    err = []
    for t, (d, fid) in enumerate(zip(frames, ids)):
        for j, o in enumerate(np.asarray(fid)):
            if o >= 0 and (rows is None or rows[t][j]):
                err.append(np.linalg.norm(np.asarray(d['location'][j]) - fill_cases.scene_row(int(o), t)['location']))
    return float(np.mean(err)), len(err)
