"""numpy float64 statement of the arithmetic of mmmot_align_points (include/mmmot_hip.h, csrc/align_points.hip): every
product and every sum is one numpy float64 operation (rounded on its own, no FMA), sums in k order 0..3, one rounding to
fp32 at the end.  The GPU tests compare the kernel with this for arbitrary shapes; tests/test_ego_cpu.py compares this
with the reference's align_points (tests/golden/ego_align.npz)."""
import numpy as np


def _affine(q, M):
    """rows (x, y, z, 1) x the 4x4 M, columns 0..2: ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + M[3][j]"""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([((x * M[0, j] + y * M[1, j]) + z * M[2, j]) + M[3, j] for j in range(3)], axis=1)


def _step(q, R, T):
    """q @ R.T + T: ((x*R[j][0] + y*R[j][1]) + z*R[j][2]) + T[j]"""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([((x * R[j, 0] + y * R[j, 1]) + z * R[j, 2]) + T[j] for j in range(3)], axis=1)


def align_points(R, T, imu2velo, points):
    """points fp32 [Q, 3|4] -> fp32 [Q, 3|4]; R, T: the reference's lists, applied from last to first"""
    points = np.asarray(points, dtype=np.float32)
    imu2velo = np.asarray(imu2velo)
    A = np.asarray(np.linalg.inv(imu2velo.T), dtype=np.float64)
    B = np.asarray(imu2velo.T, dtype=np.float64)
    q = _affine(points[:, :3].astype(np.float64), A)
    for i in range(len(R)):
        q = _step(q, np.asarray(R[-i - 1], dtype=np.float64), np.asarray(T[-i - 1], dtype=np.float64).reshape(-1))
    out = points.copy()
    out[:, :3] = _affine(q, B).astype(np.float32)
    return out


def ulp_report(got, want):
    """(largest distance in fp32 ulps of `want`, number of coordinates that differ at all, number of coordinates)"""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulps = diff / np.spacing(np.abs(want)).astype(np.float64)
    return float(ulps.max()) if ulps.size else 0.0, int((got != want).sum()), int(got.size)


def assert_close_to_reference(pairs, what=''):
    """The criterion of the alignment tests over ``pairs`` = [(got, want), ...]: every coordinate within 1 fp32 ulp, and
    at most 1 coordinate in 10 000 of all the pairs' coordinates different at all.  Returns (worst ulp distance, number
    of coordinates that differ, number of coordinates)."""
    worst, ndiff, n = 0.0, 0, 0
    for got, want in pairs:
        w, d, k = ulp_report(got, want)
        worst, ndiff, n = max(worst, w), ndiff + d, n + k
    assert worst <= 1.0, '%s: %.2f ulp' % (what, worst)
    assert ndiff * 10000 <= n, '%s: %d of %d coordinates differ' % (what, ndiff, n)
    return worst, ndiff, n
