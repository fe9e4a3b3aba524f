"""NumPy restatement of the dropout mask of the LiDAR encoder: Philox4x32-10 with 64-bit
products and 32-bit masks, and the mask the device kernels generate in registers.

    w = philox4x32_10(counter = (r, c >> 2, 0, 0), key = (seed & 0xffffffff, seed >> 32))
    keep(r, c) = w[c & 3] >= threshold
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays"""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2   # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def threshold_of(p):
    return min(int(round(float(p) * 2.0 ** 32)), MASK32)


def words(seed, R, C, row0=0):
    """uint32 [R][C]: the word every element's keep decision compares against the threshold"""
    assert C % 4 == 0
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = np.arange(row0, row0 + R, dtype=np.uint64)[:, None]
    q = np.arange(C // 4, dtype=np.uint64)[None, :]
    z = np.zeros((R, C // 4), dtype=np.uint64)
    w = philox4x32_10((r + z, q + z, z, z), (seed & MASK32, seed >> 32))
    return np.stack(w, axis=-1).reshape(R, C)


def mask(seed, threshold, R, C):
    """bool [R][C]: keep(r, c)"""
    return words(seed, R, C) >= np.uint32(threshold)
