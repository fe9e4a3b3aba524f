"""Which kernel serves a call of mmmot_gemm_rows, and with which launch geometry: the "case -> branch" table of
tests/test_wide_kernels_gpu.py, asked of the chooser itself.  csrc/wide_choice.h holds the choice as one pure host function
without a HIP dependency; tests/hip_host/wide_choice_main.cpp compiles it with g++ and prints the plan
(wide, nh, ntn, nitems, grid) of every case below.  The expected plans are literals, written down from the conditions
mmmot_gemm_wide_try and gw_launch (csrc/gemm_wide.hip) held before they became one function:

  wide kernel:  variant != 1, w_hl16, K in {256, 512}, N % 256 == 0, amode PAIR or NORM_RELU, no dbias, no colsum, no
                activation, PAIR: ldf % 4 == 0, K <= ldf, pair_uniform32; NORM_RELU: ldsc >= K; Y: ldy % 4 == 0; a device;
                variant 0: items = ((T + 1) / 2) * (N / 256) >= n_cu / 2
  NH = 2:       variant 4, or variant 0 and items >= 24 n_cu
  geometry:     ntn = N / 256, nu = ceil(T / NH), nitems = ceil(nu / 8) * 8 ntn,
                grid = floor((2 / NH) n_cu / (8 ntn)) * 8 ntn, at least 8 ntn, at most nitems
  grid limit:   n > 0: grid = min(grid, n) rounded down to whole groups of 8 ntn, at least 8 ntn
  tile kernel:  ntn = N / 128 (N % 128 == 0) or N / 64, nitems = grid = T * ntn, nh = 0

Quirks of those conditions, pinned as they are: ldy is looked at only when there is a Y (a statistics-only launch with
ldy % 4 != 0 stays on the wide kernel); ldsc counts for NORM_RELU only and ldf / pair_uniform32 for PAIR only; N = 384
passes the first N test (N % 128) and falls through at the second (N % 256); variants 3 and 4 ignore both size
thresholds (T = 1 runs the wide kernel); the items of the thresholds count PAIRS of row tiles whichever NH is chosen, so
an odd T reaches a threshold one tile earlier than the even T below it; the grid limit never changes which kernel runs;
no device (n_cu = 0) is the tile kernel.  Both CU counts: 256 (an MI355X) and 8."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

PLAIN, NORM, PAIR = 0, 1, 2
BASE = dict(variant=3, limit=0, T=20, N=512, K=512, amode=PAIR, w_hl16=1, dbias=0, colsum=0, act=0, ldf=512, uni=1,
            ldsc=512, ldy=512, Y=1)
ORDER = ('variant', 'n_cu', 'limit', 'T', 'N', 'K', 'amode', 'w_hl16', 'dbias', 'colsum', 'act', 'ldf', 'uni', 'ldsc',
         'ldy', 'Y')


def case(expect, **kw):
    d = dict(BASE)
    d.update(kw)
    return d, expect


def tile(ntn, T=20):
    return (0, 0, ntn, T * ntn, T * ntn)


def cases(n_cu):
    big = n_cu == 256
    out = []
    # ---- the eligible layer (T = 20, N = 512: ntn = 2, groups of 16 items), both amodes, every variant
    for amode in (PAIR, NORM):
        out.append(case((1, 1, 2, 48, 48 if big else 16), amode=amode))
        out.append(case((1, 2, 2, 32, 32 if big else 16), amode=amode, variant=4))
        out.append(case(tile(4), amode=amode, variant=1))
        # automatic: items = 10 * 2 = 20, below n_cu / 2 = 128 on 256 CUs, above 4 on 8 CUs (and below 24 * 8)
        out.append(case(tile(4) if big else (1, 1, 2, 48, 16), amode=amode, variant=0))
    # ---- every condition flipped on its own
    for v in (3, 4, 0):
        T = 20 if v else 600                                    # variant 0: items = 600, wide on both CU counts
        flip = lambda ntn=4, **kw: out.append(case(tile(ntn, T), variant=v, T=T, **kw))
        flip(w_hl16=0)
        for K in (128, 384, 1024):
            flip(K=K, ldf=1024)
            flip(K=K, amode=NORM, ldsc=1024)
        flip(ntn=1, N=128)
        flip(ntn=3, N=384)                                      # (passes N % 128, stopped by N % 256)
        flip(ntn=1, N=128, amode=NORM)
        flip(ntn=3, N=384, amode=NORM)
        flip(amode=PLAIN)
        for amode in (PAIR, NORM):
            flip(amode=amode, dbias=1)
            flip(amode=amode, colsum=1)
            flip(amode=amode, act=1)
            flip(amode=amode, act=2)
            flip(amode=amode, ldy=514)                          # ldy % 4 with Y
            flip(amode=amode, ldy=513)
        flip(ldf=514)                                           # ldf % 4
        flip(ldf=513)
        flip(K=512, ldf=256)                                    # K > ldf
        flip(K=512, ldf=508)
        flip(uni=0)
        flip(amode=NORM, ldsc=508)                              # ldsc < K
        flip(amode=NORM, K=512, ldsc=256)
    # ---- and what does NOT disqualify (the quirks of the docstring)
    w3 = (1, 1, 2, 48, 48 if big else 16)
    out.append(case(w3, ldy=514, Y=0))                          # ldy % 4 without Y
    out.append(case(w3, amode=NORM, ldy=513, Y=0))
    out.append(case(w3, ldsc=0))                                # PAIR: ldsc is not looked at
    out.append(case(w3, amode=NORM, ldf=3, uni=0))              # NORM_RELU: ldf and pair_uniform32 are not
    out.append(case(w3, amode=NORM, ldsc=524))
    out.append(case(w3, ldf=1024))
    out.append(case(w3, K=256, ldf=256))
    out.append(case(w3, K=256, ldf=512))
    out.append(case(w3, K=256, amode=NORM, ldsc=256))
    out.append(case((1, 1, 2, 16, 16), T=1))                    # variants 3 / 4 ignore the small-launch rule
    out.append(case((1, 2, 2, 16, 16), T=1, variant=4))
    # ---- the two thresholds of the automatic choice: items = ((T + 1) / 2) * (N / 256), one below and exactly at, odd
    # and even T
    if big:
        for amode in (PAIR, NORM):
            # N = 1024 (4 column tiles): n_cu / 2 = 128 = 32 * 4; 24 n_cu = 6144 = 1536 * 4
            out.append(case(tile(8, 61), variant=0, amode=amode, N=1024, T=61))                  # 31 pairs: 124
            out.append(case(tile(8, 62), variant=0, amode=amode, N=1024, T=62))                  # 31 pairs: 124
            out.append(case((1, 1, 4, 256, 256), variant=0, amode=amode, N=1024, T=63))          # 32 pairs: 128
            out.append(case((1, 1, 4, 256, 256), variant=0, amode=amode, N=1024, T=64))
            out.append(case((1, 1, 4, 12288, 512), variant=0, amode=amode, N=1024, T=3069))      # 1535 pairs: 6140
            out.append(case((1, 1, 4, 12288, 512), variant=0, amode=amode, N=1024, T=3070))
            out.append(case((1, 2, 4, 6144, 256), variant=0, amode=amode, N=1024, T=3071))       # 1536 pairs: 6144
            out.append(case((1, 2, 4, 6144, 256), variant=0, amode=amode, N=1024, T=3072))
        # N = 256 (one column tile)
        out.append(case(tile(2, 253), variant=0, N=256, T=253))                                  # 127
        out.append(case(tile(2, 254), variant=0, N=256, T=254))
        out.append(case((1, 1, 1, 256, 256), variant=0, N=256, T=255))                           # 128
        out.append(case((1, 1, 1, 256, 256), variant=0, N=256, T=256))
        out.append(case((1, 1, 1, 12288, 512), variant=0, N=256, T=12286))                       # 6143
        out.append(case((1, 2, 1, 6144, 256), variant=0, N=256, T=12287))                        # 6144
    else:
        for amode in (PAIR, NORM):
            # N = 256: n_cu / 2 = 4, 24 n_cu = 192
            out.append(case(tile(2, 5), variant=0, amode=amode, N=256, T=5))                     # 3
            out.append(case(tile(2, 6), variant=0, amode=amode, N=256, T=6))
            out.append(case((1, 1, 1, 8, 8), variant=0, amode=amode, N=256, T=7))                # 4
            out.append(case((1, 1, 1, 8, 8), variant=0, amode=amode, N=256, T=8))
            out.append(case((1, 1, 1, 384, 16), variant=0, amode=amode, N=256, T=381))           # 191
            out.append(case((1, 1, 1, 384, 16), variant=0, amode=amode, N=256, T=382))
            out.append(case((1, 2, 1, 192, 8), variant=0, amode=amode, N=256, T=383))            # 192
            out.append(case((1, 2, 1, 192, 8), variant=0, amode=amode, N=256, T=384))
        # N = 512: 4 = 2 pairs * 2, 192 = 96 pairs * 2
        out.append(case(tile(4, 2), variant=0, T=2))                                             # 2
        out.append(case((1, 1, 2, 16, 16), variant=0, T=3))                                      # 4
        out.append(case((1, 1, 2, 384, 16), variant=0, T=190))                                   # 190
        out.append(case((1, 2, 2, 192, 16), variant=0, T=191))                                   # 192
    # thresholds are for variant 0 only: the same sizes under variants 3 and 4
    out.append(case((1, 1, 1, 8, 8), variant=3, N=256, T=5))
    out.append(case((1, 2, 1, 8, 8), variant=4, N=256, T=5))
    out.append(case((1, 1, 4, 12288, 512 if big else 32), variant=3, N=1024, T=3072))
    out.append(case((1, 2, 4, 32, 32), variant=4, N=1024, T=7))
    # ---- geometry: nitems in groups of 8 ntn items; the automatic grid of 256 CUs (512 / 256 workgroups) is above every
    # nitems here, that of 8 CUs is two groups (NH = 1, ntn = 1) or one
    groups = {1: {1: 1, 7: 1, 8: 1, 9: 2, 16: 2, 17: 3}, 2: {1: 1, 7: 1, 8: 1, 9: 1, 16: 1, 17: 2}}
    grid8 = {(1, 1): {1: 1, 7: 1, 8: 1, 9: 2, 16: 2, 17: 2}}
    one = {1: 1, 7: 1, 8: 1, 9: 1, 16: 1, 17: 1}
    for nh in (1, 2):
        for ntn in (1, 2, 4):
            for T in (1, 7, 8, 9, 16, 17):
                g = groups[nh][T] if big else grid8.get((nh, ntn), one)[T]
                for amode in (PAIR, NORM):
                    out.append(case((1, nh, ntn, groups[nh][T] * 8 * ntn, g * 8 * ntn), variant=2 + nh, N=256 * ntn, T=T,
                                    amode=amode, ldy=1024))
    # ---- grid limits: 0, 1, 8 ntn, 8 ntn + 3, 16 ntn, far above; T = 100
    #   N = 256, NH = 2: 50 pairs -> 56 items; N = 512, NH = 1: 104 -> 208 items; N = 1024, NH = 1: 416 items
    for limit, g in ((0, 56 if big else 8), (1, 8), (8, 8), (11, 8), (16, 16 if big else 8), (100000, 56 if big else 8)):
        out.append(case((1, 2, 1, 56, g), variant=4, N=256, T=100, limit=limit))
    for limit, g in ((0, 208 if big else 16), (1, 16), (16, 16), (19, 16), (32, 32 if big else 16), (40, 32 if big else 16),
                     (100000, 208 if big else 16)):
        out.append(case((1, 1, 2, 208, g), variant=3, N=512, T=100, limit=limit))
        out.append(case((1, 1, 2, 208, g), variant=3, N=512, T=100, limit=limit, amode=NORM))
    for limit, g in ((0, 416 if big else 32), (1, 32), (32, 32), (35, 32), (64, 64 if big else 32), (100000, 416 if big else 32)):
        out.append(case((1, 1, 4, 416, g), variant=3, N=1024, T=100, limit=limit, ldy=1024))
    # a limit above nitems, and a limit on a launch of one group: nitems still caps
    out.append(case((1, 1, 2, 16, 16), T=5, limit=64))
    # the limit caps the automatic choice's grid as well, and never changes the kernel
    # (301 pairs of tiles: NH = 1 on 256 CUs, beyond 24 * 8 on 8 CUs)
    out.append(case((1, 1, 1, 608, 8) if big else (1, 2, 1, 304, 8), variant=0, N=256, T=601, limit=8))
    out.append(case(tile(4), variant=1, limit=16))
    out.append(case(tile(4), uni=0, limit=16))
    return out


@pytest.fixture(scope='module')
def chooser(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('wide_choice') / 'wide_choice_host')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(HERE, 'hip_host', 'wide_choice_main.cpp'),
                           '-o', exe])
    return exe


def ask(chooser, tmp_path, table, n_cu):
    path = str(tmp_path / 'cases.txt')
    with open(path, 'w') as f:
        for d, _ in table:
            f.write(' '.join(str(dict(d, n_cu=n_cu)[k]) for k in ORDER) + '\n')
    r = subprocess.run([chooser, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(got) == len(table)
    return got


@pytest.mark.parametrize('n_cu', [256, 8])
def test_the_plan_of_every_case(chooser, tmp_path, n_cu):
    table = cases(n_cu)
    got = ask(chooser, tmp_path, table, n_cu)
    bad = ['%s: (wide, nh, ntn, nitems, grid) = %s, expected %s' % (
        ' '.join('%s=%s' % (k, d[k]) for k in d if d[k] != BASE[k]) or 'base', g, e) for (d, e), g in zip(table, got) if g != e]
    assert not bad, '\n'.join(bad)
    assert {(e[0], e[1]) for _, e in table} == {(0, 0), (1, 1), (1, 2)}


def test_no_device_is_the_tile_kernel(chooser, tmp_path):
    table = [case(tile(4), variant=v) for v in (0, 1, 3, 4)]
    assert ask(chooser, tmp_path, table, 0) == [e for _, e in table]
