"""Which kernel serves a call of mmmot_gemm_ares: the "Case -> branch" table of tests/test_lidar_kernels_gpu.py, asked of the
chooser itself.  csrc/ares_choice.h holds the choice as one pure host function without a HIP dependency;
tests/hip_host/ares_choice_main.cpp compiles it with g++ and prints the kernel of every case below.  The expected kernels
are literals, written down from the launcher conditions the three source files held before they became one function:

  K = 64, N <= 512, unless variant 1 with N % 256 == 0:  column-sum pass (mode 2), variant != 3 and (variant 2 or
                                   2T >= 32 n_cu) -> independent-wave; everything else -> weight-resident
  else K = 128, mode 2, variant != 1, N % 512 == 0, ldx / ldsc / ldosc / lddb multiples of 4 and (variant 2 or
                                   T * (N / 512) >= 2 n_cu) -> weights-in-registers
  else N % 256 == 0 -> streaming, otherwise refused (MMMOT_EINVAL)

Two quirks of those conditions are pinned as they are: variant 1 ("the streaming kernel") at K = 64 with N % 256 != 0 stays
with the weight-resident family - the streaming kernel walks 256-channel tiles - and so a launch of 2T >= 32 n_cu half
tiles still gets the independent-wave kernel there; and a register-kernel candidate whose rows are not 16-byte multiples
falls back to the streaming kernel instead of being refused.  Both CU counts: 256 (an MI355X) and 8."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

STREAM, WRES, WAVES, WREG, REFUSE = 'streaming', 'weight-resident', 'independent-wave', 'weights-in-registers', 'refuse'


def case(K, N, mode, variant, T, expect, ldx=None, ldsc=None, ldosc=None, lddb=0):
    return (K, N, mode, variant, T, K + 12 if ldx is None else ldx, K + 12 if ldsc is None else ldsc,
            N + 12 if ldosc is None else ldosc, lddb), expect


def cases(n_cu):
    out = []
    few, many = 1, 16 * n_cu + 3          # tiles: far below and far above every threshold
    for T in (few, many):
        for v in (0, 1, 2, 3):
            for mode in (1, 2, 3):
                out.append(case(128, 256, mode, v, T, STREAM))      # N % 512 != 0: never the register kernel
                out.append(case(64, 768, mode, v, T, STREAM))       # N > 512: not weight-resident
                out.append(case(64, 640, mode, v, T, REFUSE))       # N > 512 and N % 256 != 0
                out.append(case(128, 384, mode, v, T, REFUSE))
            for mode in (1, 3):
                out.append(case(128, 1024, mode, v, T, STREAM))     # the register kernel is a column-sum pass only
        for mode in (1, 2, 3):
            for N in (256, 512):
                out.append(case(64, N, mode, 1, T, STREAM))         # variant 1 with N % 256 == 0
        # weight-resident: the statistics passes under every variant that does not ask for the streaming kernel
        for N in (128, 256, 384, 512):
            for mode in (1, 3):
                for v in (0, 2, 3):
                    out.append(case(64, N, mode, v, T, WRES))
            out.append(case(64, N, 2, 3, T, WRES))
            out.append(case(64, N, 2, 2, T, WAVES))
        for N in (128, 384):                                         # variant 1 with N % 256 != 0: not the streaming kernel
            for mode in (1, 3):
                out.append(case(64, N, mode, 1, T, WRES))
        for N in (512, 1024, 1536, 4096):
            out.append(case(128, N, 2, 2, T, WREG))
            out.append(case(128, N, 2, 1, T, STREAM if N % 256 == 0 else REFUSE))
    # K = 64 column-sum pass, automatic: independent waves from 2T = 32 n_cu on
    for v in (0, 1):                                                 # (variant 1 at N = 128: see the docstring)
        out.append(case(64, 128, 2, v, 14 if n_cu > 1 else 1, WRES))
        out.append(case(64, 128, 2, v, 16 * n_cu - 1, WRES))
        out.append(case(64, 128, 2, v, 16 * n_cu, WAVES))
        out.append(case(64, 128, 2, v, 16 * n_cu + 3, WAVES))
    out.append(case(64, 128, 2, 3, 16 * n_cu + 3, WRES))
    # K = 128 column-sum pass, automatic (variant 3: as 0): the register kernel from T * nh = 2 n_cu on
    for v in (0, 3):
        out.append(case(128, 1024, 2, v, n_cu - 1, STREAM))          # T * nh = 2 n_cu - 2
        out.append(case(128, 1024, 2, v, n_cu, WREG))
        out.append(case(128, 1024, 2, v, n_cu + 1, WREG))
        out.append(case(128, 512, 2, v, 2 * n_cu - 1, STREAM))
        out.append(case(128, 512, 2, v, 2 * n_cu, WREG))
        out.append(case(128, 1536, 2, v, (2 * n_cu + 2) // 3 - 1, STREAM))
        out.append(case(128, 1536, 2, v, (2 * n_cu + 2) // 3, WREG))
    # the register kernel's 16-byte pieces: rows that are no multiple of 4 floats go to the streaming kernel
    for v, T in ((2, 14), (0, many)):
        out.append(case(128, 512, 2, v, T, WREG, lddb=524))
        out.append(case(128, 512, 2, v, T, STREAM, lddb=525))
        out.append(case(128, 512, 2, v, T, STREAM, ldosc=526))
        out.append(case(128, 512, 2, v, T, STREAM, ldsc=141))
        out.append(case(128, 512, 2, v, T, STREAM, ldx=142))
        out.append(case(128, 512, 2, v, T, WREG, ldx=128, ldsc=128, ldosc=512))
    return out


@pytest.fixture(scope='module')
def chooser(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('ares_choice') / 'ares_choice_host')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(HERE, 'hip_host', 'ares_choice_main.cpp'),
                           '-o', exe])
    return exe


@pytest.mark.parametrize('n_cu', [256, 8])
def test_the_kernel_of_every_case(chooser, tmp_path, n_cu):
    table = cases(n_cu)
    path = str(tmp_path / 'cases.txt')
    with open(path, 'w') as f:
        for (K, N, mode, v, T, ldx, ldsc, ldosc, lddb), _ in table:
            f.write('%d %d %d %d %d %d %d %d %d %d\n' % (K, N, mode, v, n_cu, T, ldx, ldsc, ldosc, lddb))
    r = subprocess.run([chooser, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    got = r.stdout.decode().split()
    assert len(got) == len(table)
    bad = ['K%d N%d mode %d variant %d T %d ldx %d ldsc %d ldosc %d lddb %d: %s, expected %s' % (c + (g, e))
           for (c, e), g in zip(table, got) if g != e]
    assert not bad, '\n'.join(bad)
    assert {e for _, e in table} == {STREAM, WRES, WAVES, WREG, REFUSE}
