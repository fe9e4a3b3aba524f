"""csrc/crop_augment.hip compiled for the HOST (tests/hip_host/common.h: one OS thread per work-item, a barrier for
__syncthreads) and run as a stand-alone program under AddressSanitizer and UBSan: the kernel's index arithmetic - LDS
staging, aligned dword reads at the ends of the tensor, the clamp of an out-of-range table - is checked access by access
without a GPU, and its pixels against the NumPy restatement bit for bit.  Small sides only: a work-item is a thread here."""
import os
import shutil
import struct
import subprocess

import numpy as np

import augment_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'mmmot_amd', 'csrc')


def test_kernel_source_on_the_host_under_sanitizers(tmp_path):
    for src in (os.path.join(CSRC, 'crop_augment.hip'), os.path.join(CSRC, 'crop_coeff.h'),
                os.path.join(HERE, 'hip_host', 'common.h'), os.path.join(HERE, 'hip_host', 'crop_augment_main.cpp')):
        shutil.copy(src, str(tmp_path))  # side by side: "common.h" resolves to the host stand-in
    exe = str(tmp_path / 'crop_augment_host')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-x', 'c++', str(tmp_path / 'crop_augment_main.cpp'),
                           '-o', exe, '-lpthread'])
    rng = np.random.default_rng(18)
    cases = []
    for S in (1, 7, 32, 33):  # 32: four pixels per work-item, 2 row tiles; 33: an odd side, 3 row tiles
        rows = [(0, 0, S, S, 1), (S - 1, S - 1, 1, 1, 0), (0, S // 2, S, 1, 1), (S // 2, 0, 1, S, 0)]
        for _ in range(3):
            h, w = int(rng.integers(1, S + 1)), int(rng.integers(1, S + 1))
            rows.append((int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w, int(rng.integers(0, 2))))
        params = np.asarray(rows, dtype=np.int32)
        crops = rng.integers(0, 256, (len(rows), S, S, 3), dtype=np.uint8)
        u8, f32 = augment_ref.augment(crops, params)
        cases.append((S, 1, params, crops, u8, f32))
    S = 32  # tables the host check refuses: the kernel's clamp keeps every access inside the buffers all the same
    bad = np.asarray([(-5, -5, 1000, 1000, 7), (S, S, 1, 1, 0), (S - 1, S - 1, 50, 50, -1), (0, 0, 0, 0, 1),
                      (-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 1), (S + 100, -100, S, S, 1)], dtype=np.int32)
    z = np.zeros((len(bad), S, S, 3), dtype=np.uint8)
    cases.append((S, 0, bad, z, z, np.zeros((len(bad), 3, S, S), np.float32)))
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as f:
        f.write(struct.pack('i', len(cases)))
        for S, check, params, crops, u8, f32 in cases:
            f.write(struct.pack('iii', len(params), S, check))
            for a in (crops, params, u8, f32.astype(np.float32)):
                f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    assert b'%d cases, 0 bad' % len(cases) in r.stdout
