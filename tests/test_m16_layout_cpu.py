"""The M16 form of the trunk's patch kernel, modelled in numpy (no GPU).

The kernel reads the operand fragments of v_mfma_f32_32x32x16_f16 exactly as before and turns each pair (k-step 0,
k-step 1) into two operands of v_mfma_f32_16x16x32_f16 with one v_permlane16_swap_b32 per VGPR
(csrc/patch_fragments.inc).  Modelled here:

  32x32x16 operand   lane l holds row l % 32 and the 8 k-values of lane half l / 32 (4 VGPRs of two fp16 each)
  the swap           the odd 16-lane rows of the first register change places with the even ones of the second
  16x16x32           D[i][j] = sum_g sum_t A[16 g + i][t] * B[16 g + j][t] over lanes (g = k-group l / 16);
                     element r of lane l = D[4 (l / 16) + r][l % 16]

and shown: the swapped pairs give the exact 32 x 32 x 32 product of a slab (integer-valued operands: no rounding); the
epilogue's index functions (csrc/patch_m16.h, compiled with g++) put every accumulator element on its own place of
the tile with the pooling quads intact and write the staging area without bank conflicts; the per-layer rule
(mmmot_patch_m16, csrc/patch_choice.h) names the VGG layers it is meant to name."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# the trunk's layers (Cin, Cout) -> M16?  conv1_1 / conv1_2 run in the fused first launch (no M16 form)
VGG_RULE = {
    (64, 128): False,
    (128, 128): False,    # measured: gain inside twice the spread of the 32x32x16 form
    (128, 256): True,
    (256, 256): True,
    (256, 512): True,
    (512, 512): False,    # faster, but its worst element (K = 4608) passes the 2e-6 bound of a layer's output
}


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp('m16_layout')
    exe = str(d / 'm16_layout_host')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(HERE, 'hip_host', 'm16_layout_main.cpp'),
                           '-o', exe])

    def run(*args):
        r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        return [tuple(int(v) for v in line.split()) for line in r.stdout.decode().splitlines()]

    run.dir = d
    return run


@pytest.fixture(scope='module')
def index(host):
    """[si][sj][lane][r] -> (row, col, quad, slot, quad(slot))"""
    t = np.array(host('index'), dtype=np.int64)
    assert t.shape == (2 * 2 * 64 * 4, 5)
    return t.reshape(2, 2, 64, 4, 5)


def fragment_32x32x16(X, j):
    """[64 lanes][4 VGPRs][2]: k-step j of the 32-row block X[32][32]"""
    lane = np.arange(64)
    k = 16 * j + 8 * (lane // 32)[:, None] + np.arange(8)[None, :]
    return X[(lane % 32)[:, None], k].reshape(64, 4, 2)


def permlane16_swap(v0, v1):
    """one VGPR each ([64 lanes][2]): odd rows of v0 <-> even rows of v1"""
    a, b = v0.reshape(4, 16, -1).copy(), v1.reshape(4, 16, -1).copy()
    for odd, even in ((1, 0), (3, 2)):
        a[odd], b[even] = v1.reshape(4, 16, -1)[even], v0.reshape(4, 16, -1)[odd]
    return a.reshape(v0.shape), b.reshape(v1.shape)


def swap_pair(f0, f1):
    """four swaps: fragments of k-step 0 / 1 -> operands of rows 0-15 / 16-31"""
    o0, o1 = np.empty_like(f0), np.empty_like(f1)
    for w in range(4):
        o0[:, w], o1[:, w] = permlane16_swap(f0[:, w], f1[:, w])
    return o0, o1


def mfma_16x16x32(a, b):
    """operands [64][4][2] -> [64 lanes][4 elements]"""
    A, B = a.reshape(4, 16, 8), b.reshape(4, 16, 8)  # [g][i][t]
    D = np.einsum('git,gjt->ij', A, B)
    lane = np.arange(64)
    return D[4 * (lane // 16)[:, None] + np.arange(4)[None, :], (lane % 16)[:, None]]


def mfma_32x32x16(a, b):
    """operands [64][4][2] -> [64 lanes][16 elements] (row (e & 3) + 8 (e >> 2) + 4 (l / 32), column l % 32)"""
    A, B = a.reshape(2, 32, 8), b.reshape(2, 32, 8)
    D = np.einsum('git,gjt->ij', A, B)
    lane, e = np.arange(64)[:, None], np.arange(16)[None, :]
    return D[(e & 3) + 8 * (e >> 2) + 4 * (lane // 32), lane % 32]


def test_swap_semantics_on_tagged_lanes():
    """the register rows after the swap are the ones the kernel's comment states"""
    tag = lambda j: (100 * j + np.arange(64) // 16)[:, None] * np.ones((1, 2), dtype=np.int64)  # (k-step, 16-lane row)
    r0, r1 = permlane16_swap(tag(0), tag(1))
    assert [int(v) for v in r0[::16, 0]] == [0, 100, 2, 102]   # rows 0-15:  (j0,h0) (j1,h0) (j0,h1) (j1,h1)
    assert [int(v) for v in r1[::16, 0]] == [1, 101, 3, 103]   # rows 16-31: the same


def test_swapped_pairs_give_the_exact_product(index):
    rng = np.random.default_rng(16)
    for _ in range(4):
        X = rng.integers(-8, 9, size=(32, 32)).astype(np.int64)   # activations [pixel][channel]
        Wt = rng.integers(-8, 9, size=(32, 32)).astype(np.int64)  # weights [output channel][channel]
        want = X @ Wt.T
        # today's form: two 32x32x16 steps
        lane, e = np.arange(64)[:, None], np.arange(16)[None, :]
        C32 = np.zeros((32, 32), dtype=np.int64)
        acc = sum(mfma_32x32x16(fragment_32x32x16(X, j), fragment_32x32x16(Wt, j)) for j in range(2))
        C32[(e & 3) + 8 * (e >> 2) + 4 * (lane // 32), lane % 32 + 0 * e] = acc
        assert np.array_equal(C32, want)
        # M16: the same fragments, swapped, four 16x16x32 sub-tiles placed by the header's index functions
        a = swap_pair(fragment_32x32x16(X, 0), fragment_32x32x16(X, 1))
        b = swap_pair(fragment_32x32x16(Wt, 0), fragment_32x32x16(Wt, 1))
        C = np.full((32, 32), np.iinfo(np.int64).min)
        for si in range(2):
            for sj in range(2):
                d = mfma_16x16x32(a[si], b[sj])
                C[index[si, sj, :, :, 0], index[si, sj, :, :, 1]] = d
        assert np.array_equal(C, want)


def test_epilogue_index_is_a_bijection_with_quads_intact(index):
    row, col, quad, slot, back = (index[..., k] for k in range(5))
    cells = (row * 32 + col).reshape(-1)
    assert sorted(cells.tolist()) == list(range(32 * 32))          # every element of the 32 x 32 product exactly once
    assert np.array_equal(row, 4 * quad + np.arange(4))            # a lane's four registers = one pooling quad, in order
    assert np.array_equal(back, quad)                              # store loop: staged slot -> quad
    per_si = {si: sorted(set(slot[si].reshape(-1).tolist())) for si in range(2)}
    assert sorted(per_si[0] + per_si[1]) == list(range(8))         # the slots of a block are a permutation of its quads


@pytest.mark.parametrize('cld', [64 + 4, 128 + 4])
def test_staging_writes_are_conflict_free(index, cld):
    """ds_write_b32: two groups of 32 lanes, bank = dword address mod 32"""
    row, col, slot = index[..., 0], index[..., 1], index[..., 3]
    for si in range(2):
        for sj in range(2):
            for grp in (slice(0, 32), slice(32, 64)):
                pooled = (slot[si, sj, grp, 0] * cld + col[si, sj, grp, 0]) % 32
                assert len(set(pooled.tolist())) == 32
                for r in range(4):
                    plain = (row[si, sj, grp, r] * cld + col[si, sj, grp, r]) % 32
                    assert len(set(plain.tolist())) == 32


def test_rule_names_the_vgg_layers(host):
    layers = sorted(VGG_RULE)
    path = str(host.dir / 'layers.txt')
    with open(path, 'w') as f:
        for cin, cout in layers:
            f.write('%d %d 0 0\n' % (cin, cout))
        for cin, cout in layers:       # the hq8 arithmetic and the fused first launch have no M16 form
            f.write('%d %d 1 0\n' % (cin, cout))
        f.write('64 64 0 1\n')
        f.write('160 256 0 0\n')       # an odd number of 32-channel slabs: the alternating K loop needs an even one
    got = [g[0] for g in host('rule', path)]
    n = len(layers)
    assert dict(zip(layers, (bool(g) for g in got[:n]))) == VGG_RULE
    assert got[n:] == [0] * (n + 2)
