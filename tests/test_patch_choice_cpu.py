"""Which instantiation of the trunk's patch kernel serves a layer, and on how many workgroups: the "case -> branch" table of
tests/test_trunk_kernels_gpu.py, asked of the chooser itself.  csrc/patch_choice.h holds the choice as one pure host
function without a HIP dependency; tests/hip_host/patch_choice_main.cpp compiles it with g++ and prints (channels per
tile, block edge, tiles, workgroups) of every case below.  The expected values are literals, written down from the
conditions conv3x3_hl16_patch.hip held before they became one function:

  block edge   16 when H > 8 or W > 8; else 4 when H <= 4 and W <= 4 and the min-block knob is not 8; else 8
  tile width   64 when Cout % 128 != 0 (whatever is forced); else the forced width; else 64 when
               0.85 eff(2 i) > eff(i), i = ceil(blocks / blocks per tile) * Cout / 128 and
               eff(n) = n / (ceil(n / n_cu) * n_cu), the fill of the last wave of workgroups
  grid         n_cu rounded down to 8, capped by the grid-limit knob (> 0) and by the tiles rounded up to 8

With every knob at 0 a launch is the parent's launch: the same instantiation on the same grid.  Both CU counts: 256 (an
MI355X) and 8."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# (L, H, W, Cout): (tile width, block edge, tiles, workgroups) with every knob at 0
AUTO = {
    256: {
        (33, 24, 40, 128): (128, 16, 198, 200),
        (512, 16, 16, 128): (128, 16, 512, 256),
        (600, 4, 4, 512): (128, 4, 152, 152),
        (70, 4, 4, 512): (64, 4, 40, 40),
        (40, 16, 16, 256): (64, 16, 160, 160),
        (1, 16, 16, 512): (64, 16, 8, 8),
        (9, 4, 4, 512): (64, 4, 8, 8),
        (5, 8, 8, 128): (64, 8, 4, 8),
        (12, 20, 12, 256): (64, 16, 96, 96),
        (3, 25, 25, 64): (64, 16, 12, 16),      # Cout % 128 != 0
        (7, 16, 16, 192): (64, 16, 21, 24),
    },
    8: {                                          # eff() is 1 whenever the tiles are a multiple of 8: 128-channel tiles
        (33, 24, 40, 128): (128, 16, 198, 8),    # eff(198) = 198 / 200 against 0.85 eff(396) = 0.85 * 396 / 400
        (512, 16, 16, 128): (128, 16, 512, 8),
        (600, 4, 4, 512): (128, 4, 152, 8),
        (70, 4, 4, 512): (64, 4, 40, 8),         # eff(20) = 20 / 24 = 0.83 against 0.85 eff(40) = 0.85
        (40, 16, 16, 256): (128, 16, 80, 8),
        (1, 16, 16, 512): (64, 16, 8, 8),        # eff(4) = 0.5
        (9, 4, 4, 512): (64, 4, 8, 8),
        (5, 8, 8, 128): (64, 8, 4, 8),           # eff(2) = 0.25 against 0.85 eff(4) = 0.425
        (12, 20, 12, 256): (128, 16, 48, 8),
        (3, 25, 25, 64): (64, 16, 12, 8),
        (7, 16, 16, 192): (64, 16, 21, 8),
    },
}

# forced widths at 256 CUs: (L, H, W, Cout, forced): expected
FORCED = {
    (70, 4, 4, 512, 128): (128, 4, 20, 24),
    (70, 4, 4, 512, 64): (64, 4, 40, 40),
    (600, 4, 4, 512, 64): (64, 4, 304, 256),
    (600, 4, 4, 512, 128): (128, 4, 152, 152),
    (33, 24, 40, 128, 64): (64, 16, 396, 256),
    (5, 8, 8, 128, 128): (128, 8, 2, 8),
    (1, 16, 16, 512, 128): (128, 16, 4, 8),
    (3, 25, 25, 64, 128): (64, 16, 12, 16),      # Cout % 128 != 0: 64 whatever is forced
    (7, 16, 16, 192, 128): (64, 16, 21, 24),
    (7, 16, 16, 192, 0): (64, 16, 21, 24),
    (7, 16, 16, 192, 64): (64, 16, 21, 24),
}

# block-edge boundaries: (H, W, min block): edge
EDGES = {(4, 4, 0): 4, (4, 4, 4): 4, (5, 4, 0): 8, (4, 5, 0): 8, (8, 8, 0): 8, (9, 8, 0): 16, (8, 9, 0): 16, (4, 4, 8): 8,
         (1, 1, 0): 4, (1, 1, 8): 8, (9, 8, 8): 16, (3, 4, 0): 4, (7, 8, 8): 8, (20, 12, 0): 16}


@pytest.fixture(scope='module')
def chooser(tmp_path_factory):
    d = tmp_path_factory.mktemp('patch_choice')
    exe = str(d / 'patch_choice_host')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(HERE, 'hip_host', 'patch_choice_main.cpp'),
                           '-o', exe])

    def ask(rows):
        """rows of (L, H, W, Cout, n_cu, min_block, grid_limit, force_bn) -> list of (bn, bs, items, grid)"""
        path = str(d / 'cases.txt')
        with open(path, 'w') as f:
            for r in rows:
                f.write('%d %d %d %d %d %d %d %d\n' % tuple(r))
        r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        got = [tuple(int(v) for v in line.split()) for line in r.stdout.decode().splitlines()]
        assert len(got) == len(rows)
        return got
    return ask


@pytest.mark.parametrize('n_cu', [256, 8])
def test_automatic_choice_is_the_parents(chooser, n_cu):
    table = AUTO[n_cu]
    got = chooser([s + (n_cu, 0, 0, 0) for s in table])
    bad = ['%s on %d CUs: %s, expected %s' % (s, n_cu, g, e) for (s, e), g in zip(table.items(), got) if g != e]
    assert not bad, '\n'.join(bad)
    if n_cu == 256:   # every (width, edge) branch but <128, 8> has a shape in the table (none of the trunk tests' shapes reaches it)
        assert {e[:2] for e in table.values()} == {(128, 16), (128, 4), (64, 16), (64, 8), (64, 4)}


def test_forced_tile_width(chooser):
    got = chooser([k[:4] + (256, 0, 0, k[4]) for k in FORCED])
    bad = ['%s: %s, expected %s' % (k, g, e) for (k, e), g in zip(FORCED.items(), got) if g != e]
    assert not bad, '\n'.join(bad)
    # a width that is no multiple of 128 runs 64-channel tiles under every knob value, on every device
    rows = [(L, H, W, Cout, n_cu, mb, 0, f) for (L, H, W) in ((1, 3, 3), (40, 16, 16), (600, 4, 4), (33, 24, 40))
            for Cout in (64, 192, 320) for n_cu in (256, 8) for mb in (0, 8) for f in (0, 64, 128)]
    assert {g[0] for g in chooser(rows)} == {64}
    # forcing changes neither the block edge nor (for the width the heuristic picks anyway) anything else
    for n_cu in (256, 8):
        shapes = list(AUTO[n_cu])
        for s, g in zip(shapes, chooser([s + (n_cu, 0, 0, AUTO[n_cu][s][0]) for s in shapes])):
            assert g == AUTO[n_cu][s], (s, g)
        for f in (64, 128):
            for s, g in zip(shapes, chooser([s + (n_cu, 0, 0, f) for s in shapes])):
                assert g[1] == AUTO[n_cu][s][1] and g[0] == (f if s[3] % 128 == 0 else 64), (s, f, g)


def test_block_edge_boundaries(chooser):
    keys = list(EDGES)
    for Cout, f in ((128, 0), (128, 64), (128, 128), (64, 0)):
        got = chooser([(3, H, W, Cout, 256, mb, 0, f) for (H, W, mb) in keys])
        bad = ['%d x %d, min block %d: edge %d, expected %d' % (k + (g[1], EDGES[k])) for k, g in zip(keys, got) if g[1] != EDGES[k]]
        assert not bad, '\n'.join(bad)


def test_tiles_and_grid(chooser):
    """tiles = ceil(blocks / blocks per tile) * Cout / width; the grid is a multiple of 8, capped by the limit and at
    most the tiles rounded up to 8"""
    rows, want = [], []
    for n_cu in (256, 8, 20, 7):
        for limit in (0, 8, 64, 1024):
            for (L, H, W, Cout) in ((1, 1, 1, 64), (2, 20, 12, 256), (5, 7, 8, 256), (19, 3, 4, 256), (12, 20, 12, 256),
                                    (47, 7, 8, 256), (179, 3, 4, 256), (512, 16, 16, 128), (33, 24, 40, 128)):
                for f in (64, 128):
                    rows.append((L, H, W, Cout, n_cu, 0, limit, f))
                    bs = 16 if max(H, W) > 8 else 4 if max(H, W) <= 4 else 8
                    blocks = L * -(-H // bs) * -(-W // bs)
                    bn = f if Cout % 128 == 0 else 64
                    items = -(-blocks // (256 // (bs * bs))) * (Cout // bn)
                    want.append((bn, bs, items))
    got = chooser(rows)
    for r, w, g in zip(rows, want, got):
        n_cu, limit = r[4], r[6]
        assert g[:3] == w, (r, g, w)
        grid, items8 = g[3], -(-w[2] // 8) * 8
        assert grid % 8 == 0 and grid <= items8 and grid <= n_cu and (limit == 0 or grid <= limit), (r, g)
        assert grid == min(n_cu // 8 * 8, items8, limit if limit else 1 << 30), (r, g)
    # literals: the chained shapes of tests/test_trunk_kernels_gpu.py run at least three 128-channel tiles per workgroup
    lit = {(12, 20, 12, 256): (128, 16, 48, 8), (47, 7, 8, 256): (128, 8, 24, 8), (179, 3, 4, 256): (128, 4, 24, 8)}
    for (s, e), g in zip(lit.items(), chooser([s + (256, 0, 8, 128) for s in lit])):
        assert g == e, (s, g, e)
    # fewer than 8 CUs: no whole XCD, the launch is refused (grid 0)
    assert chooser([(2, 20, 12, 256, 7, 0, 0, 0), (2, 20, 12, 256, 0, 0, 0, 0)]) == [(64, 16, 16, 0), (128, 16, 8, 0)]


def test_fused_first_launch(chooser):
    """conv1_1 + conv1_2 + pool: 64 channels in 16 x 16 blocks whatever the knobs say - only the grid is chosen
    (Cout = 0 asks the program for the fused launch; the width column is ignored)"""
    rows = [(3, 2, 2, 0, 256, 0, 0, 128), (3, 18, 18, 0, 256, 8, 0, 128), (3, 36, 2, 0, 256, 0, 8, 0), (5, 64, 64, 0, 256, 0, 0, 0),
            (5, 64, 64, 0, 256, 0, 8, 0), (128, 224, 224, 0, 256, 0, 0, 0)]
    assert chooser(rows) == [(64, 16, 3, 8), (64, 16, 12, 16), (64, 16, 9, 8), (64, 16, 80, 80), (64, 16, 80, 8),
                             (64, 16, 25088, 256)]
