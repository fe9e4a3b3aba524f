"""Chain association without a GPU: the two host oracle routes of tests/association_chain_ref.py agree (the program is
the min-cost flow its LP relaxation solves), at T = 2 they agree with the frame-pair oracle, the C-ABI entry point exists
and rejects bad arguments before any launch, the host layout check refuses bad tables, the ``gt=`` shift is the
reference's expression and the operator's Meta kernel gives the output sizes."""
import numpy as np
import pytest
import torch

import association_ref as pair_ref
from association_chain_ref import feasible, lp_route, milp_route, objective, random_chain, same_assignment
from mmmot_amd import _lib

KINDS = ('normal', 'eval', 'masked')


def _instances():
    rng = np.random.default_rng(20261018)
    out = []
    fixed = [[1, 1], [1, 1, 1], [0, 3, 2], [3, 0, 3], [2, 2, 0], [12, 12, 12, 12], [2] * 8, [5, 1, 7], [12, 0, 12]]
    for k in range(300):
        T = (2, 3, 4, 8)[k % 4]
        split = fixed[k] if k < len(fixed) else [int(n) for n in rng.integers(0, 13, T)]
        if sum(split) == 0:
            split[0] = 1
        out.append((split, random_chain(rng, split, (1.0, 10.0, 1e4)[k % 3], KINDS[k % 3])))
    return out


def test_oracle_routes_agree():
    worst = 0.0
    for split, (det, new, end, links) in _instances():
        a1, o1 = milp_route(det, new, end, links, split)
        a2, o2 = lp_route(det, new, end, links, split)
        assert feasible(a1, split) and feasible(a2, split), split
        assert abs(objective(a2, det, new, end, links) - o2) <= 1e-12 * max(1.0, abs(o2))
        assert abs(o1 - o2) <= 1e-12 * max(1.0, abs(o2)), (split, o1, o2)
        worst = max(worst, abs(o1 - o2) / max(1.0, abs(o2)))
    assert worst <= 1e-12


def test_two_frames_agree_with_the_pair_oracle():
    rng = np.random.default_rng(7)
    for k in range(40):
        N, M = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        det, new, end, link = pair_ref.random_instance(rng, N, M, (1.0, 10.0, 1e4)[k % 3], KINDS[k % 3])
        want, wobj = pair_ref.milp_route(det, new, end, link, N, M)
        for route in (milp_route, lp_route):
            got, obj = route(det, new, end, [link], [N, M])
            assert abs(obj - wobj) <= 1e-12 * max(1.0, abs(wobj)), (N, M)
            assert pair_ref.feasible((got[0], got[1][0], got[2], got[3]), N, M)


def test_entry_point_exported_and_rejects_bad_arguments():
    lib = _lib.load()
    assert hasattr(lib, 'mmmot_associate_chains') and hasattr(lib, 'mmmot_set_chain_variant')
    d = 4096  # never dereferenced: the argument checks come before any launch
    f = lib.mmmot_associate_chains
    args = [d, d, d, d, d, 1, 8, 16, d, d, d, None]
    for k in (0, 1, 2, 3, 4, 8, 9, 10):  # each pointer NULL in turn
        bad = list(args)
        bad[k] = None
        assert f(*bad) == -1, k
    for B, n, L in ((0, 8, 16), (-3, 8, 16), (1, 0, 16), (1, -1, 16), (1, 513, 1024), (1, 8, 0), (1, 8, 7), (1, 8, 65),
                    (1, 512, 1025), (1, 100000, 100000)):
        bad = list(args)
        bad[5], bad[6], bad[7] = B, n, L
        assert f(*bad) == -1, (B, n, L)
    assert lib.mmmot_set_chain_variant(3) == -1 and lib.mmmot_set_chain_variant(-1) == -1
    assert lib.mmmot_set_chain_variant(1) == 0 and lib.mmmot_set_chain_variant(0) == 0


def _row(T, so, lo, ns):
    return [T, so, lo] + list(ns) + [0] * (8 - len(ns))


def test_chain_layout_sizes_and_rejections():
    from mmmot_amd.torch_ops import chain_layout
    ok = torch.tensor([_row(3, 0, 0, [3, 4, 2]), _row(2, 9, 20, [2, 2])], dtype=torch.int32)
    total, off, max_n, max_L = chain_layout(ok, 13, 24)
    assert total == 3 * 9 + 12 + 8 + 3 * 4 + 4 and off.tolist() == [0, 47] and (max_n, max_L) == (4, 9)
    one = lambda row: torch.tensor([row], dtype=torch.int32)
    bad = {
        'T = 1': _row(1, 0, 0, [4]),
        'T = 9': [9, 0, 0] + [1] * 8,
        'n_t = 513': _row(2, 0, 0, [513, 1]),
        'n_t < 0': _row(2, 0, 0, [-1, 4]),
        'L = 0': _row(3, 0, 0, [0, 0, 0]),
        'L = 1025': _row(3, 0, 0, [512, 1, 512]),
        'negative score offset': _row(2, -1, 0, [2, 2]),
        'negative link offset': _row(2, 0, -1, [2, 2]),
    }
    for name, row in bad.items():
        with pytest.raises(ValueError):
            chain_layout(one(row))
    # the limits themselves pass: T = 2 and 8, n_t = 512, L = 1 and 1024, empty frames
    for row in (_row(2, 0, 0, [512, 512]), [8, 0, 0] + [128] * 8, _row(2, 0, 0, [1, 0]), _row(3, 0, 0, [12, 0, 12])):
        chain_layout(one(row))
    with pytest.raises(ValueError):
        chain_layout(ok, 12, 24)  # scores too short
    with pytest.raises(ValueError):
        chain_layout(ok, 13, 23)  # link too short
    with pytest.raises(ValueError):
        chain_layout(ok.to(torch.int64))
    with pytest.raises(ValueError):
        chain_layout(ok[:, :10])
    with pytest.raises(ValueError):
        chain_layout(ok[:0])
    # entries past n_{T-1} are not part of the chain
    assert chain_layout(one([2, 0, 0, 2, 2, 999, -5, 0, 0, 0, 0]))[0] == 16


def test_gt_shift_is_the_reference_expression():
    """solvers.py:50-81 evaluated literally: the objective gains gt - y * gt_eff per variable, i.e. every score drops by
    gt_eff = gt + gt.eq(0).float().mul(-1)"""
    from mmmot_amd.association import _flat_scores
    rng = np.random.default_rng(3)
    split = [2, 3, 2]
    det, new, end, links = (torch.from_numpy(x) if not isinstance(x, list) else [torch.from_numpy(l)[None] for l in x]
                            for x in random_chain(rng, split))
    lab = lambda *s: torch.from_numpy(rng.integers(0, 2, s).astype(np.float32))
    gt = (lab(7), lab(7), lab(7), [lab(1, 2, 3), lab(1, 3, 2)])
    gt[0][1] = -1.0  # an ignored label: gt_eff = -1, like the reference's expression gives
    got = _flat_scores(det, links, new, end, gt)
    want = []
    for sc, g in ((det, gt[0]), (new, gt[1]), (end, gt[2])):
        eff = g + g.eq(0).float().mul(-1)
        want += [sc[i].item() - eff[i].item() for i in range(7)]
    for i in range(2):
        eff = gt[3][i] + gt[3][i].eq(0).float().mul(-1)
        for j in range(links[i][0].size(0)):
            for k in range(links[i][0].size(1)):
                want.append(links[i][0][j][k].item() - eff[0][j][k].item())
    assert got.dtype == torch.float32 and got.shape == (len(want),)
    assert np.array_equal(got.numpy(), np.asarray(want, np.float64).astype(np.float32))
    assert torch.equal(_flat_scores(det, links, new, end, None), torch.cat([det, new, end, links[0].reshape(-1),
                                                                            links[1].reshape(-1)]))
    # the oracle's gt objective is the same program: shifted scores plus the constant sum of gt
    n = lambda t: t.numpy()
    a, o = milp_route(n(det), n(new), n(end), [n(l) for l in links], split, gt=[n(gt[0]), n(gt[1]), n(gt[2]),
                                                                                [n(g) for g in gt[3]]])
    L = 7
    sh = got.numpy()
    b, o2 = milp_route(sh[0:L], sh[L:2 * L], sh[2 * L:3 * L], [sh[21:27], sh[27:33]], split)
    const = float(sum(g.sum() for g in (gt[0], gt[1], gt[2], *gt[3])))
    # the shift is rounded to fp32 once per variable: at most 2^-24 * |score - gt_eff| (< 8 here) on each of 33 variables
    assert same_assignment(a, b) and abs(o - (o2 + const)) <= 33 * 2.0 ** -24 * 8


def test_meta_kernel_shapes():
    from mmmot_amd import torch_ops  # noqa: F401
    chains = torch.tensor([_row(3, 0, 0, [3, 4, 2]), _row(2, 9, 20, [5, 2]), [8, 16, 30] + [1] * 8], dtype=torch.int32)
    d = torch.empty(24, device='meta')
    lk = torch.empty(37, device='meta')
    out, obj = torch.ops.mmmot.associate_chains(d, d, d, lk, chains)
    assert out.shape == (3 * 9 + 20 + 3 * 7 + 10 + 3 * 8 + 7,) and out.dtype == torch.float32
    assert obj.shape == (3,) and obj.dtype == torch.float64 and out.device.type == 'meta'


def test_python_surface_refuses_what_it_cannot_solve_and_answers_the_empty_chain():
    from mmmot_amd.association import associate_chain, chains_table, select_chain
    with pytest.raises(ValueError):
        associate_chain(torch.zeros(2), [], torch.zeros(2), torch.zeros(2), [2])
    with pytest.raises(ValueError):
        associate_chain(torch.zeros(5), [torch.zeros(1, 2, 2)], torch.zeros(4), torch.zeros(4), [2, 2])
    with pytest.raises(ValueError):
        chains_table([[1] * 9])
    d, lk, n, e = associate_chain(torch.zeros(0), [torch.zeros(1, 0, 0), torch.zeros(1, 0, 0)], torch.zeros(0),
                                  torch.zeros(0), [torch.tensor([0])] * 3)
    assert d.numel() == n.numel() == e.numel() == 0 and [tuple(x.shape) for x in lk] == [(1, 0, 0), (1, 0, 0)]
    det, links = torch.zeros(3, 7), [torch.zeros(3, 2, 3), torch.zeros(3, 3, 2)]
    sel = select_chain(det, links, det, det, 2)
    assert sel[0].shape == (7,) and [tuple(x.shape) for x in sel[1]] == [(1, 2, 3), (1, 3, 2)]
