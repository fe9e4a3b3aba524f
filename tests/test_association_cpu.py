"""Frame-pair association without a GPU: the two host oracle routes agree (the reduction of the two-frame program to a
matching holds), the C-ABI entry point exists and rejects bad arguments before any launch, the operator's Meta kernel
gives the output shapes, and the Python drop-in refuses what it does not solve."""
import numpy as np
import pytest
import torch

from association_ref import feasible, lsa_route, milp_route, objective, random_instance
from mmmot_amd import _lib


def _instances():
    rng = np.random.default_rng(20261016)
    out = []
    shapes = [(1, 1), (1, 5), (5, 1), (2, 7), (7, 2), (3, 3), (6, 4), (4, 6), (8, 8), (1, 8)]
    for t in range(300):
        N, M = shapes[t] if t < len(shapes) else (int(rng.integers(1, 9)), int(rng.integers(1, 9)))
        kind = ('normal', 'eval', 'negative', 'masked')[t % 4]
        scale = (1.0, 10.0, 1e4)[t % 3]
        out.append((N, M, random_instance(rng, N, M, scale, kind)))
    return out


def test_oracle_routes_agree():
    worst = 0.0
    for N, M, (det, new, end, link) in _instances():
        a1, o1 = milp_route(det, new, end, link, N, M)
        a2, o2 = lsa_route(det, new, end, link, N, M)
        assert feasible(a1, N, M) and feasible(a2, N, M)
        # both objectives are what the program scores at the returned assignment, and they agree
        assert abs(objective(a2, det, new, end, link) - o2) <= 1e-12 * max(1.0, abs(o2))
        assert abs(o1 - o2) <= 1e-12 * max(1.0, abs(o2)), (N, M, o1, o2)
        worst = max(worst, abs(o1 - o2) / max(1.0, abs(o2)))
    assert worst <= 1e-12


def test_all_gains_nonpositive_links_nothing():
    rng = np.random.default_rng(3)
    for N, M in ((1, 4), (4, 1), (5, 5)):
        det, new, end, link = random_instance(rng, N, M, 1.0, 'negative')
        a, _ = lsa_route(det, new, end, link, N, M)
        assert a[1].sum() == 0


def test_entry_point_exported_and_rejects_bad_arguments():
    lib = _lib.load()
    assert hasattr(lib, 'mmmot_associate_pairs') and hasattr(lib, 'mmmot_set_assign_variant')
    d = 4096  # never dereferenced: the argument checks come before any launch
    f = lib.mmmot_associate_pairs
    args = [d, d, d, d, d, 1, 8, d, d, d, None]
    for k in (0, 1, 2, 3, 4, 7, 8, 9):  # each pointer NULL in turn
        bad = list(args)
        bad[k] = None
        assert f(*bad) == -1, k
    for B, nm in ((0, 8), (-3, 8), (1, 0), (1, -1), (1, 513), (1, 100000)):
        bad = list(args)
        bad[5], bad[6] = B, nm
        assert f(*bad) == -1, (B, nm)
    # the LDS-staged variants hold at most 128 x 128
    assert lib.mmmot_set_assign_variant(3) == 0
    try:
        bad = list(args)
        bad[6] = 129
        assert f(*bad) == -1
    finally:
        assert lib.mmmot_set_assign_variant(0) == 0
    assert lib.mmmot_set_assign_variant(5) == -1 and lib.mmmot_set_assign_variant(-1) == -1


def test_meta_kernel_shapes():
    from mmmot_amd import torch_ops  # noqa: F401
    pairs = torch.tensor([[3, 4, 0, 0], [5, 2, 7, 12], [1, 1, 14, 22]], dtype=torch.int32)
    d = torch.empty(16, device='meta')
    lk = torch.empty(23, device='meta')
    out, obj = torch.ops.mmmot.associate(d, d, d, lk, pairs)
    assert out.shape == (3 * 7 + 12 + 3 * 7 + 10 + 3 * 2 + 1,) and out.dtype == torch.float32
    assert obj.shape == (3,) and obj.dtype == torch.float64
    assert out.device.type == 'meta'


def test_operator_rejects_bad_tables_on_the_host():
    from mmmot_amd.torch_ops import associate_layout
    ok = torch.tensor([[3, 4, 0, 0]], dtype=torch.int32)
    assert associate_layout(ok, 7, 12)[0] == 33
    with pytest.raises(ValueError):
        associate_layout(ok, 6, 12)  # scores too short
    with pytest.raises(ValueError):
        associate_layout(ok, 7, 11)  # link too short
    for bad in ([[0, 4, 0, 0]], [[3, 513, 0, 0]], [[3, 4, -1, 0]]):
        with pytest.raises(ValueError):
            associate_layout(torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError):
        associate_layout(ok.to(torch.int64))


def test_associate_refuses_chains_and_gt():
    from mmmot_amd.association import associate
    det = torch.zeros(6)
    with pytest.raises(ValueError):
        associate(det, [torch.zeros(1, 2, 2), torch.zeros(1, 2, 2)], det, det, [2, 2, 2])
    with pytest.raises(NotImplementedError):
        associate(torch.zeros(4), [torch.zeros(1, 2, 2)], torch.zeros(4), torch.zeros(4), [2, 2],
                  gt=(None, None, None, None))


def test_associate_empty_frame_is_answered_on_the_host():
    from mmmot_amd.association import associate
    det = torch.tensor([0.5, -2.0, 0.1])
    new = torch.tensor([0.0, 0.0, 0.3])
    end = torch.tensor([0.2, 0.1, -1.0])
    for split, want in (([3, 0], [1, 0, 0]), ([0, 3], [1, 0, 0])):
        d, lk, n, e = associate(det, [torch.zeros(1, split[0], split[1])], new, end, [torch.tensor([s]) for s in split])
        assert d.tolist() == want and n.tolist() == want and e.tolist() == want
        assert lk[0].shape == (1, split[0], split[1]) and d.dtype == det.dtype and not d.is_cuda
