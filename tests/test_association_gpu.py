"""The device frame-pair association (csrc/assign.hip through mmmot::associate / mmmot_amd.association) against the host
oracle of tests/association_ref.py: the exact assignment on continuous scores, the optimum on tied ones, determinism over
batch position and kernel variant, outputs written in full over poisoned memory, the ortools_solve-shaped drop-in with
host and device inputs, a real forward through tracker_glue.predict_assign and a sequence through
SequencePipeline(associate=True)."""
import numpy as np
import pytest
import torch

from association_ref import feasible, lsa_route, objective, random_instance
from mmmot_amd import TrackingNet, _lib
from mmmot_amd.association import associate, associate_batch, pairs_table, unpack
from mmmot_amd.ops import HipOps
from mmmot_amd.torch_ops import associate_layout
from mmmot_amd.weights import init_module

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 12, 31, 32, 33, 64, 65, 127, 128, 200)
SHAPES = [(n, n) for n in SIZES] + [(1, 200), (200, 1), (2, 33), (33, 2), (12, 65), (65, 12), (31, 128), (128, 31),
                                    (64, 127), (127, 64), (200, 3), (3, 200), (512, 7), (7, 512)]
_OPS = []


def ops():
    if not _OPS:
        _OPS.append(HipOps())
    return _OPS[0]


def set_variant(v):
    assert _lib.load().mmmot_set_assign_variant(v) == 0


def solve(insts, variant=0, fill=None):
    """one launch over [(N, M, (det, new, end, link)) ...] -> [(det, link N x M, new, end) numpy], objective numpy [B]"""
    splits = [(N, M) for N, M, _ in insts]
    pairs, offs = pairs_table(splits)
    cat = lambda k: torch.from_numpy(np.concatenate([np.asarray(x[2][k], np.float32).reshape(-1) for x in insts])).cuda()
    det, new, end, link = cat(0), cat(1), cat(2), cat(3)
    total, off, max_nm = associate_layout(pairs, det.numel(), link.numel())
    table = torch.cat([pairs.reshape(-1), off.to(torch.int32)]).cuda()
    out = torch.empty(total, dtype=torch.float32, device='cuda')
    obj = torch.empty(len(insts), dtype=torch.float64, device='cuda')
    if fill is not None:
        out.view(torch.uint8).fill_(fill)
        obj.view(torch.uint8).fill_(fill)
    set_variant(variant)
    try:
        ops().associate_pairs(det, new, end, link, table[:4 * len(insts)], len(insts), max_nm, out, table[4 * len(insts):],
                              obj)
        torch.cuda.synchronize()
    finally:
        set_variant(0)
    out, obj = out.cpu(), obj.cpu().numpy()
    res = []
    for (N, M), o in zip(splits, offs):
        d, lk, n, e = unpack(out[o:o + 3 * (N + M) + N * M], N, M)
        res.append((d.numpy(), lk[0].reshape(N, M).numpy(), n.numpy(), e.numpy()))
    return res, obj


def check_exact(inst, got, obj):
    N, M, (det, new, end, link) = inst
    want, wobj = lsa_route(det, new, end, link, N, M)
    assert feasible(got, N, M), (N, M)
    for g, w, name in zip(got, want, ('det', 'link', 'new', 'end')):
        assert np.array_equal(g.reshape(-1), w.reshape(-1)), (N, M, name)
    assert abs(obj - wobj) <= 1e-9 * max(1.0, abs(wobj)), (N, M, obj, wobj)
    assert abs(objective(got, det, new, end, link) - wobj) <= 1e-9 * max(1.0, abs(wobj))


def same(a, b):
    return all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


@pytest.mark.parametrize('kind', ['normal', 'eval', 'masked'])
def test_random_scores_match_the_oracle_exactly(kind):
    rng = np.random.default_rng(['normal', 'eval', 'masked'].index(kind) + 11)
    insts = [(N, M, random_instance(rng, N, M, (1.0, 10.0, 1e4)[k % 3], kind)) for k, (N, M) in enumerate(SHAPES)]
    res, obj = solve(insts)
    for inst, r, o in zip(insts, res, obj):
        check_exact(inst, r, o)
    # the same bits from every kernel variant (the LDS-staged ones hold pairs up to 128)
    small = [x for x in insts if max(x[0], x[1]) <= 128]
    ref_small = solve(small)
    for v in (1, 2, 3, 4):
        got = solve(small, v)
        assert same(got[0], ref_small[0]) and np.array_equal(got[1], ref_small[1]), v
    for v in (1, 2):
        got = solve(insts, v)
        assert same(got[0], res) and np.array_equal(got[1], obj), v


def test_ties_reach_the_optimum_deterministically():
    rng = np.random.default_rng(5)
    insts = []
    for N, M in ((1, 1), (3, 3), (12, 12), (12, 31), (31, 12), (64, 64), (65, 33), (128, 128), (200, 200)):
        L = N + M
        c = lambda *s, v=0.5: np.full(s, v, np.float32)
        insts.append((N, M, (c(L), c(L), c(L), c(N, M, v=2.0))))             # every pair gains 1: any perfect matching
        insts.append((N, M, (c(L, v=0), c(L, v=0), c(L, v=0), c(N, M, v=0))))  # every gain exactly 0
        q = lambda *s: rng.integers(-2, 3, s).astype(np.float32)
        insts.append((N, M, (q(L), q(L), q(L), q(N, M))))                   # small integers: many tied optima
    res, obj = solve(insts)
    for (N, M, sc), r, o in zip(insts, res, obj):
        _, wobj = lsa_route(*sc, N, M)
        assert feasible(r, N, M)
        assert abs(o - wobj) <= 1e-9 * max(1.0, abs(wobj)) and abs(objective(r, *sc) - wobj) <= 1e-9 * max(1.0, abs(wobj))
    again = solve(insts)
    assert same(again[0], res) and np.array_equal(again[1], obj)
    small = [x for x in insts if max(x[0], x[1]) <= 128]
    base = solve(small)
    for v in (1, 2, 3, 4):
        got = solve(small, v)
        assert same(got[0], base[0]) and np.array_equal(got[1], base[1]), v


def test_batch_equals_pairs_alone_and_shuffled():
    rng = np.random.default_rng(17)
    insts = []
    for k in range(40):
        N, M = int(rng.integers(1, 130)), int(rng.integers(1, 130))
        if k % 7 == 0:
            N, M = int(rng.integers(1, 4)), int(rng.integers(100, 201))
        insts.append((N, M, random_instance(rng, N, M, 3.0, ('normal', 'eval', 'masked')[k % 3])))
    res, obj = solve(insts)
    for k, inst in enumerate(insts):
        alone, o = solve([inst])
        assert same(alone, [res[k]]) and o[0] == obj[k], k
        check_exact(inst, res[k], obj[k])
    perm = rng.permutation(len(insts))
    sres, sobj = solve([insts[k] for k in perm])
    for pos, k in enumerate(perm):
        assert same([sres[pos]], [res[k]]) and sobj[pos] == obj[k]


@pytest.mark.parametrize('fill', [0xFF, 0x7B])
def test_workspace_poison_outputs_written_in_full(fill):
    rng = np.random.default_rng(23)
    insts = [(N, M, random_instance(rng, N, M, 2.0, 'eval')) for N, M in ((12, 12), (5, 64), (64, 5), (128, 100), (300, 9))]
    clean = solve(insts, fill=0)
    for v in (0, 1, 2):
        got = solve(insts, v, fill=fill)
        assert same(got[0], clean[0]) and np.array_equal(got[1], clean[1]), v


def test_associate_host_and_device_inputs_match_ortools_shapes():
    rng = np.random.default_rng(29)
    for N, M in ((1, 1), (12, 12), (7, 40), (40, 7), (0, 5), (5, 0)):
        det, new, end, link = (torch.from_numpy(x) for x in random_instance(rng, N, M, 1.0, 'eval'))
        link = link.reshape(1, N, M)
        split = [torch.tensor([N]), torch.tensor([M])]
        host = associate(det, [link], new, end, split)
        dev = associate(det.cuda(), [link.cuda()], new.cuda(), end.cuda(), [N, M])
        for h, d, ref in ((host[0], dev[0], det), (host[2], dev[2], det), (host[3], dev[3], det)):
            assert h.shape == ref.shape and h.dtype == ref.dtype and h.device.type == 'cpu'
            assert d.shape == ref.shape and d.dtype == ref.dtype and d.is_cuda
            assert torch.equal(h, d.cpu())
        assert len(host[1]) == 1 and host[1][0].shape == (1, N, M) and dev[1][0].shape == (1, N, M)
        assert dev[1][0].is_cuda and torch.equal(host[1][0], dev[1][0].cpu())
        if N and M:
            want, _ = lsa_route(det.numpy(), new.numpy(), end.numpy(), link.numpy(), N, M)
            got = (host[0].numpy(), host[1][0].numpy(), host[2].numpy(), host[3].numpy())
            for g, w in zip(got, want):
                assert np.array_equal(g.reshape(-1), w.reshape(-1)), (N, M)
    # associate_batch: the pairs of one launch equal associate one by one
    insts = [(N, M, random_instance(rng, N, M, 1.0, 'eval')) for N, M in ((3, 4), (12, 12), (9, 2))]
    t = lambda x: torch.from_numpy(x).cuda()
    res, obj = associate_batch([t(s[0]) for _, _, s in insts], [[t(s[3]).reshape(1, N, M)] for N, M, s in insts],
                               [t(s[1]) for _, _, s in insts], [t(s[2]) for _, _, s in insts],
                               [[N, M] for N, M, _ in insts], return_objective=True)
    for (N, M, s), r in zip(insts, res):
        one = associate(t(s[0]), [t(s[3]).reshape(1, N, M)], t(s[1]), t(s[2]), [N, M])
        assert all(torch.equal(a, b) for a, b in zip((r[0], r[1][0], r[2], r[3]), (one[0], one[1][0], one[2], one[3])))


KW = dict(seq_len=2, score_arch='branch_cls', appear_arch='vgg', appear_len=512, appear_skippool=True, appear_fpn=False,
          point_arch='v1', point_len=512, without_reflectivity=True, end_arch='v2', end_mode='avg', test_mode=2,
          neg_threshold=0.2, dropblock=0, use_dropout=False, score_fusion_arch='C', affinity_op='minus_abs',
          softmax_mode='dual_add')


def _model(**kw):
    m = TrackingNet(**dict(KW, **kw))
    init_module(m, seed=0)
    return m.eval().cuda()


def _check_pair(scores, assignment, N, M):
    det, links, new, end = scores
    want, _ = lsa_route(det.numpy(), new.numpy(), end.numpy(), links[0].numpy(), N, M)
    got = (assignment[0].numpy(), assignment[1][0].numpy(), assignment[2].numpy(), assignment[3].numpy())
    assert assignment[1][0].shape == (1, N, M) and assignment[0].shape == det.shape
    for g, w, name in zip(got, want, ('det', 'link', 'new', 'end')):
        assert np.array_equal(g.reshape(-1), w.reshape(-1)), (N, M, name)


@pytest.mark.parametrize('n', [12, 64])
def test_predict_assign_real_forward(n):
    from mmmot_amd.synth import make_pair
    from mmmot_amd.tracker_glue import predict_assign, predict_scores
    m = _model()
    dets, info, ds = make_pair(n, n, 64, 40, seed=n)
    dinfo = {k: v.cuda() for k, v in info.items()}
    scores, assignment = predict_assign(m, dets.cuda(), dinfo, ds)
    plain = predict_scores(m, dets.cuda(), dinfo, ds)
    assert all(torch.equal(a, b) for a, b in zip((scores[0], scores[1][0], scores[2], scores[3]),
                                                (plain[0], plain[1][0], plain[2], plain[3])))
    _check_pair(scores, assignment, n, n)


def test_sequence_pipeline_associate():
    from mmmot_amd.pipeline import FrameFeed, SequencePipeline
    from mmmot_amd.synth import make_frame
    S = 64
    m = _model(score_fusion_arch='A', affinity_op='multiply', softmax_mode='none')
    feeds = [FrameFeed(*make_frame(300 + t, 20000, 4 + t % 4)) for t in range(6)]
    plain = SequencePipeline(m, S).run(feeds)
    seen = []
    got = SequencePipeline(m, S, associate=True).run(feeds, on_assign=lambda t, a: seen.append(t))
    off = SequencePipeline(m, S, associate=True).run_offline(feeds, frames_per_encode=3, pairs_per_forward=2)
    assert seen == list(range(1, len(feeds)))
    assert len(got) == len(off) == len(plain) == len(feeds) - 1
    for t, (p, g, o) in enumerate(zip(plain, got, off)):
        for sc in (g[0], o[0]):
            assert all(torch.equal(a, b) for a, b in zip((sc[0], sc[1][0], sc[2], sc[3]), (p[0], p[1][0], p[2], p[3])))
        N, M = p[1][0].shape[1:]
        _check_pair(g[0], g[1], N, M)
        _check_pair(o[0], o[1], N, M)
