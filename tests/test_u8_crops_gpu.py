"""The 8-bit crop input (uint8 [L,S,S,3], the output of mmmot_amd.crops.crop_resize_u8) against its host normalisation
(oracle.crops_ref.to_tensor_normalize, ToTensor + Normalize in IEEE fp32):

  * the two kernels that read the bytes - mmmot_u8_normalize (exact-fp32 trunk, unfused first layer) and the fused first
    trunk launch mmmot_conv1_fused_u8 (ToTensor + Normalize in its raw-window loader) - bit for bit against the same
    kernels fed the host-normalised crops, and against the float64 two-layer reference;
  * the whole forward: model(u8) == model(to_tensor_normalize(u8)) bit for bit for every trunk arithmetic, with and without
    the fused first layer, on every entry point that takes crops, and within TOL of the oracle on its own terms;
  * bad layouts / sides / strides refused on the host before any operator is called.

The inputs keep the colour channels in disjoint byte ranges and crops / maps with H != W, so a swapped channel, a wrong
channel's mean or a transposed HWC index cannot pass."""
import pytest
import torch

from common import (TOL, CallLog, assert_same_scores, build_model, case_inputs, get_case, normalise_u8, scores,
                    u8_crops, u8_image)
from fake_ops import TorchOps
from mmmot_amd.crops import MEAN, STD
from mmmot_amd.pack import conv1_weight_shift, from_hl16, from_hq8_act, hl16_weight_shift, to_hl16, to_hq8_w
from test_conv_patch_gpu import small_grid  # noqa: F401  (fixture)
from test_kernels_gpu import close, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu


# ---- A. the kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,S', [(3, 37), (130, 128)])
def test_u8_normalize_is_the_host_normalisation(hip, N, S):
    """3 x 37 x 37 pixels: not a multiple of the 256-pixel workgroup; 130 x 128 x 128 > 8192 x 256 pixels: the grid is
    capped at 8192 workgroups, so the grid-stride loop runs more than once.  The NaN tail behind the output stays."""
    u8 = u8_image(N, S, S, seed=700 + N)
    n = N * 3 * S * S
    out = torch.full((n + 4096,), float('nan')).cuda()
    ms = torch.tensor(list(MEAN) + list(STD), dtype=torch.float32).cuda()
    hip.u8_normalize(u8.cuda(), ms, out, N, S)
    got = out.cpu()
    want = normalise_u8(u8)
    assert torch.equal(got[:n].view(N, 3, S, S), want), 'u8_normalize differs from ToTensor + Normalize'
    assert torch.isnan(got[n:]).all(), 'u8_normalize wrote past its output'


def _conv1_weights(seed=500):
    w1 = rnd(64, 3, 3, 3, seed=seed + 1, scale=(2.0 / 27) ** 0.5)
    b1 = rnd(64, seed=seed + 2, scale=0.1)
    w2 = rnd(9, 64, 64, seed=seed + 3, scale=(2.0 / 576) ** 0.5)
    b2 = rnd(64, seed=seed + 4, scale=0.1)
    w1p = torch.zeros(64, 32)
    w1p[:, :27] = w1.permute(0, 2, 3, 1).reshape(64, 27)
    s1, s2 = conv1_weight_shift(w1p, b1), hl16_weight_shift(w2)
    w1h = to_hl16(w1p.double() * 2.0 ** s1)
    return w1h, b1, s1, w2, b2, s2


def _bits(t):
    return t.detach().cpu().view(torch.int32)


def run_conv1_u8(hip, L, H, W, q8):
    u8 = u8_image(L, H, W, seed=710 + L * H + W)
    x = normalise_u8(u8)
    w1h, b1, s1, w2, b2, s2 = _conv1_weights()
    w2d = to_hq8_w(w2.double() * 2.0 ** s2) if q8 else to_hl16(w2.double() * 2.0 ** s2)
    args = (w1h.cuda(), b1.cuda(), 2.0 ** -s1, w2d.cuda(), b2.cuda(), 2.0 ** -s2)
    shape = (L * (H // 2) * (W // 2), 64)
    out8 = torch.full(shape, float('nan')).cuda()
    out32 = torch.full(shape, float('nan')).cuda()
    hip.conv1_fused_u8(u8.cuda(), MEAN, STD, *args[:3], *args[3:], out8, L, H, W, q8=q8)
    (hip.conv1_fused_hq8 if q8 else hip.conv1_fused_hl16)(x.cuda(), *args, out32, L, H, W)
    assert torch.equal(_bits(out8), _bits(out32)), 'conv1_fused_u8 (q8=%s) differs from the fp32-crop launch' % q8
    dec = torch.zeros(shape).cuda()
    (hip.hq8_unpack if q8 else hip.hl16_unpack)(out8, dec)
    if q8:  # the float64 emulation of the hq8 arithmetic on the host-normalised crops (tests/test_hq8_gpu.py)
        want = torch.zeros(shape)
        TorchOps(torch.float64).conv1_fused_hq8(x, w1h, b1, 2.0 ** -s1, w2d, b2, 2.0 ** -s2, want, L, H, W)
        close(dec, from_hq8_act(want), 2.5e-4, 'fused conv1 from uint8 crops (hq8) vs emulation')
    else:  # the float64 two-layer reference from the same (hl16-rounded) weights
        w1r = (from_hl16(w1h) * 2.0 ** -s1)[:, :27].view(64, 3, 3, 3).permute(0, 3, 1, 2).double()
        w2r = (from_hl16(w2d.reshape(9 * 64, 64)) * 2.0 ** -s2).view(3, 3, 64, 64).permute(2, 3, 0, 1).double()
        y = torch.relu(torch.nn.functional.conv2d(x.double(), w1r, b1.double(), padding=1))
        y = torch.relu(torch.nn.functional.conv2d(y, w2r, b2.double(), padding=1))
        ref = torch.nn.functional.max_pool2d(y, 2, 2).permute(0, 2, 3, 1).reshape(-1, 64).float()
        close(dec, ref, 3e-6, 'fused conv1 from uint8 crops vs float64')


@pytest.mark.parametrize('q8', [False, True])
@pytest.mark.parametrize('L,H,W', [(2, 16, 16), (3, 32, 48), (1, 14, 22), (5, 64, 64), (2, 8, 8)])
def test_conv1_fused_u8(hip, L, H, W, q8):
    """maps that are not multiples of the 16 x 16 block, crops smaller than a block, H != W"""
    run_conv1_u8(hip, L, H, W, q8)


@pytest.mark.parametrize('q8', [False, True])
def test_conv1_fused_u8_many_tiles_per_workgroup(hip, small_grid, q8):
    """persistent grid capped at 8 workgroups: the raw-window prefetch of the next tile reads bytes too"""
    run_conv1_u8(hip, 5, 64, 64, q8)
    run_conv1_u8(hip, 3, 32, 48, q8)


# ---- B. the whole forward ------------------------------------------------------------------------------------------
# (trunk, q8_min_crop (None: the default), fuse_conv1); the exact-fp32 trunk has no fused first layer
CONFIGS = [('f32', None, True), ('f16x3', None, True), ('f16x3', None, False), ('f16q8', None, True),
           ('f16q8', None, False), ('f16q8', 0, True), ('f16q8', 0, False)]


def _configure(m, trunk, q8min, fuse):
    m.set_trunk(trunk)
    eng = m.engine()
    eng.fuse_conv1 = fuse
    if q8min is not None:
        eng.q8_min_crop = q8min
    return eng


@pytest.mark.parametrize('name', ['s6_endmax_C', 's8_S40_C', 's8_S100_A', 'f_cfg3_C'])
def test_uint8_forward_equals_normalised_forward(name):
    """32-pixel crops, 40 and 100 (odd maps on the way down), the cfg3 batch (128-pixel crops, 64 x 64).  Entry points:
    points_split on the device (_split_behind_trunk), on the host (_trunk_first), forward_batch with two samples of
    unequal counts, forward_rows(rows=(0,))."""
    from mmmot_amd.synth import make_pair
    c, base = get_case(name)
    m = build_model(c, base, device='cuda')
    dets, info, ds = case_inputs(c)
    S = c['S']
    u8 = u8_crops(dets)
    x = normalise_u8(u8)
    u8d, xd = u8.cuda(), x.cuda()
    dinfo = {k: v.cuda() for k, v in info.items()}
    hinfo = {'points': dinfo['points'], 'points_split': info['points_split']}
    fc = [int(d) for d in ds]
    d2, i2, s2 = make_pair(3, 2, S, 7, seed=4320 + S, ragged=True)
    u8b = torch.cat([u8, u8_crops(d2)])
    u8bd, xbd = u8b.cuda(), normalise_u8(u8b).cuda()
    ps = [info['points_split'].reshape(-1).long().numpy(), i2['points_split'].reshape(-1).long().numpy()]
    ptsb = torch.cat([info['points'].reshape(-1, 3), i2['points'].reshape(-1, 3)]).contiguous().cuda()
    for trunk, q8min, fuse in CONFIGS:
        eng = _configure(m, trunk, q8min, fuse)
        what = '%s, trunk %s, q8_min_crop %s, fuse_conv1 %s' % (name, trunk, q8min, fuse)
        with torch.no_grad():
            want = scores(m(xd, dinfo, ds))
            assert_same_scores(scores(m(u8d, dinfo, ds)), want, what + ': points_split on the device')
            assert_same_scores(scores(m(u8d, hinfo, ds)), want, what + ': points_split on the host')
            assert_same_scores(scores(m.forward_rows(u8d, dinfo, ds, rows=(0,))),
                               scores(m.forward_rows(xd, dinfo, ds, rows=(0,))), what + ': forward_rows(rows=(0,))')
            plan = m.make_plan([(fc, ps[0]), ([int(d) for d in s2], ps[1])], S)
            a, b = m.forward_batch(plan, u8bd, ptsb), m.forward_batch(plan, xbd, ptsb)
            for k in range(2):
                assert_same_scores(scores(a[k]), scores(b[k]), what + ': forward_batch, sample %d' % k)
        torch.cuda.synchronize()
        assert eng.trunk == trunk and not eng.range_events, (what, eng.range_events)


def test_uint8_forward_matches_the_oracle():
    """the u8 path pinned to the reference on its own terms: oracle.restatement on the host-normalised crops"""
    from oracle import restatement as R
    c, base = get_case('s8_S40_C')
    m = build_model(c, base, device='cuda')
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    dets, info, ds = case_inputs(c)
    u8 = u8_crops(dets)
    cfg = dict(fusion=c['fusion'], affinity_op=c['aff'], softmax_mode=c['sm'], neg_threshold=base['neg_threshold'],
               score_arch=base['score_arch'], end_mode=c.get('end_mode', 'avg'))
    with torch.no_grad():
        ref = R.tracking_forward(sd, cfg, normalise_u8(u8), info['points'], info['points_split'], [int(d) for d in ds])
        for trunk in ('f16x3', 'f32'):
            m.set_trunk(trunk)
            det, links, new, end, _ = m(u8.cuda(), {k: v.cuda() for k, v in info.items()}, ds)
            err = max((det.cpu() - ref[0]).abs().max().item(), (links[0].cpu() - ref[1][0]).abs().max().item(),
                      (new.cpu() - ref[2]).abs().max().item(), (end.cpu() - ref[3]).abs().max().item())
            assert err < TOL, (trunk, err)


def test_bad_uint8_crops_are_refused_before_any_launch():
    c, base = get_case('s8_S40_C')
    m = build_model(c, base, device='cuda')
    dets, info, ds = case_inputs(c)
    S = c['S']
    u8 = u8_crops(dets).cuda()
    dinfo = {k: v.cuda() for k, v in info.items()}
    eng = m.engine()
    log = CallLog(eng.ops)
    eng.ops = log
    try:
        with torch.no_grad():
            with pytest.raises(ValueError, match=r'uint8 crops must be \[L,S,S,3\]'):
                m(u8.permute(0, 3, 1, 2).contiguous(), dinfo, ds)
            with pytest.raises(ValueError, match='crop side'):
                m(torch.zeros(dets.shape[0], 41, 41, 3, dtype=torch.uint8, device='cuda'), dinfo, ds)
            plan = m.make_plan([([int(d) for d in ds], info['points_split'].reshape(-1).long().numpy())], S)
            strided = torch.cat([u8, u8], dim=2)[:, :, :S]
            assert not strided.is_contiguous()
            with pytest.raises(ValueError, match='crops must be a contiguous'):
                m.forward_batch(plan, strided, dinfo['points'].reshape(-1, 3).contiguous())
            m.train()
            with pytest.raises(ValueError, match='uint8'):
                m(u8, dinfo, ds)
            m.eval()
        assert log.calls == [], 'operators were called before the crops were refused: %r' % log.calls
        with torch.no_grad():  # the reference-shaped call copies a strided tensor: same scores
            assert_same_scores(scores(m(strided, dinfo, ds)), scores(m(u8, dinfo, ds)), 'strided uint8 crops')
        assert 'conv1_fused_u8' in log.calls
    finally:
        eng.ops = log.ops
