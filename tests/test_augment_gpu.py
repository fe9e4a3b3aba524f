"""Training augmentation on the device (csrc/crop_augment.hip through mmmot_amd.crops / HipOps): bit for bit Pillow's
fixture and the NumPy restatement (tests/augment_ref.py), both outputs, every launch form."""
import os

import numpy as np
import pytest
import torch

import augment_ref
from mmmot_amd import augment
from mmmot_amd import crops as CR
from oracle.crops_ref import MEAN, STD, to_tensor_normalize

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = 'cuda:0'


def source_crops(L, S, seed):
    """structure plus noise per crop: ramps that differ from crop to crop under +-25 of noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    out = []
    for i in range(L):
        base = np.stack([(xx * (3 + i)) % 256, (yy * (5 + i)) % 256, ((xx + yy) * 7 + 31 * i) % 256], -1)
        out.append(np.clip(base + rng.integers(-25, 26, (S, S, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def run_op(hip, u8, params, want_out, want_u8):
    """one launch through HipOps with the outputs between guard rows; returns (out, out_u8) views (None where not asked)"""
    L, S = u8.shape[0], u8.shape[1]
    ms = torch.tensor(list(MEAN) + list(STD), dtype=torch.float32, device=DEV)
    fo = torch.full((L + 2, 3, S, S), float('nan'), device=DEV) if want_out else None
    bo = torch.full((L + 2, S, S, 3), 0xFF, dtype=torch.uint8, device=DEV) if want_u8 else None
    hip.crop_augment(torch.from_numpy(u8).to(DEV), torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(DEV),
                     ms, None if fo is None else fo[1:L + 1], None if bo is None else bo[1:L + 1], L, S)
    torch.cuda.synchronize()
    if fo is not None:
        assert torch.isnan(fo[0]).all() and torch.isnan(fo[L + 1]).all(), 'the fp32 guard rows were written'
    if bo is not None:
        assert (bo[0] == 0xFF).all() and (bo[L + 1] == 0xFF).all(), 'the 8-bit guard rows were written'
    return (None if fo is None else fo[1:L + 1].cpu().numpy()), (None if bo is None else bo[1:L + 1].cpu().numpy())


@pytest.fixture(scope='module')
def hip():
    from mmmot_amd.ops import HipOps
    return HipOps()


@pytest.mark.parametrize('S', [32, 64])
def test_fixture_rows_in_one_launch(hip, S):
    """all rows of the fixture as one launch over L copies of the source crop: both outputs, fp32 alone, bytes alone"""
    z = np.load(os.path.join(HERE, 'golden', 'augment_pil.npz'))
    src, params, want = z['src_%d' % S], z['params_%d' % S], z['out_%d' % S]
    L = len(params)
    u8 = np.ascontiguousarray(np.broadcast_to(src, (L,) + src.shape))
    want_f = np.stack([to_tensor_normalize(w) for w in want])
    for want_out, want_u8 in ((True, True), (True, False), (False, True)):
        fo, bo = run_op(hip, u8, params, want_out, want_u8)
        if want_u8:
            assert np.array_equal(bo, want), 'S=%d: %d bytes differ from Pillow' % (S, int((bo != want).sum()))
        if want_out:
            assert np.array_equal(fo.view(np.uint32), want_f.view(np.uint32)), 'S=%d: fp32 output differs' % S
    # the public call gives the same
    out, o8 = CR.augment_crops(torch.from_numpy(u8).to(DEV), params, return_u8=True)
    assert np.array_equal(o8.cpu().numpy(), want) and np.array_equal(out.cpu().numpy().view(np.uint32), want_f.view(np.uint32))


CRAFTED = {
    # identity, a 1 x 1 region, a 17 x 211 region at the bottom-right, flipped
    224: [(0, 0, 224, 224, 0), (100, 7, 1, 1, 0), (224 - 17, 224 - 211, 17, 211, 1)],
    256: [(3, 40, 250, 200, 1)],                       # the largest side
    33: [(0, 0, 33, 33, 1), (5, 9, 20, 11, 0)],        # odd: no multiple of the row tile, one-pixel stores
}


@pytest.mark.parametrize('S', sorted(CRAFTED))
def test_crafted_regions_against_the_restatement(hip, S):
    params = np.asarray(CRAFTED[S], dtype=np.int32)
    u8 = source_crops(len(params), S, seed=S)
    want_u8, want_f = augment_ref.augment(u8, params)
    fo, bo = run_op(hip, u8, params, True, True)
    assert np.array_equal(bo, want_u8), 'S=%d: %d bytes differ' % (S, int((bo != want_u8).sum()))
    assert np.array_equal(fo.view(np.uint32), want_f.view(np.uint32))
    fo2, bo2 = run_op(hip, u8, params, True, True)      # again: the same bits
    assert np.array_equal(bo2, bo) and np.array_equal(fo2.view(np.uint32), fo.view(np.uint32))
    fo3, _ = run_op(hip, u8, params, True, False)
    _, bo3 = run_op(hip, u8, params, False, True)
    assert np.array_equal(fo3.view(np.uint32), fo.view(np.uint32)) and np.array_equal(bo3, bo)


@pytest.mark.parametrize('S', [32, 33, 224])
def test_identity_reproduces_u8_normalize(hip, S):
    L = 3
    u8 = torch.from_numpy(source_crops(L, S, seed=7 + S)).to(DEV)
    ms = torch.tensor(list(MEAN) + list(STD), dtype=torch.float32, device=DEV)
    want = torch.empty(L, 3, S, S, device=DEV)
    hip.u8_normalize(u8, ms, want, L, S)
    out, o8 = CR.augment_crops(u8, augment.identity_params(L, S), return_u8=True)
    assert torch.equal(o8, u8) and torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_composition_on_a_frame():
    """crop_resize_augment(frame, bboxes, params) = augment_crops(crop_resize_u8(frame, bboxes), params), and both the
    restatement of the two resamplings"""
    img = np.load(os.path.join(HERE, 'golden', 'cropframe_small.npz'))['image']
    H, W = img.shape[:2]
    rng = np.random.default_rng(3)
    S, L = 32, 6
    xy = rng.uniform([-5, -5], [W - 30, H - 30], (L, 2))
    bb = np.concatenate([xy, xy + rng.uniform(8, 60, (L, 2))], 1)
    params = augment.RandomResizedCropFlip(S).draw(L, torch.Generator().manual_seed(9))
    frame = torch.from_numpy(img).to(DEV)
    a, a8 = CR.crop_resize_augment(frame, bb, params, size=S, return_u8=True)
    b, b8 = CR.augment_crops(CR.crop_resize_u8(frame, bb, S), params, return_u8=True)
    assert torch.equal(a8, b8) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    from oracle.crops_ref import crop_resize_normalize
    first, _ = crop_resize_normalize(img, bb, S)
    want_u8, want_f = augment_ref.augment(first, params)
    assert np.array_equal(a8.cpu().numpy(), want_u8) and np.array_equal(a.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
