"""Training augmentation, host side (no GPU): the NumPy restatement against Pillow's fixture (and Pillow itself where it
imports), the parameter draws of mmmot_amd.augment, the table validation of crops.augment_crops, the refusals of
build_augmentation and the launcher's argument checks."""
import os

import numpy as np
import pytest
import torch

import augment_ref
from mmmot_amd import _lib, augment, crops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment_pil.npz')


def valid(p, S):
    return bool(((p[:, 0] >= 0) & (p[:, 2] >= 1) & (p[:, 0] + p[:, 2] <= S) & (p[:, 1] >= 0) & (p[:, 3] >= 1) &
                 (p[:, 1] + p[:, 3] <= S) & ((p[:, 4] == 0) | (p[:, 4] == 1))).all())


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [32, 64])
def test_restatement_equals_the_pillow_fixture(S):
    z = np.load(GOLD)
    src, params, want = z['src_%d' % S], z['params_%d' % S], z['out_%d' % S]
    assert len(params) >= 28 and valid(params, S) and want.dtype == np.uint8
    for i, row in enumerate(params):
        assert np.array_equal(augment_ref.augment_u8(src, row), want[i]), (S, i, row.tolist())


@pytest.mark.parametrize('S', [32, 64, 224])
def test_restatement_equals_pillow_on_fresh_regions(S):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(S)
    src = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    rows = [(0, 0, S, S, 1), (S - 1, 0, 1, 1, 0), (S - 17, S - 21, 17, 21, 1)]
    for _ in range(4 if S == 224 else 12):
        h, w = int(rng.integers(1, S + 1)), int(rng.integers(1, S + 1))
        rows.append((int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w, int(rng.integers(0, 2))))
    for top, left, h, w, flip in rows:
        o = Image.fromarray(src).crop((left, top, left + w, top + h)).resize((S, S), Image.BILINEAR)
        if flip:
            o = o.transpose(Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(augment_ref.augment_u8(src, (top, left, h, w, flip)), np.asarray(o)), (top, left, h, w, flip)


# ---- the draws -------------------------------------------------------------------------------------------------------
def test_draw_rows_are_valid_and_repeat_with_the_seed():
    for S in (32, 224):
        aug = augment.RandomResizedCropFlip(S)
        a = aug.draw(500, torch.Generator().manual_seed(11))
        b = aug.draw(500, torch.Generator().manual_seed(11))
        c = aug.draw(500, torch.Generator().manual_seed(12))
        assert a.dtype == np.int32 and a.shape == (500, 5) and valid(a, S)
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        area = a[:, 2].astype(np.int64) * a[:, 3] / float(S * S)
        # scale = (0.08, 1): the rounding of w and h moves an area by at most (w + h + 1) / S^2 around its draw
        assert area.min() > 0.08 - 3.0 / S and area.max() <= 1.0 and area.std() > 0.15
        ratio = a[:, 3] / a[:, 2]
        assert ratio.min() > 0.6 and ratio.max() < 1.6 and (ratio < 0.95).any() and (ratio > 1.05).any()
        assert len({tuple(r[:2]) for r in a.tolist()}) > 50  # tops and lefts vary


def test_draw_leaves_the_global_generator_alone():
    torch.manual_seed(5)
    want = torch.rand(3)
    torch.manual_seed(5)
    augment.RandomResizedCropFlip(64).draw(20, torch.Generator().manual_seed(1))
    assert torch.equal(torch.rand(3), want)


def test_draw_whole_crop_and_fallback():
    S = 48
    g = torch.Generator().manual_seed(3)
    whole = augment.RandomResizedCropFlip(S, scale=(1, 1), ratio=(1, 1)).draw(40, g)
    assert (whole[:, :4] == [0, 0, S, S]).all()
    assert np.array_equal(augment.identity_params(40, S)[:, :4], whole[:, :4])
    assert (augment.identity_params(40, S)[:, 4] == 0).all()
    # a ratio range no attempt can satisfy at this scale: w = h = round(sqrt(1.5) S) > S ten times -> the centre crop
    # with the square's ratio, 1, inside the range: the whole crop
    fb = augment.RandomResizedCropFlip(S, scale=(1.5, 1.5), ratio=(1, 1)).draw(40, g)
    assert (fb[:, :4] == [0, 0, S, S]).all()
    fb = augment.RandomResizedCropFlip(S, scale=(2, 3)).draw(40, g)  # the default ratio range around 1 likewise
    assert (fb[:, :4] == [0, 0, S, S]).all()
    # a ratio range that excludes the square's: the centre crop with the ratio clamped to its nearer end
    tall = augment.RandomResizedCropFlip(S, scale=(1, 1), ratio=(2, 3)).draw(5, g)
    assert (tall[:, :4] == [S // 4, 0, S // 2, S]).all()
    wide = augment.RandomResizedCropFlip(S, scale=(1, 1), ratio=(0.25, 0.5)).draw(5, g)
    assert (wide[:, :4] == [0, S // 4, S, S // 2]).all()


def test_flip_share():
    p = augment.RandomResizedCropFlip(32).draw(10000, torch.Generator().manual_seed(0))
    assert abs(p[:, 4].mean() - 0.5) <= 0.02
    assert augment.RandomResizedCropFlip(32, p_flip=0.0).draw(50, torch.Generator().manual_seed(0))[:, 4].sum() == 0
    assert augment.RandomResizedCropFlip(32, p_flip=1.0).draw(50, torch.Generator().manual_seed(0))[:, 4].sum() == 50


def test_draw_refuses_bad_arguments():
    with pytest.raises(ValueError):
        augment.RandomResizedCropFlip(32, scale=(0.5, 0.2))
    with pytest.raises(ValueError):
        augment.RandomResizedCropFlip(32, ratio=(0.0, 1.0))
    with pytest.raises(TypeError):
        augment.RandomResizedCropFlip(32).draw(3, None)


# ---- the table validation, before the library is touched -------------------------------------------------------------
@pytest.mark.parametrize('col,val', [(0, -1), (0, 8), (2, 0), (2, 9), (1, -1), (1, 8), (3, 0), (3, 9), (4, 2), (4, -1)])
def test_augment_crops_refuses_an_invalid_table(monkeypatch, col, val):
    def no_library():
        raise AssertionError('the table must be refused before the library is loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    S = 8
    u8 = torch.zeros(2, S, S, 3, dtype=torch.uint8)  # a host tensor: the table is looked at first
    p = augment.identity_params(2, S)
    p[1, col] = val
    with pytest.raises(ValueError):
        crops.augment_crops(u8, p)
    p = augment.identity_params(2, S)
    p[0, :4] = (3, 2, 6, 7)  # top + h and left + w leave the crop
    with pytest.raises(ValueError):
        crops.augment_crops(u8, p)


def test_augment_crops_refuses_shapes_and_host_crops(monkeypatch):
    monkeypatch.setattr(_lib, 'load', lambda: (_ for _ in ()).throw(AssertionError('library loaded')))
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        crops.augment_crops(u8, augment.identity_params(3, 8))           # one row too many
    with pytest.raises(ValueError):
        crops.augment_crops(u8, augment.identity_params(2, 8).astype(np.float32))
    with pytest.raises(TypeError):
        crops.augment_crops(u8.float(), augment.identity_params(2, 8))
    with pytest.raises(RuntimeError):                                     # a valid table, but host crops: no CPU path
        crops.augment_crops(u8, augment.identity_params(2, 8))


# ---- build_augmentation ----------------------------------------------------------------------------------------------
def test_build_augmentation():
    aug = augment.build_augmentation({'input_size': 224, 'test_resize': 224})
    assert isinstance(aug, augment.RandomResizedCropFlip) and aug.size == 224
    assert aug.scale == (0.08, 1.0) and aug.ratio == (3 / 4, 4 / 3) and aug.p_flip == 0.5
    for extra in ({'rotation': 10}, {'colorjitter': [0.4, 0.4, 0.4]}, {'cutout': True, 'cutout_length': 16}):
        with pytest.raises(NotImplementedError):
            augment.build_augmentation(dict({'input_size': 224, 'test_resize': 224}, **extra))
    assert augment.build_augmentation({'input_size': 64, 'test_resize': 64, 'rotation': 0}).size == 64
    with pytest.raises(ValueError):
        augment.build_augmentation({'input_size': 224, 'test_resize': 256})


# ---- the launcher's argument checks (no launch, safe without a GPU) --------------------------------------------------
def test_launcher_argument_checks_without_gpu():
    lib = _lib.load()
    d = 4096  # never dereferenced: the argument checks come before any launch
    assert lib.mmmot_crop_augment(None, d, 1, 32, d, d, None, None) == -1      # no crops
    assert lib.mmmot_crop_augment(d, None, 1, 32, d, d, None, None) == -1      # no table
    assert lib.mmmot_crop_augment(d, d, 1, 32, d, None, None, None) == -1      # neither output
    assert lib.mmmot_crop_augment(d, d, 0, 32, d, d, d, None) == -1            # L < 1
    assert lib.mmmot_crop_augment(d, d, -3, 32, d, d, d, None) == -1
    assert lib.mmmot_crop_augment(d, d, 1, 0, d, d, d, None) == -1             # S < 1
    assert lib.mmmot_crop_augment(d, d, 1, 257, d, d, d, None) == -1           # S > 256
    assert lib.mmmot_abi_version() == 10
