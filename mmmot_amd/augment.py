"""The reference's training augmentation of the detection crops (utils/build_util.py:110-144, ``train_transform``):
``RandomResizedCrop(input_size)`` -> ``RandomHorizontalFlip()`` -> ``ToTensor`` -> ``Normalize``, applied to the 8-bit
``input_size`` x ``input_size`` crop of every detection (dataset/patchwise_dataset.py:161-171).

Two halves.  The random parameters are drawn here, on the host, as one small int32 table per sample -
``RandomResizedCropFlip.draw`` -> rows (top, left, h, w, flip).  The pixels are made on the device from that table in one
launch for all crops of the sample (``mmmot_amd.crops.augment_crops``, csrc/crop_augment.hip), bit for bit what Pillow and
torchvision make of the same parameters.

What is pinned is torchvision's DISTRIBUTION, not its random stream: ``draw`` restates the documented algorithm of
``RandomResizedCrop.get_params`` and ``RandomHorizontalFlip`` and takes its numbers from a ``torch.Generator`` the caller
passes in.  A run here does not repeat the draws of a torchvision run with the same seed - and could not repeat the
reference's: its 2019 torchvision drew from Python's ``random`` module, later versions from torch's global generator.
"""
import math

import numpy as np
import torch


def identity_params(L, S):
    """[L, 5] table of the whole crop, not flipped: the augmentation that changes nothing"""
    p = np.zeros((int(L), 5), dtype=np.int32)
    p[:, 2] = p[:, 3] = int(S)
    return p


def check_params(params, L, S):
    """the conditions ``augment_crops`` puts on a table, for L crops of side S: returns it as int32 [L, 5] or raises
    ValueError.  0 <= top, 1 <= h, top + h <= S; the same for left / w; flip 0 or 1."""
    p = np.asarray(params)
    if p.shape != (L, 5) or p.dtype.kind not in 'iu':
        raise ValueError('augmentation table: an integer array [%d, 5] (top, left, h, w, flip), got %s %s'
                         % (L, p.dtype, p.shape))
    p = p.astype(np.int64)
    for name, o, n in (('top', 0, 2), ('left', 1, 3)):
        size = 'hw'[o]
        bad = np.nonzero((p[:, o] < 0) | (p[:, n] < 1) | (p[:, o] + p[:, n] > S))[0]
        if bad.size:
            i = int(bad[0])
            raise ValueError('augmentation table row %d: %s = %d, %s = %d leave the %d-pixel crop (0 <= %s, 1 <= %s, '
                             '%s + %s <= %d)' % (i, name, p[i, o], size, p[i, n], S, name, size, name, size, S))
    bad = np.nonzero((p[:, 4] != 0) & (p[:, 4] != 1))[0]
    if bad.size:
        raise ValueError('augmentation table row %d: flip = %d, must be 0 or 1' % (int(bad[0]), p[int(bad[0]), 4]))
    return np.ascontiguousarray(p, dtype=np.int32)


class RandomResizedCropFlip:
    """``RandomResizedCrop(size, scale, ratio)`` + ``RandomHorizontalFlip(p_flip)`` on a ``size`` x ``size`` image, as the
    table of their parameters."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), p_flip=0.5):
        self.size = int(size)
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.p_flip = float(p_flip)
        if self.size < 1:
            raise ValueError('RandomResizedCropFlip: size must be positive, got %d' % self.size)
        if not 0 < self.scale[0] <= self.scale[1] or not 0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError('RandomResizedCropFlip: scale and ratio are (min, max) with 0 < min <= max, got %s and %s'
                             % (self.scale, self.ratio))
        if not 0.0 <= self.p_flip <= 1.0:
            raise ValueError('RandomResizedCropFlip: p_flip is a probability, got %s' % self.p_flip)

    def _region(self, generator):
        S = self.size
        area = float(S * S)
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        u = torch.empty(2, dtype=torch.float64)
        for _ in range(10):
            u[0].uniform_(self.scale[0], self.scale[1], generator=generator)
            u[1].uniform_(lo, hi, generator=generator)
            target, aspect = area * float(u[0]), math.exp(float(u[1]))  # log-uniform aspect ratio
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= S and 0 < h <= S:
                top = int(torch.randint(0, S - h + 1, (1,), generator=generator))
                left = int(torch.randint(0, S - w + 1, (1,), generator=generator))
                return top, left, h, w
        # no attempt fitted: the centre crop with the image's ratio (1: a square) clamped into the range
        if 1.0 < self.ratio[0]:
            w, h = S, int(round(S / self.ratio[0]))
        elif 1.0 > self.ratio[1]:
            h, w = S, int(round(S * self.ratio[1]))
        else:
            w, h = S, S
        return (S - h) // 2, (S - w) // 2, h, w

    def draw(self, L, generator):
        """int32 ndarray [L, 5]: per crop (top, left, h, w, flip), the region first, then one Bernoulli(p_flip), crop
        after crop, all from ``generator`` (a host torch.Generator)."""
        if not isinstance(generator, torch.Generator) or generator.device.type != 'cpu':
            raise TypeError('RandomResizedCropFlip.draw: generator must be a host torch.Generator')
        out = np.zeros((int(L), 5), dtype=np.int32)
        for i in range(int(L)):
            out[i, :4] = self._region(generator)
            out[i, 4] = int(float(torch.rand(1, dtype=torch.float64, generator=generator)) < self.p_flip)
        return out


def build_augmentation(config):
    """The training augmentation of a reference ``augmentation:`` section (a mapping; every published config holds
    ``input_size: 224`` and ``test_resize: 224`` and nothing else): ``RandomResizedCropFlip(input_size)``.  The options
    no config sets - ``rotation`` > 0, ``colorjitter``, ``cutout`` - have no kernel and raise NotImplementedError;
    ``test_resize`` other than ``input_size`` would make the reference's evaluation transform resize again, which the
    device crops do not do: ValueError."""
    get = config.get if hasattr(config, 'get') else (lambda k, d=None: getattr(config, k, d))
    size = get('input_size')
    if size is None:
        raise ValueError("build_augmentation: the section needs 'input_size'")
    if get('rotation', 0) > 0:
        raise NotImplementedError('build_augmentation: rotation is not implemented on the device (no config sets it)')
    if get('colorjitter', None) is not None:
        raise NotImplementedError('build_augmentation: colorjitter is not implemented on the device (no config sets it)')
    if get('cutout', None) is not None:
        raise NotImplementedError('build_augmentation: cutout is not implemented on the device (no config sets it)')
    if get('test_resize', size) != size:
        raise ValueError('build_augmentation: test_resize = %s differs from input_size = %s' % (get('test_resize'), size))
    return RandomResizedCropFlip(int(size))
