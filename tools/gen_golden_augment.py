#!/usr/bin/env python
"""Writes tests/golden/augment_pil.npz: what Pillow makes of the training augmentation's pixel half.

For S = 32 and S = 64: one structured-plus-noise source crop uint8 [S, S, 3], about 30 parameter rows (top, left, h, w,
flip) and per row ``img.crop((left, top, left + w, top + h)).resize((S, S), BILINEAR)``, with
``.transpose(FLIP_LEFT_RIGHT)`` behind it when flip is set - for a PIL image that is torchvision's ``resized_crop`` and
``hflip``.  Pillow and NumPy only.  The rows: the whole crop, 1 x 1 regions in both corners, strips one pixel wide and one
high, regions that touch the bottom-right edge, S x (S - 1) and (S - 1) x S, and random draws of
``RandomResizedCrop.get_params``'s algorithm (restated here on its own), each flipped and not.

    python tools/gen_golden_augment.py
"""
import math
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'augment_pil.npz')


def source(S, rng):
    """ramps in x and y, a diagonal sawtooth, a bright block - plus noise: every tap position matters"""
    yy, xx = np.mgrid[0:S, 0:S]
    img = np.stack([xx * 255 // (S - 1), yy * 255 // (S - 1), ((xx + 2 * yy) * 11) % 256], -1).astype(np.int64)
    img[S // 4:S // 2, S // 3:S // 3 + 5] = 250
    return np.clip(img + rng.integers(-30, 31, (S, S, 3)), 0, 255).astype(np.uint8)


def random_region(S, rng, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    for _ in range(10):
        area = S * S * rng.uniform(*scale)
        r = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
        if 0 < w <= S and 0 < h <= S:
            return int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w
    return 0, 0, S, S


def rows_for(S, rng):
    rows = [(0, 0, S, S), (0, 0, 1, 1), (S - 1, S - 1, 1, 1), (0, S // 3, S, 1), (S // 2, 0, 1, S),
            (S - 5, S - 9, 5, 9), (S // 2, S // 2, S - S // 2, S - S // 2), (0, 0, S, S - 1), (0, 0, S - 1, S),
            (1, 0, S - 1, S), (0, 1, S, S - 1), (3, 5, 2, S - 5)]
    rows += [random_region(S, rng) for _ in range(4)]
    out = []
    for i, r in enumerate(rows):
        out.append(r + (i % 2,))
    out += [r[:4] + (1 - r[4],) for r in out[:1] + out[-4:] + out[5:7] + out[11:12]]  # both flips of some
    out += [random_region(S, rng) + (int(rng.integers(0, 2)),) for _ in range(6)]
    return np.asarray(out, dtype=np.int32)


def pillow(img, row, S):
    top, left, h, w, flip = (int(v) for v in row)
    o = Image.fromarray(img).crop((left, top, left + w, top + h)).resize((S, S), Image.BILINEAR)
    if flip:
        o = o.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(o)


def main():
    rng = np.random.default_rng(20240)
    z = {'pillow_version': np.asarray(PIL.__version__)}
    for S in (32, 64):
        img = source(S, rng)
        rows = rows_for(S, rng)
        z['src_%d' % S] = img
        z['params_%d' % S] = rows
        z['out_%d' % S] = np.stack([pillow(img, r, S) for r in rows])
    np.savez_compressed(OUT, **z)
    print('wrote %s: %d bytes, rows %s' % (OUT, os.path.getsize(OUT), [len(z['params_%d' % S]) for S in (32, 64)]))


if __name__ == '__main__':
    main()
