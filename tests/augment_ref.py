"""NumPy restatement of the training augmentation's pixel half (TEST INFRASTRUCTURE ONLY): torchvision's
``resized_crop`` + ``hflip`` + ``to_tensor`` + ``normalize`` on an 8-bit S x S crop, out of the oracle's pieces.  Bit for
bit Pillow's result (tests/golden/augment_pil.npz; tests/test_augment_cpu.py compares with Pillow itself where it
imports)."""
import numpy as np

from oracle.crops_ref import crop_u8, resize_bilinear_u8, to_tensor_normalize


def augment_u8(src, row):
    """src uint8 [S, S, 3]; row = (top, left, h, w, flip) -> the augmented uint8 [S, S, 3]"""
    top, left, h, w, flip = (int(v) for v in row)
    S = src.shape[0]
    res = resize_bilinear_u8(crop_u8(src, (left, top, left + w, top + h)), S)
    return np.ascontiguousarray(res[:, ::-1]) if flip else res


def augment(crops, params):
    """crops uint8 [L, S, S, 3], params [L, 5] -> (uint8 [L, S, S, 3], fp32 [L, 3, S, S])"""
    u8 = np.stack([augment_u8(c, r) for c, r in zip(crops, params)])
    return u8, np.stack([to_tensor_normalize(u) for u in u8])
