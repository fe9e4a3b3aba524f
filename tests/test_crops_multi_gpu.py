"""The crops of several images in one launch pair (mmmot_crop_resize_norm_multi through mmmot_amd.crops) against the
single-image form, which tests/test_crops_gpu.py pins to Pillow: ``out`` and ``out_u8`` bit for bit the per-image results
concatenated, between poisoned guard bytes; images of different sizes, one with a row pitch above 3 W; an empty launch;
and the table checks that only Python can make."""
import math

import numpy as np
import pytest
import torch

from mmmot_amd import _lib
from mmmot_amd.crops import (MEAN, STD, boxes_of_bboxes, check_image_index, crop_resize_multi, crop_resize_normalize,
                             crop_resize_u8_multi, image_table)

pytestmark = pytest.mark.gpu

S = 32
SIZES = [(40, 56), (64, 48), (33, 71)]
BBOXES = [
    # leaves the frame on two sides | one pixel | an ordinary fractional box
    np.array([[-7.5, -4.2, 20.3, 18.9], [10.0, 12.0, 11.0, 13.0], [3.2, 5.7, 40.1, 30.4]]),
    np.zeros((0, 4)),
    # wider than 3 S (many taps) and leaving the frame right and below | taller than 3 S | small | one pixel at the corner
    np.array([[-30.0, 2.0, 70.9, 20.0], [5.0, -40.0, 30.0, 70.5], [60.2, 25.1, 69.0, 32.9], [70.0, 32.0, 71.0, 33.0]]),
]
GUARD = 64


def images(pitched=None):
    rng = np.random.default_rng(11)
    out = []
    for i, (H, W) in enumerate(SIZES):
        img = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        if i == pitched:  # the same pixels as a view into wider rows, filled with other bytes
            wide = torch.full((H, W + 5, 3), 0xA5, dtype=torch.uint8, device='cuda')
            wide[:, :W] = img
            img = wide[:, :W]
            assert img.stride(0) == 3 * (W + 5) and not img.is_contiguous()
        out.append(img)
    return out


_WANT = []


def want():
    """per-image ``crop_resize_normalize(..., return_u8=True)`` concatenated: computed once"""
    if not _WANT:
        res = [crop_resize_normalize(im, b, S, return_u8=True) for im, b in zip(images(), BBOXES)]
        _WANT.append((torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res])))
        assert max((boxes_of_bboxes(b)[:, 2:] - boxes_of_bboxes(b)[:, :2]).max() for b in BBOXES if len(b)) > 3 * S
    return _WANT[0]


def raw(frames, boxes, img_of, fill):
    """the C entry point writing between guard bytes"""
    N = boxes.shape[0]
    dev = frames[0].device
    no, nu = N * 3 * S * S, N * S * S * 3
    out = torch.empty(no + 2 * GUARD, dtype=torch.float32, device=dev)
    u8 = torch.empty(nu + 2 * GUARD, dtype=torch.uint8, device=dev)
    out.view(torch.uint8).fill_(fill)
    u8.fill_(fill)
    ext = int(max((boxes[:, 2] - boxes[:, 0]).max(), (boxes[:, 3] - boxes[:, 1]).max(), 1))
    kmax = 2 * int(math.ceil(max(1.0, ext / float(S)))) + 1
    table = torch.from_numpy(image_table(frames)).cuda()
    dboxes = torch.from_numpy(boxes).cuda()
    dimg = torch.from_numpy(np.asarray(img_of, dtype=np.int32)).cuda()
    ms = torch.tensor(list(MEAN) + list(STD), dtype=torch.float32, device=dev)
    work = torch.empty(N * 2 * S * (2 + kmax), dtype=torch.int32, device=dev)
    st = _lib.load().mmmot_crop_resize_norm_multi(table.data_ptr(), len(frames), dimg.data_ptr(), dboxes.data_ptr(), N, S,
                                                  kmax, ms.data_ptr(), work.data_ptr(), out[GUARD:].data_ptr(),
                                                  u8[GUARD:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return out, u8, no, nu


@pytest.mark.parametrize('pitched', [None, 2], ids=['packed', 'pitched'])
@pytest.mark.parametrize('fill', [0x00, 0xFF])
def test_bit_equal_to_the_single_form_between_guards(pitched, fill):
    frames = images(pitched)
    boxes = np.concatenate([boxes_of_bboxes(b) for b in BBOXES])
    img_of = np.repeat(np.arange(3), [len(b) for b in BBOXES])
    assert boxes.shape[0] == 7
    out, u8, no, nu = raw(frames, boxes, img_of, fill)
    w_out, w_u8 = want()
    assert torch.equal(out[GUARD:GUARD + no].view(torch.int32), w_out.reshape(-1).view(torch.int32))
    assert torch.equal(u8[GUARD:GUARD + nu], w_u8.reshape(-1))
    for buf, n in ((out.view(torch.uint8), 4 * no), (u8, nu)):
        g = 4 * GUARD if buf is not u8 else GUARD
        assert (buf[:g] == fill).all() and (buf[g + n:] == fill).all()


def test_the_kernel_skips_a_crop_with_an_image_index_outside_the_table():
    """what the C call cannot check on the host: crops 1 and 2 name images 3 and -1 and keep their poison, crop 0 is
    served"""
    frames = images()
    boxes = boxes_of_bboxes(BBOXES[0])
    out, u8, no, nu = raw(frames, boxes, [0, 3, -1], 0xFF)
    w_out, w_u8 = want()
    one = S * S * 3
    assert torch.equal(u8[GUARD:GUARD + one], w_u8[0].reshape(-1)) and (u8[GUARD + one:] == 0xFF).all()
    assert torch.equal(out[GUARD:GUARD + one].view(torch.int32), w_out[0].reshape(-1).view(torch.int32))
    assert (out.view(torch.uint8)[4 * (GUARD + one):] == 0xFF).all()


def test_python_forms():
    frames = images(1)
    w_out, w_u8 = want()
    u8, counts = crop_resize_u8_multi(frames, BBOXES, S)
    assert counts == [3, 0, 4] and u8.shape == (7, S, S, 3) and torch.equal(u8, w_u8)
    boxes = np.concatenate([boxes_of_bboxes(b) for b in BBOXES])
    img_of = np.repeat(np.arange(3), counts)
    out, u8 = crop_resize_multi(frames, boxes, img_of, S)
    assert torch.equal(out.view(torch.int32), w_out.view(torch.int32)) and torch.equal(u8, w_u8)
    # crops in any order of the images
    perm = np.array([4, 0, 6, 1, 3, 2, 5])
    out, u8 = crop_resize_multi(frames, boxes[perm], img_of[perm], S)
    assert torch.equal(out.view(torch.int32), w_out[perm].view(torch.int32)) and torch.equal(u8, w_u8[perm])


def test_an_empty_launch_is_a_no_op():
    frames = images()
    u8, counts = crop_resize_u8_multi(frames, [np.zeros((0, 4))] * 3, S)
    assert counts == [0, 0, 0] and u8.shape == (0, S, S, 3)
    p = frames[0].data_ptr()
    assert _lib.load().mmmot_crop_resize_norm_multi(p, 1, p, p, 0, S, 3, p, p, p, p, None) == 0
    assert _lib.load().mmmot_crop_resize_norm_multi(None, 1, None, None, 0, S, 3, None, None, None, None, None) == 0
    for bad in ((None, 1, p, p, 1, S, 3, p, p, p, p), (p, 0, p, p, 1, S, 3, p, p, p, p), (p, 1, p, p, -1, S, 3, p, p, p, p),
                (p, 1, p, p, 1, 257, 3, p, p, p, p), (p, 1, p, p, 1, S, 2, p, p, p, p), (p, 1, p, p, 1, S, 3, p, p, None, None)):
        assert _lib.load().mmmot_crop_resize_norm_multi(*bad, None) == -1
    torch.cuda.synchronize()


def test_the_table_is_checked_in_python():
    frames = images()
    boxes = boxes_of_bboxes(BBOXES[0])
    with pytest.raises(ValueError, match='image index 3'):
        crop_resize_multi(frames, boxes, [0, 3, 1], S)       # an image index of S
    with pytest.raises(ValueError, match='image index -1'):
        check_image_index([0, -1], 3)
    with pytest.raises(ValueError):
        crop_resize_multi(frames, boxes, [0, 1], S)          # two indices for three boxes
    with pytest.raises(ValueError):
        crop_resize_u8_multi(frames, BBOXES[:2], S)
    with pytest.raises(ValueError):
        crop_resize_multi(frames, boxes, [0, 0, 0], 257)
    with pytest.raises(TypeError):
        image_table([frames[0].to(torch.float32)])
    with pytest.raises(ValueError):
        image_table([frames[0].permute(1, 0, 2)])            # rows that are not rows
    with pytest.raises(RuntimeError):
        image_table([frames[0].cpu()])
    torch.cuda.synchronize()
