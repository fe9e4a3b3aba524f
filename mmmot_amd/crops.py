"""Device image preparation: frame + 2D boxes -> the model input ``dets`` [N, 3, S, S].

Mirror of the per-detection loop of ``TestSequence._generate_img_lidar`` (reference
dataset/test_seq_dataset.py:212-218) with the valid-transform of utils/build_util.py:137-142:

    x1, y1, x2, y2 = floor(bbox[0]), floor(bbox[1]), ceil(bbox[2]), ceil(bbox[3])
    transform(img.crop((x1, y1, x2, y2)).resize((224, 224), Image.BILINEAR))

One launch pair for all detections of a frame (csrc/crop_resize.hip); the result is bit-identical to the
Pillow / torchvision pipeline and stays on the device.  No CPU fallback.  ``crop_resize_u8_multi`` does the same for the
frames of several sequences, of different sizes, in one launch pair (``mmmot_crop_resize_norm_multi``).

Training (dataset/patchwise_dataset.py:161-171 with the train-transform of utils/build_util.py:113-131): the same 8-bit
crop, then ``augment_crops`` - RandomResizedCrop + RandomHorizontalFlip + ToTensor + Normalize for given parameters, one
launch for all crops of a sample (csrc/crop_augment.hip; the parameters come from mmmot_amd.augment).
"""
import math

import numpy as np
import torch

from . import _lib
from .ops import _iptr, _ptr

MEAN = (0.485, 0.456, 0.406)   # utils/build_util.py:111-112
STD = (0.229, 0.224, 0.225)


def boxes_of_bboxes(bboxes):
    """float [N, 4] detections -> int32 [N, 4] crop boxes (floor top-left, ceil bottom-right)."""
    b = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)
    return np.stack([np.floor(b[:, 0]), np.floor(b[:, 1]), np.ceil(b[:, 2]), np.ceil(b[:, 3])], 1).astype(np.int32)


def crop_resize_u8(frame, bboxes, size=224):
    """The 8-bit crops only: device uint8 [N, size, size, 3] - the input ``TrackingNet.forward`` takes in place of the
    fp32 ``dets`` (ToTensor / Normalize are then applied inside the first trunk launch; the fp32 tensor never exists)."""
    return crop_resize_normalize(frame, bboxes, size, only_u8=True)


def crop_resize_normalize(frame, bboxes, size=224, mean=MEAN, std=STD, return_u8=False, only_u8=False):
    """frame: device uint8 [H, W, 3] (RGB); bboxes: [N, 4] floats (host).  Returns device fp32 [N, 3, size, size]
    (and the uint8 resized crops [N, size, size, 3] when ``return_u8``; ``only_u8``: just those)."""
    if not frame.is_cuda:
        raise RuntimeError('crop_resize_normalize needs a device frame; there is no CPU fallback')
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
        raise TypeError('frame must be uint8 [H, W, 3]')
    lib = _lib.load()
    frame = frame.contiguous()
    H, W = int(frame.shape[0]), int(frame.shape[1])
    boxes = boxes_of_bboxes(bboxes)
    N = boxes.shape[0]
    out = None if only_u8 else torch.empty(N, 3, size, size, dtype=torch.float32, device=frame.device)
    u8 = torch.empty(N, size, size, 3, dtype=torch.uint8, device=frame.device) if (return_u8 or only_u8) else None
    if N == 0:
        return u8 if only_u8 else ((out, u8) if return_u8 else out)
    ext = int(max((boxes[:, 2] - boxes[:, 0]).max(), (boxes[:, 3] - boxes[:, 1]).max(), 1))
    kmax = 2 * int(math.ceil(max(1.0, ext / float(size)))) + 1
    dboxes = torch.from_numpy(boxes).to(frame.device)
    ms = torch.tensor(list(mean) + list(std), dtype=torch.float32, device=frame.device)
    work = torch.empty(N * 2 * size * (2 + kmax), dtype=torch.int32, device=frame.device)
    st = lib.mmmot_crop_resize_norm(frame.data_ptr(), H, W, _iptr(dboxes), N, size, kmax, _ptr(ms), _iptr(work),
                                    None if out is None else _ptr(out), None if u8 is None else u8.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(st, 'mmmot_crop_resize_norm')
    return u8 if only_u8 else ((out, u8) if return_u8 else out)


def image_table(frames):
    """host int64 [S, 4] of (device address, H, W, row pitch in bytes) for device uint8 frames [H, W, 3]; a frame may be
    a view with a row pitch above 3 W (unit strides inside a row).  Everything the kernel cannot check is checked here."""
    rows = []
    for i, f in enumerate(frames):
        if not torch.is_tensor(f) or not f.is_cuda:
            raise RuntimeError('crop_resize_u8_multi needs device frames; there is no CPU fallback')
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise TypeError('frame %d must be uint8 [H, W, 3]' % i)
        if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]:
            raise ValueError('frame %d: pixels must be packed within a row and rows at least 3 W bytes apart' % i)
        rows.append((f.data_ptr(), int(f.shape[0]), int(f.shape[1]), int(f.stride(0))))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


def check_image_index(img_of, n_images):
    """int32 [N] per-crop image indices, refused unless every one lies in [0, n_images)"""
    img_of = np.asarray(img_of, dtype=np.int64).reshape(-1)
    if img_of.size and (img_of.min() < 0 or img_of.max() >= n_images):
        raise ValueError('crop_resize_multi: image index %d outside [0, %d)'
                         % (int(img_of.max() if img_of.max() >= n_images else img_of.min()), n_images))
    return img_of.astype(np.int32)


def crop_resize_multi(frames, boxes, img_of, size=224, mean=MEAN, std=STD, want_out=True, want_u8=True):
    """ONE launch pair for the crops of several frames (``mmmot_crop_resize_norm_multi``): ``boxes`` int32 [N, 4] crop
    boxes and ``img_of`` [N] the frame each is cut from.  Returns (fp32 [N, 3, size, size] or None, uint8
    [N, size, size, 3] or None), bit for bit what ``crop_resize_normalize`` gives per frame."""
    if not 1 <= int(size) <= 256:
        raise ValueError('crop_resize_multi: crops of side 1 .. 256, got %s' % (size,))
    table = image_table(frames)
    img_of = check_image_index(img_of, len(frames))
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    N = boxes.shape[0]
    if img_of.shape[0] != N:
        raise ValueError('crop_resize_multi: %d image indices for %d boxes' % (img_of.shape[0], N))
    if not len(frames):
        raise ValueError('crop_resize_multi: no frames')
    dev = frames[0].device
    out = torch.empty(N, 3, size, size, dtype=torch.float32, device=dev) if want_out else None
    u8 = torch.empty(N, size, size, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    if N == 0:
        return out, u8
    ext = int(max((boxes[:, 2] - boxes[:, 0]).max(), (boxes[:, 3] - boxes[:, 1]).max(), 1))
    kmax = 2 * int(math.ceil(max(1.0, ext / float(size)))) + 1  # for the largest box of the launch
    # ONE upload: [image table as int32 pairs | boxes | image indices | mean, std bits]
    S = len(frames)
    a, b, c = 8 * S, 8 * S + 4 * N, 8 * S + 5 * N
    stage = torch.empty(c + 6, dtype=torch.int32, pin_memory=True)
    stage[:a] = torch.from_numpy(table).view(torch.int32).reshape(-1)
    stage[a:b] = torch.from_numpy(boxes).reshape(-1)
    stage[b:c] = torch.from_numpy(img_of)
    stage[c:].view(torch.float32).copy_(torch.tensor(list(mean) + list(std), dtype=torch.float32))
    dbuf = stage.to(dev, non_blocking=True)
    work = torch.empty(N * 2 * size * (2 + kmax), dtype=torch.int32, device=dev)
    st = _lib.load().mmmot_crop_resize_norm_multi(
        dbuf.data_ptr(), S, _iptr(dbuf[b:c]), _iptr(dbuf[a:b]), N, int(size), kmax, _ptr(dbuf[c:].view(torch.float32)),
        _iptr(work), None if out is None else _ptr(out), None if u8 is None else u8.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, 'mmmot_crop_resize_norm_multi')
    return out, u8


def crop_resize_u8_multi(frames, bboxes_per_frame, size=224):
    """The 8-bit crops of several frames, whose sizes may differ, in one launch pair: ``frames`` device uint8 [H, W, 3]
    each, ``bboxes_per_frame`` per frame its [n, 4] float detections.  Returns (device uint8 [sum n, size, size, 3],
    the frames' crops one after the other, and the per-frame counts)."""
    if len(frames) != len(bboxes_per_frame):
        raise ValueError('crop_resize_u8_multi: %d frames, %d box lists' % (len(frames), len(bboxes_per_frame)))
    boxes = [boxes_of_bboxes(b) for b in bboxes_per_frame]
    counts = [int(b.shape[0]) for b in boxes]
    img_of = np.repeat(np.arange(len(frames)), counts)
    _, u8 = crop_resize_multi(frames, np.concatenate(boxes + [np.zeros((0, 4), np.int32)]), img_of, size,
                              want_out=False)
    return u8, counts


def u8_normalize(crops_u8, mean=MEAN, std=STD):
    """ToTensor + Normalize of device uint8 crops [L, S, S, 3] -> device fp32 [L, 3, S, S] (``mmmot_u8_normalize``): the
    evaluation transform's second half, for the training-mode forward, which does not take the bytes"""
    if not crops_u8.is_cuda:
        raise RuntimeError('u8_normalize needs device crops; there is no CPU fallback')
    if crops_u8.dtype != torch.uint8 or crops_u8.dim() != 4 or crops_u8.shape[3] != 3 or crops_u8.shape[1] != crops_u8.shape[2]:
        raise TypeError('u8_normalize: crops_u8 must be uint8 [L, S, S, 3]')
    lib = _lib.load()
    crops_u8 = crops_u8.contiguous()
    L, S = int(crops_u8.shape[0]), int(crops_u8.shape[1])
    out = torch.empty(L, 3, S, S, dtype=torch.float32, device=crops_u8.device)
    if L:
        ms = torch.tensor(list(mean) + list(std), dtype=torch.float32, device=crops_u8.device)
        _lib.check(lib.mmmot_u8_normalize(crops_u8.data_ptr(), L, S, _ptr(ms), _ptr(out),
                                          torch.cuda.current_stream(crops_u8.device).cuda_stream), 'mmmot_u8_normalize')
    return out


def augment_crops(crops_u8, params, mean=MEAN, std=STD, return_u8=False):
    """The reference's training transform (utils/build_util.py:113-131: RandomResizedCrop, RandomHorizontalFlip, ToTensor,
    Normalize) of the 8-bit crops, with the random parameters given: crops_u8 device uint8 [L, S, S, 3] (``crop_resize_u8``),
    params a host integer table [L, 5] of (top, left, h, w, flip) - ``augment.RandomResizedCropFlip.draw`` or
    ``augment.identity_params``.  One launch for all crops (csrc/crop_augment.hip).  Returns device fp32 [L, 3, S, S], the
    input of the training-mode forward; with ``return_u8`` also the augmented 8-bit crops [L, S, S, 3], bit for bit
    Pillow's ``crop((left, top, left + w, top + h)).resize((S, S), BILINEAR)`` (``.transpose(FLIP_LEFT_RIGHT)``).  The
    table is validated here, before anything is queued: ValueError for a region that leaves the crop."""
    from .augment import check_params
    if not torch.is_tensor(crops_u8) or crops_u8.dtype != torch.uint8 or crops_u8.dim() != 4 or crops_u8.shape[3] != 3 \
            or crops_u8.shape[1] != crops_u8.shape[2]:
        raise TypeError('augment_crops: crops_u8 must be uint8 [L, S, S, 3]')
    L, S = int(crops_u8.shape[0]), int(crops_u8.shape[1])
    if not 1 <= S <= 256:
        raise ValueError('augment_crops: crops of side 1 .. 256, got %d' % S)
    table = check_params(params, L, S)
    if not crops_u8.is_cuda:
        raise RuntimeError('augment_crops needs device crops; there is no CPU fallback')
    lib = _lib.load()
    crops_u8 = crops_u8.contiguous()
    dev = crops_u8.device
    out = torch.empty(L, 3, S, S, dtype=torch.float32, device=dev)
    u8 = torch.empty(L, S, S, 3, dtype=torch.uint8, device=dev) if return_u8 else None
    if L == 0:
        return (out, u8) if return_u8 else out
    # ONE upload: the table and the six floats behind it, in a pinned buffer of this call's own
    stage = torch.empty(L * 5 + 6, dtype=torch.int32, pin_memory=True)
    stage[:L * 5] = torch.from_numpy(table).reshape(-1)
    stage[L * 5:].view(torch.float32).copy_(torch.tensor(list(mean) + list(std), dtype=torch.float32))
    dbuf = stage.to(dev, non_blocking=True)
    st = lib.mmmot_crop_augment(crops_u8.data_ptr(), _iptr(dbuf[:L * 5]), L, S, _ptr(dbuf[L * 5:].view(torch.float32)),
                                _ptr(out), None if u8 is None else u8.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, 'mmmot_crop_augment')
    return (out, u8) if return_u8 else out


def crop_resize_augment(frame, bboxes, params, size=224, mean=MEAN, std=STD, return_u8=False):
    """frame + boxes -> the augmented model input: ``crop_resize_u8`` then ``augment_crops`` (two resamplings with
    Pillow's 8-bit crop between them, like the reference's dataset)."""
    return augment_crops(crop_resize_u8(frame, bboxes, size), params, mean, std, return_u8)
