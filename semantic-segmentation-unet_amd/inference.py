#!/usr/bin/env python3
"""`inference` -- caller of the eval-mode forward + argmax (reference UNet/inference.py), on the HIP engine.

Flags are the reference's (UNet/inference.py:234-241).  Behaviour kept: image -> float32 -> z-score over the whole image
(:201-206); reflect-pad bottom/right to a multiple of 16 (:30-47,143-157); images larger than 1024 px go through the
tiled path: zones of responsibility of 1024 - 2*radius with a halo of `radius` clamped at the borders, eval forward per
tile, halo stripped, pasted (:54-129); mask = argmax over classes, first maximum wins (:107,166), cast to
uint8/uint16/int32 by its maximum (:215-220), written as the reference's imsave call asks (:221-227): a deflate-compressed BigTIFF
in 1024 x 1024 tiles (tifffile when importable, else the writer below).  The argmax runs on the device (`unet_argmax`).  Reading:
.npy, or anything Pillow opens (the reference uses scikit-image, absent here).

Two drivers compute the same mask.  `segment_image` (the default) keeps the image on the device: the raw image goes up once, every
tile of `tile_plan` is cut out of the reflect padding, z-scored (`unet_image_tile_gather`), classified and pasted
(`unet_argmax_paste`) on the current stream without a host synchronisation, and one narrow mask comes back; the file of image i is
written by a worker thread while image i + 1 is segmented.  `_inference` / `_inference_tiling` (`host_pipeline=True`,
`--host_pipeline`) are the reference's line-for-line host loop.
"""
import argparse
import collections
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import components
from . import model as unet_model_module
from ._lib import lib
from .readers import zscore_normalize

TILE_SIZE = 1024
SIZE_FACTOR = unet_model_module.UNet.SIZE_FACTOR


def _pad_to_factor(img):
    if img.ndim not in (2, 3):
        raise IOError("Invalid number of dimensions for input image. Expecting HW or HWC dimension ordering.")
    if img.ndim == 2:
        img = img[:, :, None]
    pad_y = (-img.shape[0]) % SIZE_FACTOR
    pad_x = (-img.shape[1]) % SIZE_FACTOR
    if pad_x or pad_y:
        img = np.pad(img, ((0, pad_y), (0, pad_x), (0, 0)), mode="reflect")
    return img, pad_y, pad_x


def _predict(unet, tile_hwc):
    """HWC fp32 tile -> int32 [H,W] class map via the eval-mode forward and the device argmax."""
    x = torch.as_tensor(np.ascontiguousarray(tile_hwc.transpose(2, 0, 1))[None].astype(np.float32))
    e = unet.engine
    return e.argmax(e.forward(x, training=False))[0].cpu().numpy()


def _inference(img, unet, predict=_predict):
    """(`predict(unet, tile_hwc) -> int32 [H, W]`: the forward + argmax of one tile; the default runs the HIP engine.  The hook exists so that
    tests/test_inference_golden.py can drive this function's pad / crop index work with the same stand-in network as the fixtures made
    by the reference's own UNet/inference.py:139-173.)"""
    img, pad_y, pad_x = _pad_to_factor(img)
    mask = predict(unet, img)
    return mask[:mask.shape[0] - pad_y, :mask.shape[1] - pad_x]


def _inference_tiling(img, unet, tile_size, predict=_predict):
    img, pad_y, pad_x = _pad_to_factor(img)
    height, width = img.shape[:2]
    mask = np.zeros((height, width), dtype=np.int32)
    radius = unet.estimate_radius()
    assert tile_size % SIZE_FACTOR == 0 and radius % SIZE_FACTOR == 0
    zone = tile_size - 2 * radius
    assert zone >= radius
    for y0 in range(0, height, zone):
        for x0 in range(0, width, zone):
            y1, x1 = min(y0 + zone, height), min(x0 + zone, width)
            # halo of `radius` on every side that exists; the reference drops the far halo entirely when the padded
            # window would cross the image edge (UNet/inference.py:86-96), which is reproduced here
            ty0 = y0 - radius if y0 - radius >= 0 else 0
            tx0 = x0 - radius if x0 - radius >= 0 else 0
            ty1 = y0 + zone + radius if y0 + zone + radius <= height else height
            tx1 = x0 + zone + radius if x0 + zone + radius <= width else width
            pred = predict(unet, img[ty0:ty1, tx0:tx1])
            oy, ox = y0 - ty0, x0 - tx0
            mask[y0:y1, x0:x1] = pred[oy:oy + (y1 - y0), ox:ox + (x1 - x0)]
    return mask[:height - pad_y, :width - pad_x]


def tile_plan(height, width, tile_size, radius, tiled=None):
    """The (tile rect, zone rect) pairs the drivers above visit, in their order, for an image of `height` x `width` AFTER padding to a
    multiple of 16; rects are (y0, x0, h, w) in padded-image coordinates.  Pure host arithmetic.

    An image that fits in one tile is the single whole-image entry of `_inference` (`radius` is not looked at and may be None) -- the
    dispatch of `inference()`.  Anything larger is `_inference_tiling`'s loop: zones of responsibility of tile_size - 2 * radius, a
    halo of `radius` on every side that exists, and the reference's far-halo rule at the image edge (the far halo is dropped
    entirely when the padded window would cross the edge, UNet/inference.py:86-96).  `tiled=True` returns that loop whatever the size
    (what `_inference_tiling` does when called directly on an image between one zone and one tile), `tiled=False` the whole-image entry."""
    assert height > 0 and width > 0 and height % SIZE_FACTOR == 0 and width % SIZE_FACTOR == 0
    if tiled is None:
        tiled = height > tile_size or width > tile_size
    if not tiled:
        return [((0, 0, height, width), (0, 0, height, width))]
    assert tile_size % SIZE_FACTOR == 0 and radius % SIZE_FACTOR == 0
    zone = tile_size - 2 * radius
    assert zone >= radius
    plan = []
    for y0 in range(0, height, zone):
        for x0 in range(0, width, zone):
            y1, x1 = min(y0 + zone, height), min(x0 + zone, width)
            ty0 = y0 - radius if y0 - radius >= 0 else 0
            tx0 = x0 - radius if x0 - radius >= 0 else 0
            ty1 = y0 + zone + radius if y0 + zone + radius <= height else height
            tx1 = x0 + zone + radius if x0 + zone + radius <= width else width
            plan.append(((ty0, tx0, ty1 - ty0, tx1 - tx0), (y0, x0, y1 - y0, x1 - x0)))
    return plan


_RAW_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}      # unet_image_tile_gather's dtype argument


def _zscore_scalars(img_hwc):
    """Per channel (mean, std) as float32, std = 1 where the reader only subtracts the mean (std <= 1, UNet/imagereader.py:33-49).  The
    same numpy calls on the same contiguous float32 channel as `readers.zscore_normalize`, so the same scalars to the last bit."""
    c = img_hwc.shape[2]
    coef = np.empty((2, c), np.float32)
    for k in range(c):
        ch = np.ascontiguousarray(img_hwc[:, :, k], dtype=np.float32)
        std, mean = float(np.std(ch)), float(np.mean(ch))
        coef[0, k] = mean
        coef[1, k] = 1.0 if std <= 1.0 else std
    return coef


def _check_truth(truth, confusion, h, w):
    """the ground-truth class map of an h x w image as a contiguous uint8 / uint16 / int32 array (anything else is converted to int32)"""
    if truth is None or confusion is None:
        raise ValueError("scoring needs both `truth` and `confusion`")
    truth = np.asarray(truth)
    if truth.dtype.kind not in "iu":
        raise ValueError("the ground-truth class map must have an integer dtype, not %s" % truth.dtype)
    if truth.shape != (h, w):
        raise ValueError("the ground-truth class map is %s, the image %s" % (truth.shape, (h, w)))
    if truth.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int32)):
        truth = truth.astype(np.int32)
    return np.ascontiguousarray(truth)


def _host_confusion(mask, truth, confusion, ignore_label=-1):
    """what `unet_confusion_masks` counts, with np.bincount on the host: rows = truth, columns = prediction; truth == ignore_label is
    skipped (-1: nothing is), labels outside [0, K) go to confusion.out_of_range"""
    k = confusion.number_classes
    t, p = np.asarray(truth).astype(np.int64).ravel(), np.asarray(mask).astype(np.int64).ravel()
    keep = np.ones(t.shape, bool) if ignore_label == -1 else t != ignore_label
    inside = (t >= 0) & (t < k) & (p >= 0) & (p < k)
    sel = keep & inside
    confusion.add_counts(np.bincount(t[sel] * k + p[sel], minlength=k * k).reshape(k, k))
    confusion.out_of_range += int((keep & ~inside).sum())


TTA_CHOICES = (1, 2, 4, 8)
SegmentResult = collections.namedtuple("SegmentResult", ["mask", "confidence", "probabilities"])
InstanceResult = collections.namedtuple("InstanceResult", ["mask", "confidence", "probabilities", "labels", "count", "objects"])


def _check_instances(instances, connectivity, background, min_object_area, max_objects):
    """-> None when no instance stage is asked for, else (connectivity, background or -1, min_area, max_objects), checked"""
    if not instances and not min_object_area:
        return None
    return (connectivity,) + components._check_options(connectivity, background, min_object_area, max_objects)


def _check_tta(tta):
    if isinstance(tta, bool) or tta not in TTA_CHOICES:
        raise ValueError("tta must be one of %s (the identity, + the horizontal flip, all flips, the whole dihedral group), not %r"
                         % (list(TTA_CHOICES), tta))
    return int(tta)


def tta_apply(x_chw, t):
    """Transform code `t` (0..7) on a [C, th, tw] tile: bit 2 = transpose the two spatial axes, then bit 1 = flip rows, then bit 0 = flip
    columns -- the dihedral group of the square, 0 the identity (what `unet_image_tile_gather_tta` writes).  A view, not a copy."""
    if not 0 <= t <= 7:
        raise ValueError("transform code %r is not in 0..7" % (t,))
    x = np.asarray(x_chw)
    if t & 4:
        x = x.transpose(0, 2, 1)
    if t & 2:
        x = x[:, ::-1, :]
    if t & 1:
        x = x[:, :, ::-1]
    return x


def tta_invert(p_hwk, t):
    """The inverse of `tta_apply(., t)` on the NHWC side, a [th', tw', K] softmax: the steps undone in reverse order -- flip columns, flip
    rows, transpose back -- so that pixel (y, x) is the tile's again (what `unet_prob_accumulate` reads).  A view, not a copy."""
    if not 0 <= t <= 7:
        raise ValueError("transform code %r is not in 0..7" % (t,))
    p = np.asarray(p_hwk)
    if t & 1:
        p = p[:, ::-1, :]
    if t & 2:
        p = p[::-1, :, :]
    if t & 4:
        p = p.transpose(1, 0, 2)
    return p


def _segment_tta_host(img, unet, tile_size, tta=1):
    """Z-scored HWC image -> (mask int32 [H, W], confidence fp32 [H, W], probabilities fp32 [H, W, K]): the host statement of the device
    pipeline with test-time augmentation.  Walks `tile_plan`; per tile the `tta` transforms 0 .. tta - 1 go through the eval forward with
    numpy flips around it and are summed in that order in float32, acc = ((P_0 + P_1) + P_2) + ...; mask = first maximum of the
    UNSCALED sum, confidence and probabilities = the sum times float32(1 / tta) (a power of two: exact).  Bit for bit what
    `segment_image` returns, given that the eval forward is deterministic for one input."""
    tta = _check_tta(tta)
    img, pad_y, pad_x = _pad_to_factor(img)
    hp, wp = img.shape[:2]
    tiled = hp > tile_size or wp > tile_size
    plan = tile_plan(hp, wp, tile_size, unet.estimate_radius() if tiled else None)
    e, k = unet.engine, unet.number_classes
    total = np.empty((hp, wp, k), np.float32)
    for (ty, tx, th, tw), (zy, zx, zh, zw) in plan:
        g = img[ty:ty + th, tx:tx + tw].transpose(2, 0, 1)
        acc = None
        for t in range(tta):
            x = torch.as_tensor(np.ascontiguousarray(tta_apply(g, t))[None].astype(np.float32))
            p = tta_invert(e.forward(x, training=False)[0].cpu().numpy(), t)
            if acc is None:
                acc = p.copy()
            else:
                acc += p
        oy, ox = zy - ty, zx - tx
        total[zy:zy + zh, zx:zx + zw] = acc[oy:oy + zh, ox:ox + zw]
    total = total[:hp - pad_y, :wp - pad_x]
    scale = np.float32(1.0 / tta)
    return np.argmax(total, axis=-1).astype(np.int32), total.max(axis=-1) * scale, total * scale


def _segment_host_pipeline(raw, unet, tile_size=TILE_SIZE, truth=None, confusion=None, ignore_label=-1, tta=1, return_confidence=False,
                           return_probabilities=False, instances=False, connectivity=8, background=0, min_object_area=0, max_objects=65536):
    """the reference's loop (UNet/inference.py:201-213): float32, z-score over the whole image, whole-image or tiled driver.  With
    truth / confusion the mask is scored on the host (the counts `segment_image` takes on the device).  tta / return_confidence /
    return_probabilities: as `segment_image`, through `_segment_tta_host`.  instances / min_object_area: as `segment_image`, through
    `components.label_components_host`, before the scoring."""
    tta = _check_tta(tta)
    inst = _check_instances(instances, connectivity, background, min_object_area, max_objects)
    if truth is not None or confusion is not None:
        truth = _check_truth(truth, confusion, raw.shape[0], raw.shape[1])
    img = raw.astype(np.float32)
    hwc = img[:, :, None] if img.ndim == 2 else img
    img = zscore_normalize(hwc.transpose(2, 0, 1)).transpose(1, 2, 0)
    conf = probs = None
    if tta > 1 or return_confidence or return_probabilities:
        mask, conf, probs = _segment_tta_host(img, unet, tile_size, tta)
    elif img.shape[0] > tile_size or img.shape[1] > tile_size:
        mask = _inference_tiling(img, unet, tile_size)
    else:
        mask = _inference(img, unet)
    if inst is not None:
        labels, count, objects, mask = components.label_components_host(mask, *inst)
    if confusion is not None:
        _host_confusion(mask, truth, confusion, ignore_label)
    if inst is not None:
        return InstanceResult(mask, conf if return_confidence else None, probs if return_probabilities else None, labels, count, objects)
    if return_confidence or return_probabilities:
        return SegmentResult(mask, conf if return_confidence else None, probs if return_probabilities else None)
    return mask


def segment_image(img, unet, tile_size=TILE_SIZE, radius=None, truth=None, confusion=None, ignore_label=-1, tta=1, return_confidence=False,
                  return_probabilities=False, instances=False, connectivity=8, background=0, min_object_area=0, max_objects=65536):
    """Raw image (HW or HWC, any dtype `_read` returns) -> class map [H, W], the mask `_inference` / `_inference_tiling` compute on the
    z-scored image, bit for bit, with the whole pipeline on the device: one upload of the image in its raw dtype (uint8 / uint16 / fp32;
    anything else is converted to fp32 on the host first, as the host path does), then per entry of `tile_plan` gather (reflect padding,
    z-score, NCHW) -> eval forward -> argmax + paste of the zone of responsibility, all on the current stream with no host
    synchronisation in between, then one download of the mask and one synchronise.  The mask is uint8 when number_classes <= 256, else
    int32 (the caller's `seg.astype(mask_dtype(seg.max()))` is unchanged).

    The per-channel mean and std stay ONE HOST PASS over the image (`_zscore_scalars`: numpy's pairwise float32 summation picks the
    scalars, and a device reduction cannot reproduce it bit for bit).  `radius`: None = `unet.estimate_radius()`, asked only when the
    image is tiled.  An image with a one-pixel axis has no reflection to pad it with on the device and takes the host path (which asks
    `unet.estimate_radius()` itself).

    truth + confusion (both or neither): a host ground-truth class map [H, W] of any integer dtype (uint8 / uint16 / int32 go up as they
    are, beside the image, from pinned memory; the rest as int32) and a metrics.ConfusionMatrix.  After the last paste ONE
    `unet_confusion_masks` launch on the same stream scores the device mask -- before the download's synchronise, still the only one --
    and adds the K x K counts to `confusion` (truth == ignore_label skipped, -1 skips nothing; labels outside [0, K) counted in
    confusion.out_of_range).  The returned mask is unchanged by it.

    tta in {1, 2, 4, 8} (anything else: ValueError, before any device work): test-time augmentation with the transforms 0 .. tta - 1 of
    `tta_apply` -- 2 adds the horizontal flip, 4 is all flips, 8 the whole dihedral group of the square.  Per tile and per transform:
    `unet_image_tile_gather_tta` -> eval forward -> `unet_prob_accumulate` (enqueued before the next forward, which reuses the softmax
    buffer), then the paste of the arg-max of the sum.  return_confidence / return_probabilities: the return value becomes
    `SegmentResult(mask, confidence, probabilities)` -- fp32 [H, W] probability of the winning class, fp32 [H, W, K] mean softmax, None for
    what was not asked -- written by `unet_argmax_paste_conf` (with tta = 1 straight from the softmax, no accumulate), each downloaded once
    behind the same single synchronise.  `_segment_tta_host` states the arithmetic; both agree bit for bit.  With tta = 1 and nothing
    asked for, the launches and the returned array are exactly those described above.

    instances=True, or min_object_area > 0: ONE `unet_label_components` call (components.label_components) follows the last paste on the same
    stream, before the scoring: connected components of the class map (`connectivity` 4 or 8; pixels of class `background` -- None: no such
    class -- belong to no object), objects of fewer than min_object_area pixels turned into background, numbered by first pixel.  The return
    value becomes `InstanceResult(mask, confidence, probabilities, labels, count, objects)`: mask the FILTERED class map (what truth /
    confusion then score), labels int32 [H, W] (0 = background), count the number of objects, objects int64 [max_objects, 8] (class, area,
    y0, x0, y1, x1, sum y, sum x; `components.objects_table` turns it into centroids), each one more non-blocking download behind the single
    synchronise.  `components.label_components_host` states it on the host; both agree exactly.  With neither option set nothing changes."""
    tta = _check_tta(tta)
    inst = _check_instances(instances, connectivity, background, min_object_area, max_objects)
    img = np.asarray(img)
    if img.ndim not in (2, 3):
        raise IOError("Invalid number of dimensions for input image. Expecting HW or HWC dimension ordering.")
    if img.ndim == 2:
        img = img[:, :, None]
    if img.dtype not in _RAW_DTYPES:
        img = img.astype(np.float32)
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    scoring = truth is not None or confusion is not None
    if scoring:
        truth = _check_truth(truth, confusion, h, w)
    hp, wp = h + (-h) % SIZE_FACTOR, w + (-w) % SIZE_FACTOR
    if h == 1 or w == 1:                             # padded to 16: unet_image_tile_gather refuses it (UNET_EINVAL)
        return _segment_host_pipeline(img, unet, tile_size, truth=truth, confusion=confusion, ignore_label=ignore_label, tta=tta,
                                      return_confidence=return_confidence, return_probabilities=return_probabilities, instances=instances,
                                      connectivity=connectivity, background=background, min_object_area=min_object_area, max_objects=max_objects)
    e, L = unet.engine, lib()
    dev = e.dev
    if scoring and (confusion.device != torch.empty(0, device=dev).device or confusion.number_classes != unet.number_classes):
        # (checked here: the kernel takes the matrix by pointer, and a host matrix -- legal for add_counts -- would be a fault on the device)
        raise ValueError("the confusion matrix must live on the network's device (%s, not %s) and count its %d classes (not %d)"
                         % (dev, confusion.device, unet.number_classes, confusion.number_classes))
    tiled = hp > tile_size or wp > tile_size
    if tiled and radius is None:
        radius = unet.estimate_radius()
    plan = tile_plan(hp, wp, tile_size, radius)
    coef_host = torch.from_numpy(_zscore_scalars(img)).pin_memory()
    raw_host = torch.from_numpy(img.reshape(-1).view(np.uint8)).pin_memory()
    coef = coef_host.to(dev, non_blocking=True)
    raw = raw_host.to(dev, non_blocking=True)
    if scoring:
        truth_host = torch.from_numpy(truth.reshape(-1).view(np.uint8)).pin_memory()
        truth_dev = truth_host.to(dev, non_blocking=True).view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[truth.dtype.itemsize]).view(h, w)
    k = unet.number_classes
    mdt = torch.uint8 if k <= 256 else torch.int32
    mask = torch.empty((h, w), dtype=mdt, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    tiles = {}
    extra = return_confidence or return_probabilities
    conf = torch.empty((h, w), dtype=torch.float32, device=dev) if return_confidence else None
    probs = torch.empty((h, w, k), dtype=torch.float32, device=dev) if return_probabilities else None
    accs = {}                                        # (th, tw) -> [th, tw, K] sum of the inverse-transformed softmaxes, tile coordinates
    for (ty, tx, th, tw), (zy, zx, zh, zw) in plan:
        if tta == 1 and not extra:
            x = tiles.get((th, tw))
            if x is None:
                x = tiles[(th, tw)] = torch.empty((1, c, th, tw), dtype=torch.float32, device=dev)
            st = e._stream()
            L.unet_image_tile_gather(ptr(raw), _RAW_DTYPES[img.dtype], h, w, c, ptr(coef[0]), ptr(coef[1]), ty, tx, th, tw, ptr(x), st)
            prob = e.forward(x, training=False)
            L.unet_argmax_paste(ptr(prob), k, th, tw, k, zy - ty, zx - tx, zh, zw, ptr(mask), mask.element_size(), w, zy, zx, h, w, st)
            continue
        st = e._stream()
        for t in range(tta):
            shape = (tw, th) if t & 4 else (th, tw)  # a transposed tile is a shape of its own
            x = tiles.get(shape)
            if x is None:
                x = tiles[shape] = torch.empty((1, c) + shape, dtype=torch.float32, device=dev)
            L.unet_image_tile_gather_tta(ptr(raw), _RAW_DTYPES[img.dtype], h, w, c, ptr(coef[0]), ptr(coef[1]), ty, tx, th, tw, t, ptr(x), st)
            src = e.forward(x, training=False)       # (the engine's softmax buffer: valid until the next forward only)
            if tta > 1:
                acc = accs.get((th, tw))
                if acc is None:
                    acc = accs[(th, tw)] = torch.empty((th, tw, k), dtype=torch.float32, device=dev)
                L.unet_prob_accumulate(ptr(src), k, th, tw, k, t, 1 if t == 0 else 0, ptr(acc), k, st)
        if tta > 1:
            src = acc
        if extra:
            L.unet_argmax_paste_conf(ptr(src), k, th, tw, k, 1.0 / tta, zy - ty, zx - tx, zh, zw, ptr(mask), mask.element_size(), w, zy, zx, h, w,
                                     None if conf is None else ptr(conf), w, None if probs is None else ptr(probs), st)
        else:
            L.unet_argmax_paste(ptr(src), k, th, tw, k, zy - ty, zx - tx, zh, zw, ptr(mask), mask.element_size(), w, zy, zx, h, w, st)
    if inst is not None:
        if inst[1] > 255 and mdt == torch.uint8:
            raise ValueError("the class map has no class %d to use as background" % inst[1])
        comp = components.label_components(mask, inst[0], inst[1], inst[2], inst[3], want_objects=True, want_mask=inst[2] > 0, stream=st, library=L)
        if comp.mask is not None:
            mask = comp.mask
        labels_out = torch.empty((h, w), dtype=torch.int32, pin_memory=True)
        labels_out.copy_(comp.labels, non_blocking=True)
        count_out = torch.empty((), dtype=torch.int32, pin_memory=True)
        count_out.copy_(comp.count, non_blocking=True)
        objects_out = torch.empty((inst[3], 8), dtype=torch.int64, pin_memory=True)
        objects_out.copy_(comp.objects, non_blocking=True)
    if scoring:
        confusion.update_from_masks(mask, truth_dev, ignore_label, st)
    out = torch.empty((h, w), dtype=mdt, pin_memory=True)
    out.copy_(mask, non_blocking=True)
    if conf is not None:
        conf_out = torch.empty((h, w), dtype=torch.float32, pin_memory=True)
        conf_out.copy_(conf, non_blocking=True)
    if probs is not None:
        probs_out = torch.empty((h, w, k), dtype=torch.float32, pin_memory=True)
        probs_out.copy_(probs, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    del raw_host, coef_host                          # (pinned sources of the uploads: alive until the synchronise above)
    if scoring:
        del truth_host
    if inst is not None:
        return InstanceResult(out.numpy(), conf_out.numpy() if conf is not None else None, probs_out.numpy() if probs is not None else None,
                              labels_out.numpy(), int(count_out.numpy()), objects_out.numpy())
    if extra:
        return SegmentResult(out.numpy(), conf_out.numpy() if conf is not None else None, probs_out.numpy() if probs is not None else None)
    return out.numpy()


def _read(path):
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    return np.array(Image.open(path))


def _write_bigtiff_tiled(path, mask, tile=1024, level=6):
    """The file `skimage.io.imsave(path, mask, compress=6, bigtiff=True, tile=(1024, 1024))` asks tifffile for (reference
    UNet/inference.py:221-222): a little-endian BigTIFF, one image, 1024 x 1024 tiles (edge tiles zero-padded to full size), every tile
    zlib-deflated at level 6 (Compression = 8, Adobe deflate), one sample per pixel, MinIsBlack.  A float32 array (the confidence map of
    --confidence_folder) is written the same way with SampleFormat 3 (IEEE floating point)."""
    import struct
    import zlib
    assert mask.ndim == 2 and mask.dtype in (np.uint8, np.uint16, np.int32, np.float32)
    h, w = mask.shape
    ty, tx = (h + tile - 1) // tile, (w + tile - 1) // tile
    tiles = []
    for j in range(ty):
        for i in range(tx):
            t = np.zeros((tile, tile), mask.dtype)
            blk = mask[j * tile:(j + 1) * tile, i * tile:(i + 1) * tile]
            t[:blk.shape[0], :blk.shape[1]] = blk
            tiles.append(zlib.compress(t.astype(mask.dtype.newbyteorder("<")).tobytes(), level))
    n = len(tiles)
    # (tag, type, count, value): types 3 = SHORT, 4 = LONG, 16 = LONG8; tags in ascending order
    fmt = 3 if mask.dtype == np.float32 else 2 if mask.dtype == np.int32 else 1      # SampleFormat: IEEE float, signed, unsigned
    entries = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, mask.dtype.itemsize * 8), (259, 3, 1, 8), (262, 3, 1, 1), (277, 3, 1, 1),
               (284, 3, 1, 1), (322, 4, 1, tile), (323, 4, 1, tile), (324, 16, n, None), (325, 16, n, None), (339, 3, 1, fmt)]
    ifd_off = 16
    ifd_len = 8 + 20 * len(entries) + 8
    arrays_off = ifd_off + ifd_len                    # tile offsets, then byte counts (only out of line when n > 1)
    data_off = arrays_off + (16 * n if n > 1 else 0)
    offs, cur = [], data_off
    for t in tiles:
        offs.append(cur)
        cur += len(t) + (len(t) & 1)                  # word-aligned tiles
    with open(path, "wb") as f:
        f.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, ifd_off))
        f.write(struct.pack("<Q", len(entries)))
        for tag, typ, cnt, val in entries:
            if tag == 324:
                val = offs[0] if n == 1 else arrays_off
            elif tag == 325:
                val = len(tiles[0]) if n == 1 else arrays_off + 8 * n
            f.write(struct.pack("<HHQQ", tag, typ, cnt, val))
        f.write(struct.pack("<Q", 0))
        if n > 1:
            f.write(struct.pack("<%dQ" % n, *offs))
            f.write(struct.pack("<%dQ" % n, *[len(t) for t in tiles]))
        for t in tiles:
            f.write(t)
            if len(t) & 1:
                f.write(b"\0")


def _write(path, mask, image_format="tif"):
    if path.endswith(".npy"):
        np.save(path, mask)
        return
    if "tif" in image_format:                         # UNet/inference.py:221-222
        try:
            import tifffile                           # what scikit-image's imsave delegates to
            tifffile.imwrite(path, mask, bigtiff=True, tile=(TILE_SIZE, TILE_SIZE), compression="zlib", compressionargs={"level": 6})
        except (ImportError, TypeError, ValueError):  # no tifffile, or one without the compression / compressionargs keywords: the writer below
            _write_bigtiff_tiled(path, mask, TILE_SIZE, 6)
        return
    from PIL import Image                             # UNet/inference.py:224-227 (compress where the format has it)
    try:
        Image.fromarray(mask).save(path, compress_level=6)
    except TypeError:
        Image.fromarray(mask).save(path)


def mask_dtype(max_label):
    """uint8 / uint16 / int32 by the largest label, the reference's rule (UNet/inference.py:215-220): 0..255 -> uint8,
    256..65535 -> uint16, anything else stays the arg-max's int32"""
    if 0 <= max_label <= 255:
        return np.uint8
    if 255 < max_label < 65536:
        return np.uint16
    return np.int32


def inference(checkpoint_filepath, image_folder, output_folder, number_classes, number_channels, image_format, compute_dtype=None,
              host_pipeline=False, mask_folder=None, ignore_label=-1, tta=1, confidence_folder=None, instance_folder=None, connectivity=8,
              background_class=0, min_object_area=0, max_objects=65536):
    """host_pipeline: the reference's host loop per tile (`_inference` / `_inference_tiling`) instead of `segment_image`; the masks are
    the same.  The file of image i is written by one worker thread while image i + 1 is segmented: files appear in order, every write
    has finished when this returns, and the first exception of a write is raised here.

    mask_folder (opt-in extra): ground-truth class maps with the images' file names.  Every mask is scored against its ground truth
    (on the device, or on the host with host_pipeline: the same counts) and the output folder also receives `scores.csv` -- one row per
    image and a final `total` row: image, pixel_accuracy, mean_iou, iou_0.., dice_0.. -- and `confusion.npy`, the summed int64 matrix
    (rows = truth).  A missing ground-truth file is an error before anything is segmented.

    tta (opt-in extra): test-time augmentation, see `segment_image`; the masks written (and scored) are those of the averaged softmax.
    confidence_folder (opt-in extra): receives one fp32 [H, W] file per image with the image's name, the probability of the winning
    class, written by the same worker thread right after the mask (.npy, or a TIFF like the mask's when the format is a TIFF).

    instance_folder (opt-in extra): receives one label map per image with the image's name (0 = background, objects numbered from 1 by
    first pixel; uint16 when the image has fewer than 65536 objects, else int32; .npy or a TIFF by the format), and the output folder
    `objects.csv` (one row per object: image, label, class, area, y0, x0, y1, x1, centroid_y, centroid_x; at most max_objects per image)
    and `object_counts.csv` (image, objects).  connectivity / background_class (-1: none) / min_object_area / max_objects: see
    `segment_image`.  min_object_area alone writes the filtered masks and none of the instance files."""
    tta = _check_tta(tta)
    inst_kw = {}
    if instance_folder is not None or min_object_area:
        background = None if background_class is None or background_class < 0 else background_class
        _check_instances(True, connectivity, background, min_object_area, max_objects)
        inst_kw = dict(instances=True, connectivity=connectivity, background=background, min_object_area=min_object_area, max_objects=max_objects)
    if instance_folder is not None:
        if image_format != "npy" and "tif" not in image_format:
            raise ValueError("--instance_folder writes uint16 / int32 files: --image_format must be npy or a TIFF, not %s" % image_format)
        os.makedirs(instance_folder, exist_ok=True)
    object_rows, count_rows = [], []
    if confidence_folder is not None:
        if image_format != "npy" and "tif" not in image_format:
            raise ValueError("--confidence_folder writes float32 files: --image_format must be npy or a TIFF, not %s" % image_format)
        os.makedirs(confidence_folder, exist_ok=True)
    os.makedirs(output_folder, exist_ok=True)
    names = sorted(f for f in os.listdir(image_folder) if f.endswith("." + image_format))
    if mask_folder is not None:
        for name in names:
            if not os.path.isfile(os.path.join(mask_folder, name)):
                raise FileNotFoundError("no ground-truth mask for image %s: %s is missing" % (name, os.path.join(mask_folder, name)))
    unet = unet_model_module.UNet(number_classes, 1, number_channels, 1e-4, compute_dtype=compute_dtype)
    unet.load_checkpoint(checkpoint_filepath)
    score_rows, total = [], np.zeros((number_classes, number_classes), np.int64)
    if mask_folder is not None:
        from . import metrics
        per_image = metrics.ConfusionMatrix(number_classes, device=unet.engine.dev)
    writer = ThreadPoolExecutor(max_workers=1)
    writes = []
    try:
        for i, name in enumerate(names):
            print("{}/{}".format(i, len(names)))
            raw = _read(os.path.join(image_folder, name))
            kw = {}
            if mask_folder is not None:
                per_image.reset_states()
                kw = dict(truth=_read(os.path.join(mask_folder, name)), confusion=per_image, ignore_label=ignore_label)
            if tta != 1 or confidence_folder is not None:
                kw.update(tta=tta, return_confidence=confidence_folder is not None)
            kw.update(inst_kw)
            seg = _segment_host_pipeline(raw, unet, **kw) if host_pipeline else segment_image(raw, unet, **kw)
            conf = labels = None
            if inst_kw:
                if instance_folder is not None:
                    labels = seg.labels.astype(np.uint16 if seg.count < 65536 else np.int32)
                    count_rows.append("%s,%d" % (name, seg.count))
                    for r in components.objects_table(seg.count, seg.objects):
                        object_rows.append("%s,%d,%d,%d,%d,%d,%d,%d,%r,%r" % ((name, r["label"], r["class"], r["area"]) + tuple(r["bbox"])
                                                                               + (float(r["centroid_y"]), float(r["centroid_x"]))))
                seg, conf = seg.mask, seg.confidence
            elif confidence_folder is not None:
                seg, conf = seg.mask, seg.confidence
            if mask_folder is not None:
                counts = per_image.result()
                total += counts
                score_rows.append(metrics.csv_row(name, metrics.summarize(counts)))
            seg = seg.astype(mask_dtype(int(seg.max())))
            if writes and writes[-1].done() and writes[-1].exception() is not None:
                break                                 # a write has failed: segment no further images, report it below
            writes.append(writer.submit(_write, os.path.join(output_folder, name), seg, image_format))
            if conf is not None:                      # the same single worker: behind the mask of this image, before the next one's
                writes.append(writer.submit(_write, os.path.join(confidence_folder, name), conf, image_format))
            if labels is not None:
                writes.append(writer.submit(_write, os.path.join(instance_folder, name), labels, image_format))
    finally:
        writer.shutdown(wait=True)                    # drain: every submitted write has run (or failed) before this returns
    for f in writes:
        f.result()                                    # re-raises the first exception of a write, in file order
    if mask_folder is not None:
        with open(os.path.join(output_folder, "scores.csv"), "w") as f:
            f.write(metrics.csv_header("image", number_classes) + "\n")
            f.writelines(r + "\n" for r in score_rows + [metrics.csv_row("total", metrics.summarize(total))])
        np.save(os.path.join(output_folder, "confusion.npy"), total)
    if instance_folder is not None:
        with open(os.path.join(output_folder, "objects.csv"), "w") as f:
            f.write("image,label,class,area,y0,x0,y1,x1,centroid_y,centroid_x\n")
            f.writelines(r + "\n" for r in object_rows)
        with open(os.path.join(output_folder, "object_counts.csv"), "w") as f:
            f.write("image,objects\n")
            f.writelines(r + "\n" for r in count_rows)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="inference", description="Script to detect stars with the selected unet model")
    ap.add_argument("--checkpoint_filepath", dest="checkpoint_filepath", type=str, required=True)
    ap.add_argument("--image_folder", dest="image_folder", type=str, required=True)
    ap.add_argument("--output_folder", dest="output_folder", type=str, required=True)
    ap.add_argument("--number_classes", dest="number_classes", type=int, required=True)
    ap.add_argument("--number_channels", dest="number_channels", type=int, required=True)
    ap.add_argument("--image_format", dest="image_format", type=str, default="tif")
    ap.add_argument("--compute_dtype", choices=["fp32", "bf16"], default=None,
                    help="opt-in extra: bf16 = mixed-precision contractions (fp32 is the reference's arithmetic and the default)")
    ap.add_argument("--host_pipeline", dest="host_pipeline", action="store_true",
                    help="cut, normalise, argmax and paste every tile on the host (the reference's loop) instead of on the device; same masks")
    ap.add_argument("--mask_folder", dest="mask_folder", type=str, default=None,
                    help="opt-in extra: ground-truth masks (same file names as the images); also writes scores.csv (per-image and total "
                         "pixel accuracy, mean IoU, per-class IoU and Dice) and confusion.npy into the output folder")
    ap.add_argument("--ignore_label", dest="ignore_label", type=int, default=-1,
                    help="with --mask_folder: ground-truth label whose pixels are not scored (-1: score every pixel)")
    ap.add_argument("--tta", dest="tta", type=int, choices=list(TTA_CHOICES), default=1,
                    help="opt-in extra: test-time augmentation -- average the softmax over the first N transforms of the square's dihedral "
                         "group (2: + horizontal flip, 4: all flips, 8: + the transpositions); N forwards per tile")
    ap.add_argument("--confidence_folder", dest="confidence_folder", type=str, default=None,
                    help="opt-in extra: also write the probability of the winning class per pixel, one float32 file per image with the "
                         "image's name (.npy or TIFF by --image_format)")
    ap.add_argument("--instance_folder", dest="instance_folder", type=str, default=None,
                    help="opt-in extra: also write an instance label map per image (connected components of the mask, 0 = background) with the "
                         "image's name, and objects.csv / object_counts.csv into the output folder")
    ap.add_argument("--connectivity", dest="connectivity", type=int, choices=[4, 8], default=8, help="with the instance options: 4- or 8-neighbours")
    ap.add_argument("--background_class", dest="background_class", type=int, default=0,
                    help="with the instance options: the class whose pixels belong to no object (-1: every class forms objects)")
    ap.add_argument("--min_object_area", dest="min_object_area", type=int, default=0,
                    help="opt-in extra: objects of fewer pixels are turned into background in the written masks (alone: no instance files)")
    ap.add_argument("--max_objects", dest="max_objects", type=int, default=65536, help="with --instance_folder: rows of objects.csv per image at most")
    a = ap.parse_args(argv)
    inference(a.checkpoint_filepath, a.image_folder, a.output_folder, a.number_classes, a.number_channels, a.image_format,
              compute_dtype=a.compute_dtype, host_pipeline=a.host_pipeline, mask_folder=a.mask_folder, ignore_label=a.ignore_label,
              tta=a.tta, confidence_folder=a.confidence_folder, instance_folder=a.instance_folder, connectivity=a.connectivity,
              background_class=a.background_class, min_object_area=a.min_object_area, max_objects=a.max_objects)


if __name__ == "__main__":
    main()
