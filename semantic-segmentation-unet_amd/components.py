"""Instance labels from class maps: connected components on the device (`unet_label_components`, csrc/components.hip), the host
restatement the `--host_pipeline` route uses, and the object table.

Definition (include/unet_hip.h has it in full): two pixels of one image are connected when they are 4- or 8-neighbours, carry the same
class and that class is not `background`.  labels = 0 on background, else 1 + the rank of the component among its image's components
ordered by the row-major index of each component's first pixel; `min_area` removes smaller components (their pixels become background,
the survivors keep their order); the object table is int64 [N, max_objects, 8]: class, area, y0, x0, y1, x1 (inclusive), sum y, sum x."""
import collections
import ctypes

import numpy as np
import torch

from ._lib import lib

Components = collections.namedtuple("Components", ["labels", "count", "objects", "mask"])
OBJECT_COLUMNS = ("class", "area", "y0", "x0", "y1", "x1", "sum_y", "sum_x")
OBJECT_DTYPE = np.dtype([("label", np.int32), ("class", np.int64), ("area", np.int64), ("bbox", np.int64, (4,)),
                         ("centroid_y", np.float64), ("centroid_x", np.float64)])
_ELEM = {torch.uint8: 1, torch.int32: 4}
_workspaces = {}                                     # (device index, N, H, W) -> uint8 tensor


def _check_options(connectivity, background, min_area, max_objects):
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, not %r" % (connectivity,))
    background = -1 if background is None else int(background)
    if background < -1:
        raise ValueError("background must be a class >= 0, or None / -1 for no background class")
    min_area, max_objects = int(min_area), int(max_objects)
    if min_area < 0:
        raise ValueError("min_area must be >= 0")
    if min_area > 0 and background < 0:
        raise ValueError("min_area needs a background class: removed components have to become something")
    if max_objects < 1:
        raise ValueError("max_objects must be >= 1")
    return background, min_area, max_objects


def label_components(mask, connectivity=8, background=0, min_area=0, max_objects=65536, want_objects=True, want_mask=None, stream=None,
                     library=None):
    """mask: device class map [H, W] or [N, H, W], uint8 or int32, rows contiguous (a pitched view is taken as it is).
    -> Components(labels int32, count int32 [N] (a 0-d tensor for a 2-D mask), objects int64 [N, max_objects, 8] or None, mask or None),
    device tensors shaped like the input, enqueued on `stream` (None: the current stream; a torch stream or a raw handle) with NO host
    synchronisation; the outputs are allocated, and the table zeroed, under that stream too, and `mask` must be ready on it.  objects is
    zero beyond min(count, max_objects) rows.  want_mask: None = only when min_area > 0; the filtered class map.
    The workspace is cached per (device, shape): calls of one shape belong on one stream."""
    background, min_area, max_objects = _check_options(connectivity, background, min_area, max_objects)
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.dim() in (2, 3) and mask.dtype in _ELEM and mask.numel() > 0):
        raise ValueError("mask must be a non-empty device tensor [H, W] or [N, H, W] of uint8 or int32")
    m3 = mask if mask.dim() == 3 else mask.unsqueeze(0)
    n, h, w = m3.shape
    if n * h * w >= 2 ** 31:
        raise ValueError("N * H * W must stay below 2^31")
    pitch = m3.stride(1) if h > 1 else w
    if m3.stride(2) != 1 or pitch < w or (n > 1 and m3.stride(0) != h * pitch) or (w == 1 and h > 1):
        m3 = m3.contiguous()
        pitch = w
    if background > 255 and m3.dtype == torch.uint8:
        raise ValueError("a uint8 class map has no class %d" % background)
    if want_mask is None:
        want_mask = min_area > 0
    L = library if library is not None else lib()
    dev = m3.device
    current = torch.cuda.current_stream(dev)
    if stream is None:
        stream = current
    elif not isinstance(stream, torch.cuda.Stream):  # a raw handle
        handle = (stream.value or 0) if isinstance(stream, ctypes.c_void_p) else int(stream)
        stream = current if handle == current.cuda_stream else torch.cuda.ExternalStream(handle, device=dev)
    key = (dev.index, n, h, w)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.stream(stream):                  # the allocations and the zero fill belong to the stream the kernels run on
        ws = _workspaces.get(key)
        if ws is None:
            ws = _workspaces[key] = torch.empty(L.unet_label_components_workspace(n, h, w), dtype=torch.uint8, device=dev)
        labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        objects = torch.zeros((n, max_objects, 8), dtype=torch.int64, device=dev) if want_objects else None
        out = torch.empty((n, h, w), dtype=m3.dtype, device=dev) if want_mask else None
        L.unet_label_components(ptr(m3), _ELEM[m3.dtype], pitch, n, h, w, connectivity, background, min_area, ptr(labels), ptr(count), ptr(out),
                                ptr(objects), max_objects, ptr(ws), ws.numel(), ctypes.c_void_p(stream.cuda_stream))
    if mask.dim() == 2:
        return Components(labels[0], count[0], objects[0] if objects is not None else None, out[0] if out is not None else None)
    return Components(labels, count, objects, out)


def objects_table(count, objects):
    """Host side, after the download: count (int) and objects int64 [max_objects, 8] of ONE image -> a structured array (OBJECT_DTYPE:
    label, class, area, bbox = (y0, x0, y1, x1) inclusive, centroid_y, centroid_x) of min(count, max_objects) rows.  With count [N] and
    objects [N, max_objects, 8]: a list of N such arrays."""
    objects = np.asarray(objects)
    if objects.ndim == 3:
        return [objects_table(c, o) for c, o in zip(np.asarray(count).reshape(-1), objects)]
    rows = min(int(count), objects.shape[0])
    o = objects[:rows]
    t = np.zeros(rows, OBJECT_DTYPE)
    t["label"] = np.arange(1, rows + 1)
    t["class"], t["area"], t["bbox"] = o[:, 0], o[:, 1], o[:, 2:6]
    t["centroid_y"] = o[:, 6] / np.maximum(o[:, 1], 1)
    t["centroid_x"] = o[:, 7] / np.maximum(o[:, 1], 1)
    return t


def _label_one_host(cm, connectivity, background):
    """int64 [H, W] -> (labels int32, count): union-find over the runs of equal class of each row, roots = smallest run index, so the
    numbering by first pixel is the order of the root runs"""
    h, w = cm.shape
    fg = np.ones((h, w), bool) if background < 0 else cm != background
    start = np.ones((h, w), bool)
    start[:, 1:] = cm[:, 1:] != cm[:, :-1]
    start &= fg                                      # first pixel of every foreground run (background runs carry no id)
    run_id = np.cumsum(start.ravel()).reshape(h, w) - 1
    run_id = np.where(fg, run_id, -1)                # (a pixel inside a run has counted exactly the starts up to its own run's)
    nruns = int(start.sum())
    parent = np.arange(nruns)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    shifts = (0,) if connectivity == 4 else (-1, 0, 1)
    for s in shifts:                                 # pixel (y, x) against (y - 1, x + s)
        lo, hi = max(0, -s), w - max(0, s)
        if hi <= lo or h < 2:
            continue
        a, b = run_id[1:, lo:hi], run_id[:-1, lo + s:hi + s]
        same = (a >= 0) & (b >= 0) & (cm[1:, lo:hi] == cm[:-1, lo + s:hi + s])
        pairs = np.unique(np.stack([a[same], b[same]], 1), axis=0)
        for x, y in pairs:
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    roots = np.array([find(i) for i in range(nruns)], np.int64)
    is_root = roots == np.arange(nruns)
    rank = np.cumsum(is_root)                        # 1-based rank of each root run, in row-major order of the runs' first pixels
    labels = np.zeros((h, w), np.int32)
    if nruns:
        labels[fg] = rank[roots[run_id[fg]]]
    return labels, int(is_root.sum())


def label_components_host(mask, connectivity=8, background=0, min_area=0, max_objects=65536):
    """The same definition in numpy (what `--host_pipeline` runs): mask [H, W] or [N, H, W] of any integer dtype ->
    (labels int32, count int32 [N] or an int, objects int64 [N, max_objects, 8] zero beyond the rows written, filtered mask in the
    input's dtype), shaped like the input."""
    background, min_area, max_objects = _check_options(connectivity, background, min_area, max_objects)
    mask = np.asarray(mask)
    m3 = mask if mask.ndim == 3 else mask[None]
    n, h, w = m3.shape
    labels, count = np.zeros((n, h, w), np.int32), np.zeros(n, np.int32)
    objects, out = np.zeros((n, max_objects, 8), np.int64), m3.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        lab, cnt = _label_one_host(m3[i].astype(np.int64), connectivity, background)
        area = np.bincount(lab.ravel(), minlength=cnt + 1)
        if min_area > 0:
            keep = area >= min_area
            keep[0] = False
            new = np.cumsum(keep) * keep             # old label -> new label, 0 for the removed
            out[i][(lab > 0) & (new[lab] == 0)] = background
            lab = new[lab].astype(np.int32)
            cnt = int(keep.sum())
            area = np.bincount(lab.ravel(), minlength=cnt + 1)
        labels[i], count[i] = lab, cnt
        rows = min(cnt, max_objects)
        if rows:
            sel = (lab > 0) & (lab <= rows)
            l1, ys, xs = lab[sel] - 1, yy[sel], xx[sel]
            o = objects[i]
            first = np.full(rows, h * w, np.int64)
            np.minimum.at(first, l1, (ys * w + xs))
            o[:rows, 0] = m3[i].ravel()[first]
            o[:rows, 1] = area[1:rows + 1]
            o[:rows, 2], o[:rows, 3], o[:rows, 4], o[:rows, 5] = h, w, -1, -1
            np.minimum.at(o[:, 2], l1, ys); np.minimum.at(o[:, 3], l1, xs)
            np.maximum.at(o[:, 4], l1, ys); np.maximum.at(o[:, 5], l1, xs)
            o[:rows, 6] = np.bincount(l1, weights=ys, minlength=rows).astype(np.int64)
            o[:rows, 7] = np.bincount(l1, weights=xs, minlength=rows).astype(np.int64)
    if mask.ndim == 2:
        return labels[0], int(count[0]), objects[0], out[0]
    return labels, count, objects, out
