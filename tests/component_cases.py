"""Connected components restated on the CPU, and the inputs the tests share.  Plain numpy / Python, no scipy.

`label_reference` assumes nothing about union-find, tiles or scans: it walks the image in row-major order and flood-fills every
unvisited foreground pixel with the next number, so the numbering by first pixel holds by construction.  Filter and object table are
direct reductions over `labels == i`."""
import functools

import numpy as np

NEIGHBOURS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def label_one(cm, connectivity, background):
    """int [H, W], background a class or None -> (labels int32 [H, W], count)"""
    cm = np.asarray(cm)
    h, w = cm.shape
    c = cm.tolist()
    lab = [[0] * w for _ in range(h)]
    nb = NEIGHBOURS[connectivity]
    count = 0
    for y in range(h):
        for x in range(w):
            if lab[y][x] or (background is not None and c[y][x] == background):
                continue
            count += 1
            cls = c[y][x]
            lab[y][x] = count
            stack = [(y, x)]
            while stack:
                py, px = stack.pop()
                for dy, dx in nb:
                    qy, qx = py + dy, px + dx
                    if 0 <= qy < h and 0 <= qx < w and not lab[qy][qx] and c[qy][qx] == cls:
                        lab[qy][qx] = count
                        stack.append((qy, qx))
    return np.array(lab, np.int32).reshape(h, w), count


def table_of(cm, lab, count, max_objects, fill=0):
    """int64 [max_objects, 8]: class, area, y0, x0, y1, x1, sum y, sum x of labels 1..min(count, max_objects); `fill` elsewhere"""
    t = np.full((max_objects, 8), fill, np.int64)
    for i in range(1, min(count, max_objects) + 1):
        ys, xs = np.nonzero(lab == i)
        t[i - 1] = [cm[ys[0], xs[0]], len(ys), ys.min(), xs.min(), ys.max(), xs.max(), ys.sum(), xs.sum()]
    return t


def label_reference(mask, connectivity=8, background=0, min_area=0, max_objects=64, fill=0):
    """mask int [N, H, W] -> (labels int32 [N,H,W], count int32 [N], objects int64 [N, max_objects, 8], filtered mask in the input's dtype)"""
    mask = np.asarray(mask)
    if connectivity not in (4, 8):
        raise ValueError("connectivity")
    if min_area > 0 and background is None:
        raise ValueError("min_area needs a background class")
    n, h, w = mask.shape
    labels, count = np.zeros((n, h, w), np.int32), np.zeros(n, np.int32)
    objects, out = np.full((n, max_objects, 8), fill, np.int64), mask.copy()
    for i in range(n):
        lab, cnt = label_one(mask[i], connectivity, background)
        if min_area > 0:
            new, kept = np.zeros(cnt + 1, np.int32), 0
            for j in range(1, cnt + 1):
                if int((lab == j).sum()) >= min_area:
                    kept += 1
                    new[j] = kept
            out[i][(lab > 0) & (new[lab] == 0)] = background
            lab, cnt = new[lab], kept
        labels[i], count[i] = lab, cnt
        objects[i] = table_of(mask[i], lab, cnt, max_objects, fill)
    return labels, count, objects, out


def canonical(lab):
    """any labelling with 0 = background -> the same partition numbered by first pixel in row-major order"""
    lab = np.asarray(lab)
    ids, first = np.unique(lab.ravel(), return_index=True)
    new = np.zeros(int(lab.max()) + 1, np.int32)
    rank = 0
    for k in np.argsort(first):
        if ids[k] > 0:
            rank += 1
            new[ids[k]] = rank
    return new[lab]


# ---- contents ---------------------------------------------------------------------------------------------------------------------------------
def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2 == 0).astype(np.int64)                 # class 1 on the even squares (the corner included), background between


def serpentine(h, w):
    """a one-pixel path through the whole image: every even row, joined alternately at the right and the left end"""
    m = np.zeros((h, w), np.int64)
    m[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def double_spiral(h, w):
    """a one-pixel rectangular spiral of class 1 walked inwards from the corner, and what it leaves free, itself a spiral, as class 2"""
    m = np.zeros((h, w), np.int64)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    inside = lambda a, b: 0 <= a < h and 0 <= b < w
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if inside(ny, nx) and m[ny, nx] == 0 and not (inside(ny + dy, nx + dx) and m[ny + dy, nx + dx] == 1):
                break
            dy, dx = dx, -dy                                     # turn right
        else:
            break
        y, x = ny, nx
        m[y, x] = 1
    m[m == 0] = 2
    return m


def nested_rings(h, w):
    """concentric one-pixel rectangles of classes 1, 2, 1, 2, ... touching each other: no background at all"""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx))
    return (1 + d % 2).astype(np.int64)


def u_shape(h, w):
    """two arms in the first and last column that meet only in the last row"""
    m = np.zeros((h, w), np.int64)
    m[:, 0] = 1; m[:, w - 1] = 1; m[h - 1, :] = 1
    return m


def comb(h, w):
    """teeth in every other column joined only by the last row: every tooth is its own component until the very end"""
    m = np.zeros((h, w), np.int64)
    m[:, 0::2] = 1
    m[h - 1, :] = 1
    return m


def percolation(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.int64)


def blobs(h, w, k, count, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(count):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 5 + 1))
        out[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(0, k)
    return out


SHAPES = [(1, 1), (1, 67), (67, 1), (17, 33), (64, 64), (65, 129), (130, 257)]
DENSITY = {4: 0.59, 8: 0.41}                                     # site percolation thresholds of the square lattice, near enough
CONTENTS = ["checkerboard", "serpentine", "double_spiral", "nested_rings", "u_shape", "comb", "background", "one_class", "blobs"]


def content(name, h, w):
    if name == "background":
        return np.zeros((h, w), np.int64)
    if name == "one_class":
        return np.ones((h, w), np.int64)
    if name == "blobs":
        return blobs(h, w, 4, 12, h * 1000 + w)
    return globals()[name](h, w)


@functools.lru_cache(maxsize=None)
def reference(name, h, w, connectivity, background=0, min_area=0, max_objects=64):
    """(mask int64 [1,H,W], labels, count, objects, filtered mask) of one named content; computed once, read-only"""
    if name.startswith("percolation"):
        m = percolation(h, w, DENSITY[connectivity], int(name.split("_")[1]))
    else:
        m = content(name, h, w)
    out = (m[None],) + label_reference(m[None], connectivity, background, min_area, max_objects, fill=-777)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch3(h, w):
    """three different images of one shape in one call: blobs of 4 classes, percolation noise, a comb"""
    m = np.stack([blobs(h, w, 4, 10, 7 + h), percolation(h, w, 0.5, 11 + w), comb(h, w)])
    m.setflags(write=False)
    return m


def filter_image():
    """one image holding squares of area 8, 9 and 10 (A - 1, A, A + 1 for A = 9), a second class and a single pixel"""
    m = np.zeros((24, 40), np.int64)
    m[1:3, 1:5] = 1                      # 8
    m[5:8, 1:4] = 1                      # 9
    m[10:12, 1:6] = 1                    # 10
    m[1:9, 20:30] = 2                    # 80, another class
    m[20, 35] = 3                        # 1
    m[14:17, 10:13] = 2                  # 9, class 2
    return m
