"""The border-distance weight map restated on the CPU, and the inputs its tests share.

A class map here is int64 [H, W] with -1 for an unlabeled pixel; the kernel takes the one-hot rows (`onehot`), an all-zero row for -1.
`d2_bruteforce` assumes nothing about the transform (no separability): for every pixel, the minimum over ALL border pixels of the squared
Euclidean distance in int64.  `weights_fp64` is the weight in double, with the exponent's constant the fp32 value the kernel is handed."""
import functools

import numpy as np

NONE = 2 ** 31 - 1                      # UNET_BORDER_NONE


def border_set(classmap):
    """bool [H, W]: labeled pixels with a labeled 4-neighbour inside the image of another class"""
    c = np.asarray(classmap)
    b = np.zeros(c.shape, bool)
    lab = c >= 0

    def mark(a, an, la, lan, out_a, out_an):
        d = la & lan & (a != an)
        out_a |= d
        out_an |= d

    mark(c[:-1], c[1:], lab[:-1], lab[1:], b[:-1], b[1:])
    mark(c[:, :-1], c[:, 1:], lab[:, :-1], lab[:, 1:], b[:, :-1], b[:, 1:])
    return b


def d2_bruteforce(classmap):
    """int64 [H, W]: min over every pixel of B of dy^2 + dx^2; NONE when B is empty"""
    b = border_set(classmap)
    h, w = b.shape
    ys, xs = np.nonzero(b)
    if len(ys) == 0:
        return np.full((h, w), NONE, np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    step = max(1, (1 << 22) // (h * w))                         # sites per slab: bounded memory
    for i in range(0, len(ys), step):
        d = (yy[None] - ys[i:i + step, None, None]) ** 2 + (xx[None] - xs[i:i + step, None, None]) ** 2
        out = np.minimum(out, d.min(0))
    return out


def d2_separable(classmap):
    """the same by another route: vertical distance to the nearest B pixel of each column, then the row minimum of dx^2 + g^2"""
    b = border_set(classmap)
    h, w = b.shape
    big = 1 << 30                                                # big^2 + dx^2 stays inside int64
    g = np.full((h, w), big, np.int64)
    for x in range(w):
        ys = np.nonzero(b[:, x])[0]
        if len(ys):
            g[:, x] = np.abs(np.arange(h)[:, None] - ys[None, :]).min(1)
    out = np.empty((h, w), np.int64)
    xs = np.arange(w)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                       # [x, x']
    for y in range(h):
        out[y] = (dx2 + g[y][None, :] ** 2).min(1)
    out[out >= big] = NONE
    return out


def weights_fp64(d2, w0, sigma, m=None):
    """(1 + w0 exp(d2 c)) m in double, c = the fp32 value of -1 / (2 sigma^2) (formed in double, rounded once); term 0 where d2 == NONE"""
    c = float(np.float32(-1.0 / (2.0 * float(sigma) ** 2)))
    d = np.asarray(d2, np.float64)
    term = np.where(np.asarray(d2) == NONE, 0.0, float(w0) * np.exp(np.where(np.asarray(d2) == NONE, 0.0, d) * c))
    w = 1.0 + term
    return w if m is None else w * np.asarray(m, np.float64)


def onehot(classmaps, k):
    """int [N, H, W] with -1 = unlabeled -> int32 one-hot [N, H, W, K]"""
    c = np.asarray(classmaps)
    return (c[..., None] == np.arange(k)).astype(np.int32)


def _blobs(rng, n, h, w, k, count):
    """random discs of random classes on a class-0 ground"""
    out = np.zeros((n, h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        for _ in range(count):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(2, max(3, min(h, w) // 4))
            out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(0, k)
    return out


def _build():
    rng = np.random.default_rng(41)
    cases = {}

    def add(name, classmaps, k, m=None):
        cases[name] = (np.asarray(classmaps, np.int64), k, m)

    add("one_pixel", np.zeros((1, 1, 1)), 2)
    row = np.zeros((1, 1, 67)); row[0, 0, 40:] = 1
    add("one_row", row, 2)
    add("one_column", row.transpose(0, 2, 1), 2)
    two = np.zeros((2, 16, 16)); two[1] = 1
    add("two_uniform_images", two, 2, rng.uniform(0.0, 2.0, (2, 16, 16)).astype(np.float32))
    wide = np.ones((1, 8, 1100)); wide[0, :, 0] = 0
    add("border_at_the_left_edge", wide, 2)
    tall = np.ones((1, 130, 5)); tall[0, 0, :] = 0
    add("border_at_the_top_edge", tall, 2)
    # K = 5 blobs in the left and upper part only: the columns from 90 on and the rows from 26 on hold no B pixel
    g = np.zeros((3, 37, 130), np.int64)
    g[:, :24, :84] = _blobs(rng, 3, 24, 84, 5, 9)
    add("blobs_k5", g, 5)
    yy, xx = np.mgrid[0:32, 0:32]
    add("checkerboard", ((yy + xx) % 2)[None], 2)
    yy, xx = np.mgrid[0:33, 0:65]
    add("diagonal", (2 * yy > xx).astype(np.int64)[None], 2)
    band = np.zeros((1, 24, 40), np.int64); band[0, :, 20:] = 1; band[0, :, 18:21] = -1
    add("unlabeled_band_between_classes", band, 2)
    blob = np.zeros((1, 24, 40), np.int64); blob[0, :, 30:] = 1; blob[0, 5:15, 8:20] = -1
    add("unlabeled_blob_beside_a_border", blob, 2)
    add("blobs_k2_with_pixel_weights", _blobs(rng, 2, 64, 64, 2, 6), 2, rng.uniform(0.0, 2.0, (2, 64, 64)).astype(np.float32))
    return cases


SHAPES = {"one_pixel": (1, 1, 1), "one_row": (1, 1, 67), "one_column": (1, 67, 1), "two_uniform_images": (2, 16, 16),
          "border_at_the_left_edge": (1, 8, 1100), "border_at_the_top_edge": (1, 130, 5), "blobs_k5": (3, 37, 130), "checkerboard": (1, 32, 32),
          "diagonal": (1, 33, 65), "unlabeled_band_between_classes": (1, 24, 40), "unlabeled_blob_beside_a_border": (1, 24, 40),
          "blobs_k2_with_pixel_weights": (2, 64, 64)}
NAMES = list(SHAPES)
SETTINGS = [(10.0, 5.0), (1.0, 0.5), (3.0, 40.0)]       # the usual one; a term that underflows one pixel away; one alive across the image


@functools.lru_cache(maxsize=None)
def _cases():
    c = _build()
    assert list(c) == NAMES and all(c[n][0].shape == SHAPES[n] for n in NAMES)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (class maps int64 [N,H,W] with -1 = unlabeled, K, caller pixel weights fp32 [N,H,W] or None, brute-force d2 int64 [N,H,W]);
    computed once, read-only"""
    cm, k, m = _cases()[name]
    d2 = np.stack([d2_bruteforce(c) for c in cm])
    for a in (cm, d2, m):
        if a is not None:
            a.setflags(write=False)
    return cm, k, m, d2
