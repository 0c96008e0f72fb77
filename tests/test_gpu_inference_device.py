"""GPU: whole-image inference on the device -- `unet_image_tile_gather`, `unet_argmax_paste`, `inference.segment_image` and the CLI's two
pipelines.  Everything is compared for EQUALITY: the gather against np.pad(zscore_normalize(...), mode="reflect") cut and transposed, the
paste against np.argmax, the masks of `segment_image` against the host loop (`_inference` / `_inference_tiling`) on the same engine."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DTYPES = {"uint8": (np.uint8, 0), "uint16": (np.uint16, 1), "fp32": (np.float32, 2)}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_image(h, w, c, dtype, seed, low_std_channel):
    """[h, w, c]: a smooth pattern plus noise over most of the dtype's range; `low_std_channel` (or None) holds two adjacent values only,
    so its std is <= 1 and the reader's rule subtracts the mean without dividing"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    top = {np.uint8: 255.0, np.uint16: 60000.0, np.float32: 900.0}[dtype]
    out = np.empty((h, w, c), dtype)
    for k in range(c):
        v = 0.5 + 0.3 * np.sin(yy / (5.0 + k)) * np.cos(xx / (4.0 + 2 * k)) + 0.1 * rng.standard_normal((h, w))
        v = np.clip(v, 0.0, 1.0) * top
        if k == low_std_channel:
            v = 7.0 + (rng.random((h, w)) < 0.4)
        if dtype == np.float32:
            v = v + rng.random((h, w)) * 0.37 - 11.0                       # not integer-valued, both signs
        out[:, :, k] = v.astype(dtype)
    return out


GATHER_TILES = {   # (y0, x0, th, tw) in padded coordinates: interior (vector and scalar widths), across the bottom-right corner, the whole padded image
    (37, 53): [(8, 12, 16, 32), (3, 5, 7, 9), (32, 32, 16, 32), (30, 46, 18, 18), (0, 0, 48, 64)],
    (5, 40): [(1, 4, 3, 20), (0, 3, 4, 7), (2, 30, 14, 18), (0, 16, 16, 32), (0, 0, 16, 48)],      # H = 5 -> 16 reflects more than once
}


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", sorted(GATHER_TILES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_tile_gather_is_the_reflect_padded_zscored_tile(hip, dt, hw, c):
    inf, readers = pkg("inference"), pkg("readers")
    npdt, code = DTYPES[dt]
    h, w = hw
    low = 1 if c == 3 else (0 if h == 5 else None)
    raw = _raw_image(h, w, c, npdt, seed=h * 7 + c, low_std_channel=low)
    z = readers.zscore_normalize(raw.astype(np.float32).transpose(2, 0, 1)).transpose(1, 2, 0)
    coef = inf._zscore_scalars(raw)
    stds = [float(np.std(np.ascontiguousarray(raw[:, :, k], dtype=np.float32))) for k in range(c)]
    if low is not None:
        assert stds[low] <= 1.0 and coef[1, low] == 1.0
    assert any(s > 1.0 for s in stds) or c == 1
    padded = np.pad(z, ((0, (-h) % 16), (0, (-w) % 16), (0, 0)), mode="reflect")
    d_raw = torch.from_numpy(raw.reshape(-1).view(np.uint8)).cuda()
    d_coef = torch.from_numpy(coef).cuda()
    for (y0, x0, th, tw) in GATHER_TILES[hw]:
        out = torch.full((1, c, th, tw), float("nan"), device="cuda")
        hip.unet_image_tile_gather(_ptr(d_raw), code, h, w, c, _ptr(d_coef[0]), _ptr(d_coef[1]), y0, x0, th, tw, _ptr(out), _stream())
        want = padded[y0:y0 + th, x0:x0 + tw].transpose(2, 0, 1)[None]
        assert np.array_equal(out.cpu().numpy(), want), (dt, hw, c, (y0, x0, th, tw))


def test_tile_gather_refuses_a_one_pixel_axis_that_needs_padding(hip):
    UnetHipError = pkg("_lib").UnetHipError
    raw = torch.arange(40, dtype=torch.float32, device="cuda")
    coef = torch.tensor([[0.0], [1.0]], device="cuda")
    out = torch.zeros((1, 1, 16, 48), device="cuda")
    args = lambda h, w, th, tw: (_ptr(raw), 2, h, w, 1, _ptr(coef[0]), _ptr(coef[1]), 0, 0, th, tw, _ptr(out), _stream())
    with pytest.raises(UnetHipError, match="bad argument"):
        hip.unet_image_tile_gather(*args(1, 40, 16, 48))
    with pytest.raises(UnetHipError, match="bad argument"):
        hip.unet_image_tile_gather(*args(40, 1, 48, 16))
    hip.unet_image_tile_gather(*args(1, 40, 1, 40))                          # no padding to read: the row itself
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(-1)[:40], np.arange(40, dtype=np.float32))


PASTE_ZONES = [   # (oy, ox, zh, zw), (my, mx), (Hm, Wm), pitch -- the tile is 24 x 40
    ((3, 5, 10, 13), (7, 9), (50, 61), 61),        # strictly inside the tile and the mask, odd sizes, nothing aligned
    ((4, 8, 16, 32), (8, 16), (40, 64), 64),       # every store a full aligned vector
    ((3, 5, 10, 13), (25, 30), (30, 37), 42),      # clipped at the mask's bottom and right edge (5 rows, 7 columns survive), pitch > Wm
    ((0, 0, 24, 40), (0, 0), (24, 40), 40),        # the whole tile
]


@pytest.mark.parametrize("esize", [1, 4])
@pytest.mark.parametrize("k,ldp", [(2, 2), (3, 3), (3, 4), (300, 300)])
def test_argmax_paste_writes_the_first_maximum_into_the_zone_only(hip, k, ldp, esize):
    th, tw = 24, 40
    rng = np.random.default_rng(k * 10 + ldp)
    prob = np.full((th, tw, ldp), 9.0, np.float32)                         # (the slack of ldp > K would win if it were read)
    prob[:, :, :k] = rng.integers(0, 4, (th, tw, k)).astype(np.float32) / 4.0       # four values: exact ties in almost every pixel
    am = np.argmax(prob[:, :, :k], axis=-1)
    tied = (prob[:, :, :k] == prob[:, :, :k].max(-1, keepdims=True)).sum(-1) > 1
    assert tied.mean() > 0.2 and am.max() > 0
    d_prob = torch.from_numpy(prob).cuda()
    npdt, sentinel = (np.uint8, 0xAB) if esize == 1 else (np.int32, -7)
    UnetHipError = pkg("_lib").UnetHipError
    for (oy, ox, zh, zw), (my, mx), (hm, wm), pitch in PASTE_ZONES:
        d_mask = torch.full((hm + 2, pitch), sentinel, dtype=torch.uint8 if esize == 1 else torch.int32, device="cuda")
        call = lambda: hip.unet_argmax_paste(_ptr(d_prob), ldp, th, tw, k, oy, ox, zh, zw, _ptr(d_mask), esize, pitch, my, mx, hm, wm, _stream())
        if esize == 1 and k > 256:
            with pytest.raises(UnetHipError, match="bad argument"):
                call()
            continue
        call()
        want = np.full((hm + 2, pitch), sentinel, npdt)
        rows, cols = min(zh, hm - my), min(zw, wm - mx)
        want[my:my + rows, mx:mx + cols] = am[oy:oy + rows, ox:ox + cols]
        assert np.array_equal(d_mask.cpu().numpy(), want), (k, ldp, esize, (oy, ox, zh, zw))


# ---- end to end on the real engine -------------------------------------------------------------------------------------------------------
_NETS = {}
# random-init weights.  The masks must not be flat (asserted below): with 3 channels / 4 classes seed 0 leaves class 1 on 0.2 % of the pixels
# of these images, seed 1 gives every class 2.8 % or more (measured on an MI355X); 1 channel / 2 classes splits 40 : 60 at seed 0
_SEED = {(1, 2): 0, (3, 4): 1}


def _net(c, k, compute_dtype=None):
    key = (c, k, compute_dtype)
    if key not in _NETS:
        _NETS[key] = pkg("model").UNet(k, 1, c, seed=_SEED[(c, k)], compute_dtype=compute_dtype)
    return _NETS[key]


def _uint16_image(h, w, c, seed):
    return _raw_image(h, w, c, np.uint16, seed, None)


E2E = [   # (channels, classes, (h, w), compute_dtype); tile_size 64, radius 16: 6 to 12 tiles of at most 64 x 64, edge tiles of several shapes
    (1, 2, (100, 75), None), (1, 2, (130, 64), None), (3, 4, (100, 75), None), (3, 4, (130, 64), None),
    (1, 2, (100, 75), "bf16"),
    (3, 4, (48, 40), None),                                                  # fits in one tile: the whole-image path
]


@pytest.mark.parametrize("c,k,hw,cd", E2E, ids=["c%dk%d_%dx%d_%s" % (c, k, hw[0], hw[1], cd or "fp32") for c, k, hw, cd in E2E])
def test_segment_image_equals_the_host_loop(c, k, hw, cd, monkeypatch):
    inf, readers = pkg("inference"), pkg("readers")
    net = _net(c, k, cd)
    tile, radius = 64, 16
    monkeypatch.setattr(net, "estimate_radius", lambda: radius, raising=False)
    h, w = hw
    raw = _uint16_image(h, w, c, seed=h + c)
    z = readers.zscore_normalize(raw.astype(np.float32).transpose(2, 0, 1)).transpose(1, 2, 0)
    tiled = h > tile or w > tile
    host = inf._inference_tiling(z, net, tile) if tiled else inf._inference(z, net)
    assert host.shape == (h, w)
    labels, counts = np.unique(host, return_counts=True)
    print("host mask labels", labels.tolist(), "pixel share", (counts / host.size).round(4).tolist())
    # equality of two constant masks would prove nothing
    assert len(labels) >= 2 and counts.min() >= 0.01 * host.size, (labels, counts)
    got = inf.segment_image(raw, net, tile_size=tile)                        # radius None: asks the (patched) estimate_radius
    assert got.dtype == np.uint8 and got.shape == (h, w)
    assert np.array_equal(got, host), "%d pixels differ" % int((got != host).sum())
    if tiled:
        assert np.array_equal(inf.segment_image(raw[:, :, 0] if c == 1 else raw, net, tile_size=tile, radius=radius), host)


def test_cli_device_and_host_pipelines_write_identical_files(tmp_path):
    inf = pkg("inference")
    net = _net(1, 2)
    stem = str(tmp_path / "checkpoint" / "ckpt")
    net.save_checkpoint(stem)
    imgs = tmp_path / "imgs"; imgs.mkdir()
    np.save(imgs / "a.npy", _uint16_image(70, 83, 1, 1)[:, :, 0])
    np.save(imgs / "b.npy", _raw_image(40, 40, 1, np.uint8, 2, None)[:, :, 0])
    np.save(imgs / "c.npy", _raw_image(33, 50, 1, np.float32, 3, None))
    common = ["--checkpoint_filepath", stem, "--image_folder", str(imgs), "--number_classes", "2", "--number_channels", "1", "--image_format", "npy"]
    inf.main(common + ["--output_folder", str(tmp_path / "dev")])
    inf.main(common + ["--output_folder", str(tmp_path / "host"), "--host_pipeline"])
    for name in ("a.npy", "b.npy", "c.npy"):
        dev, host = open(tmp_path / "dev" / name, "rb").read(), open(tmp_path / "host" / name, "rb").read()
        assert dev == host and len(dev) > 128, name
    assert sorted(os.listdir(tmp_path / "dev")) == ["a.npy", "b.npy", "c.npy"]
    # a write that fails on the worker thread is raised by inference(): here the second file's path is a directory
    bad = tmp_path / "bad"
    (bad / "b.npy").mkdir(parents=True)
    with pytest.raises(OSError):
        inf.main(common + ["--output_folder", str(bad)])
    assert os.path.isfile(bad / "a.npy")                                      # the write before it was drained, in order
