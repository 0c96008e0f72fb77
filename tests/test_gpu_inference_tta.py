"""GPU: test-time augmentation and confidence maps of whole-image inference -- `unet_image_tile_gather_tta`, `unet_prob_accumulate`,
`unet_argmax_paste_conf`, `inference.segment_image(tta=, return_confidence=, return_probabilities=)` and the CLI's --tta /
--confidence_folder.  Everything new is a permutation, a fixed-order fp32 sum, a power-of-two scale and a comparison, so everything is
compared for EQUALITY: the kernels against `tta_apply` / `tta_invert` in numpy, the device pipeline against the host loop
(`_segment_host_pipeline`) on the same engine."""
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
    """[h, w, c]: a smooth pattern plus noise over most of the dtype's range (the images of tests/test_gpu_inference_device.py);
    `low_std_channel` (or None) holds two adjacent values only, so the reader's rule subtracts its mean without dividing"""
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
            v = v + rng.random((h, w)) * 0.37 - 11.0
        out[:, :, k] = v.astype(dtype)
    return out


# ---- per kernel --------------------------------------------------------------------------------------------------------------------------
GATHER_TILES = {   # (y0, x0, th, tw) in padded coordinates: non-square interior tiles (vector and scalar widths; 7 x 9 and 18 x 18 are less than
                   # one 32 x 32 staging block, 48 x 64 is several), across the bottom-right reflect corner, the whole padded image
    (37, 53): [(8, 12, 16, 32), (3, 5, 7, 9), (32, 32, 16, 32), (30, 46, 18, 18), (0, 0, 48, 64)],
    (5, 40): [(1, 4, 3, 20), (0, 3, 4, 7), (2, 30, 14, 18), (0, 16, 16, 32), (0, 0, 16, 48)],      # H = 5 -> 16 reflects more than once
}
GUARD = 96          # floats behind the output that must keep their sentinel


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", sorted(GATHER_TILES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_gather_tta_is_the_transform_of_the_plain_gather(hip, dt, hw, c):
    inf = pkg("inference")
    npdt, code = DTYPES[dt]
    h, w = hw
    low = 1 if c == 3 else (0 if h == 5 else None)
    raw = _raw_image(h, w, c, npdt, seed=h * 7 + c, low_std_channel=low)
    coef = inf._zscore_scalars(raw)
    d_raw = torch.from_numpy(raw.reshape(-1).view(np.uint8)).cuda()
    d_coef = torch.from_numpy(coef).cuda()
    for (y0, x0, th, tw) in GATHER_TILES[hw]:
        plain = torch.full((c, th, tw), float("nan"), device="cuda")
        hip.unet_image_tile_gather(_ptr(d_raw), code, h, w, c, _ptr(d_coef[0]), _ptr(d_coef[1]), y0, x0, th, tw, _ptr(plain), _stream())
        g = plain.cpu().numpy()
        assert np.isfinite(g).all() and g.std() > 0
        n = c * th * tw
        for t in range(8):
            buf = torch.full((n + GUARD,), -7.0, device="cuda")
            buf[:n] = float("nan")                                            # exactly th' * tw' * C floats, then the guard
            hip.unet_image_tile_gather_tta(_ptr(d_raw), code, h, w, c, _ptr(d_coef[0]), _ptr(d_coef[1]), y0, x0, th, tw, t, _ptr(buf), _stream())
            got = buf.cpu().numpy()
            want = np.ascontiguousarray(inf.tta_apply(g, t))
            assert want.shape == ((c, tw, th) if t & 4 else (c, th, tw))
            assert np.array_equal(got[:n].reshape(want.shape), want), (dt, hw, c, (y0, x0, th, tw), t)
            assert (got[n:] == -7.0).all(), (dt, hw, c, (y0, x0, th, tw), t)


def test_gather_tta_refuses_bad_arguments(hip):
    UnetHipError = pkg("_lib").UnetHipError
    raw = torch.arange(40 * 3, dtype=torch.float32, device="cuda")
    coef = torch.tensor([[0.0], [1.0]], device="cuda")
    out = torch.zeros((16 * 48,), device="cuda")
    args = lambda h, w, th, tw, t: (_ptr(raw), 2, h, w, 1, _ptr(coef[0]), _ptr(coef[1]), 0, 0, th, tw, t, _ptr(out), _stream())
    for t in (-1, 8):
        with pytest.raises(UnetHipError, match="bad argument"):
            hip.unet_image_tile_gather_tta(*args(3, 40, 16, 48, t))
    for t in (0, 3, 5):                                                       # a one-pixel axis with padding to read: no reflection exists
        with pytest.raises(UnetHipError, match="bad argument"):
            hip.unet_image_tile_gather_tta(*args(1, 40, 16, 48, t))
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


@pytest.mark.parametrize("k,ld", [(2, 2), (3, 4), (5, 5)])
@pytest.mark.parametrize("thw", [(24, 40), (7, 9)], ids=lambda s: "%dx%d" % s)
def test_prob_accumulate_is_the_ordered_sum_of_the_inverse_transforms(hip, thw, k, ld):
    inf = pkg("inference")
    th, tw = thw
    rng = np.random.default_rng(th * 100 + k * 10 + ld)

    def softmax_like(t):
        """[th', tw', ld]: multiples of 2**-10 in the first K floats (sums are exact whatever the order and the denormal mode), and a
        slack that would show in the sum if it were read"""
        shape = (tw, th) if t & 4 else (th, tw)
        p = np.full(shape + (ld,), 9.0, np.float32)
        p[:, :, :k] = rng.integers(0, 1025, shape + (k,)).astype(np.float32) / 1024.0
        return p

    for t in range(8):
        order = [t, (t + 1) % 8, (t + 3) % 8, (t + 6) % 8]                    # the first call and three further ones, transforms mixed
        probs = [softmax_like(u) for u in order]
        acc = torch.full((th, tw, ld), float("nan"), device="cuda")
        acc[:, :, k:] = -7.0
        want = None
        for i, (u, p) in enumerate(zip(order, probs)):
            d_p = torch.from_numpy(p).cuda()
            hip.unet_prob_accumulate(_ptr(d_p), ld, th, tw, k, u, 1 if i == 0 else 0, _ptr(acc), ld, _stream())
            q = inf.tta_invert(p[:, :, :k], u)
            if want is None:
                want = q.copy()
            else:
                want += q
            got = acc.cpu().numpy()
            assert want.dtype == np.float32 and np.array_equal(got[:, :, :k], want), (thw, k, ld, order[:i + 1])
            assert (got[:, :, k:] == -7.0).all(), (thw, k, ld, order[:i + 1])
        # first != 0 on a used accumulator overwrites it
        hip.unet_prob_accumulate(_ptr(d_p), ld, th, tw, k, order[-1], 1, _ptr(acc), ld, _stream())
        assert np.array_equal(acc.cpu().numpy()[:, :, :k], inf.tta_invert(probs[-1][:, :, :k], order[-1]))


def test_prob_accumulate_refuses_bad_arguments(hip):
    UnetHipError = pkg("_lib").UnetHipError
    th, tw, k = 7, 9, 3
    p = torch.zeros((th * tw * 4 + 8,), device="cuda")
    a = torch.zeros((th * tw * 4,), device="cuda")
    ok = lambda **kw: hip.unet_prob_accumulate(kw.get("p", _ptr(p)), kw.get("ldp", 4), th, tw, kw.get("k", k), kw.get("t", 0), 1,
                                               kw.get("a", _ptr(a)), kw.get("lda", 4), _stream())
    ok()
    for bad in (dict(t=8), dict(t=-1), dict(lda=2), dict(ldp=2), dict(k=0), dict(a=_ptr(p)), dict(a=ctypes.c_void_p(p.data_ptr() + 16))):
        with pytest.raises(UnetHipError, match="bad argument"):
            ok(**bad)


PASTE_ZONES = [   # (oy, ox, zh, zw), (my, mx), (Hm, Wm), pitch -- the tile is 24 x 40 (the zones of tests/test_gpu_inference_device.py)
    ((3, 5, 10, 13), (7, 9), (50, 61), 61),        # strictly inside the tile and the mask, odd sizes, nothing aligned
    ((4, 8, 16, 32), (8, 16), (40, 64), 64),       # every store a full aligned vector
    ((3, 5, 10, 13), (25, 30), (30, 37), 42),      # clipped at the mask's bottom and right edge (5 rows, 7 columns survive), pitch > Wm
    ((0, 0, 24, 40), (0, 0), (24, 40), 40),        # the whole tile
]


@pytest.mark.parametrize("esize", [1, 4])
@pytest.mark.parametrize("k,ldp", [(2, 2), (3, 4), (300, 300)])
def test_argmax_paste_conf_is_the_plain_paste_plus_scaled_probabilities(hip, k, ldp, esize):
    th, tw = 24, 40
    scale = 0.25                                                              # four accumulated transforms
    rng = np.random.default_rng(k * 10 + ldp)
    acc = np.full((th, tw, ldp), 9.0, np.float32)                            # (the slack of ldp > K would win if it were read)
    acc[:, :, :k] = rng.integers(0, 4, (th, tw, k)).astype(np.float32) / 4.0         # four values: exact ties in almost every pixel
    tied = (acc[:, :, :k] == acc[:, :, :k].max(-1, keepdims=True)).sum(-1) > 1
    assert tied.mean() > 0.2
    d_acc = torch.from_numpy(acc).cuda()
    mdt, npdt, sentinel = (torch.uint8, np.uint8, 0xAB) if esize == 1 else (torch.int32, np.int32, -7)
    UnetHipError = pkg("_lib").UnetHipError
    for (oy, ox, zh, zw), (my, mx), (hm, wm), pitch in PASTE_ZONES:
        new = lambda: torch.full((hm + 2, pitch), sentinel, dtype=mdt, device="cuda")
        d_mask, d_conf, d_prob = new(), torch.full((hm + 2, pitch), -3.0, device="cuda"), torch.full((hm + 1, wm, k), -3.0, device="cuda")

        def call(mask, conf, prob):
            hip.unet_argmax_paste_conf(_ptr(d_acc), ldp, th, tw, k, scale, oy, ox, zh, zw, _ptr(mask), esize, pitch, my, mx, hm, wm,
                                       None if conf is None else _ptr(conf), pitch, None if prob is None else _ptr(prob), _stream())

        if esize == 1 and k > 256:
            with pytest.raises(UnetHipError, match="bad argument"):
                call(d_mask, d_conf, d_prob)
            continue
        with pytest.raises(UnetHipError, match="bad argument"):               # nothing asked for: that is unet_argmax_paste
            call(d_mask, None, None)
        plain = new()
        hip.unet_argmax_paste(_ptr(d_acc), ldp, th, tw, k, oy, ox, zh, zw, _ptr(plain), esize, pitch, my, mx, hm, wm, _stream())
        call(d_mask, d_conf, d_prob)
        rows, cols = min(zh, hm - my), min(zw, wm - mx)
        zone = acc[oy:oy + rows, ox:ox + cols, :k]
        want_mask = np.full((hm + 2, pitch), sentinel, npdt)
        want_mask[my:my + rows, mx:mx + cols] = np.argmax(zone, axis=-1)
        want_conf = np.full((hm + 2, pitch), -3.0, np.float32)
        want_conf[my:my + rows, mx:mx + cols] = zone.max(-1) * np.float32(scale)
        want_prob = np.full((hm + 1, wm, k), -3.0, np.float32)
        want_prob[my:my + rows, mx:mx + cols] = zone * np.float32(scale)
        where = (k, ldp, esize, (oy, ox, zh, zw))
        assert np.array_equal(plain.cpu().numpy(), want_mask), where
        assert np.array_equal(d_mask.cpu().numpy(), plain.cpu().numpy()), where
        assert np.array_equal(d_conf.cpu().numpy(), want_conf), where
        assert np.array_equal(d_prob.cpu().numpy(), want_prob), where
        # either output alone
        m2, c2 = new(), torch.full((hm + 2, pitch), -3.0, device="cuda")
        call(m2, c2, None)
        assert np.array_equal(m2.cpu().numpy(), want_mask) and np.array_equal(c2.cpu().numpy(), want_conf), where
        m3, p3 = new(), torch.full((hm + 1, wm, k), -3.0, device="cuda")
        call(m3, None, p3)
        assert np.array_equal(m3.cpu().numpy(), want_mask) and np.array_equal(p3.cpu().numpy(), want_prob), where


# ---- end to end on the real engine -------------------------------------------------------------------------------------------------------
_NETS = {}
# random-init weights and seeds of tests/test_gpu_inference_device.py: the masks must not be flat (asserted below)
_SEED = {(1, 2): 0, (3, 4): 1}
TILE, RADIUS = 64, 16


def _net(c, k, compute_dtype=None):
    key = (c, k, compute_dtype)
    if key not in _NETS:
        _NETS[key] = pkg("model").UNet(k, 1, c, seed=_SEED[(c, k)], compute_dtype=compute_dtype)
    return _NETS[key]


def _uint16_image(h, w, c, seed):
    return _raw_image(h, w, c, np.uint16, seed, None)


@pytest.mark.parametrize("c,k,cd", [(1, 2, None), (3, 4, None), (1, 2, "bf16")], ids=["c1k2_fp32", "c3k4_fp32", "c1k2_bf16"])
def test_eval_forward_is_deterministic_for_one_input(c, k, cd):
    """the precondition of the bit-for-bit contract: two eval forwards of one 64 x 48 tile give identical bits"""
    net = _net(c, k, cd)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((1, c, 64, 48)).astype(np.float32)).cuda()
    e = net.engine
    first = e.forward(x, training=False).clone()
    other = torch.from_numpy(np.random.default_rng(6).standard_normal((1, c, 48, 64)).astype(np.float32)).cuda()
    e.forward(other, training=False)                                          # another shape in between, as the tta loop does
    second = e.forward(x, training=False)
    dev = (first - second).abs().max().item()
    print("largest deviation between two forwards of one tile:", dev)
    assert torch.equal(first, second), dev
    p = first.cpu().numpy()
    assert np.isfinite(p).all() and p.std() > 0


E2E = [   # (channels, classes, (h, w), compute_dtype, tta)
    (1, 2, (100, 75), None, 8), (1, 2, (130, 64), None, 8), (3, 4, (100, 75), None, 8), (1, 2, (100, 75), "bf16", 8),
    (3, 4, (48, 40), None, 8),                                               # fits in one tile: the whole-image path, non-square
    (1, 2, (100, 75), None, 2), (1, 2, (100, 75), None, 4),
]


@pytest.mark.parametrize("c,k,hw,cd,tta", E2E, ids=["c%dk%d_%dx%d_%s_tta%d" % (c, k, hw[0], hw[1], cd or "fp32", n) for c, k, hw, cd, n in E2E])
def test_segment_image_with_tta_equals_the_host_loop(c, k, hw, cd, tta, monkeypatch):
    inf = pkg("inference")
    net = _net(c, k, cd)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    h, w = hw
    raw = _uint16_image(h, w, c, seed=h + c)
    host = inf._segment_host_pipeline(raw, net, TILE, tta=tta, return_confidence=True, return_probabilities=True)
    dev = inf.segment_image(raw, net, tile_size=TILE, tta=tta, return_confidence=True, return_probabilities=True)
    assert isinstance(dev, inf.SegmentResult) and isinstance(host, inf.SegmentResult)
    assert dev.mask.dtype == np.uint8 and dev.mask.shape == (h, w)
    assert dev.confidence.dtype == np.float32 and dev.confidence.shape == (h, w)
    assert dev.probabilities.dtype == np.float32 and dev.probabilities.shape == (h, w, k)
    labels, counts = np.unique(host.mask, return_counts=True)
    plain = inf.segment_image(raw, net, tile_size=TILE)
    changed = int((plain != dev.mask).sum())
    print("mask labels", labels.tolist(), "share", (counts / host.mask.size).round(4).tolist(), "| confidence min %.6f max %.6f"
          % (host.confidence.min(), host.confidence.max()), "| pixels that tta=%d changes: %d" % (tta, changed))
    # what keeps the comparison honest: a mask that is not flat, probabilities that are probabilities, an ensemble that does something
    # (at least two labels hold 1 % of the pixels each.  Not "every label that occurs": the ensemble of the random-init 4-class net leaves
    # classes 1 and 2 on 0.7 % and 0.3 % of the 100 x 75 image beside 3.2 % and 95.9 % for classes 0 and 3 -- measured on an MI355X)
    assert int((counts >= 0.01 * host.mask.size).sum()) >= 2, (labels, counts)
    assert host.confidence.min() >= np.float32(1.0 / k) and host.confidence.max() <= 1.0
    assert np.abs(host.probabilities.sum(-1, dtype=np.float64) - 1.0).max() < 1e-5
    if tta == 8:
        assert changed >= 1
    assert np.array_equal(dev.mask, host.mask), "%d pixels differ" % int((dev.mask != host.mask).sum())
    assert np.array_equal(dev.confidence, host.confidence), "largest difference %g" % np.abs(dev.confidence - host.confidence).max()
    assert np.array_equal(dev.probabilities, host.probabilities)
    assert np.array_equal(dev.confidence, dev.probabilities.max(-1)) and np.array_equal(dev.mask, np.argmax(dev.probabilities, -1))
    # without the extra outputs the return value is the bare mask, and asking for one leaves the other None
    only = inf.segment_image(raw, net, tile_size=TILE, radius=RADIUS, tta=tta)
    assert isinstance(only, np.ndarray) and np.array_equal(only, host.mask)
    if tta == 2:                                                              # (once is enough: the suite runs for every later change)
        conf_only = inf.segment_image(raw, net, tile_size=TILE, tta=tta, return_confidence=True)
        assert conf_only.probabilities is None and np.array_equal(conf_only.confidence, host.confidence) and np.array_equal(conf_only.mask, host.mask)


def test_tta_1_with_confidence_keeps_the_mask_and_reports_the_softmax_maximum(monkeypatch):
    inf, readers = pkg("inference"), pkg("readers")
    for c, k, (h, w) in ((3, 4, (48, 40)), (1, 2, (100, 75))):
        net = _net(c, k)
        monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
        raw = _uint16_image(h, w, c, seed=h + c)
        plain = inf.segment_image(raw, net, tile_size=TILE)
        res = inf.segment_image(raw, net, tile_size=TILE, tta=1, return_confidence=True)
        assert isinstance(plain, np.ndarray) and res.probabilities is None
        assert np.array_equal(res.mask, plain)
        host = inf._segment_host_pipeline(raw, net, TILE, return_confidence=True)
        assert np.array_equal(host.mask, plain) and np.array_equal(host.confidence, res.confidence)
        if h <= TILE and w <= TILE:                                           # one tile: a direct forward of the padded, z-scored image
            z = readers.zscore_normalize(raw.astype(np.float32).transpose(2, 0, 1)).transpose(1, 2, 0)
            padded = np.pad(z, ((0, (-h) % 16), (0, (-w) % 16), (0, 0)), mode="reflect")
            x = torch.from_numpy(np.ascontiguousarray(padded.transpose(2, 0, 1))[None]).cuda()
            p = net.engine.forward(x, training=False)[0].cpu().numpy()
            assert np.array_equal(res.confidence, p.max(-1)[:h, :w])
            assert np.array_equal(res.mask, np.argmax(p, -1)[:h, :w])


class _Recorder:
    """the library object with every call's name written down"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_default_path_issues_the_launches_it_always_did(monkeypatch):
    inf = pkg("inference")
    net = _net(1, 2)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    rec = _Recorder(pkg("_lib").lib())
    monkeypatch.setattr(inf, "lib", lambda: rec)
    raw = _uint16_image(100, 75, 1, seed=101)
    ntiles = len(inf.tile_plan(112, 80, TILE, RADIUS))
    assert ntiles > 1
    got = inf.segment_image(raw, net, tile_size=TILE)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (100, 75)
    assert rec.calls == ["unet_image_tile_gather", "unet_argmax_paste"] * ntiles
    del rec.calls[:]
    res = inf.segment_image(raw, net, tile_size=TILE, tta=2, return_confidence=True)
    per_tile = ["unet_image_tile_gather_tta", "unet_prob_accumulate"] * 2 + ["unet_argmax_paste_conf"]
    assert rec.calls == per_tile * ntiles and isinstance(res, inf.SegmentResult)
    del rec.calls[:]
    inf.segment_image(raw, net, tile_size=TILE, tta=1, return_probabilities=True)      # tta = 1: no accumulate, the paste reads the softmax
    assert rec.calls == ["unet_image_tile_gather_tta", "unet_argmax_paste_conf"] * ntiles


def test_cli_tta_and_confidence_folder_on_both_pipelines(tmp_path):
    inf, metrics = pkg("inference"), pkg("metrics")
    net = _net(1, 2)
    stem = str(tmp_path / "checkpoint" / "ckpt")
    net.save_checkpoint(stem)
    imgs, truths = tmp_path / "imgs", tmp_path / "truth"
    imgs.mkdir(); truths.mkdir()
    rng = np.random.default_rng(0)
    images = {"a.npy": _uint16_image(70, 83, 1, 1)[:, :, 0], "b.npy": _raw_image(40, 40, 1, np.uint8, 2, None)[:, :, 0]}
    for name, im in images.items():
        np.save(imgs / name, im)
        np.save(truths / name, rng.integers(0, 2, im.shape).astype(np.uint8))
    common = ["--checkpoint_filepath", stem, "--image_folder", str(imgs), "--number_classes", "2", "--number_channels", "1", "--image_format", "npy",
              "--tta", "4"]
    inf.main(common + ["--output_folder", str(tmp_path / "dev"), "--confidence_folder", str(tmp_path / "conf")])
    inf.main(common + ["--output_folder", str(tmp_path / "host"), "--confidence_folder", str(tmp_path / "conf2"), "--host_pipeline"])
    for name, im in images.items():
        assert open(tmp_path / "dev" / name, "rb").read() == open(tmp_path / "host" / name, "rb").read(), name
        assert open(tmp_path / "conf" / name, "rb").read() == open(tmp_path / "conf2" / name, "rb").read(), name
        conf = np.load(tmp_path / "conf" / name)
        assert conf.dtype == np.float32 and conf.shape == im.shape and conf.min() >= 0.5 and conf.max() <= 1.0 and conf.std() > 0
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(os.listdir(tmp_path / "conf")) == ["a.npy", "b.npy"]
    # scoring scores the FINAL mask: the total row is the summary of the host count of the written masks
    inf.main(common + ["--output_folder", str(tmp_path / "scored"), "--mask_folder", str(truths)])
    cm = metrics.ConfusionMatrix(2, device="cpu")
    for name in images:
        written = np.load(tmp_path / "scored" / name)
        assert np.array_equal(written, np.load(tmp_path / "dev" / name))
        inf._host_confusion(written, np.load(truths / name), cm)
    lines = open(tmp_path / "scored" / "scores.csv").read().splitlines()
    assert lines[-1] == metrics.csv_row("total", metrics.summarize(cm.result()))
    assert np.array_equal(np.load(tmp_path / "scored" / "confusion.npy"), cm.result())
