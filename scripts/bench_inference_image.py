"""GPU benchmark of whole-image inference, host array -> host mask (reference UNet/inference.py:27-136,201-213): the device pipeline
(`inference.segment_image`: one upload, per tile gather -> forward -> argmax + paste on the stream, one mask download) against the host
loop (`zscore_normalize` + `_inference_tiling`: per tile slice, transpose, pageable upload, forward, argmax, blocking download, paste).

A seeded synthetic 4096 x 4096 uint16 image, one channel, two classes, random-init weights; both drivers in the same process at the same
radius (96; `estimate_radius` is patched for the host loop, whose probe draws from the global numpy RNG); fp32 and bf16; 1 warm-up and 3
timed runs each, the median reported.  Only the ratio of the two times of one run is comparable across machines."""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
model = importlib.import_module("semantic-segmentation-unet_amd.model")
inf = importlib.import_module("semantic-segmentation-unet_amd.inference")
readers = importlib.import_module("semantic-segmentation-unet_amd.readers")
assert torch.cuda.is_available(), "needs an MI355X"
HW, RADIUS, RUNS = int(os.environ.get("HW", 4096)), 96, 3
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:HW, 0:HW].astype(np.float32)
img = np.clip(20000.0 + 9000.0 * np.sin(yy / 37.0) * np.cos(xx / 53.0) + 2500.0 * rng.standard_normal((HW, HW), dtype=np.float32), 0, 65535).astype(np.uint16)
del yy, xx
tiles = len(inf.tile_plan(HW + (-HW) % 16, HW + (-HW) % 16, inf.TILE_SIZE, RADIUS))
print("image %d x %d uint16, 1 channel, 2 classes, radius %d: %d tiles of at most %d x %d" % (HW, HW, RADIUS, tiles, inf.TILE_SIZE, inf.TILE_SIZE), flush=True)


def host_loop(net):
    z = readers.zscore_normalize(img.astype(np.float32)[None]).transpose(1, 2, 0)
    return inf._inference_tiling(z, net, inf.TILE_SIZE)


def device(net):
    return inf.segment_image(img, net, radius=RADIUS)


def timed(fn, net):
    out = fn(net)                                    # warm-up: every tile shape, every buffer
    ts = []
    for _ in range(RUNS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn(net)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts, np.array(out)


for cd in ("fp32", "bf16"):
    net = model.UNet(2, 1, 1, 1e-4, seed=0, compute_dtype=cd)
    net.estimate_radius = lambda: RADIUS
    t_dev, all_dev, m_dev = timed(device, net)
    t_host, all_host, m_host = timed(host_loop, net)
    share = np.bincount(m_host.reshape(-1).astype(np.int64), minlength=2) / m_host.size
    print("%s: device pipeline %.1f ms (%s), host loop %.1f ms (%s), host / device = %.2f, masks equal: %s, class shares %s"
          % (cd, t_dev * 1e3, " ".join("%.1f" % (t * 1e3) for t in all_dev), t_host * 1e3, " ".join("%.1f" % (t * 1e3) for t in all_host),
             t_host / t_dev, bool(np.array_equal(m_dev, m_host)), np.round(share, 4).tolist()), flush=True)
    del net
