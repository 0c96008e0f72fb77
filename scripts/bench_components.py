"""HIP-event time of the device connected components and what they add to `segment_image`: python scripts/bench_components.py [out.txt]

Kernel part.  `unet_label_components` (all its launches between one pair of events; labels, count, the object table and the filtered mask
written, min_area 4) at 8 x 512^2 and 1 x 4096^2, uint8, on: about 40 discs per image (the masks of scripts/bench_border_weights.py); one
component filling the image (the contention worst case of the atomics); a one-pixel serpentine through the whole image (the depth worst
case of the union-find); Bernoulli noise at site density 0.59 under 4-connectivity and 0.41 under 8-connectivity (near percolation).
Every call reads a mask, and writes labels and a filtered mask, that it has not touched for ROTATE - 1 calls; ROTATE is chosen per shape so
that these rotated buffers (6 bytes per pixel per set) together exceed the 256 MB Infinity Cache.  The workspace (8 bytes per pixel) is
one buffer, written and read back inside every call: its traffic is not compulsory and may be served by the cache.  Compulsory bytes = the mask read once, labels and filtered mask written
once (6 bytes per pixel); bytes / time stands beside the 5.4 - 5.9 TB/s the BatchNorm passes reach.  In the same run: the route this
replaces, the download of the mask plus `scipy.ndimage.label` per class (host clock; skipped when scipy is absent).

Pipeline part.  `segment_image` on a 4096^2 uint8 image with a random-init network, with and without instances=True, alternating; the
legs without launch exactly what the parent commit launches.  Written to profiles/components.txt by default."""
import ctypes, importlib, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
L = importlib.import_module("semantic-segmentation-unet_amd._lib").lib()
model = importlib.import_module("semantic-segmentation-unet_amd.model")
inference = importlib.import_module("semantic-segmentation-unet_amd.inference")
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
assert torch.cuda.is_available(), "needs an MI355X: a CPU run cannot give a time"
try:
    from scipy import ndimage
except ImportError:
    ndimage = None
WARM, REPS = 2, 9
ROTATE = 6                                           # set per shape below: the rotated buffers together exceed the 256 MB Infinity Cache
MAX_OBJECTS, MIN_AREA = 65536, 4
SEG_BLOCKS = 5


def discs(n, h, w, count, rmax, g):
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    out = torch.zeros(n, h, w, dtype=torch.uint8, device="cuda")
    for i in range(n):
        for _ in range(count):
            cy, cx = (int(torch.randint(0, s, (1,), generator=g)) for s in (h, w))
            r = int(torch.randint(4, rmax, (1,), generator=g))
            out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return out


def serpentine(n, h, w):
    m = torch.zeros(n, h, w, dtype=torch.uint8, device="cuda")
    m[:, 0::2] = 1
    m[:, 1::4, w - 1] = 1
    m[:, 3::4, 0] = 1
    return m


def block_ms(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ROTATE)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        fn(i)
        e1.record()
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in ev) / ROTATE


def host_route_ms(mask_dev, connectivity):
    """download + scipy.ndimage.label per image (one foreground class here), host clock around work that ends in the arrays"""
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = mask_dev.cpu().numpy()
        for img in m:
            ndimage.label(img, structure=structure)
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


g = torch.Generator().manual_seed(0)
gd = torch.Generator(device="cuda").manual_seed(0)
lines = ["connected components, %s, median of %d blocks of ROTATE calls (HIP events); labels + count + table + filtered mask, min_area %d"
         % (torch.cuda.get_device_name(0), REPS, MIN_AREA)]
for n, h, w, ROTATE in ((8, 512, 512, 26), (1, 4096, 4096, 6)):
    pix = n * h * w
    rmax = 40 * h // 512
    inputs = [("about 40 discs per image", 8, lambda: discs(n, h, w, 40, rmax, g)),
              ("one component fills the image", 8, lambda: torch.ones(n, h, w, dtype=torch.uint8, device="cuda")),
              ("one-pixel serpentine", 4, lambda: serpentine(n, h, w)),
              ("noise, density 0.59, 4-connectivity", 4, lambda: (torch.rand(n, h, w, device="cuda", generator=gd) < 0.59).to(torch.uint8)),
              ("noise, density 0.41, 8-connectivity", 8, lambda: (torch.rand(n, h, w, device="cuda", generator=gd) < 0.41).to(torch.uint8))]
    labels = [torch.empty(pix, dtype=torch.int32, device="cuda") for _ in range(ROTATE)]
    fmask = [torch.empty(pix, dtype=torch.uint8, device="cuda") for _ in range(ROTATE)]
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    objects = torch.empty(n * MAX_OBJECTS * 8, dtype=torch.int64, device="cuda")
    nb = L.unet_label_components_workspace(n, h, w)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    lines.append("class maps [%d, %d, %d] uint8; compulsory bytes %.1f MB (mask read, labels and filtered mask written); ROTATE %d sets = %.0f MB"
                 % (n, h, w, 6 * pix / 1e6, ROTATE, ROTATE * 6 * pix / 1e6))
    for name, conn, make in inputs:
        masks = [make() for _ in range(ROTATE)]
        fn = lambda i: L.unet_label_components(P(masks[i]), 1, w, n, h, w, conn, 0, MIN_AREA, P(labels[i]), P(count), P(fmask[i]), P(objects),
                                               MAX_OBJECTS, P(ws), nb, ST())
        for _ in range(WARM):
            block_ms(fn)
        ms = [block_ms(fn) for _ in range(REPS)]
        med = statistics.median(ms)
        torch.cuda.synchronize()
        host = ""
        if ndimage is not None:
            hm = host_route_ms(masks[0], conn)
            host = "  | download + scipy.ndimage.label: %9.2f ms = %6.1f x" % (hm, hm / med)
        else:
            host = "  | scipy absent: host route not measured"
        lines.append("  %-38s %9.3f ms (min %9.3f, max %9.3f)  %6.3f TB/s  objects of image 0: %d%s"
                     % (name, med, min(ms), max(ms), 6 * pix / (med * 1e-3) / 1e12, int(count[0]), host))
        del masks
    del labels, fmask, objects, ws
    torch.cuda.empty_cache()

# ---- segment_image on a 4096^2 image ------------------------------------------------------------------------------------------------------
net = model.UNet(2, 1, 1, seed=0)
raw = np.random.default_rng(0).integers(0, 256, (4096, 4096)).astype(np.uint8)
radius = 96                                                          # (a fixed halo: the probe of estimate_radius is not what is timed)
legs = {"segment_image (the parent's launches)": {}, "segment_image(instances=True)": {"instances": True},
        "segment_image(instances=True, min_object_area=4)": {"instances": True, "min_object_area": 4}}
t = {k: [] for k in legs}
for rep in range(SEG_BLOCKS + 1):
    for name, kw in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = inference.segment_image(raw, net, radius=radius, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:                                                      # (the first round warms every tile shape)
            t[name].append(dt)
lines.append("segment_image, 4096 x 4096 uint8, 2 classes, random-init network, host clock around the call (it ends in its one synchronise), %d calls each, alternating"
             % SEG_BLOCKS)
base = statistics.median(t["segment_image (the parent's launches)"])
for name in legs:
    med = statistics.median(t[name])
    lines.append("  %-50s median %9.2f ms  min %9.2f  max %9.2f  (%+.2f ms, %+.2f %%)" % (name, med, min(t[name]), max(t[name]), med - base, 100 * (med - base) / base))
lines.append("  objects in the last result: %d" % res.count)
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "components.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write(text)
