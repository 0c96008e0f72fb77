"""GPU benchmark of test-time augmentation and confidence maps in whole-image inference: python scripts/bench_inference_tta.py [out.txt]

Part 1, host array -> host result (`inference.segment_image`), the image of scripts/bench_inference_image.py: a seeded synthetic
4096 x 4096 uint16 image, one channel, two classes, random-init weights, radius 96 (25 tiles), fp32 and bf16, 1 warm-up and 3 timed runs
each, the median reported: tta 1, 2, 4 and 8 without confidence, tta 1 and 8 with the confidence map, and t(n) / (n * t(1)) from the same
run (1 = n forwards cost n forwards; the gather, accumulate and paste launches are what is above it).

Part 2, the three new kernels at the driver's tile (1024 x 1024, one channel, two classes) between HIP events, one pair per launch
(exclusive time), every launch on a buffer set it has not touched for ROTATE - 1 launches (the sets together exceed the 256 MB Infinity
Cache, so these are HBM figures), median over REPS blocks of the mean per launch; bytes are the algorithmic ones (every element read or
written once), against the 6.29 TB/s the project reports every HBM-bound pass against.  No threshold: the numbers are recorded.

`--default-only` times nothing but the default path (tta = 1, no confidence) and prints its runs: the script then runs unchanged on a tree
without this feature, for the alternating comparison of the default path before and after.  Written to profiles/inference_tta.txt by default."""
import ctypes, importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("UNET_TREE", ROOT))          # (another checkout of the project: the before / after comparison)
import numpy as np
import torch
model = importlib.import_module("semantic-segmentation-unet_amd.model")
inf = importlib.import_module("semantic-segmentation-unet_amd.inference")
L = importlib.import_module("semantic-segmentation-unet_amd._lib").lib()
assert torch.cuda.is_available(), "needs an MI355X"
HW, RADIUS, RUNS = int(os.environ.get("HW", 4096)), 96, 3
DEFAULT_ONLY = "--default-only" in sys.argv
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:HW, 0:HW].astype(np.float32)
img = np.clip(20000.0 + 9000.0 * np.sin(yy / 37.0) * np.cos(xx / 53.0) + 2500.0 * rng.standard_normal((HW, HW), dtype=np.float32), 0, 65535).astype(np.uint16)
del yy, xx
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(net, **kw):
    out = inf.segment_image(img, net, radius=RADIUS, **kw)      # warm-up: every tile shape, every buffer
    ts = []
    for _ in range(RUNS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = inf.segment_image(img, net, radius=RADIUS, **kw)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts, out


fmt = lambda ts: " ".join("%.1f" % (t * 1e3) for t in ts)
tiles = len(inf.tile_plan(HW + (-HW) % 16, HW + (-HW) % 16, inf.TILE_SIZE, RADIUS))
say("image %d x %d uint16, 1 channel, 2 classes, radius %d: %d tiles of at most %d x %d, %s; median of %d after 1 warm-up"
    % (HW, HW, RADIUS, tiles, inf.TILE_SIZE, inf.TILE_SIZE, torch.cuda.get_device_name(0), RUNS))
for cd in ("fp32", "bf16"):
    net = model.UNet(2, 1, 1, 1e-4, seed=0, compute_dtype=cd)
    t1, all1, m1 = timed(net)
    say("%s: tta 1                  %8.1f ms (%s)" % (cd, t1 * 1e3, fmt(all1)))
    if DEFAULT_ONLY:
        del net
        continue
    for n in (2, 4, 8):
        tn, alln, mn = timed(net, tta=n)
        say("%s: tta %d                  %8.1f ms (%s)  t(%d) / (%d t(1)) = %.3f, %.2f %% of the pixels change class"
            % (cd, n, tn * 1e3, fmt(alln), n, n, tn / (n * t1), 100.0 * float((mn != m1).mean())))
    for n in (1, 8):
        tn, alln, res = timed(net, tta=n, return_confidence=True)
        say("%s: tta %d + confidence map %8.1f ms (%s)  t / (%d t(1)) = %.3f, confidence min %.4f mean %.4f"
            % (cd, n, tn * 1e3, fmt(alln), n, tn / (n * t1), float(res.confidence.min()), float(res.confidence.mean())))
    del net

if not DEFAULT_ONLY:
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ROTATE, WARM, REPS, PEAK = 64, 2, 10, 6.29e12
    T, K = inf.TILE_SIZE, 2

    def block_ms(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ROTATE)]
        for i, (e0, e1) in enumerate(ev):
            e0.record()
            fn(i)
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / ROTATE

    def measure(fns):
        for _ in range(WARM):
            for f in fns.values():
                block_ms(f)
        t = {k: [] for k in fns}
        for _ in range(REPS):
            for k, f in fns.items():
                t[k].append(block_ms(f))
        return t

    def row(name, ms, nbytes):
        med = statistics.median(ms)
        bw = nbytes / (med * 1e-3)
        return "%-44s %8.2f us  (min %8.2f, max %8.2f)  %6.1f MB  %5.2f TB/s  %5.1f %% of 6.29 TB/s" % (
            name, med * 1e3, min(ms) * 1e3, max(ms) * 1e3, nbytes / 1e6, bw / 1e12, 100.0 * bw / PEAK)

    say("")
    say("kernels at one %d x %d tile, 1 channel (uint16 source), %d classes; ROTATE %d buffer sets, median of %d blocks of %d launches (HIP events)"
        % (T, T, K, ROTATE, REPS, ROTATE))
    raw = torch.from_numpy(img.reshape(-1).view(np.uint8)).cuda()
    coef = torch.tensor([[20000.0], [9000.0]], device="cuda")
    outs = [torch.empty(T * T, device="cuda") for _ in range(ROTATE)]
    spots = [(y, x) for y in range(0, HW - T + 1, 512) for x in range(0, HW - T + 1, 512)]      # 49 overlapping tile origins, all interior
    gather = lambda t: lambda i: L.unet_image_tile_gather_tta(P(raw), 1, HW, HW, 1, P(coef[0]), P(coef[1]), spots[i % len(spots)][0],
                                                              spots[i % len(spots)][1], T, T, t, P(outs[i]), ST())
    fns = {"unet_image_tile_gather": lambda i: L.unet_image_tile_gather(P(raw), 1, HW, HW, 1, P(coef[0]), P(coef[1]), spots[i % len(spots)][0],
                                                                        spots[i % len(spots)][1], T, T, P(outs[i]), ST())}
    fns.update({"unet_image_tile_gather_tta t=%d" % t: gather(t) for t in (1, 2, 4, 7)})
    for name, ms in measure(fns).items():
        say(row(name, ms, T * T * (2 + 4)))
    del outs
    g = torch.Generator(device="cuda").manual_seed(0)
    prob = [torch.rand(T * T, K, device="cuda", generator=g) for _ in range(ROTATE)]
    acc = [torch.zeros(T * T, K, device="cuda") for _ in range(ROTATE)]
    accum = lambda t, first: lambda i: L.unet_prob_accumulate(P(prob[i]), K, T, T, K, t, first, P(acc[i]), K, ST())
    fns = {"unet_prob_accumulate t=0 first (store)": accum(0, 1)}
    fns.update({"unet_prob_accumulate t=%d (add)" % t: accum(t, 0) for t in (0, 1, 2, 4, 7)})
    for name, ms in measure(fns).items():
        say(row(name, ms, T * T * K * 4 * (2 if "first" in name else 3)))
    del prob
    z = T - 2 * RADIUS
    mask = [torch.empty(z, z, dtype=torch.uint8, device="cuda") for _ in range(ROTATE)]
    conf = [torch.empty(z, z, device="cuda") for _ in range(ROTATE)]
    pout = [torch.empty(z, z, K, device="cuda") for _ in range(ROTATE)]
    paste = lambda c, p: lambda i: L.unet_argmax_paste_conf(P(acc[i]), K, T, T, K, 0.125, RADIUS, RADIUS, z, z, P(mask[i]), 1, z, 0, 0, z, z,
                                                            P(conf[i]) if c else None, z, P(pout[i]) if p else None, ST())
    fns = {"unet_argmax_paste (interior zone %d x %d)" % (z, z): lambda i: L.unet_argmax_paste(P(acc[i]), K, T, T, K, RADIUS, RADIUS, z, z, P(mask[i]), 1, z,
                                                                                              0, 0, z, z, ST()),
           "unet_argmax_paste_conf, confidence": paste(1, 0), "unet_argmax_paste_conf, confidence + prob.": paste(1, 1)}
    nbytes = {0: z * z * (K * 4 + 1), 1: z * z * (K * 4 + 1 + 4), 2: z * z * (K * 4 + 1 + 4 + K * 4)}
    for j, (name, ms) in enumerate(measure(fns).items()):
        say(row(name, ms, nbytes[j]))

text = "\n".join(lines) + "\n"
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out = args[0] if args else (None if DEFAULT_ONLY else os.path.join(ROOT, "profiles", "inference_tta.txt"))
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
