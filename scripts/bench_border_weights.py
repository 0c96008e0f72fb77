"""HIP-event time of the border-distance weight map and what it adds to a training step: python scripts/bench_border_weights.py [out.txt]

Kernel part.  At the BASELINE config-2 train shape (one-hot labels [8, 512, 512, K], K = 2 and K = 4) it times, in the same process, on the
same labels and in alternating blocks: `unet_border_weights` (its four launches between one pair of events; weights and d2 written, a caller
pixel-weight map multiplied in; and once with neither) and `unet_softmax_ce_weighted` with class + pixel weights + ignore, the kernel the map
feeds.  Masks: about 40 discs of random classes per image (the synthetic reader's kind); one small disc per image, the worst case for the
outward row search (most lanes walk far before they meet a finite column); and one class only, where the row search is skipped and the call
is the one-hot pass plus three passes over 1 .. 4 byte per pixel tensors -- the one-hot pass's bytes over that WHOLE call's time is a lower
bound of the pass's rate (a stage alone cannot be launched through the C ABI).
Every launch reads a label set it has not touched for ROTATE - 1 launches (the sets are together larger than the 256 MB Infinity Cache).

Step part.  Whole training steps of model.UNet with border_weight 10 / sigma 5 and without, same process, same parameters, alternating blocks
of STEPS steps, one host sync per block, at BASELINE config 2 (fp32, 8 x 512^2 x 1, K = 2) and the config-4 shape (bf16, 8 x 512^2 x 3,
K = 4).  The "off" legs launch exactly what the parent commit launches, so their min .. max over the blocks is the parent's own run-to-run
range on this box; the file sets the difference of the medians against it and against the expectation written down before any run: well
under 1 % of the step.  Written to profiles/border_weights.txt by default."""
import ctypes, importlib, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
L = importlib.import_module("semantic-segmentation-unet_amd._lib").lib()
model = importlib.import_module("semantic-segmentation-unet_amd.model")
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
assert torch.cuda.is_available(), "needs an MI355X: a CPU run cannot give a time"
ROTATE, WARM, REPS = 12, 3, 25
STEPS, STEP_BLOCKS = 20, 7
COPY_TBS = 6.29
W0, SIGMA = 10.0, 5.0
C = float(np.float32(-1.0 / (2.0 * SIGMA * SIGMA)))


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


def discs(n, h, w, k, count, rmax, g):
    """class maps [n, h, w] (int64, device): `count` discs of random classes per image on a class-0 ground"""
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    out = torch.zeros(n, h, w, dtype=torch.int64, device="cuda")
    for i in range(n):
        for _ in range(count):
            cy, cx = (int(torch.randint(0, s, (1,), generator=g)) for s in (h, w))
            r = int(torch.randint(4, rmax, (1,), generator=g))
            out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1 + int(torch.randint(0, k - 1, (1,), generator=g)) if k > 1 else 0
    return out


def onehot(cls, k):
    return torch.nn.functional.one_hot(cls, k).to(torch.int32).contiguous()


n, h, w = 8, 512, 512
pix = n * h * w
g = torch.Generator().manual_seed(0)
gd = torch.Generator(device="cuda").manual_seed(0)
lines = ["border-distance weight map, %s, ROTATE %d label sets, median of %d blocks of %d calls (HIP events)" % (
    torch.cuda.get_device_name(0), ROTATE, REPS, ROTATE)]
for k in (2, 4):
    masks = {"40 discs per image": [onehot(discs(n, h, w, k, 40, 40, g), k) for _ in range(ROTATE)],
             "one small disc per image": [onehot(discs(n, h, w, k, 1, 12, g), k) for _ in range(ROTATE)],
             "no border (one class)": [onehot(torch.zeros(n, h, w, dtype=torch.int64, device="cuda"), k) for _ in range(ROTATE)]}
    pw = [torch.rand(pix, device="cuda", generator=gd) * 2 for _ in range(ROTATE)]
    wout = [torch.empty(pix, device="cuda") for _ in range(ROTATE)]
    d2 = [torch.empty(pix, dtype=torch.int32, device="cuda") for _ in range(ROTATE)]
    nb = L.unet_border_weights_workspace(n, h, w)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    z = [torch.randn(pix, k, device="cuda", generator=gd) for _ in range(ROTATE)]
    prob = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
    dl = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
    cw = torch.rand(k, device="cuda", generator=gd) * 3.75 + 0.25
    stats = torch.zeros(4, device="cuda")
    nbw = L.unet_softmax_ce_weighted_workspace(pix)
    wsw = torch.empty(nbw + 256, dtype=torch.uint8, device="cuda")

    def border(lab, with_d2=True, with_pw=True):
        return lambda i: L.unet_border_weights(P(lab[i]), k, P(pw[i]) if with_pw else None, W0, C, P(wout[i]), P(d2[i]) if with_d2 else None,
                                               n, h, w, P(ws), nb, ST())
    lab0 = masks["40 discs per image"]
    fns = {"unet_border_weights, " + name: border(lab) for name, lab in masks.items()}
    fns["unet_border_weights, 40 discs, no d2_out, no pixel_weight_in"] = border(lab0, False, False)
    fns["unet_softmax_ce_weighted, class + pixel weights + ignore"] = lambda i: L.unet_softmax_ce_weighted(
        P(z[i]), k, P(lab0[i]), P(cw), P(wout[i]), 1, P(prob[i]), P(dl[i]), k, pix, k, 0.0, 1.0 / pix, 1.0 / pix, 0.0, P(stats), P(wsw), nbw, ST())
    t = measure(fns)
    lines.append("one-hot labels [%d, %d, %d, %d] int32 (BASELINE config 2, train step)" % (n, h, w, k))
    for name, ms in t.items():
        lines.append("%-66s %8.2f us  (min %8.2f, max %8.2f)" % (name, statistics.median(ms) * 1e3, min(ms) * 1e3, max(ms) * 1e3))
    # the one-hot pass reads 4 K bytes per pixel and writes 1; on the image without border the row pass skips its search, so the whole call is
    # the one-hot pass + three passes over 1 .. 4 byte per pixel tensors: bytes of the one-hot pass over the time of the WHOLE call is a lower
    # bound of that pass's rate
    med = statistics.median(t["unet_border_weights, no border (one class)"])
    onehot_bytes = pix * (4 * k + 1)
    all_bytes = onehot_bytes + pix * (1 + 4.0 / 32) + pix * (4.0 / 32 + 4) + pix * (4 + 4 + 4 + 4)
    lines.append("one-hot pass: %.1f MB; over the whole no-border call's time: >= %.2f TB/s; all four passes' algorithmic bytes %.1f MB: %.2f TB/s "
                 "(a copy kernel reaches %.2f)" % (onehot_bytes / 1e6, onehot_bytes / (med * 1e-3) / 1e12, all_bytes / 1e6,
                                                   all_bytes / (med * 1e-3) / 1e12, COPY_TBS))
    del masks, pw, wout, d2, z, prob, dl, lab0, fns
torch.cuda.empty_cache()

# ---- whole steps -----------------------------------------------------------------------------------------------------------------------
for title, dtype, ch, k in (("BASELINE config 2: fp32, 8 x 512^2 x 1, K = 2", "fp32", 1, 2), ("config-4 shape: bf16, 8 x 512^2 x 3, K = 4", "bf16", 3, 4)):
    img = torch.randn(n, ch, h, w, device="cuda", generator=gd)
    lab = onehot(discs(n, h, w, k, 40, 40, g), k)
    nets = {"off": model.UNet(k, n, ch, compute_dtype=dtype), "on": model.UNet(k, n, ch, compute_dtype=dtype, border_weight=W0, border_sigma=SIGMA)}

    def block(net):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            net.train_step((img, lab, None, None))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS
    for net in nets.values():
        block(net)                                                   # warm-up: buffers, plans, operand transforms
    t = {name: [] for name in nets}
    for _ in range(STEP_BLOCKS):
        for name, net in nets.items():
            t[name].append(block(net))
    off, on_ = statistics.median(t["off"]), statistics.median(t["on"])
    rng = max(t["off"]) - min(t["off"])
    lines.append(title + ", alternating blocks of %d steps, %d blocks each (ms per step)" % (STEPS, STEP_BLOCKS))
    for name in nets:
        lines.append("  border weight %-3s  median %8.3f  min %8.3f  max %8.3f" % (name, statistics.median(t[name]), min(t[name]), max(t[name])))
    lines.append("  on - off = %+.3f ms = %+.2f %% of the step; the off legs (the parent's launches) range over %.3f ms = %.2f %%: expectation "
                 "(well under 1 %%) %s" % (on_ - off, 100 * (on_ - off) / off, rng, 100 * rng / off, "MET" if (on_ - off) < 0.005 * off else "NOT MET (taken as: under 0.5 %)"))
    del nets
    torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "border_weights.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write(text)
