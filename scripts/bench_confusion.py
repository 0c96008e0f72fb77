"""HIP-event time of the confusion-matrix kernels beside the loss kernel they follow: python scripts/bench_confusion.py [out.txt]

At the BASELINE config-2 eval shape (logits / one-hot labels [8, 512, 512, 2]) it times `unet_confusion_scores` and a forward-only
`unet_softmax_ce` launch (labels given, dlogits NULL, prob written, loss and accuracy reduced) on the SAME tensors in the same run, and
`unet_confusion_masks` on a 4096 x 4096 uint8 prediction / ground-truth pair.  Every launch reads a buffer set it has not touched for
ROTATE - 1 launches (ROTATE sets, together larger than the 256 MB Infinity Cache), so the figures are HBM figures, not cache ones.  The two
score kernels alternate in blocks of ROTATE launches, every launch between its own pair of events (exclusive time); the table is the median
over REPS blocks of the mean per launch, the spread its min .. max.  Bytes are the algorithmic ones (every tensor read or written once).  Written to profiles/confusion_metrics.txt by default."""
import ctypes, importlib, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
L = importlib.import_module("semantic-segmentation-unet_amd._lib").lib()
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
assert torch.cuda.is_available(), "needs an MI355X: a CPU run cannot give a time"
ROTATE, WARM, REPS = 12, 3, 25


def block_ms(fn):
    """ms per launch over one block of ROTATE launches, one per buffer set; every launch sits between its own pair of events (exclusive time:
    the host's gaps between launches are not in it)"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ROTATE)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        fn(i)
        e1.record()
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in ev) / ROTATE


def measure(fns):
    """alternate the candidates block by block -> {name: [ms per launch of every timed block]}"""
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
    return "%-34s %9.2f us  (min %8.2f, max %8.2f)  %8.1f MB  %7.2f TB/s" % (name, med * 1e3, min(ms) * 1e3, max(ms) * 1e3, nbytes / 1e6, nbytes / (med * 1e-3) / 1e12)


n, h, w, k = 8, 512, 512, 2
pix = n * h * w
g = torch.Generator(device="cuda").manual_seed(0)
z = [torch.randn(pix, k, device="cuda", generator=g) for _ in range(ROTATE)]
lab = [torch.nn.functional.one_hot(torch.randint(0, k, (pix,), device="cuda", generator=g), k).to(torch.int32).contiguous() for _ in range(ROTATE)]
prob = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
loss = torch.zeros(2, device="cuda")
nb = L.unet_softmax_ce_workspace(pix)
ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
cm = torch.zeros(k, k, dtype=torch.int64, device="cuda")
fns = {
    "unet_softmax_ce (forward only)": lambda i: L.unet_softmax_ce(P(z[i]), k, P(lab[i]), P(prob[i]), None, 0, pix, k, 0.0, 1.0 / pix, 0.0, 0.0,
                                                                  P(loss[0:1]), P(loss[1:2]), P(ws), nb, ST()),
    "unet_confusion_scores": lambda i: L.unet_confusion_scores(P(z[i]), k, P(lab[i]), pix, k, P(cm), ST()),
}
t = measure(fns)
# the two agree on what they count: trace of the last launch's matrix == the loss kernel's accuracy count
cm.zero_(); fns["unet_confusion_scores"](0); fns["unet_softmax_ce (forward only)"](0); torch.cuda.synchronize()
assert int(cm.diagonal().sum().item()) == int(loss[1].item()) and int(cm.sum().item()) == pix
lines = ["confusion-matrix kernels, %s, ROTATE %d buffer sets, median of %d blocks of %d launches (HIP events)" % (torch.cuda.get_device_name(0), ROTATE, REPS, ROTATE),
         "scores / one-hot labels [%d, %d, %d, %d] fp32 / int32 (BASELINE config 2, eval step)" % (n, h, w, k),
         row("unet_softmax_ce (forward only)", t["unet_softmax_ce (forward only)"], pix * k * 4 * 3),
         row("unet_confusion_scores", t["unet_confusion_scores"], pix * k * 4 * 2)]
ratio = statistics.median(t["unet_confusion_scores"]) / statistics.median(t["unet_softmax_ce (forward only)"])
lines.append("unet_confusion_scores / unet_softmax_ce = %.3f (must be <= 1: fewer bytes, no expf / logf)" % ratio)
del z, lab, prob
hm = wm = 4096
pred = [torch.randint(0, 2, (hm, wm), device="cuda", generator=g, dtype=torch.uint8) for _ in range(ROTATE)]
truth = [torch.randint(0, 2, (hm, wm), device="cuda", generator=g, dtype=torch.uint8) for _ in range(ROTATE)]
oor = torch.zeros(1, dtype=torch.int64, device="cuda")
tm = measure({"m": lambda i: L.unet_confusion_masks(P(pred[i]), 1, wm, P(truth[i]), 1, wm, hm, wm, 2, -1, P(cm), P(oor), ST())})
lines += ["class maps %d x %d uint8 against uint8, K = 2" % (hm, wm), row("unet_confusion_masks", tm["m"], 2 * hm * wm)]
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "confusion_metrics.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write(text)
