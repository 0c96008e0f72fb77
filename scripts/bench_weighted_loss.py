"""HIP-event time of the weighted loss kernel beside the unweighted one it stands next to: python scripts/bench_weighted_loss.py [out.txt]

At the BASELINE config-2 train shape (logits / one-hot labels [8, 512, 512, K], K = 2 and K = 4) it times, in the same process and on the
SAME tensors: `unet_softmax_ce` (loss, accuracy, prob and dlogits written), `unet_softmax_ce_weighted` with no option, with class weights, and
with class + pixel weights + ignore_empty (~10 % unlabeled rows).  Every launch reads a buffer set it has not touched for ROTATE - 1
launches (ROTATE sets, together larger than the 256 MB Infinity Cache), so the figures are HBM figures.  The candidates alternate in blocks
of ROTATE launches, every entry-point call (its two launches: the pass and the one-workgroup finalize) between its own pair of events; the
table is the median over REPS blocks of the mean per call, the spread its min .. max.  Bytes are the algorithmic ones (every tensor read or
written once: 32 B per pixel at K = 2, + 4 B with a pixel-weight map), set against the 8 TB/s HBM peak and the 6.29 TB/s a copy kernel
reaches.  The file states the outcome against the expectation written down before any run:
  no option    no slower than unet_softmax_ce beyond that kernel's own spread (max / min over the blocks);
  all options  within the byte ratio ((32 + 4) / 32 at K = 2) times that spread.
Written to profiles/weighted_loss.txt by default."""
import ctypes, importlib, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
L = importlib.import_module("semantic-segmentation-unet_amd._lib").lib()
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
assert torch.cuda.is_available(), "needs an MI355X: a CPU run cannot give a time"
ROTATE, WARM, REPS = 12, 3, 25
COPY_TBS, PEAK_TBS = 6.29, 8.0


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
    tbs = nbytes / (med * 1e-3) / 1e12
    return "%-44s %8.2f us  (min %8.2f, max %8.2f)  %6.1f MB  %5.2f TB/s = %3.0f %% of %.2f / %3.0f %% of %.0f" % (
        name, med * 1e3, min(ms) * 1e3, max(ms) * 1e3, nbytes / 1e6, tbs, 100 * tbs / COPY_TBS, COPY_TBS, 100 * tbs / PEAK_TBS, PEAK_TBS)


n, h, w = 8, 512, 512
pix = n * h * w
g = torch.Generator(device="cuda").manual_seed(0)
lines = ["weighted loss kernel, %s, ROTATE %d buffer sets, median of %d blocks of %d calls (HIP events)" % (torch.cuda.get_device_name(0), ROTATE, REPS, ROTATE)]
for k in (2, 4):
    z = [torch.randn(pix, k, device="cuda", generator=g) for _ in range(ROTATE)]
    lab = []
    for _ in range(ROTATE):
        t = torch.nn.functional.one_hot(torch.randint(0, k, (pix,), device="cuda", generator=g), k).to(torch.int32)
        t[torch.rand(pix, device="cuda", generator=g) < 0.10] = 0
        lab.append(t.contiguous())
    pw = [torch.rand(pix, device="cuda", generator=g) * 2 for _ in range(ROTATE)]
    cw = torch.rand(k, device="cuda", generator=g) * 3.75 + 0.25
    prob = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
    dl = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
    loss, stats = torch.zeros(2, device="cuda"), torch.zeros(4, device="cuda")
    nb, nbw = L.unet_softmax_ce_workspace(pix), L.unet_softmax_ce_weighted_workspace(pix)
    ws = torch.empty(max(nb, nbw) + 256, dtype=torch.uint8, device="cuda")
    s = 1.0 / pix

    def weighted(cwt, pws, ignore):
        return lambda i: L.unet_softmax_ce_weighted(P(z[i]), k, P(lab[i]), P(cwt), P(pws[i]) if pws else None, ignore, P(prob[i]), P(dl[i]), k, pix, k,
                                                    0.0, s, s, 0.0, P(stats), P(ws), nbw, ST())
    fns = {
        "unet_softmax_ce": lambda i: L.unet_softmax_ce(P(z[i]), k, P(lab[i]), P(prob[i]), P(dl[i]), k, pix, k, 0.0, s, s, 0.0,
                                                       P(loss[0:1]), P(loss[1:2]), P(ws), nb, ST()),
        "weighted, no option": weighted(None, None, 0),
        "weighted, class weights": weighted(cw, None, 0),
        "weighted, class + pixel weights + ignore": weighted(cw, pw, 1),
    }
    t = measure(fns)
    # same inputs, same answer: with no option the two entry points write the same prob / dlogits bits
    fns["unet_softmax_ce"](0); torch.cuda.synchronize(); p0, d0 = prob[0].clone(), dl[0].clone()
    fns["weighted, no option"](0); torch.cuda.synchronize()
    assert torch.equal(p0, prob[0]) and torch.equal(d0, dl[0]) and stats[1].item() == loss[1].item()
    base = 3 * pix * k * 4 + pix * k * 4                     # logits, labels, prob, dlogits
    med = {name: statistics.median(v) for name, v in t.items()}
    spread = max(t["unet_softmax_ce"]) / min(t["unet_softmax_ce"])
    lines.append("logits / one-hot labels [%d, %d, %d, %d] fp32 / int32, prob and dlogits written (BASELINE config 2, train step)" % (n, h, w, k))
    for name in fns:
        lines.append(row(name, t[name], base + (pix * 4 if "pixel" in name else 0)))
    r0 = med["weighted, no option"] / med["unet_softmax_ce"]
    r3 = med["weighted, class + pixel weights + ignore"] / med["unet_softmax_ce"]
    bytes_ratio = (base + pix * 4) / base
    lines.append("spread of unet_softmax_ce over the blocks (max / min) = %.3f" % spread)
    lines.append("weighted, no option / unet_softmax_ce = %.3f: expectation (<= spread %.3f) %s" % (r0, spread, "MET" if r0 <= spread else "NOT MET"))
    lines.append("weighted, all options / unet_softmax_ce = %.3f: expectation (<= byte ratio %.3f x spread = %.3f) %s"
                 % (r3, bytes_ratio, bytes_ratio * spread, "MET" if r3 <= bytes_ratio * spread else "NOT MET"))
    del z, lab, pw, prob, dl
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "weighted_loss.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write(text)
