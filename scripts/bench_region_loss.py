"""HIP-event time of the region term's launches beside the CE launch they stand behind: python scripts/bench_region_loss.py [out.txt]

At the BASELINE config-2 train shape (prob / one-hot labels / dlogits [8, 512, 512, K], K = 2 and K = 4, ~10 % unlabeled rows) it times, in
the same process and on the SAME tensors: `unet_softmax_ce` (the step's loss launch, for scale), `unet_region_loss_sums` (its two launches:
the pass over prob and labels and the one-workgroup finalize, between one pair of events) and `unet_region_loss_bwd` (the read-modify-write of
dlogits); and `unet_region_loss_sums` on 8 images of 64 pixels, which is the finalize launch and two launch overheads with next to no pass.
Every launch reads a buffer set it has not touched for ROTATE - 1 launches (ROTATE sets, together larger than the 256 MB Infinity Cache), so
the figures are HBM figures.  The candidates alternate in blocks of ROTATE launches; the table is the median over REPS blocks of the mean
per call, the spread its min .. max.  Bytes are the algorithmic ones (every tensor read or written once: sums 16 B, backward 32 B, CE 32 B
per pixel at K = 2), set against the 8 TB/s HBM peak and the 6.29 TB/s a copy kernel reaches.  No threshold is set: the file
records the numbers.  Written to profiles/region_loss.txt by default."""
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
hw = h * w
pix = n * hw
g = torch.Generator(device="cuda").manual_seed(0)
lines = ["region term of the loss, %s, ROTATE %d buffer sets, median of %d blocks of %d calls (HIP events)" % (torch.cuda.get_device_name(0), ROTATE, REPS, ROTATE)]
for k in (2, 4):
    z = [torch.randn(pix, k, device="cuda", generator=g) for _ in range(ROTATE)]
    lab = []
    for _ in range(ROTATE):
        t = torch.nn.functional.one_hot(torch.randint(0, k, (pix,), device="cuda", generator=g), k).to(torch.int32)
        t[torch.rand(pix, device="cuda", generator=g) < 0.10] = 0
        lab.append(t.contiguous())
    prob = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
    dl = [torch.empty(pix, k, device="cuda") for _ in range(ROTATE)]
    loss, coef, stats = torch.zeros(2, device="cuda"), torch.zeros(n, k, 2, device="cuda"), torch.zeros(1 + k, device="cuda")
    nb, nbr = L.unet_softmax_ce_workspace(pix), L.unet_region_loss_workspace(n, hw, k)
    ws = torch.empty(max(nb, nbr) + 256, dtype=torch.uint8, device="cuda")
    s = 1.0 / pix
    ce = lambda i: L.unet_softmax_ce(P(z[i]), k, P(lab[i]), P(prob[i]), P(dl[i]), k, pix, k, 0.0, s, s, 0.0, P(loss[0:1]), P(loss[1:2]), P(ws), nb, ST())
    for i in range(ROTATE):
        ce(i)                                                # real probabilities and CE gradients in every set
    fns = {
        "unet_softmax_ce (the CE launch, for scale)": ce,
        "unet_region_loss_sums (pass + finalize)": lambda i: L.unet_region_loss_sums(P(prob[i]), k, P(lab[i]), 1, n, hw, k, 0.3, 0.7, 1.0, 1.0 / n, None,
                                                                                      P(coef), P(stats), P(ws), nbr, ST()),
        "unet_region_loss_bwd": lambda i: L.unet_region_loss_bwd(P(prob[i]), k, P(lab[i]), 1, P(coef), P(dl[i]), k, n, hw, k, ST()),
        "unet_region_loss_sums, 8 x 64 pixels": lambda i: L.unet_region_loss_sums(P(prob[i]), k, P(lab[i]), 1, n, 64, k, 0.3, 0.7, 1.0, 1.0 / n, None,
                                                                                   P(coef), P(stats), P(ws), nbr, ST()),
    }
    t = measure(fns)
    # same inputs, same answer: two runs of the sums give the same bits
    fns["unet_region_loss_sums (pass + finalize)"](0); torch.cuda.synchronize(); c0, s0 = coef.clone(), stats.clone()
    fns["unet_region_loss_sums (pass + finalize)"](0); torch.cuda.synchronize()
    assert torch.equal(c0, coef) and torch.equal(s0, stats) and torch.isfinite(stats).all()
    one = pix * k * 4
    nbytes = {"unet_softmax_ce (the CE launch, for scale)": 4 * one, "unet_region_loss_sums (pass + finalize)": 2 * one, "unet_region_loss_bwd": 4 * one,
              "unet_region_loss_sums, 8 x 64 pixels": 2 * n * 64 * k * 4}
    lines.append("prob / one-hot labels / dlogits [%d, %d, %d, %d] fp32 / int32 / fp32 (BASELINE config 2, train step), ignore_empty, ~10 %% unlabeled" % (n, h, w, k))
    for name in fns:
        lines.append(row(name, t[name], nbytes[name]))
    med = {name: statistics.median(v) for name, v in t.items()}
    term = med["unet_region_loss_sums (pass + finalize)"] + med["unet_region_loss_bwd"]
    lines.append("region term (three launches) = %.2f us = %.2f x the CE launch; spread of the CE launch over the blocks (max / min) = %.3f"
                 % (term * 1e3, term / med["unet_softmax_ce (the CE launch, for scale)"],
                    max(t["unet_softmax_ce (the CE launch, for scale)"]) / min(t["unet_softmax_ce (the CE launch, for scale)"])))
    del z, lab, prob, dl
text = "\n".join(lines) + "\n"
print(text, end="", flush=True)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "region_loss.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
open(out, "w").write(text)
