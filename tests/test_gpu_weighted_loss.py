"""The weighted training loss on the device: `unet_softmax_ce_weighted` against its fp64 restatement (weighted_loss_cases.py) on every path
(dense K = 2 / 4, generic), against the unweighted kernel bit for bit, its two companions (`unet_labels_onehot_ignore`,
`unet_confusion_scores_valid`) and the plumbing up to `model.UNet` against the oracle.  Tolerances are those of `unet_softmax_ce`'s own test
(test_gpu_kernels.py: prob 2e-6, dlogits 5e-6, loss 2e-6, 2e-5 on the clip path, each relative to the largest reference magnitude)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import unet_numpy as on
import weighted_loss_cases as wl

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
SIZES = [1, 63, 64, 65, 255, 257, 70001]                # odd counts on the pixel-pair path, the last pass ending mid-wave
WRAP = 3 * 1024 * 256 + 4465                            # more pixels than 1024 workgroups x 256 lanes: the grid-stride loop wraps
PATHS = [(2, 2, 0), (2, 2, 8), (2, 2, 4), (3, 4, 0), (4, 4, 0), (4, 6, 0), (5, 5, 0), (21, 21, 0)]       # (K, ldz, byte offset)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


@functools.lru_cache(maxsize=None)
def case(npix, k):
    z, lab, cw, pw = wl.make_case(npix, k, seed=11)
    for a in (z, lab, cw, pw):
        a.setflags(write=False)
    return z, lab, cw, pw


def placed(a, ld, offset_bytes, dtype, fill):
    """a [P, K] -> a device view [P, K] with leading dimension ld, starting offset_bytes into a 256-byte-aligned allocation; everything
    else in the allocation holds `fill`"""
    npix, k = a.shape
    off = offset_bytes // 4
    buf = torch.full((off + npix * ld + 4,), fill, dtype=dtype, device=DEV)
    view = buf[off:off + npix * ld].view(npix, ld)
    view[:, :k] = torch.as_tensor(np.array(a)).to(DEV)
    assert view.data_ptr() % 256 == offset_bytes
    return buf, view


def run_weighted(hip, z, lab, cw=None, pw=None, ignore=0, ls=0.0, scale=1.0, clip=0.0, ld=None, offset=0):
    """-> prob [P, K], dlogits [P, K] (numpy), stats [4] (numpy), after checking that nothing outside the K columns was written"""
    npix, k = z.shape
    ld = ld or k
    _, zd = placed(z, ld, offset, torch.float32, 1e30)           # a padding column read as a logit would wreck the row
    _, labd = placed(lab, k, offset, torch.int32, 7)
    pbuf, prob = placed(np.full((npix, k), SENTINEL, np.float32), k, offset, torch.float32, SENTINEL)
    dbuf, dl = placed(np.full((npix, k), SENTINEL, np.float32), ld, offset, torch.float32, SENTINEL)
    cwd = torch.as_tensor(np.array(cw)).to(DEV) if cw is not None else None
    pwd = torch.as_tensor(np.array(pw)).to(DEV) if pw is not None else None
    stats = torch.full((4,), SENTINEL, device=DEV)
    nb = hip.unet_softmax_ce_weighted_workspace(npix)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    hip.unet_softmax_ce_weighted(P(zd), ld, P(labd), P(cwd), P(pwd), int(ignore), P(prob), P(dl), ld, npix, k, float(ls), float(scale), float(scale),
                                 float(clip), P(stats), P(ws), nb, ST())
    torch.cuda.synchronize()
    inside = torch.zeros_like(dbuf, dtype=torch.bool)
    off = offset // 4
    inside[off:off + npix * ld].view(npix, ld)[:, :k] = True
    assert (dbuf[~inside] == SENTINEL).all() and (pbuf[:off] == SENTINEL).all() and (pbuf[off + npix * k:] == SENTINEL).all()
    return prob[:, :k].cpu().numpy(), dl[:, :k].cpu().numpy(), stats.cpu().numpy()


def check_against_restatement(hip, npix, k, ld, offset, opt):
    _, use_cw, use_pw, ignore, ls, clip = opt
    z, lab, cw, pw = case(npix, k)
    scale = 1.0 / (4 * npix)
    ref = wl.weighted_ce(z, lab, cw if use_cw else None, pw if use_pw else None, ignore, ls, scale, scale, clip)
    prob, dl, stats = run_weighted(hip, z, lab, cw if use_cw else None, pw if use_pw else None, ignore, ls, scale, clip, ld, offset)
    what = (npix, k, ld, offset, opt[0])
    assert not (prob == SENTINEL).any() and not (dl == SENTINEL).any(), what            # every row of both was written
    assert relerr(prob, ref["prob"]) < 2e-6, what
    assert relerr(dl, ref["dlogits"]) < 5e-6, what
    assert abs(stats[0] - ref["loss"]) <= (2e-5 if clip else 2e-6) * abs(ref["loss"]), what
    assert stats[1] == ref["correct"] and stats[2] == ref["valid"], what
    assert abs(stats[3] - ref["weight_sum"]) <= 1e-6 * abs(ref["weight_sum"]), what
    if ignore:
        rows = dl[lab.max(-1) == 0]
        assert (rows == 0).all() and not np.signbit(rows).any(), what                   # bitwise +0.0


@pytest.mark.parametrize("opt", wl.OPTIONS, ids=[o[0] for o in wl.OPTIONS])
@pytest.mark.parametrize("path", PATHS, ids=["K%d_ld%d_off%d" % p for p in PATHS])
def test_weighted_ce_matches_the_fp64_restatement(hip, path, opt):
    k, ld, offset = path
    for npix in SIZES:
        check_against_restatement(hip, npix, k, ld, offset, opt)


@pytest.mark.parametrize("path", [(2, 2, 0), (4, 4, 0), (5, 5, 0)], ids=["dense2", "dense4", "generic"])
def test_weighted_ce_grid_stride_wraps(hip, path):
    k, ld, offset = path
    check_against_restatement(hip, WRAP, k, ld, offset, wl.OPTIONS[3])


@pytest.mark.parametrize("k", [2, 4, 5])
def test_every_pixel_unlabeled(hip, k):
    npix = 257
    z, _, cw, pw = case(npix, k)
    lab = np.zeros((npix, k), np.int32)
    for ls in (0.0, 0.1):
        prob, dl, stats = run_weighted(hip, z, lab, cw, pw, 1, ls, 1.0 / npix)
        assert not (prob == SENTINEL).any() and relerr(prob, wl.weighted_ce(z, lab)["prob"]) < 2e-6
        assert (dl == 0).all() and not np.signbit(dl).any()
        assert np.array_equal(stats, np.zeros(4, np.float32)) and not np.signbit(stats[0])
    # the same rows without ignore_empty behave as in unet_softmax_ce: class 0
    _, _, stats = run_weighted(hip, z, lab, None, None, 0, 0.0, 1.0 / npix)
    assert stats[1] == (z.argmax(-1) == 0).sum() and stats[2] == npix


def run_parent(hip, z, lab, scale):
    npix, k = z.shape
    zd, labd = torch.as_tensor(np.array(z)).to(DEV), torch.as_tensor(np.array(lab)).to(DEV)
    prob, dl = torch.empty(npix, k, device=DEV), torch.empty(npix, k, device=DEV)
    res = torch.zeros(2, device=DEV)
    nb = hip.unet_softmax_ce_workspace(npix)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    hip.unet_softmax_ce(P(zd), k, P(labd), P(prob), P(dl), k, npix, k, 0.0, float(scale), float(scale), 0.0, P(res[0:1]), P(res[1:2]), P(ws), nb, ST())
    torch.cuda.synchronize()
    return prob.cpu().numpy(), dl.cpu().numpy(), res.cpu().numpy()


def labeled_case(npix, k):
    z, lab, _, _ = case(npix, k)
    lab = lab.copy()
    lab[lab.max(-1) == 0, k - 1] = 1                       # proper one-hot rows: ysum == 1
    return z, lab


@pytest.mark.parametrize("path", [(2, 0), (2, 4), (4, 0), (5, 0), (21, 0)], ids=["dense2", "generic2", "dense4", "K5", "K21"])
def test_unit_weights_are_the_unweighted_kernel_bit_for_bit(hip, path):
    k, offset = path
    for npix in (257, 70001):
        z, lab = labeled_case(npix, k)
        scale = 1.0 / (2 * npix)
        p0, d0, r0 = run_parent(hip, z, lab, scale)
        p1, d1, s1 = run_weighted(hip, z, lab, np.ones(k, np.float32), np.ones(npix, np.float32), 0, 0.0, scale, 0.0, k, offset)
        assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
        assert abs(float(s1[0]) - float(r0[0])) <= np.spacing(np.float32(r0[0]))          # 1 fp32 ulp: the partial sums are grouped differently
        assert s1[1] == r0[1] and s1[2] == npix and s1[3] == npix
        # with no option at all the entry is the same function
        p2, d2, s2 = run_weighted(hip, z, lab, None, None, 0, 0.0, scale, 0.0, k, offset)
        assert np.array_equal(p2.view(np.uint32), p0.view(np.uint32)) and np.array_equal(d2.view(np.uint32), d0.view(np.uint32))
        assert np.array_equal(s2, s1)
        # class_weight = c * ones, c a power of two: dlogits scale exactly
        _, d3, s3 = run_weighted(hip, z, lab, np.full(k, 0.5, np.float32), None, 0, 0.0, scale, 0.0, k, offset)
        assert np.array_equal(d3.view(np.uint32), (np.float32(0.5) * d0).view(np.uint32))
        assert s3[3] == 0.5 * npix


def test_bad_arguments_are_refused(hip):
    lib = pkg("_lib")
    z, lab, cw, pw = case(64, 2)
    zd, cwd = torch.as_tensor(np.array(z)).to(DEV), torch.as_tensor(np.array(cw)).to(DEV)
    prob = torch.empty(64, 2, device=DEV)
    nb = hip.unet_softmax_ce_weighted_workspace(64)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    hip.unet_softmax_ce_weighted(P(zd), 2, None, None, None, 0, P(prob), None, 0, 64, 2, 0.0, 0.0, 0.0, 0.0, None, P(ws), nb, ST())     # inference: prob only
    torch.cuda.synchronize()
    assert relerr(prob.cpu().numpy(), wl.weighted_ce(z, lab)["prob"]) < 2e-6
    for kw in ({"cw": cwd}, {"ignore": 1}):                 # weights / ignore_empty need the labels
        with pytest.raises(lib.UnetHipError, match="bad argument"):
            hip.unet_softmax_ce_weighted(P(zd), 2, None, P(kw.get("cw")), None, kw.get("ignore", 0), P(prob), None, 0, 64, 2, 0.0, 0.0, 0.0, 0.0,
                                         None, P(ws), nb, ST())
    with pytest.raises(lib.UnetHipError, match="workspace too small"):
        hip.unet_softmax_ce_weighted(P(zd), 2, None, None, None, 0, P(prob), None, 0, 64, 2, 0.0, 0.0, 0.0, 0.0, None, P(ws), nb - 1, ST())


@pytest.mark.parametrize("k", [2, 5])
def test_labels_onehot_ignore(hip, k):
    npix = 70001
    rng = np.random.default_rng(k)
    cls = rng.integers(0, k + 2, npix).astype(np.uint8)                     # k and k + 1 are out of range
    cls[rng.choice(npix, 500, replace=False)] = 255
    cd = torch.as_tensor(cls).to(DEV)

    def run(fn, *extra):
        out = torch.full((npix, k), 9, dtype=torch.int32, device=DEV)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        fn(P(cd), P(out), npix, k, *extra, P(bad), ST())
        torch.cuda.synchronize()
        return out.cpu().numpy(), int(bad.item())

    old, bad_old = run(hip.unet_labels_onehot)
    assert bad_old == (cls >= k).sum()
    for ign in (-1, 0, k - 1, 255):
        got, bad = run(hip.unet_labels_onehot_ignore, ign)
        want = ((cls[:, None] == np.arange(k)) & (cls[:, None] != ign)).astype(np.int32)
        assert np.array_equal(got, want), ign
        assert bad == ((cls >= k) & (cls != ign)).sum(), ign
        if ign == -1:
            assert np.array_equal(got, old) and bad == bad_old


@pytest.mark.parametrize("path", [(2, 2, 0), (2, 2, 8), (2, 2, 4), (3, 4, 0), (4, 4, 0), (5, 5, 0), (21, 21, 0), (70, 70, 0)],
                         ids=lambda p: "K%d_ld%d_off%d" % p)
def test_confusion_scores_valid(hip, path):
    k, ld, offset = path
    for npix in (1, 65, 70001):
        z, lab, _, _ = case(npix, k)
        labeled = lab.max(-1) > 0
        _, zd = placed(z, ld, offset, torch.float32, 1e30)
        _, labd = placed(lab, k, offset, torch.int32, 7)
        cm = torch.zeros(k, k, dtype=torch.int64, device=DEV)
        hip.unet_confusion_scores_valid(P(zd), ld, P(labd), npix, k, P(cm), ST())
        torch.cuda.synchronize()
        want = np.bincount(lab.argmax(-1)[labeled] * k + z.argmax(-1)[labeled], minlength=k * k).reshape(k, k)
        assert np.array_equal(cm.cpu().numpy(), want), (npix, path)
        if k <= 21:
            _, _, stats = run_weighted(hip, z, lab, None, None, 1, 0.0, 1.0 / npix, 0.0, ld, offset)
            assert np.trace(want) == stats[1] and want.sum() == stats[2], (npix, path)       # the invariant of DESIGN.md 5.1
        full = torch.zeros(k, k, dtype=torch.int64, device=DEV)                              # the unweighted form still counts such rows as class 0
        hip.unet_confusion_scores(P(zd), ld, P(labd), npix, k, P(full), ST())
        assert int(full.sum().item()) == npix


# ---- end to end: N = 2, C = 1, 32 x 32, K = 2, fp32, both matrix routes ------------------------------------------------------------------
ROUTES = ["bf16x6", "native"]
N, C, K, HW = 2, 1, 2, 32


def e2e_case():
    rng = np.random.default_rng(23)
    img, lab = on.synthetic_batch(N, C, K, HW, HW, seed=23)
    prm = on.init_params(C, K, seed=23)
    for key in prm:
        if key.endswith(("bias", "beta")):
            prm[key] = rng.normal(0, 0.1, prm[key].shape).astype(np.float32)
        if key.endswith("gamma"):
            prm[key] = rng.uniform(0.5, 1.5, prm[key].shape).astype(np.float32)
    masks = {"drop_4": rng.integers(0, 2, (N, 512, HW // 8, HW // 8)), "drop_b": rng.integers(0, 2, (N, 1024, HW // 16, HW // 16))}
    lab = lab.copy()
    lab[rng.uniform(size=(N, HW, HW)) < 0.10] = 0                    # ~10 % unlabeled rows
    pw = rng.uniform(0.0, 2.0, (N, HW, HW)).astype(np.float32)
    pw[rng.uniform(size=pw.shape) < 0.05] = 0.0
    return img, lab, prm, masks, pw


def make_net(route, **kw):
    net = pkg("model").UNet(K, N, C, **kw)
    net.engine.opt.fp32_matrix = route
    return net


@pytest.mark.parametrize("route", ROUTES)
def test_unit_class_weights_leave_the_step_bit_identical(route):
    img, lab, prm, masks, _ = e2e_case()
    out = []
    for kw in ({}, {"class_weights": [1.0, 1.0]}):
        net = make_net(route, **kw)
        net.engine.load_parameters(prm)
        net.engine.profile = {}
        loss = float(net.train_step((img, lab, None, None), dropout_masks=masks).numpy())
        fams = set(net.engine.profile)
        net.engine.profile = None
        assert ("softmax_ce_weighted" in fams) == bool(kw) and ("softmax_ce" in fams) != bool(kw)
        out.append((net.engine.bufs["dy_logits"].cpu().numpy(), net.engine.bufs["softmax"].cpu().numpy(), loss))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    assert abs(out[0][2] - out[1][2]) <= np.spacing(np.float32(out[0][2]))


@pytest.mark.parametrize("route", ROUTES)
def test_weighted_step_matches_the_oracle(route, monkeypatch):
    img, lab, prm, masks, pw = e2e_case()
    cw = [0.5, 3.0]
    net = make_net(route, class_weights=cw, ignore_unlabeled=True)
    e = net.engine
    e.load_parameters(prm)
    it = torch.as_tensor(img)
    e.forward(it, training=True, dropout_masks=masks, labels=torch.as_tensor(lab), global_batch_size=N, want_grad=True,
              **net._loss_kw(pw, it))
    e.backward()
    torch.cuda.synchronize()
    assert e.weighted_loss
    # the oracle with its loss replaced by the weighted restatement (oracle/ itself is untouched) and the device run's branch decisions
    held = {}

    def ce_fwd(logits, labels, G, ls, contract):
        n, h, w, k = logits.shape
        s = 1.0 / (G * h * w)
        r = wl.weighted_ce(logits.reshape(-1, k), labels.reshape(-1, k), np.float32(cw), pw.reshape(-1), True, ls, s, s,
                           0.0 if contract.ce_from_softmax_logits else contract.ce_clip_eps)
        held["dl"], held["r"] = r["dlogits"].reshape(n, h, w, k), r
        return r["loss"], r["prob"].reshape(n, h, w, k), labels

    monkeypatch.setattr(on, "ce_loss_fwd", ce_fwd)
    monkeypatch.setattr(on, "ce_loss_bwd", lambda p, y, G, contract=None: held["dl"])
    relu = {name: (e.saved[name][1].float().permute(0, 3, 1, 2) > 0).cpu().numpy() for name, kind, _, _ in e.layers if kind != "deconv"}
    pidx = {"pool_%d" % l: e.idx[l].permute(0, 3, 1, 2).cpu().numpy().astype(np.int64) for l in (1, 2, 3, 4)}
    ref = on.OracleUNet(K, N, C, params=prm, dtype=np.float64)
    loss_ref, _, g_ref, _, _ = ref.loss_and_grads(img, lab, masks, relu_masks=relu, pool_idx=pidx)
    stats = e.loss_stats.cpu().numpy()
    assert abs(stats[0] - loss_ref) < 1e-5 * abs(loss_ref) and e.loss_buf[0].item() == stats[0]
    assert stats[2] == (lab.max(-1) > 0).sum() and abs(stats[3] - held["r"]["weight_sum"]) < 1e-6 * held["r"]["weight_sum"]
    g_hip = e.export_gradients()
    errs = {}
    for key, r in g_ref.items():
        r = np.asarray(r, dtype=np.float64)
        errs[key] = np.linalg.norm(g_hip[key].astype(np.float64) - r) / max(np.linalg.norm(r), 1e-6 * np.sqrt(r.size))
    for l in (1, 2, 3, 4):                                   # exactly-zero gradients (a bias in front of BatchNorm): test_gpu_unet.py
        errs.pop("up_%d/bias" % l)
    assert max(errs.values()) < 1e-4, sorted(errs.items(), key=lambda t: -t[1])[:6]


def test_test_step_accuracy_counts_labeled_pixels_only():
    model, metrics = pkg("model"), pkg("metrics")
    img, lab, prm, _, pw = e2e_case()
    net = make_net("bf16x6", class_weights=[0.5, 3.0], ignore_unlabeled=True)
    net.engine.load_parameters(prm)
    acc, lm = model.CategoricalAccuracy(), model.Mean()
    cm = metrics.ConfusionMatrix(K, device=net.engine.dev)
    net.test_step((img, lab, lm, acc), confusion=cm, pixel_weights=pw)
    stats = net.engine.loss_stats.cpu().numpy()
    valid = int((lab.max(-1) > 0).sum())
    assert 0 < valid < N * HW * HW and stats[2] == valid
    assert acc.total == stats[1] and acc.count == valid and acc.result() == np.float32(stats[1] / valid)
    m = cm.result()
    assert np.trace(m) == stats[1] and m.sum() == valid
    logits = net.engine.bufs["y_logits"].cpu().numpy().reshape(-1, K)
    assert stats[1] == ((lab.reshape(-1, K).argmax(-1) == logits.argmax(-1)) & (lab.reshape(-1, K).max(-1) > 0)).sum()
    with pytest.raises(ValueError):
        net.test_step((img, lab, None, None), pixel_weights=-pw)
    with pytest.raises(ValueError):
        model.UNet(K, N, C, class_weights=[1.0, 2.0, 3.0])


def test_bf16_step_uses_the_same_kernel(hip):
    img, lab, prm, masks, pw = e2e_case()
    cw = np.float32([0.5, 3.0])
    net = make_net("bf16x6", compute_dtype="bf16", class_weights=cw, ignore_unlabeled=True)
    net.engine.load_parameters(prm)
    loss = float(net.train_step((img, lab, None, None), dropout_masks=masks, pixel_weights=pw).numpy())
    e = net.engine
    z = e.bufs["y_logits"].cpu().numpy().reshape(-1, K)
    assert z.dtype == np.float32                                       # the logits are fp32 in both modes
    s = 1.0 / (N * HW * HW)
    _, dl, stats = run_weighted(hip, z, lab.reshape(-1, K), cw, pw.reshape(-1), 1, 0.0, s)
    assert np.array_equal(e.bufs["dy_logits"].cpu().numpy().reshape(-1, K).view(np.uint32), dl.view(np.uint32))
    assert np.isfinite(loss) and np.float32(loss) == stats[0]
