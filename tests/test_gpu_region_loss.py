"""The region term (soft Dice / Tversky per image) on the device: `unet_region_loss_sums` / `unet_region_loss_bwd` behind the CE kernel against
their fp64 restatement (region_loss_cases.py) on every path (dense K = 2 / 4, generic up to the K cap), their edge cases, split invariance,
determinism, refused arguments, and the plumbing up to `model.UNet` against the oracle.  Tolerances are the CE kernel's own
(test_gpu_kernels.py, test_gpu_weighted_loss.py): total dlogits (CE + region) 5e-6 relative to the largest reference magnitude, the region
loss and each mean T 2e-6 relative; test_region_loss_reference.py shows on the CPU that the device's operation order fits them."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import unet_numpy as on
import region_loss_cases as rl
import weighted_loss_cases as wl

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
K_CAP = 32                                               # include/unet_hip.h: K <= 32
SIZES = [1, 63, 64, 65, 257, 1022, 70001, 70002]         # odd counts take the generic path at K = 2; 1022 / 70002: the pixel-pair path with a tail wave
PATHS = [(2, 2, 0), (2, 2, 8), (2, 2, 4), (3, 4, 0), (4, 4, 0), (4, 6, 0), (5, 5, 0), (21, 21, 0), (K_CAP, K_CAP, 0)]    # (K, ld, byte offset)
# (name, alpha, beta, ignore, class weights)
OPTIONS = [("dice", 0.5, 0.5, False, False), ("tversky_ignore_cw", 0.3, 0.7, True, True), ("a1_b1_ignore_cw", 1.0, 1.0, True, True)]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def placed(a, ld, offset_bytes, dtype, fill):
    """a [P, K] -> (allocation, device view [P, ld]) starting offset_bytes into a 256-byte-aligned allocation filled with `fill`"""
    npix, k = a.shape
    off = offset_bytes // 4
    buf = torch.full((off + npix * ld + 4,), fill, dtype=dtype, device=DEV)
    view = buf[off:off + npix * ld].view(npix, ld)
    view[:, :k] = torch.as_tensor(np.array(a)).to(DEV)
    assert view.data_ptr() % 256 == offset_bytes
    return buf, view


def run_region(hip, z, lab, N, HW, alpha=0.5, beta=0.5, smooth=1.0, scale=1.0, cw=None, ignore=False, ld=None, offset=0, ce_scale=None,
               ce_cw=None, ce_pw=None, bwd=True):
    """The CE kernel, then the region launches on its prob and dlogits -> dict(prob, ce (the CE kernel's dlogits), total (after the region
    backward), coef [N, K, 2], stats [1 + K]) as numpy, after checking that nothing outside the K columns of dlogits was written and that
    prob and labels were only read"""
    npix, k = z.shape
    assert npix == N * HW
    ld = ld or k
    ce_scale = 1.0 / (4 * HW) if ce_scale is None else ce_scale
    _, zd = placed(z, ld, offset, torch.float32, 1e30)
    lbuf, labd = placed(lab, k, offset, torch.int32, 7)
    _, prob = placed(np.zeros((npix, k), np.float32), k, offset, torch.float32, SENTINEL)
    dbuf, dl = placed(np.full((npix, k), SENTINEL, np.float32), ld, offset, torch.float32, SENTINEL)
    dev = lambda a: torch.as_tensor(np.array(a)).to(DEV) if a is not None else None
    cwd, ce_cwd, ce_pwd = dev(cw), dev(ce_cw), dev(ce_pw)
    ce_stats = torch.zeros(4, device=DEV)
    nb = hip.unet_softmax_ce_weighted_workspace(npix)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    hip.unet_softmax_ce_weighted(P(zd), ld, P(labd), P(ce_cwd), P(ce_pwd), int(ignore), P(prob), P(dl), ld, npix, k, 0.0, float(ce_scale),
                                 float(ce_scale), 0.0, P(ce_stats), P(ws), nb, ST())
    ce = dl[:, :k].cpu().numpy()
    pbuf, pr = placed(prob.cpu().numpy(), ld, offset, torch.float32, 1e30)          # the region kernels' prob, with the path's leading dimension
    p_before, l_before = pbuf.clone(), lbuf.clone()
    coef = torch.full((N, k, 2), SENTINEL, device=DEV)
    stats = torch.full((1 + k,), SENTINEL, device=DEV)
    nbr = hip.unet_region_loss_workspace(N, HW, k)
    wsr = torch.empty(nbr + 256, dtype=torch.uint8, device=DEV)
    hip.unet_region_loss_sums(P(pr), ld, P(labd), int(ignore), N, HW, k, float(alpha), float(beta), float(smooth), float(scale), P(cwd),
                              P(coef), P(stats), P(wsr), nbr, ST())
    if bwd:
        hip.unet_region_loss_bwd(P(pr), ld, P(labd), int(ignore), P(coef), P(dl), ld, N, HW, k, ST())
    torch.cuda.synchronize()
    inside = torch.zeros_like(dbuf, dtype=torch.bool)
    off = offset // 4
    inside[off:off + npix * ld].view(npix, ld)[:, :k] = True
    assert (dbuf[~inside] == SENTINEL).all() and torch.equal(pbuf, p_before) and torch.equal(lbuf, l_before)
    return {"prob": prob.cpu().numpy(), "ce": ce, "total": dl[:, :k].cpu().numpy(), "coef": coef.cpu().numpy(), "stats": stats.cpu().numpy(),
            "ce_stats": ce_stats.cpu().numpy()}


def check_against_restatement(hip, N, HW, k, ld, offset, opt):
    _, alpha, beta, ignore, use_cw = opt
    z, lab, cw = rl.make_case(N, HW, k, seed=11)
    a, b, s, scale, ce_scale = rl.f32(alpha), rl.f32(beta), 1.0, rl.f32(0.8 / 4), 1.0 / (4 * HW)
    ref = rl.region_loss(z, lab, N, HW, a, b, s, scale, cw if use_cw else None, ignore)
    ce_ref = wl.weighted_ce(z, lab, None, None, ignore, 0.0, ce_scale, ce_scale)
    got = run_region(hip, z, lab, N, HW, a, b, s, scale, cw if use_cw else None, ignore, ld, offset, ce_scale)
    what = (N, HW, k, ld, offset, opt[0])
    total_ref = ce_ref["dlogits"] + ref["dlogits"]
    e_dl, e_loss = relerr(got["total"], total_ref), abs(got["stats"][0] - ref["loss"]) / abs(ref["loss"])
    e_t = (np.abs(got["stats"][1:] - ref["tbar"]) / ref["tbar"]).max()
    print("region loss %s: dlogits %.2e loss %.2e mean T %.2e" % (what, e_dl, e_loss, e_t))
    assert not (got["total"] == SENTINEL).any() and np.isfinite(got["total"]).all() and np.isfinite(got["coef"]).all(), what
    assert e_dl < 5e-6, what
    assert e_loss <= 2e-6 and e_t <= 2e-6, what
    assert np.abs(got["total"] - got["ce"]).max() > 0, what                          # the backward launch did add something
    if ignore:
        rows = got["total"][lab.max(-1) == 0]
        assert (rows == 0).all() and not np.signbit(rows).any(), what                 # bitwise +0.0


@pytest.mark.parametrize("opt", OPTIONS, ids=[o[0] for o in OPTIONS])
@pytest.mark.parametrize("path", PATHS, ids=["K%d_ld%d_off%d" % p for p in PATHS])
def test_region_kernels_match_the_fp64_restatement(hip, path, opt):
    k, ld, offset = path
    for N in (1, 3):
        for HW in SIZES:
            check_against_restatement(hip, N, HW, k, ld, offset, opt)


# more pixels per image than the 256 workgroup shares x 256 lanes of one pass (the loop over an image wraps), and with N = 5 more slots than
# the 1024 workgroups of the grid (the loop over the slots wraps)
@pytest.mark.parametrize("path", [(2, 2 * 65536 + 4466), (4, 65536 + 4465), (5, 65536 + 4465), (K_CAP, 65536 + 4465)],
                         ids=["dense2", "dense4", "generic", "generic_cap"])
def test_region_kernels_grid_stride_wraps(hip, path):
    k, HW = path
    check_against_restatement(hip, 5 if k < K_CAP else 1, HW, k, k, 0, OPTIONS[1])
    if k == K_CAP:
        check_against_restatement(hip, 5, 70002, k, k, 0, OPTIONS[1])


@pytest.mark.parametrize("k", [2, 4, 5])
def test_unlabeled_image_absent_class_and_zero_weight(hip, k):
    for HW in (256, 257):
        z, lab, cw = rl.make_case(2, HW, k, seed=3)
        # an image whose every pixel is unlabeled: T = 1, region loss exactly 0, dlogits rows bitwise +0.0
        got = run_region(hip, z[:HW], np.zeros((HW, k), np.int32), 1, HW, 0.3, 0.7, 1.0, 0.5, cw, True)
        assert np.array_equal(got["stats"], np.float32([0.0] + [1.0] * k)) and not np.signbit(got["stats"][0])
        assert (got["total"] == 0).all() and not np.signbit(got["total"]).any() and np.isfinite(got["coef"]).all()
        # next to a labeled image it adds nothing: the batch is the labeled image alone (same scale), its T = 1 enters the mean
        lab2 = lab.copy()
        lab2[:HW] = 0
        both = run_region(hip, z, lab2, 2, HW, 0.3, 0.7, 1.0, 0.5, cw, True)
        alone = run_region(hip, z[HW:], lab2[HW:], 1, HW, 0.3, 0.7, 1.0, 0.5, cw, True)
        assert both["stats"][0] == alone["stats"][0] and np.array_equal(bits(both["total"][HW:]), bits(alone["total"]))
        assert (both["total"][:HW] == 0).all() and not np.signbit(both["total"][:HW]).any()
        assert np.allclose(both["stats"][1:], (1.0 + alone["stats"][1:].astype(np.float64)) / 2, rtol=2e-7, atol=0)      # two fp32 roundings
        # a class absent from the image (make_case: class k - 1 in image 0) stays finite, with and without ignore
        for ignore in (False, True):
            got = run_region(hip, z[:HW], lab[:HW], 1, HW, 0.5, 0.5, 1e-3, 1.0, None, ignore)
            assert lab[:HW, k - 1].sum() == 0 and np.isfinite(got["total"]).all() and np.isfinite(got["coef"]).all() and np.isfinite(got["stats"]).all()
            ref = rl.region_loss(z[:HW], lab[:HW], 1, HW, 0.5, 0.5, rl.f32(1e-3), 1.0, None, ignore)
            assert abs(got["stats"][0] - ref["loss"]) <= 2e-6 * ref["loss"]
        # dice_weight = 0 passed through the kernels: the CE kernel's dlogits, bit for bit
        got = run_region(hip, z, lab, 2, HW, 0.5, 0.5, 1.0, 0.0, cw, True)
        assert np.array_equal(bits(got["total"]), bits(got["ce"])) and got["stats"][0] == 0


@pytest.mark.parametrize("k", [2, 4, 5])
def test_split_invariance(hip, k):
    """the point of the per-image definition: an image's dlogits rows and loss do not depend on the batch it arrives in"""
    for HW in (257, 1024, 70002):
        z, lab, cw = rl.make_case(2, HW, k, seed=7)
        scale = rl.f32(0.8 / 2)
        kw = dict(alpha=0.3, beta=0.7, smooth=1.0, scale=scale, cw=cw, ignore=True, ce_scale=1.0 / (2 * HW))
        both = run_region(hip, z, lab, 2, HW, **kw)
        one = [run_region(hip, z[i * HW:(i + 1) * HW], lab[i * HW:(i + 1) * HW], 1, HW, **kw) for i in (0, 1)]
        for i in (0, 1):
            assert np.array_equal(bits(both["total"][i * HW:(i + 1) * HW]), bits(one[i]["total"])), (k, HW, i)
            assert np.array_equal(bits(both["coef"][i]), bits(one[i]["coef"][0])), (k, HW, i)
        lb = np.float32(both["stats"][0])
        assert abs((float(one[0]["stats"][0]) + float(one[1]["stats"][0])) - float(lb)) <= np.spacing(lb), (k, HW)


@pytest.mark.parametrize("path", [(2, 2, 0), (2, 2, 4), (4, 4, 0), (21, 21, 0)], ids=lambda p: "K%d_ld%d_off%d" % p)
def test_two_runs_give_the_same_bits(hip, path):
    k, ld, offset = path
    z, lab, cw = rl.make_case(3, 70002, k, seed=9)
    a, b = (run_region(hip, z, lab, 3, 70002, 0.3, 0.7, 1.0, 0.25, cw, True, ld, offset) for _ in range(2))
    for key in ("coef", "stats", "total"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key


def test_bad_arguments_are_refused(hip):
    lib = pkg("_lib")
    N, HW, k = 1, 64, 2
    f = lambda *s: torch.zeros(*s, device=DEV)
    prob, lab, coef, stats, dl = f(64, 2), torch.zeros(64, 2, dtype=torch.int32, device=DEV), f(1, 2, 2), f(3), f(64, 2)
    big_p, big_l, big_c, big_s = f(64, K_CAP + 1), torch.zeros(64, K_CAP + 1, dtype=torch.int32, device=DEV), f(1, K_CAP + 1, 2), f(K_CAP + 2)
    nb = hip.unet_region_loss_workspace(N, HW, K_CAP + 1)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)

    def sums(prob=prob, lab=lab, k=k, alpha=0.5, beta=0.5, smooth=1.0, coef=coef, stats=stats, nbytes=nb):
        hip.unet_region_loss_sums(P(prob), k, P(lab), 0, N, HW, k, alpha, beta, smooth, 1.0, None, P(coef), P(stats), P(ws), nbytes, ST())

    sums()                                                  # the arguments the refusals below vary are fine as they stand
    sums(big_p[:, :K_CAP].contiguous(), big_l[:, :K_CAP].contiguous(), K_CAP, coef=big_c, stats=big_s)
    for kw in (dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float("nan")), dict(alpha=-0.1), dict(beta=-0.1),
               dict(prob=big_p, lab=big_l, k=K_CAP + 1, coef=big_c, stats=big_s), dict(prob=None), dict(lab=None), dict(coef=None), dict(stats=None)):
        with pytest.raises(lib.UnetHipError, match="bad argument"):
            sums(**kw)
    with pytest.raises(lib.UnetHipError, match="workspace too small"):
        sums(nbytes=hip.unet_region_loss_workspace(N, HW, k) - 1)
    with pytest.raises(lib.UnetHipError, match="bad argument"):
        hip.unet_region_loss_bwd(P(big_p), K_CAP + 1, P(big_l), 0, P(big_c), P(big_p.clone()), K_CAP + 1, N, HW, K_CAP + 1, ST())
    for kw in (dict(coef=None), dict(dl=None)):
        with pytest.raises(lib.UnetHipError, match="bad argument"):
            hip.unet_region_loss_bwd(P(prob), k, P(lab), 0, P(kw.get("coef", coef)), P(kw.get("dl", dl)), k, N, HW, k, ST())
    torch.cuda.synchronize()


# ---- end to end: N = 2, C = 1, 32 x 32, K = 2, both matrix routes --------------------------------------------------------------------------
ROUTES = ["bf16x6", "native"]
N, C, K, HW = 2, 1, 2, 32
REGION = dict(dice_weight=0.7, tversky=(0.3, 0.7), dice_smooth=1.0, dice_class_weights=[1.0, 3.0])
CW = [0.5, 3.0]


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


def region_ref(z, lab, ignore):
    a, b = (rl.f32(v) for v in REGION["tversky"])
    return rl.region_loss(z, lab, N, HW * HW, a, b, REGION["dice_smooth"], rl.f32(REGION["dice_weight"] / N), np.float32(REGION["dice_class_weights"]),
                          ignore)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain_ce", "weighted_ce"])
@pytest.mark.parametrize("route", ROUTES)
def test_compound_step_matches_the_oracle(route, weighted, monkeypatch):
    img, lab, prm, masks, pw = e2e_case()
    net = make_net(route, **REGION, **(dict(class_weights=CW, ignore_unlabeled=True) if weighted else {}))
    e = net.engine
    e.load_parameters(prm)
    it = torch.as_tensor(img)
    e.forward(it, training=True, dropout_masks=masks, labels=torch.as_tensor(lab), global_batch_size=N, want_grad=True,
              **net._loss_kw(pw if weighted else None, it))
    e.backward()
    torch.cuda.synchronize()
    assert e.weighted_loss == weighted
    # the oracle with its loss replaced by CE + the region restatement (oracle/ itself is untouched) and the device run's branch decisions
    held = {}

    def ce_fwd(logits, labels, G, ls, contract):
        n, h, w, k = logits.shape
        s = 1.0 / (G * h * w)
        clip = 0.0 if contract.ce_from_softmax_logits else contract.ce_clip_eps
        z2, l2 = logits.reshape(-1, k), labels.reshape(-1, k)
        r = wl.weighted_ce(z2, l2, np.float32(CW), pw.reshape(-1), True, ls, s, s, clip) if weighted else wl.weighted_ce(z2, l2, None, None, False, ls, s, s, clip)
        rg = region_ref(z2, l2, weighted)
        held["dl"], held["region"], held["tbar"] = (r["dlogits"] + rg["dlogits"]).reshape(n, h, w, k), rg["loss"], rg["tbar"]
        return r["loss"] + rg["loss"], r["prob"].reshape(n, h, w, k), labels

    monkeypatch.setattr(on, "ce_loss_fwd", ce_fwd)
    monkeypatch.setattr(on, "ce_loss_bwd", lambda p, y, G, contract=None: held["dl"])
    relu = {name: (e.saved[name][1].float().permute(0, 3, 1, 2) > 0).cpu().numpy() for name, kind, _, _ in e.layers if kind != "deconv"}
    pidx = {"pool_%d" % l: e.idx[l].permute(0, 3, 1, 2).cpu().numpy().astype(np.int64) for l in (1, 2, 3, 4)}
    ref = on.OracleUNet(K, N, C, params=prm, dtype=np.float64)
    loss_ref, _, g_ref, _, _ = ref.loss_and_grads(img, lab, masks, relu_masks=relu, pool_idx=pidx)
    loss = e.loss_buf[0].item()
    rs = e.region_stats.cpu().numpy()
    print("compound step %s weighted=%s: loss %.3e region %.3e" % (route, weighted, abs(loss - loss_ref) / abs(loss_ref), abs(rs[0] - held["region"]) / held["region"]))
    assert held["region"] > 0.05 * loss_ref                              # the term is a real share of the loss it is checked in
    assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref)
    assert abs(rs[0] - held["region"]) < 1e-5 * held["region"] and np.abs(rs[1:] - held["tbar"]).max() < 1e-5
    if weighted:
        assert e.loss_stats[0].item() == loss
    g_hip = e.export_gradients()
    errs = {}
    for key, r in g_ref.items():
        r = np.asarray(r, dtype=np.float64)
        errs[key] = np.linalg.norm(g_hip[key].astype(np.float64) - r) / max(np.linalg.norm(r), 1e-6 * np.sqrt(r.size))
    for l in (1, 2, 3, 4):                                   # exactly-zero gradients (a bias in front of BatchNorm): test_gpu_unet.py
        errs.pop("up_%d/bias" % l)
    assert max(errs.values()) < 1e-4, sorted(errs.items(), key=lambda t: -t[1])[:6]


@pytest.mark.parametrize("route", ROUTES)
def test_region_off_is_the_step_of_before(route):
    img, lab, prm, masks, _ = e2e_case()
    out = []
    for kw in ({}, dict(dice_weight=0.0, tversky=(0.3, 0.7), dice_smooth=0.5, dice_class_weights=[1.0, 3.0]), REGION):
        net = make_net(route, **kw)
        net.engine.load_parameters(prm)
        net.engine.profile = {}
        loss = float(net.train_step((img, lab, None, None), dropout_masks=masks).numpy())
        fams = set(net.engine.profile)
        net.engine.profile = None
        out.append((fams, bits(net.engine.bufs["dy_logits"].cpu().numpy()), loss, net.engine.region_stats, set(net.engine.bufs)))
    assert out[0][0] == out[1][0] and not any(f.startswith("region") for f in out[0][0]) and "softmax_ce" in out[0][0]
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert out[1][3] is None and out[0][4] == out[1][4] and not any(b.startswith("region") for b in out[1][4])       # no buffer either
    assert out[2][0] == out[0][0] | {"region_sums", "region_bwd"} and out[2][2] > out[0][2] and not np.array_equal(out[2][1], out[0][1])


def test_bf16_step_uses_the_same_kernels(hip):
    img, lab, prm, masks, pw = e2e_case()
    net = make_net("bf16x6", compute_dtype="bf16", class_weights=CW, ignore_unlabeled=True, **REGION)
    net.engine.load_parameters(prm)
    loss = float(net.train_step((img, lab, None, None), dropout_masks=masks, pixel_weights=pw).numpy())
    e = net.engine
    z = e.bufs["y_logits"].cpu().numpy().reshape(-1, K)
    assert z.dtype == np.float32                                       # the logits are fp32 in both modes
    got = run_region(hip, z, lab.reshape(-1, K), N, HW * HW, *REGION["tversky"], REGION["dice_smooth"], REGION["dice_weight"] / N,
                     np.float32(REGION["dice_class_weights"]), True, ce_scale=1.0 / (N * HW * HW), ce_cw=np.float32(CW), ce_pw=pw.reshape(-1))
    assert np.array_equal(bits(e.bufs["dy_logits"].cpu().numpy().reshape(-1, K)), bits(got["total"]))
    assert np.array_equal(bits(e.region_stats.cpu().numpy()), bits(got["stats"]))
    assert np.isfinite(loss) and np.float32(loss) == np.float32(got["ce_stats"][0]) + np.float32(got["stats"][0])


def test_test_step_returns_the_compound_loss():
    model = pkg("model")
    img, lab, prm, _, pw = e2e_case()
    res = []
    for kw in ({}, REGION):
        net = make_net("bf16x6", class_weights=CW, ignore_unlabeled=True, **kw)
        net.engine.load_parameters(prm)
        acc, lm = model.CategoricalAccuracy(), model.Mean()
        loss = net.test_step((img, lab, lm, acc), pixel_weights=pw).numpy()
        res.append((loss, lm.result(), acc.total, acc.count, net.engine.loss_stats.cpu().numpy(), net.engine.region_stats))
    ce, total = res[0], res[1]
    rs = total[5].cpu().numpy()
    ref = region_ref(net.engine.bufs["y_logits"].cpu().numpy().reshape(-1, K), lab.reshape(-1, K), True)
    assert ce[5] is None and abs(rs[0] - ref["loss"]) < 1e-5 * ref["loss"] and rs[0] > 0
    assert total[0] == np.float32(ce[0]) + np.float32(rs[0]) and total[1] == total[0] and total[4][0] == total[0]     # CE + region, in the metric too
    valid = int((lab.max(-1) > 0).sum())
    assert total[2] == ce[2] == total[4][1] and total[3] == ce[3] == valid                                            # the accuracy is as before
    assert "dy_logits" not in net.engine.bufs                                                                         # no gradient, no backward launch
