"""The border-distance weight map on the device: `unet_border_weights` against the CPU restatement (border_weight_cases.py) -- the squared
distances bit for bit against the brute force, the weights within a derived bound of the fp64 value (and, printed, how many differ from
its fp32 rounding at all: the kernel evaluates in double and rounds once) -- its refusals, and the plumbing up to
`model.UNet(border_weight=, border_sigma=)` against a second network that is handed the restatement's map as explicit pixel_weights.

Weight bound: |w - w64| <= 4 * 2^-24 * (1 + w0) * max(m).  Derived: rounding the exponent's argument moves the term by at most
max_x x e^-x * 2^-24 = 0.37 * 2^-24 of w0; expf is within 1 ulp; the multiply by w0, the add of 1 and the multiply by m add half an ulp each."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import unet_numpy as on
import border_weight_cases as bw

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
ISENTINEL = -777
PAD = 64                                   # elements of sentinel on either side of an output (256 bytes: the views stay 16-byte aligned)
EINVAL, ENOSPC = -1, -2


@pytest.fixture(scope="module", autouse=True)
def leave_the_global_generators_as_found():
    """networks built here reseed torch's generators; tests elsewhere draw unseeded inputs from them, so hand them back untouched"""
    state = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state())
    yield
    torch.set_rng_state(state[0]); torch.cuda.set_rng_state_all(state[1]); np.random.set_state(state[2])


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def framed(n, dtype, fill):
    """-> (allocation, view of n elements PAD elements in); all of it holds `fill`"""
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def run_border(hip, lab, m, w0, sigma, want_d2=True, label_offset=0):
    """lab int32 one-hot [N,H,W,K] (numpy or device tensor), m fp32 [N,H,W] or None -> (weights fp32 [N,H,W], d2 int32 [N,H,W] or None) as
    numpy, after checking that nothing around the outputs was written and that the inputs are unchanged.  label_offset (int32 elements):
    where the labels start in their allocation (4 bytes off: not 16-byte aligned, the generic one-hot pass)"""
    lab = torch.as_tensor(np.ascontiguousarray(lab)) if not torch.is_tensor(lab) else lab
    n, h, w, k = lab.shape
    npix = n * h * w
    lbuf = torch.full((npix * k + 8,), 7, dtype=torch.int32, device=DEV)
    labd = lbuf[label_offset:label_offset + npix * k]
    labd.copy_(lab.reshape(-1))
    lab_before = lbuf.clone()
    md = torch.as_tensor(np.array(m)).to(DEV) if m is not None else None       # (a copy: the shared cases are read-only)
    m_before = md.clone() if md is not None else None
    wbuf, wv = framed(npix, torch.float32, SENTINEL)
    dbuf, dv = framed(npix, torch.int32, ISENTINEL) if want_d2 else (None, None)
    nb = hip.unet_border_weights_workspace(n, h, w)
    assert nb > 0
    wsbuf, ws = framed(nb, torch.uint8, 0x5A)
    c = float(np.float32(-1.0 / (2.0 * float(sigma) ** 2)))
    hip.unet_border_weights(P(labd), k, P(md), float(w0), c, P(wv), P(dv), n, h, w, P(ws), nb, ST())
    torch.cuda.synchronize()
    assert (wbuf[:PAD] == SENTINEL).all() and (wbuf[PAD + npix:] == SENTINEL).all()
    assert (wsbuf[:PAD] == 0x5A).all() and (wsbuf[PAD + nb:] == 0x5A).all()                 # the workspace is used within its declared size
    if want_d2:
        assert (dbuf[:PAD] == ISENTINEL).all() and (dbuf[PAD + npix:] == ISENTINEL).all()
    assert torch.equal(lbuf, lab_before) and (md is None or torch.equal(md, m_before))
    wout = wv.cpu().numpy().reshape(n, h, w)
    return wout, (dv.cpu().numpy().reshape(n, h, w) if want_d2 else None)


def weight_bound(w0, m):
    return 4.0 * 2.0 ** -24 * (1.0 + w0) * (float(np.max(m)) if m is not None else 1.0)


@pytest.mark.parametrize("name", bw.NAMES)
def test_d2_is_the_brute_force_and_weights_meet_the_derived_bound(hip, name):
    cm, k, m, d2_ref = bw.case(name)
    lab = bw.onehot(cm, k)
    for w0, sigma in bw.SETTINGS:
        wout, d2 = run_border(hip, lab, m, w0, sigma)
        assert d2.dtype == np.int32 and np.array_equal(d2.astype(np.int64), d2_ref), (name, w0, sigma)
        ref = bw.weights_fp64(d2_ref, w0, sigma, m)
        err = np.abs(wout.astype(np.float64) - ref).max()
        print("%s w0=%g sigma=%g: max |w - w64| = %.3g (bound %.3g), %d of %d differ from float32(w64)" % (
            name, w0, sigma, err, weight_bound(w0, m), int((wout != ref.astype(np.float32)).sum()), wout.size))
        assert err <= weight_bound(w0, m), (name, w0, sigma, err)
        if (d2_ref == bw.NONE).all():                                                        # no border: w == m exactly
            assert np.array_equal(wout, m if m is not None else np.ones_like(wout)), name
    # the labels 4 bytes off a 16-byte boundary: K = 2 then takes the generic one-hot pass; same bits
    w_off, d2_off = run_border(hip, lab, m, *bw.SETTINGS[0], label_offset=1)
    w_al, _ = run_border(hip, lab, m, *bw.SETTINGS[0])
    assert np.array_equal(d2_off.astype(np.int64), d2_ref) and np.array_equal(w_off.view(np.uint32), w_al.view(np.uint32)), name


def test_k4_takes_the_packed_one_hot_pass(hip):
    cm = bw.case("blobs_k5")[0] % 4                                                         # 3 x 37 x 130 = 14430 pixels: a tail of 2
    d2_ref = np.stack([bw.d2_bruteforce(c) for c in cm])
    assert (d2_ref > 0).any() and (d2_ref == 0).any()
    _, d2 = run_border(hip, bw.onehot(cm, 4), None, 10.0, 5.0)
    assert np.array_equal(d2.astype(np.int64), d2_ref)


def test_first_maximum_and_non_positive_rows(hip):
    """the class is the FIRST maximum of the row, as in unet_softmax_ce_weighted; a row without a positive entry is unlabeled"""
    cm = np.array([[[0, 0, 1, 1, -1, 2, 2, 2]] * 4])
    lab = bw.onehot(cm, 3)
    lab[0, :, 2, :] = [0, 5, 5]              # first maximum: class 1
    lab[0, :, 3, :] = [-3, 2, 1]             # class 1
    lab[0, :, 4, :] = [0, -1, 0]             # no positive entry: unlabeled
    lab[0, :, 5, :] = [1, 1, 3]              # class 2
    for off in (0, 1):
        _, d2 = run_border(hip, lab, None, 1.0, 1.0, label_offset=off)
        assert np.array_equal(d2.astype(np.int64), np.stack([bw.d2_bruteforce(cm[0])]))
    assert d2[0, 0].tolist() == [1, 0, 0, 1, 4, 9, 16, 25]


def test_grid_stride_loops_wrap_and_the_widest_rows(hip):
    """70 x 8 x 16000: more column chunks than 4096 workgroups x 256 lanes and more pixel quads than that too, rows of 64000 bytes of LDS
    (the limit is 16384 columns); vertical stripes 50 wide, so d2 is known in closed form and no search is long"""
    assert 70 * ((8 + 31) // 32) * 16000 > 4096 * 256 and 70 * 8 * 16000 // 4 > 4096 * 256
    for n, h, w in ((70, 8, 16000), (1, 2, 16384)):                  # and the limit itself: a row of exactly 64 KiB
        striped(hip, n, h, w, 50)


def striped(hip, n, h, w, period):
    x = np.arange(w)
    border = ((x % period == 0) & (x > 0)) | ((x % period == period - 1) & (x < w - 1))
    bx = np.nonzero(border)[0]
    d2_row = (np.abs(x[:, None] - bx[None, :]).min(1) ** 2).astype(np.int32)
    cls = torch.as_tensor((x // period) % 2).to(DEV)
    lab = torch.stack([1 - cls, cls], -1).to(torch.int32).expand(n, h, w, 2).contiguous()
    wout, d2 = run_border(hip, lab, None, 10.0, 5.0)
    assert np.array_equal(d2, np.broadcast_to(d2_row, (n, h, w)))
    ref = bw.weights_fp64(d2_row, 10.0, 5.0)
    assert np.abs(wout.astype(np.float64) - ref).max() <= weight_bound(10.0, None)


def test_null_pixel_weights_and_null_d2_change_nothing(hip):
    for name in ("blobs_k5", "blobs_k2_with_pixel_weights", "two_uniform_images"):
        cm, k, _, _ = bw.case(name)
        lab = bw.onehot(cm, k)
        w_full, _ = run_border(hip, lab, np.ones(cm.shape, np.float32), 10.0, 5.0, want_d2=True)
        w_bare, none = run_border(hip, lab, None, 10.0, 5.0, want_d2=False)
        assert none is None and np.array_equal(w_full.view(np.uint32), w_bare.view(np.uint32)), name


def test_two_calls_with_another_shape_in_between_give_the_same_bits():
    eng = pkg("engine").Engine(2, 1)
    cm, k, m, d2_ref = bw.case("blobs_k2_with_pixel_weights")
    lab, md = torch.as_tensor(bw.onehot(cm, k)).to(DEV), torch.as_tensor(np.array(m)).to(DEV)
    other = torch.as_tensor(bw.onehot(bw.case("diagonal")[0], 2)).to(DEV)
    w1, d1 = (t.clone() for t in eng.border_weights(lab, 10.0, 5.0, pixel_weights=md, return_d2=True))
    eng.border_weights(other, 3.0, 40.0)
    w2, d2 = eng.border_weights(lab, 10.0, 5.0, pixel_weights=md, return_d2=True)
    assert torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and torch.equal(d1, d2)
    assert np.array_equal(d2.cpu().numpy().astype(np.int64), d2_ref)
    with pytest.raises(ValueError):
        eng.border_weights(lab, -1.0, 5.0)
    with pytest.raises(ValueError):
        eng.border_weights(lab, 1.0, 0.0)
    with pytest.raises(ValueError):
        eng.border_weights(lab, 1.0, 5.0, pixel_weights=md[:1])


def test_refusals_launch_nothing(hip):
    raw = hip.cdll.unet_border_weights                    # the unchecked entry point: the status is the result
    n, h, w, k = 1, 8, 8, 2
    lab = torch.as_tensor(bw.onehot(np.zeros((n, h, w), np.int64), k)).to(DEV)
    wbuf, wv = framed(n * h * w, torch.float32, SENTINEL)
    dbuf, dv = framed(n * h * w, torch.int32, ISENTINEL)
    nb = hip.unet_border_weights_workspace(n, h, w)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    c = -1.0 / 50.0

    def status(K=k, w0=10.0, cc=c, H=h, W=w, nbytes=nb):
        return raw(P(lab), K, None, w0, cc, P(wv), P(dv), n, H, W, P(ws), nbytes, ST())

    assert status(H=16385) == EINVAL and status(W=16385) == EINVAL
    assert hip.unet_border_weights_workspace(1, 16385, 8) == 0 and hip.unet_border_weights_workspace(1, 16384, 16384) > 0
    assert status(w0=-1.0) == EINVAL and status(w0=float("nan")) == EINVAL and status(w0=float("inf")) == EINVAL
    assert status(cc=0.0) == EINVAL and status(cc=0.5) == EINVAL and status(cc=float("nan")) == EINVAL
    assert status(K=0) == EINVAL and status(K=256) == EINVAL
    assert status(nbytes=nb - 1) == ENOSPC
    torch.cuda.synchronize()
    assert (wbuf == SENTINEL).all() and (dbuf == ISENTINEL).all()
    assert status() == 0
    torch.cuda.synchronize()
    assert (wv == 1.0).all() and (dv == bw.NONE).all()


# ---- plumbing: N = 2, C = 1, 32 x 32, K = 2 ------------------------------------------------------------------------------------------------
N, C, K, HW = 2, 1, 2, 32
W0, SIGMA = 10.0, 5.0


@functools.lru_cache(maxsize=None)
def e2e_case():
    rng = np.random.default_rng(29)
    img, lab = on.synthetic_batch(N, C, K, HW, HW, seed=29)
    prm = on.init_params(C, K, seed=29)
    for key in prm:                                                  # no tensor starts at zero: "its largest magnitude" means something
        if key.endswith(("bias", "beta")):
            prm[key] = rng.normal(0, 0.1, prm[key].shape).astype(np.float32)
        if key.endswith("gamma"):
            prm[key] = rng.uniform(0.5, 1.5, prm[key].shape).astype(np.float32)
    masks = {"drop_4": rng.integers(0, 2, (N, 512, HW // 8, HW // 8)), "drop_b": rng.integers(0, 2, (N, 1024, HW // 16, HW // 16))}
    m = rng.uniform(0.25, 2.0, (N, HW, HW)).astype(np.float32)
    d2 = np.stack([bw.d2_bruteforce(c) for c in lab.argmax(-1)])
    assert (d2 == 0).any() and (d2 > 4).any() and (d2 < bw.NONE).all()
    return img, lab, prm, masks, m, d2


def one_step(kind, dtype, border, pixel_weights):
    """-> (loss, loss_stats, parameters after the step | gradients | None) of a fresh network from the same seed and parameters"""
    img, lab, prm, masks, _, _ = e2e_case()
    kw = {"border_weight": W0, "border_sigma": SIGMA} if border else {}
    net = pkg("model").UNet(K, N, C, compute_dtype=dtype, **kw)
    e = net.engine
    e.load_parameters(prm)
    if kind == "train":
        loss = net.train_step((img, lab, None, None), dropout_masks=masks, pixel_weights=pixel_weights)
    elif kind == "test":
        loss = net.test_step((img, lab, None, None), pixel_weights=pixel_weights)
    else:                                                            # "grad": the train step up to its gradients, without Adam
        it, lt = torch.as_tensor(img), torch.as_tensor(lab)
        e.forward(it, training=True, dropout_masks=masks, labels=lt, global_batch_size=N, want_grad=True, **net._loss_kw(pixel_weights, it, lt))
        e.backward()
        loss = pkg("model")._Loss(e.loss_buf[0:1].clone())
    assert e.weighted_loss
    after = {"train": e.export_parameters, "grad": e.export_gradients}.get(kind, lambda: None)()
    return float(loss.numpy()), e.loss_stats.cpu().numpy().copy(), after


def ranked_differences(a, b):
    """[(max |a - b| over a tensor / that tensor's largest magnitude in b, name)], largest first"""
    return sorted(((np.abs(a[key] - b[key]).max() / max(np.abs(b[key]).max(), 1e-30), key) for key in b), reverse=True)


@pytest.mark.parametrize("with_caller_weights", [False, True], ids=["map_alone", "times_caller_weights"])
@pytest.mark.parametrize("kind, dtype", [("train", "fp32"), ("test", "fp32"), ("train", "bf16"), ("grad", "fp32")])
def test_step_with_border_weight_is_the_step_with_the_explicit_map(kind, dtype, with_caller_weights):
    """Tolerances: the weighted-loss test's own (loss 2e-6 relative, counts exact, weight sum 1e-6 relative) and every parameter after the
    step within 1e-5 of its tensor's largest magnitude; the same in bf16.  The parameter bound cannot be met by a map that differs from the
    fp64 one in its last bit: measured with an fp32 expf in the kernel, bott_a/kernel sat at 2.0e-3 / 3.7e-3 of its magnitude, and two
    EXPLICIT maps one ulp apart (printed below for the record) at 2.4e-3, because the first Adam step moves an element by
    lr g / (|g| + 1e-7).  The kernel therefore evaluates the weight in double and rounds once, so both runs see the same map.  The "grad"
    cases hold the gradients before Adam to the weighted-loss test's own gradient bound."""
    _, _, _, _, m, d2 = e2e_case()
    caller = m if with_caller_weights else None
    explicit = bw.weights_fp64(d2, W0, SIGMA, caller).astype(np.float32)
    loss_a, stats_a, prm_a = one_step(kind, dtype, True, caller)
    loss_b, stats_b, prm_b = one_step(kind, dtype, False, explicit)
    print("%s %s: loss %.9g vs %.9g" % (kind, dtype, loss_a, loss_b))
    assert abs(loss_a - loss_b) <= 2e-6 * abs(loss_b)
    assert abs(stats_a[0] - stats_b[0]) <= 2e-6 * abs(stats_b[0]) and stats_a[1] == stats_b[1] and stats_a[2] == stats_b[2]
    assert abs(stats_a[3] - stats_b[3]) <= 1e-6 * abs(stats_b[3])
    assert abs(stats_b[3] - explicit.astype(np.float64).sum()) <= 1e-6 * stats_b[3]          # and the map really is in the loss
    if prm_b is not None:
        ranked = ranked_differences(prm_a, prm_b)
        print("largest differences relative to the tensor's magnitude:", ["%s %.3g" % (key, v) for v, key in ranked[:4]])
        if kind == "train" and dtype == "fp32":                      # (a figure only: what a one-ulp change of the explicit map itself does)
            _, _, prm_c = one_step(kind, dtype, False, np.nextafter(explicit, np.float32(np.inf)))
            print("two explicit maps one ulp apart:", ["%s %.3g" % (key, v) for v, key in ranked_differences(prm_c, prm_b)[:4]])
        if kind == "grad":
            # gradients: the weighted-loss test's own measure and bound against the oracle (L2 error over the tensor's norm < 1e-4, the
            # transposed convs' biases left out: in front of BatchNorm their gradient is exactly zero and what is stored is rounding noise)
            errs = {key: np.linalg.norm(prm_a[key].astype(np.float64) - prm_b[key]) / max(np.linalg.norm(prm_b[key]), 1e-6 * np.sqrt(prm_b[key].size))
                    for key in prm_b if not (key.startswith("up_") and key.endswith("/bias"))}
            print("largest gradient L2 error:", sorted(((v, key) for key, v in errs.items()), reverse=True)[:3])
            assert max(errs.values()) < 1e-4
        else:
            assert ranked[0][0] <= 1e-5, ranked[:4]


def test_default_step_is_unchanged():
    img, lab, prm, masks, _, _ = e2e_case()
    out = []
    for kw in ({}, {"border_weight": 0.0, "border_sigma": 3.0}):
        net = pkg("model").UNet(K, N, C, **kw)
        net.engine.load_parameters(prm)
        net.engine.profile = {}
        loss = net.train_step((img, lab, None, None), dropout_masks=masks)
        fams = set(net.engine.profile)
        net.engine.profile = None
        assert net.engine.weighted_loss is False and net.border is None and net._loss_kw(None, torch.as_tensor(img), torch.as_tensor(lab)) == {}
        assert "border_weights" not in fams and "softmax_ce" in fams and "softmax_ce_weighted" not in fams
        out.append((np.float32(loss.numpy()), net.engine.bufs["dy_logits"].cpu().numpy()))
        with pytest.raises(ValueError):
            net.border_weight_map(lab)
    assert out[0][0].view(np.uint32) == out[1][0].view(np.uint32) and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    on_net = pkg("model").UNet(K, N, C, border_weight=W0, border_sigma=SIGMA)
    on_net.engine.load_parameters(prm)
    on_net.engine.profile = {}
    on_net.train_step((img, lab, None, None), dropout_masks=masks)
    assert {"border_weights", "softmax_ce_weighted"} <= set(on_net.engine.profile)


def test_border_weight_map_of_labels_from_the_feed_with_an_ignore_label():
    feed = pkg("feed")
    net = pkg("model").UNet(2, 1, 1, border_weight=W0, border_sigma=SIGMA)
    for name in ("unlabeled_band_between_classes", "unlabeled_blob_beside_a_border"):
        cm, k, _, d2_ref = bw.case(name)
        cls = torch.as_tensor(np.where(cm < 0, 255, cm).astype(np.uint8))
        f = feed.DeviceFeed(iter([(torch.zeros(1, 1, *cm.shape[1:]), cls)]), torch.device(DEV, 0), classmap=True, number_classes=k, ignore_label=255)
        _, lab = next(f)
        f.close()
        assert lab.is_cuda and (lab.sum(-1) == 0).any()
        m = np.full(cm.shape, 0.5, np.float32)
        wmap, d2 = net.border_weight_map(lab, pixel_weights=m, return_distance=True)
        assert np.array_equal(d2.cpu().numpy().astype(np.int64), d2_ref), name
        assert np.abs(wmap.cpu().numpy() - bw.weights_fp64(d2_ref, W0, SIGMA, m)).max() <= weight_bound(W0, m)
        assert np.array_equal(net.border_weight_map(lab.cpu().numpy()).cpu().numpy(), 2.0 * wmap.cpu().numpy())      # numpy labels, no caller weights


def test_train_cli_with_the_augmentation_on(tmp_path):
    out = str(tmp_path / "out")
    pkg("train").main(["--output_dir", out, "--batch_size", "2", "--test_every_n_steps", "2", "--synthetic", "64x64x1x8", "--max_epochs", "1",
                       "--border_weight", "10", "--border_sigma", "5"])                      # --use_augmentation defaults to 1
    losses = [float(v) for v in open(tmp_path / "out" / "test_loss.csv").read().split()]
    assert len(losses) == 1 and np.isfinite(losses[0])
