"""The full-resolution tensors at the class-map end of an fp32 training step that are formed on load instead of stored:
dec_1b's dy inside its BatchNorm backward (unet_bn_bwd_classmap) and dec_1b's BatchNorm output inside the class map's forward and weight
gradient (unet_conv1x1_fwd_bn / unet_conv1x1_wgrad_bn).  Both paths call the same device functions for dy / dz / y and keep the order of
every sum, so every comparison here is BIT-identity (torch.equal / array_equal) against the path that stores the tensor: kernel level
first, then whole train steps with each switch on and off."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (N, H, W, C, K): P = 60 / 512 / 35 pixels -- one block with a tail, several blocks, an odd pixel count; K = 2 and 4 take the vector loads of
# the class gradients, K = 6 the scalar ones and the 8-accumulator kernels; C = 128 is 16 lanes per pixel and the generic 1x1 kernels
CASES = [(1, 6, 10, 64, 2), (2, 16, 16, 64, 4), (1, 5, 7, 128, 6)]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def half_zero_relu(shape, gen):
    """a post-ReLU tensor: roughly half of the elements exactly 0, so the ReLU mask of the backward matters"""
    return torch.relu(torch.randn(shape, generator=gen, device=DEV))


def batch_stats(r, c):
    flat = r.reshape(-1, c).double()
    mean = flat.mean(0)
    invstd = 1.0 / torch.sqrt(flat.var(0, unbiased=False) + 1e-3)
    return mean.float().contiguous(), invstd.float().contiguous()


@pytest.mark.parametrize("case", CASES)
def test_bn_bwd_from_classmap_dz_is_bit_identical_to_dgrad_then_bn_bwd(hip, case):
    n, h, w, c, k = case
    pix = n * h * w
    gen = torch.Generator(device=DEV).manual_seed(100 + pix + k)
    r = half_zero_relu((n, h, w, c), gen)
    dzl = torch.randn((n, h, w, k), generator=gen, device=DEV)
    wk = torch.randn((c, k), generator=gen, device=DEV) * 0.3
    gm = torch.rand(c, generator=gen, device=DEV) + 0.5
    mean, invstd = batch_stats(r, c)
    nb = hip.unet_bn_workspace(pix, c)
    out = []
    for fused in (False, True):
        dz = torch.full((n, h, w, c), float("nan"), device=DEV)
        dgamma, dbeta, dbias, dbias_deferred = (torch.full((c,), float("nan"), device=DEV) for _ in range(4))
        ws = torch.zeros(nb + 256, dtype=torch.uint8, device=DEV)
        rows = ctypes.c_int(0)
        for deferred in (False, True):                    # the finished bias gradient, and the form the engine uses (partials + unet_bn_bwd_bias)
            hb = ctypes.byref(rows) if deferred else None
            db = None if deferred else dbias
            if fused:
                hip.unet_bn_bwd_classmap(P(dzl), k, P(wk), k, n, h, w, P(r), c, P(gm), P(mean), P(invstd), c, 1, P(dz), c,
                                         P(dgamma), P(dbeta), P(db), P(ws), nb, ST(), hb)
            else:
                dy = torch.empty((n, h, w, c), device=DEV)
                hip.unet_conv1x1_dgrad(P(dzl), k, P(wk), P(dy), c, 0, pix, c, k, ST())
                hip.unet_bn_bwd_any(P(dy), c, None, 0, None, n, h, w, P(r), c, P(gm), P(mean), P(invstd), c, 1, P(dz), c, 0,
                                    P(dgamma), P(dbeta), P(db), None, 0, P(ws), nb, ST(), 0, 0, 0, hb)
        assert rows.value > 0
        hip.unet_bn_bwd_bias(P(ws), rows.value, c, P(dbias_deferred), ST())
        out.append((dz, dgamma, dbeta, dbias, dbias_deferred, rows.value))
    torch.cuda.synchronize()
    (dz0, dg0, db0, bi0, bd0, rows0), (dz1, dg1, db1, bi1, bd1, rows1) = out
    assert rows0 == rows1
    assert torch.isfinite(dz1).all() and (dz1[r == 0] == 0).all() and bool((r == 0).float().mean() > 0.3)
    assert torch.equal(dz0, dz1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert torch.equal(bi0, bi1) and torch.equal(bd0, bd1) and torch.equal(bi1, bd1)
    # ... and both are the BatchNorm backward of dy = dz_logits . w^T (fp64 restatement; 2e-5 as for the other backward kernels)
    dy64 = dzl.double().reshape(-1, k) @ wk.double().t()
    r64 = r.double().reshape(-1, c)
    xhat = (r64 - mean.double()) * invstd.double()
    a = gm.double() * invstd.double()
    dz64 = (r64 > 0) * a * (dy64 - dy64.mean(0) - xhat * (dy64 * xhat).mean(0))
    assert float((dz1.double().reshape(-1, c) - dz64).abs().max()) < 2e-5 * float(dz64.abs().max())


@pytest.mark.parametrize("case", CASES)
def test_classmap_reading_r_through_batchnorm_is_bit_identical_to_apply_then_classmap(hip, case):
    n, h, w, c, k = case
    pix = n * h * w
    gen = torch.Generator(device=DEV).manual_seed(200 + pix + k)
    r = half_zero_relu((n, h, w, c), gen)
    scale = torch.randn(c, generator=gen, device=DEV)
    shift = torch.randn(c, generator=gen, device=DEV)
    scale[3] = 0.0                                         # a channel with gamma = 0: y is the constant shift there
    wk = torch.randn((c, k), generator=gen, device=DEV) * 0.3
    bias = torch.randn(k, generator=gen, device=DEV)
    dzl = torch.randn((n, h, w, k), generator=gen, device=DEV)
    y = torch.empty_like(r)
    hip.unet_bn_apply_any(P(r), c, 0, P(scale), P(shift), P(y), c, 0, None, 0, None, n, h, w, c, ST())
    out0, out1 = torch.full((n, h, w, k), float("nan"), device=DEV), torch.full((n, h, w, k), float("nan"), device=DEV)
    hip.unet_conv1x1_fwd(P(y), c, 0, P(wk), P(bias), P(out0), k, pix, c, k, 1, ST())
    hip.unet_conv1x1_fwd_bn(P(r), c, P(scale), P(shift), P(wk), P(bias), P(out1), k, pix, c, k, 1, ST())
    nb = hip.unet_conv1x1_wgrad_workspace(pix, c, k)
    ws = torch.zeros(nb + 256, dtype=torch.uint8, device=DEV)
    dw0, dw1 = torch.full((c, k), float("nan"), device=DEV), torch.full((c, k), float("nan"), device=DEV)
    hip.unet_conv1x1_wgrad(P(y), c, 0, P(dzl), k, P(dw0), pix, c, k, P(ws), nb, ST())
    hip.unet_conv1x1_wgrad_bn(P(r), c, P(scale), P(shift), P(dzl), k, P(dw1), pix, c, k, P(ws), nb, ST())
    torch.cuda.synchronize()
    assert torch.isfinite(out1).all() and torch.isfinite(dw1).all()
    assert torch.equal(out0, out1) and torch.equal(dw0, dw1)
    y64 = r.double() * scale.double() + shift.double()
    ref = torch.relu(y64.reshape(-1, c) @ wk.double() + bias.double())
    assert float((out1.double().reshape(-1, k) - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    dwref = y64.reshape(-1, c).t() @ dzl.double().reshape(-1, k)
    assert float((dw1.double() - dwref).norm() / dwref.norm()) < 2e-6


# ------------------------------------------------------------------------------------------------------------ whole train steps
def recorded(e, fn):
    """fn() with the engine's launch recording on -> (fn's result, {family: launches})"""
    e.profile = {}
    try:
        out = fn()
    finally:
        counts = {key: len(v) for key, v in e.profile.items()}
        e.profile = None
    return out, counts


SWITCHES = ("classmap_dy_on_load", "classmap_bn_on_load")


def run_step(cfg, route, off):
    """one recorded forward + backward, then a whole train_step (Adam) from the same parameters -> loss, flat gradient, theta, counts"""
    n, c, k, hw = cfg
    img, lab = on.synthetic_batch(n, c, k, hw, hw, seed=5)
    prm = on.init_params(c, k, seed=5)
    rng = np.random.default_rng(5)
    masks = {"drop_4": rng.integers(0, 2, (n, 512, hw // 8, hw // 8)), "drop_b": rng.integers(0, 2, (n, 1024, hw // 16, hw // 16))}
    net = pkg("model").UNet(k, n, c, learning_rate=3e-4)
    e = net.engine
    e.opt.fp32_matrix = route
    for name in off:
        setattr(e.opt, name, False)
    e.load_parameters(prm)

    def step():
        e.forward(torch.as_tensor(img), training=True, dropout_masks=masks, labels=torch.as_tensor(lab), global_batch_size=n, want_grad=True)
        e.backward()
    _, counts = recorded(e, step)
    grad = e.grad.detach().cpu().numpy().copy()
    loss0 = e.loss_buf[0].item()
    e.load_parameters(prm)                                 # (the moving statistics moved)
    loss = float(net.train_step((img, lab, None, None), dropout_masks=masks).numpy())
    assert loss == loss0
    return loss, grad, e.grad.detach().cpu().numpy().copy(), e.theta.detach().cpu().numpy().copy(), counts, e.pl


@pytest.mark.parametrize("route", ["bf16x6", "native"])
@pytest.mark.parametrize("cfg", [(2, 1, 2, 32), (2, 3, 4, 32)])
def test_train_step_is_bit_identical_with_each_switch_on_and_off(cfg, route):
    base = run_step(cfg, route, off=SWITCHES)              # the schedule that stores both tensors
    assert "classmap_dgrad" in base[4] and not base[5].layer["dec_1b"].dy_from_classmap and base[5].layer["dec_1b"].y is not None
    for off in ((), ("classmap_dy_on_load",), ("classmap_bn_on_load",)):
        loss, grad, grad2, theta, counts, pl = run_step(cfg, route, off)
        assert loss == base[0], off
        assert np.array_equal(grad, base[1]) and np.array_equal(grad2, base[2]) and np.array_equal(theta, base[3]), off
        assert np.isfinite(theta).all()
        dy_on, bn_on = "classmap_dy_on_load" not in off, "classmap_bn_on_load" not in off
        assert pl.layer["dec_1b"].dy_from_classmap == dy_on and (pl.layer["logits"].dx is None) == dy_on
        assert pl.layer["dec_1b"].y_in_classmap == bn_on and pl.layer["logits"].x_bn_on_load == bn_on
        # the launches: no class-map data gradient, one BatchNorm apply fewer, as many BatchNorm backward calls as before
        assert ("classmap_dgrad" not in counts) == dy_on, (off, counts)
        assert counts["bn_apply"] == base[4]["bn_apply"] - (1 if bn_on else 0), (off, counts)
        assert counts["bn_bwd"] == base[4]["bn_bwd"] == 23 and counts["classmap_fwd"] == counts["classmap_wgrad"] == 1, (off, counts)


def test_inference_and_eval_backward_keep_every_buffer(hip):
    # test_step / inference / the eval-mode input gradient (estimate_radius) run the schedule they ran before: nothing deferred
    n, c, k, hw = 1, 1, 2, 32
    img, lab = on.synthetic_batch(n, c, k, hw, hw, seed=6)
    net = pkg("model").UNet(k, n, c)
    e = net.engine
    e.load_parameters(on.init_params(c, k, seed=6))
    prob, counts = recorded(e, lambda: e.forward(torch.as_tensor(img)))
    assert not e.pl.layer["dec_1b"].y_in_classmap and not e.pl.layer["dec_1b"].dy_from_classmap and "y_dec_1b" in e.bufs
    g, counts = recorded(e, lambda: e.input_gradient_eval(torch.ones_like(prob)))
    assert counts.get("classmap_dgrad") == 1 and tuple(g.shape) == (n, c, hw, hw) and bool(torch.isfinite(g).all())
