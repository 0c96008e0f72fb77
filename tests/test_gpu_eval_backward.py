"""The eval-mode backward chain (Engine.input_gradient_eval behind UNet.input_gradient / UNet.estimate_radius, reference
UNet/model.py:165-202) against fp64: every kernel that runs only on this path through the C ABI, on identical inputs, and the whole chain
end to end with the device run's branch decisions imposed on the oracle.  Every output buffer wider than its tensor carries a sentinel
in the padding channels, which must survive."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import unet_numpy as on
from oracle import unet_torch as ot
from test_gpu_unet import ROUTES, make_case, make_net, recorded

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -777.25          # exactly representable; no kernel under test produces it


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ unet_softmax_bwd
def _softmax_bwd_case(hip, npix, k, lddz, seed):
    rng = np.random.default_rng(seed)
    p32 = on.softmax_lastaxis(rng.standard_normal((npix, k)) * 3.0).astype(np.float32)
    g32 = rng.standard_normal((npix, k)).astype(np.float32)
    p, g = p32.astype(np.float64), g32.astype(np.float64)          # the reference starts from the values the kernel reads
    ref = p * (g - (g * p).sum(-1, keepdims=True))
    dz = torch.full((npix, lddz), SENT, device=DEV)
    pd, gd = torch.as_tensor(p32).to(DEV), torch.as_tensor(g32).to(DEV)
    hip.unet_softmax_bwd(P(pd), P(gd), P(dz), lddz, npix, k, ST())
    out = dz.cpu().numpy()
    return out[:, :k].astype(np.float64), out[:, k:], ref


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
def test_softmax_bwd_matches_fp64_formula(hip, k, pad):
    # dz_k = p_k (g_k - sum_j g_j p_j): a K-term fp32 dot product and one multiply -- the arithmetic of unet_softmax_ce's gradient, and its
    # bound (test_softmax_ce_accuracy_argmax: 2e-6 of max|ref|).  2*16*24 + 5 pixels: four blocks, the last one ragged.
    npix = 2 * 16 * 24 + 5
    got, padding, ref = _softmax_bwd_case(hip, npix, k, k + pad, seed=100 + k)
    if k == 1:
        assert ref.max() == 0 and not got.any()                     # one class: p = 1, the gradient is exactly zero
    else:
        assert np.abs(ref).max() > 0.1
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    assert (padding == SENT).all()


def test_softmax_bwd_grid_stride_loop_wraps(hip):
    # the grid is capped at 4096 blocks of 256 pixels: 300 pixels more than that are reached only by the second trip of the loop
    npix = 4096 * 256 + 300
    got, padding, ref = _softmax_bwd_case(hip, npix, 2, 3, seed=7)
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max()
    assert np.abs(ref[-300:]).max() > 0.1 and np.abs(got[-300:] - ref[-300:]).max() <= 2e-6 * np.abs(ref).max()
    assert (padding == SENT).all()


# ------------------------------------------------------------------------------------------------------------------ unet_bn_eval_bwd
def _bn_eval_bwd_case(hip, npix, c, lddy, off, ldr, lddz, relu, seed):
    """dy = channels [off, off + c) of a [npix, lddy] buffer; r [npix, ldr] and dz [npix, lddz] wider than c where the case says so"""
    g = torch.Generator().manual_seed(seed)
    dybuf = torch.randn(npix, lddy, generator=g)
    rbuf = torch.randn(npix, ldr, generator=g)                      # (both signs: the mask is the kernel's business, not the producer's)
    special = torch.tensor([0.0, -0.0, 1e-40, 1.4e-45, -1e-40, 1e-38], dtype=torch.float32)     # +0, -0, denormals of both signs
    where = torch.randperm(npix * c, generator=g)[:6 * 8]
    rows, cols = where // c, where % c
    rbuf[rows, cols] = special.repeat(8)
    scale = torch.randn(c, generator=g)
    scale[0], scale[1], scale[2] = -1.5, 0.0, 1e-6
    dy, r = dybuf[:, off:off + c], rbuf[:, :c]
    mask = r > 0                                                   # strictly: +0 and -0 are off, every positive denormal is on
    assert bool(mask[rows[2], cols[2]]) and bool(mask[rows[3], cols[3]]) and not bool(mask[rows[0], cols[0]]) and not bool(mask[rows[1], cols[1]])
    prod = dy * scale                                              # one fp32 multiply
    want = torch.where(mask, prod, torch.zeros(())) if relu else prod
    want64 = dy.double() * scale.double()
    if relu:
        want64 = torch.where(mask, want64, torch.zeros((), dtype=torch.float64))
    dyd, rd, sd = dybuf.to(DEV), rbuf.to(DEV), scale.to(DEV)
    dz = torch.full((npix, lddz), SENT, device=DEV)
    hip.unet_bn_eval_bwd(ctypes.c_void_p(dyd.data_ptr() + 4 * off), lddy, P(rd), ldr, P(sd), P(dz), lddz, npix, c, relu, ST())
    out = dz.cpu()
    assert torch.equal(bits(out[:, :c]), bits(want)), "not the fp32 product / select, bit for bit"
    assert relerr(out[:, :c].double().numpy(), want64.numpy()) < 1e-6
    assert (out[:, c:] == SENT).all()
    assert torch.equal(dyd.cpu(), dybuf) and torch.equal(bits(rd.cpu()), bits(rbuf))


BN_EVAL_CASES = {   # npix, C, lddy, channel offset of dy, ldr, lddz
    "vector": (1003, 64, 64, 0, 64, 64),
    "scalar": (1003, 6, 6, 0, 6, 6),
    "misaligned_slice_takes_scalar_path": (1003, 4, 8, 2, 4, 4),         # C % 4 == 0 and every ld % 4 == 0, but dy starts 8 bytes into a 16-byte group
    "up_N_call": (2 * 6 * 10, 128, 256, 128, 128, 128),                  # dy = dcat[..., 128:], lddy = 256
    "vector_wide_r_dz": (1003, 64, 64, 0, 72, 68),
    "scalar_wide_r_dz": (1003, 6, 6, 0, 9, 7),
}


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", sorted(BN_EVAL_CASES))
def test_bn_eval_bwd_is_one_fp32_multiply_and_a_select(hip, case, relu):
    _bn_eval_bwd_case(hip, *BN_EVAL_CASES[case], relu=relu, seed=len(case) + relu)


def test_bn_eval_bwd_grid_stride_loop_wraps(hip):
    # 8192 blocks of 256 float4 groups cover 131072 pixels of 64 channels: eight pixels more (34 MB per tensor)
    npix = 131073 + 7
    assert npix * 64 // 4 > 8192 * 256
    _bn_eval_bwd_case(hip, npix, 64, 64, 0, 64, 64, relu=1, seed=5)


# ------------------------------------------------------------------------------------------------------------ unet_conv3x3_dgrad_direct
def _dgrad_direct(hip, dz_nchw, wt, cin, lddz, lddx):
    """dz_nchw [N,Cout,H,W], wt [3,3,Cin,Cout] (numpy) -> (dx [N,Cin,H,W] float64, the padding channels of the dx buffer)"""
    n, cout, h, w = dz_nchw.shape
    dzb = torch.full((n, h, w, lddz), float("nan"), device=DEV)                  # a read past Cout poisons the result
    dzb[..., :cout] = torch.as_tensor(np.ascontiguousarray(dz_nchw.transpose(0, 2, 3, 1)).astype(np.float32)).to(DEV)
    wd = torch.as_tensor(np.ascontiguousarray(wt).astype(np.float32)).to(DEV)
    dx = torch.full((n, h, w, lddx), SENT, device=DEV)
    hip.unet_conv3x3_dgrad_direct(P(dzb), lddz, P(wd), P(dx), lddx, n, h, w, cin, cout, ST())
    out = dx.cpu().numpy()
    return out[..., :cin].transpose(0, 3, 1, 2).astype(np.float64), out[..., cin:]


@pytest.mark.parametrize("shape", [(2, 5, 7, 1, 64), (1, 6, 4, 3, 64), (2, 3, 3, 4, 64), (1, 1, 9, 5, 64), (1, 2, 1, 2, 8)])
def test_conv3x3_dgrad_direct_matches_oracle(hip, shape):
    # the first layer's data gradient (only the eval-mode chain computes it): every pixel of these images but a few is a border pixel
    n, h, w, ci, co = shape
    rng = np.random.default_rng(sum(shape))
    wt = (rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32).astype(np.float64)
    dz = rng.standard_normal((n, co, h, w)).astype(np.float32).astype(np.float64)
    dx_ref, _, _ = on.conv_same_bwd(np.zeros((n, ci, h, w)), wt, dz)
    dx, padding = _dgrad_direct(hip, dz, wt, ci, co + 4, ci + 3)
    assert relerr(dx, dx_ref) < 2e-5
    assert (padding == SENT).all()


def test_conv3x3_dgrad_direct_is_the_adjoint_of_the_first_layer_forward(hip):
    # <fwd(x), dz> == <x, dgrad(dz)> (no bias, no ReLU), products in fp64: a tap read from the wrong side passes neither this nor the oracle
    n, h, w, ci, co = 2, 5, 7, 3, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, h, w, ci, generator=g).to(DEV)
    dz = torch.randn(n, h, w, co, generator=g).to(DEV)
    wt = (torch.randn(3, 3, ci, co, generator=g) / float(np.sqrt(9 * ci))).to(DEV)
    y = torch.full((n, h, w, co), SENT, device=DEV)
    dx = torch.full((n, h, w, ci), SENT, device=DEV)
    hip.unet_conv3x3_fwd_direct(P(x), ci, P(wt), None, P(y), co, n, h, w, ci, co, 0, ST())
    hip.unet_conv3x3_dgrad_direct(P(dz), co, P(wt), P(dx), ci, n, h, w, ci, co, ST())
    dot = lambda a, b: float((a.double() * b.double()).sum())
    assert abs(dot(y, dz) - dot(x, dx)) <= 1e-5 * np.sqrt(dot(y, y) * dot(dz, dz))


def test_conv3x3_dgrad_direct_grid_stride_loop_wraps(hip):
    # 1 x 1024 x 1024 x 3 input elements, one per lane: 1.5 trips of the 8192 x 256 grid.  Reference: torch fp64 on the CPU (the gradient of
    # a 'same' cross-correlation is the transposed convolution with the same kernel)
    n, h, w, ci, co = 1, 1024, 1024, 3, 4
    assert n * h * w * ci > 8192 * 256
    rng = np.random.default_rng(3)
    wt = (rng.standard_normal((3, 3, ci, co)) / 6.0).astype(np.float32).astype(np.float64)
    dz = rng.standard_normal((n, co, h, w)).astype(np.float32).astype(np.float64)
    dx_ref = torch.nn.functional.conv_transpose2d(torch.as_tensor(dz), torch.as_tensor(wt).permute(3, 2, 0, 1).contiguous(), padding=1).numpy()
    small = on.conv_same_bwd(np.zeros((1, ci, 6, 1024)), wt, dz[:, :, :6])[0]                  # (the two references agree where both apply)
    assert np.abs(small[:, :, :5] - dx_ref[:, :, :5]).max() < 1e-12
    dx, padding = _dgrad_direct(hip, dz, wt, ci, co + 4, ci + 3)
    assert relerr(dx, dx_ref) < 2e-5
    assert relerr(dx[:, :, 700:], dx_ref[:, :, 700:]) < 2e-5                                  # the rows of the second trip
    assert (padding == SENT).all()


# ------------------------------------------------------------------------------------------- unet_maxpool2x2_bwd, the eval backward's call
@pytest.mark.parametrize("c", [64, 6])
def test_maxpool_bwd_accumulates_into_the_skip_half_only(hip, c):
    # accumulate = 1 into dcat[..., :ch], leading dimension 2 ch, whose upper half holds the gradient up_N has yet to read (C = 6: scalar path)
    n, h, w = 2, 6, 10
    rng = np.random.default_rng(c)
    dy = rng.standard_normal((n, c, h // 2, w // 2)).astype(np.float32)
    idx = rng.integers(0, 4, (n, c, h // 2, w // 2))
    base = rng.standard_normal((n, h, w, 2 * c)).astype(np.float32)
    ref = on.maxpool2x2_bwd(dy.astype(np.float64), idx) + base[..., :c].transpose(0, 3, 1, 2).astype(np.float64)
    dcat = torch.as_tensor(base).to(DEV)
    dyd = torch.as_tensor(np.ascontiguousarray(dy.transpose(0, 2, 3, 1))).to(DEV)
    idxd = torch.as_tensor(np.ascontiguousarray(idx.transpose(0, 2, 3, 1)).astype(np.uint8)).to(DEV)
    hip.unet_maxpool2x2_bwd(P(dyd), c, P(idxd), P(dcat), 2 * c, n, h, w, c, 1, 0, ST())
    out = dcat.cpu().numpy()
    assert relerr(out[..., :c].transpose(0, 3, 1, 2).astype(np.float64), ref) < 1e-6
    assert np.array_equal(out[..., c:], base[..., c:])


# ------------------------------------------------------------------------------------------------------------------ unet_labels_onehot
@pytest.mark.parametrize("k", [1, 2, 3, 256])
def test_labels_onehot_direct(hip, k):
    npix = 1000
    rng = np.random.default_rng(k)
    cls = rng.integers(0, min(k + 2, 256), npix).astype(np.uint8)        # labels >= K among them (none can exist for K = 256)
    cls[::97] = 255
    cls[5] = 0
    cls[6] = k - 1
    want = (cls[:, None].astype(np.int64) == np.arange(k)[None, :]).astype(np.int32)
    nbad = int((cls.astype(np.int64) >= k).sum())
    assert (nbad > 0) == (k < 256)
    cd = torch.as_tensor(cls).to(DEV)
    for with_counter in (True, False):
        onehot = torch.full((npix * k + 16,), -5, dtype=torch.int32, device=DEV)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        hip.unet_labels_onehot(P(cd), P(onehot), npix, k, P(bad) if with_counter else None, ST())
        out = onehot.cpu().numpy()
        assert np.array_equal(out[:npix * k].reshape(npix, k), want)
        assert (out[npix * k:] == -5).all()
        assert int(bad.item()) == (nbad if with_counter else 0)


# ------------------------------------------------------------------------------------------------------------------ the whole chain
def _nchw(t):
    return t.float().permute(0, 3, 1, 2).cpu().numpy()


def _device_decisions(e):
    relu = {name: _nchw(e.saved[name][1]) > 0 for name, kind, _, _ in e.layers if kind != "deconv"}
    pidx = {"pool_%d" % l: e.idx[l].permute(0, 3, 1, 2).cpu().numpy().astype(np.int64) for l in (1, 2, 3, 4)}
    return relu, pidx


def _layer_report(e, keep):
    """relative L2 distance of every stored dz / data gradient of the device chain from the oracle's, in backward order (failure message)"""
    rows = []
    for name in pkg("engine").BACKWARD_ORDER:
        for buf, key in (("dz_" + name, "dz_" + name), ("dy_in_" + name, "dx_" + name)):
            if buf in e.bufs and key in keep and tuple(_nchw(e.bufs[buf]).shape) == keep[key].shape:
                rows.append("%s %.2e" % (buf, np.linalg.norm(_nchw(e.bufs[buf]) - keep[key]) / (np.linalg.norm(keep[key]) + 1e-300)))
    return rows


_ORACLE_FORWARD = {}


def _case(cfg):
    """inputs, parameters, the fp64 oracle and its eval-mode forward pass: evaluated once per shape, shared by both routes"""
    if cfg not in _ORACLE_FORWARD:
        n, c, k, hw = cfg
        img, _, prm, _ = make_case(53, n, c, k, hw)
        h, w = hw if isinstance(hw, tuple) else (hw, hw)
        dprob = np.random.default_rng(54).standard_normal((n, h, w, k)).astype(np.float32)
        ref = on.OracleUNet(k, n, c, params=prm, dtype=np.float64)
        _ORACLE_FORWARD[cfg] = (img, prm, dprob, ref, ref.forward(img, training=False)[1])
    return _ORACLE_FORWARD[cfg]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cfg", [(1, 1, 2, 32), (2, 3, 4, (32, 48)), (1, 3, 4, 64), (1, 5, 3, 32), (1, 1, 2, 128)])
def test_input_gradient_matches_oracle_given_the_same_branch_decisions(cfg, route):
    # test_input_gradient_and_estimate_radius_match_oracle bounds this gradient by 5e-2, which is what flipped ReLU decisions cost and
    # enough to hide a wrong border tap, a wrong ReLU flag on one layer, one channel of a scale vector or a mis-stepped slice.  Here the
    # fp64 oracle's backward pass takes the device run's own decisions (r > 0 of every layer, the pools' first-max indices) -- checked to
    # be decisions it could have taken -- and what remains is one linear map evaluated in fp32 and in fp64: 1e-4 in relative L2, the
    # bound of the training gradients through the same data-gradient kernels (no batch statistics here, so no 5e-4 exception), over the
    # whole gradient and for every image channel on its own.
    n, c, k, hw = cfg
    img, prm, dprob, ref, cache = _case(cfg)
    h, w = hw if isinstance(hw, tuple) else (hw, hw)
    net = make_net(route, k, n, c)
    e = net.engine
    e.load_parameters(prm)
    e.forward(torch.as_tensor(img), training=False)
    g, counts = recorded(e, lambda: e.input_gradient_eval(torch.as_tensor(dprob)))
    torch.cuda.synchronize()
    g = g.cpu().numpy().astype(np.float64)
    assert g.shape == (n, c, h, w)
    # the route: every wide 3x3 data gradient on the route's Winograd family (the two bottleneck layers of an odd tile on the implicit-GEMM
    # kernel), the first layer's on the direct kernel (not recorded), nothing of the training step's BatchNorm backward
    want = 15 if ((h // 16) % 2 or (w // 16) % 2) else 17
    mine, other = ("_x6", "_fused") if route == "bf16x6" else ("_fused", "_x6")
    assert counts.get("conv3x3_dgrad_winograd" + mine) == want and "conv3x3_dgrad_winograd" + other not in counts, (route, counts)
    assert counts.get("conv3x3_dgrad", 0) == 17 - want, counts
    if route == "native":
        assert not [key for key in counts if key.endswith("_x6")], counts
    assert counts.get("classmap_dgrad") == 1 and "bn_bwd" not in counts, counts
    assert counts.get("convt_dgrad", 0) + counts.get("convt_dgrad_x6", 0) == 4 and counts.get("pool") == 4, counts
    assert e.pl.layer["conv_1a"].dgrad == "direct" and not [key for key in counts if "wgrad" in key], counts

    relu, pidx = _device_decisions(e)
    for name, m in relu.items():
        r64 = cache[name][1]
        assert np.abs(r64[m != (r64 > 0)]).max(initial=0.0) < 1e-4 * np.abs(r64).max(), name
    keep = {}
    g_ref = ref.input_gradient_eval(img, dprob, relu_masks=relu, pool_idx=pidx, keep=keep, cache=cache)
    norm = np.linalg.norm(g_ref)
    err = np.linalg.norm(g - g_ref) / norm
    per_channel = [np.linalg.norm(g[:, ch] - g_ref[:, ch]) / norm for ch in range(c)]
    print("eval input gradient", cfg, route, "rel L2 %.3e" % err, "per channel", ["%.2e" % v for v in per_channel])
    assert norm > 0 and all(np.linalg.norm(g_ref[:, ch]) > 1e-2 * norm for ch in range(c))
    assert err < 1e-4, (err, _layer_report(e, keep))
    assert max(per_channel) < 1e-4, (per_channel, _layer_report(e, keep))


_RADIUS_CASE = []


def _radius_case():
    """A probe that RESPONDS.  The probe's loss gradient is g_k = -sign(1 - 2 p_k) / K at the centre pixel: with more than two classes
    every p_k is usually below 1/2, all g_k are equal and the softmax backward gives exactly zero -- estimate_radius then returns its
    fallback, the theoretical 96, whatever the backward chain computes (the K = 4 case of test_input_gradient_and_estimate_radius_match_oracle
    compares two fallbacks).  Two classes always respond; gamma scaled by 0.8 lets the response die out inside the probe, 45 pixels from the
    centre in fp64, so the answer (48) is neither the fallback nor the probe's edge.  (UNet.estimate_radius once seeded the chain with the
    derivative of |1 - 2 p_k|, twice the reference's: every gradient doubled, the extent five to six pixels wider on each side, 64 reported here.)"""
    if not _RADIUS_CASE:
        c, k = 1, 2
        _, _, prm, _ = make_case(31, 1, c, k, 32)
        for key in prm:
            if key.endswith("gamma"):
                prm[key] = (prm[key] * 0.8).astype(np.float32)
        probe = np.random.default_rng(7).normal(size=(1, c, 192, 192)).astype(np.float32)
        ref = ot.TorchUNet(k, 1, c, params=prm, dtype=torch.float64)
        r_ref = ref.estimate_radius(probe)
        assert ref.erf_extent is not None and 0 < ref.erf_extent[0] < ref.erf_extent[1] < 191 and r_ref < on.RADIUS, (r_ref, ref.erf_extent)
        _RADIUS_CASE.append((c, k, prm, probe, r_ref))
    return _RADIUS_CASE[0]


@pytest.mark.parametrize("route", ROUTES)
def test_estimate_radius_matches_oracle_on_a_probe_that_responds(route, capsys):
    # |grad| > 1e-8 on the 192 x 192 probe, extent / 2 rounded up to a multiple of 16
    c, k, prm, probe, r_ref = _radius_case()
    net = make_net(route, k, 1, c)
    net.engine.load_parameters(prm)
    r_hip, counts = recorded(net.engine, lambda: net.estimate_radius(probe))
    mine, other = ("_x6", "_fused") if route == "bf16x6" else ("_fused", "_x6")
    assert counts.get("conv3x3_dgrad_winograd" + mine) == 17 and "conv3x3_dgrad_winograd" + other not in counts, (route, counts)
    if route == "native":
        assert not [key for key in counts if key.endswith("_x6")], counts
    assert "computed radius" in capsys.readouterr().out                 # not the fallback
    assert r_hip % 16 == 0 and r_hip == r_ref, (r_hip, r_ref)


def test_input_gradient_bf16_mode_is_the_oracles_linear_map_at_bf16_grade():
    # compute_dtype="bf16": the forward values are a bf16 evaluation's, far from the oracle's own, so the device's masks, pool winners AND
    # softmax are imposed -- what is compared is the linear backward map alone.  Its data gradients round dz and the kernel to bf16; the
    # oracle evaluated a second time with exactly that rounding (bf16_dgrad) is e_model away from the unrounded one, and the device must
    # stay within 3 e_model of the unrounded one (the factor: fp32 accumulation order, and activations the model does not round).
    # Measured on an MI355X: e_model = 4.9e-3, device error = 4.3e-3 (both are printed).
    n, c, k, hw = 1, 3, 4, 64
    img, prm, dprob, ref, cache = _case((n, c, k, hw))
    net = pkg("model").UNet(k, n, c, compute_dtype="bf16")
    e = net.engine
    e.load_parameters(prm)
    prob = e.forward(torch.as_tensor(img), training=False).cpu().numpy().astype(np.float64)
    g, counts = recorded(e, lambda: e.input_gradient_eval(torch.as_tensor(dprob)))
    torch.cuda.synchronize()
    g = g.cpu().numpy().astype(np.float64)
    assert counts.get("conv3x3_dgrad_bf16") == 17 and counts.get("convt_dgrad_bf16") == 4 and "bn_bwd" not in counts, counts
    relu, pidx = _device_decisions(e)
    g_ref = ref.input_gradient_eval(img, dprob, relu_masks=relu, pool_idx=pidx, prob=prob, cache=cache)
    g_model = ref.input_gradient_eval(img, dprob, relu_masks=relu, pool_idx=pidx, prob=prob, cache=cache, bf16_dgrad=True)
    norm = np.linalg.norm(g_ref)
    e_model = np.linalg.norm(g_model - g_ref) / norm
    err = np.linalg.norm(g - g_ref) / norm
    print("bf16 eval input gradient: e_model %.3e, device error %.3e" % (e_model, err))
    assert 2.0 ** -12 < e_model < 2.0 ** -5, e_model            # a few bf16 roundings' worth: the model is neither switched off nor something else
    assert err < 3 * e_model, (err, e_model)
