"""The region term (soft Dice / Tversky per image) without a GPU: the fp64 numpy restatement the kernel tests compare against
(region_loss_cases.py) is checked against torch autograd in fp64; the device's operation order, emulated in fp32 numpy, is shown to land
inside the tolerances the kernel tests hold the device to; and the `train` command line / constructor validation is exercised."""
import numpy as np
import pytest
import torch

from conftest import pkg
import region_loss_cases as rl
import weighted_loss_cases as wl

# the kernel tests' tolerances (test_gpu_region_loss.py): total dlogits relative to the largest reference magnitude; region loss and each mean T
TOL_DLOGITS, TOL_LOSS = 5e-6, 2e-6


def _torch_region(z, lab, N, HW, alpha, beta, smooth, scale, cw, ignore):
    """the definition written with torch ops in fp64 -> (loss, d loss / d logits, mean T per class)"""
    K = z.shape[1]
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    labt = torch.tensor(lab)
    p = torch.softmax(zt, -1).reshape(N, HW, K)
    y = torch.nn.functional.one_hot(labt.argmax(-1), K).double().reshape(N, HW, K)
    m = (labt.max(-1).values > 0).double().reshape(N, HW, 1) if ignore else torch.ones(N, HW, 1, dtype=torch.float64)
    I, S, Y = (m * p * y).sum(1), (m * p).sum(1), (m * y).sum(1)
    T = (I + smooth) / ((1 - alpha - beta) * I + alpha * S + beta * Y + smooth)
    c = torch.ones(K, dtype=torch.float64) if cw is None else torch.tensor(cw, dtype=torch.float64)
    loss = scale * ((c / c.sum()) * (1 - T)).sum()
    loss.backward()
    return float(loss.detach()), zt.grad.numpy(), T.detach().mean(0).numpy()


@pytest.mark.parametrize("use_cw", [False, True], ids=["unit", "class_weights"])
@pytest.mark.parametrize("ignore", [False, True], ids=["all_pixels", "ignore"])
@pytest.mark.parametrize("ab", rl.TVERSKY, ids=lambda t: "a%g_b%g" % t)
@pytest.mark.parametrize("k", [2, 4, 5])
def test_restatement_is_torch_autograd_in_fp64(k, ab, ignore, use_cw):
    N, HW = 3, 257
    z, lab, cw = rl.make_case(N, HW, k, seed=5)
    assert (lab.max(-1) == 0).sum() >= 1 and (cw == 0).sum() == 1
    assert lab[:HW, k - 1].sum() == 0 and lab[HW:, k - 1].sum() > 0                     # a class absent from image 0 only
    assert (wl.weighted_ce(z, lab)["prob"] < 1e-17).any()                               # the extreme pixels
    scale = 0.7 / 4
    ref = rl.region_loss(z, lab, N, HW, ab[0], ab[1], 1.0, scale, cw if use_cw else None, ignore)
    loss_t, grad_t, tbar_t = _torch_region(z, lab, N, HW, ab[0], ab[1], 1.0, scale, cw if use_cw else None, ignore)
    assert abs(ref["loss"] - loss_t) <= 1e-12 * abs(loss_t)
    assert np.abs(ref["dlogits"] - grad_t).max() <= 1e-12 * np.abs(grad_t).max()
    assert np.abs(ref["tbar"] - tbar_t).max() <= 1e-13
    assert np.isfinite(ref["dlogits"]).all() and np.isfinite(ref["T"]).all()
    if ignore:
        assert (ref["dlogits"][lab.max(-1) == 0] == 0).all()
    assert np.array_equal(ref["prob"], wl.weighted_ce(z, lab)["prob"])                  # the softmax of the CE restatement


def test_restatement_edge_cases():
    # a wholly unlabeled image: T = 1, no loss, no gradient; soft Dice is (2 I + 2 s) / (S + Y + 2 s); the term is per image
    N, HW, K = 2, 65, 3
    z, lab, _ = rl.make_case(N, HW, K, seed=2)
    lab = lab.copy()
    lab[:HW] = 0
    r = rl.region_loss(z, lab, N, HW, ignore_empty=True, scale=0.5)
    assert (r["T"][0] == 1.0).all() and (r["dlogits"][:HW] == 0).all() and np.isfinite(r["dlogits"]).all()
    alone = rl.region_loss(z[HW:], lab[HW:], 1, HW, ignore_empty=True, scale=0.5)
    assert abs(alone["loss"] - r["loss"]) < 1e-15 and np.abs(alone["dlogits"] - r["dlogits"][HW:]).max() < 1e-18
    p, y = r["prob"][HW:], (lab[HW:].argmax(-1)[:, None] == np.arange(K)) * (lab[HW:].max(-1) > 0)[:, None]
    m = (lab[HW:].max(-1) > 0)[:, None]
    dice = (2 * (p * y).sum(0) + 2.0) / ((m * p).sum(0) + y.sum(0) + 2.0)
    assert np.abs(dice - r["T"][1]).max() < 1e-14


@pytest.mark.parametrize("ignore", [False, True], ids=["all_pixels", "ignore"])
@pytest.mark.parametrize("ab", rl.TVERSKY, ids=lambda t: "a%g_b%g" % t)
@pytest.mark.parametrize("k", [2, 4, 5, 21])
def test_device_operation_order_fits_the_kernel_tolerances(k, ab, ignore):
    """fp32 probabilities, double sums, fp32 coefficients, the fp32 backward expression added to the CE kernel's fp32 dlogits: inside the
    tolerances of test_gpu_region_loss.py at every size that test uses"""
    worst = [0.0, 0.0, 0.0]
    for N in (1, 3):
        for HW in (1, 63, 64, 65, 257, 70001):
            z, lab, cw = rl.make_case(N, HW, k, seed=11)
            a, b, s, lam = rl.f32(ab[0]), rl.f32(ab[1]), 1.0, 1.0
            ce_scale, scale = 1.0 / (4 * HW), rl.f32(lam / 4)
            ce = wl.weighted_ce(z, lab, None, None, ignore, 0.0, ce_scale, ce_scale)
            ref = rl.region_loss(z, lab, N, HW, a, b, s, scale, cw, ignore)
            dev = rl.region_loss_device_order(z, lab, N, HW, a, b, s, scale, cw, ignore)
            total_ref = ce["dlogits"] + ref["dlogits"]
            total_dev = (ce["dlogits"].astype(np.float32) + dev["dlogits"]).astype(np.float32)
            worst[0] = max(worst[0], np.abs(total_dev - total_ref).max() / np.abs(total_ref).max())
            worst[1] = max(worst[1], abs(float(dev["loss"]) - ref["loss"]) / abs(ref["loss"]))
            worst[2] = max(worst[2], (np.abs(dev["tbar"] - ref["tbar"]) / ref["tbar"]).max())
    print("device-order emulation, K = %d: dlogits %.2e (tolerance %.0e), loss %.2e, mean T %.2e (tolerance %.0e)"
          % (k, worst[0], TOL_DLOGITS, worst[1], worst[2], TOL_LOSS))
    assert worst[0] < TOL_DLOGITS and worst[1] < TOL_LOSS and worst[2] < TOL_LOSS


# ---- constructor arguments and the command line ---------------------------------------------------------------------------------------------
def test_region_settings_are_validated_on_the_host():
    model = pkg("model")
    assert model.check_region(0.0, (0.5, 0.5), 1.0, None, 2) is None                    # weight 0: the term is off
    lam, a, b, s, cw = model.check_region(0.5, (0.3, 0.7), 1e-3, [0, 2], 2)
    assert (lam, a, b, s) == (0.5, 0.3, 0.7, 1e-3) and cw.dtype == np.float32 and cw.tolist() == [0.0, 2.0]
    bad = [dict(dice_weight=-1.0), dict(dice_weight=float("nan")), dict(tversky=(-0.1, 0.5)), dict(tversky=(0.5, -0.1)), dict(tversky=(0.5,)),
           dict(tversky=(0.5, float("inf"))), dict(dice_smooth=0.0), dict(dice_smooth=-1.0), dict(dice_class_weights=[1.0]),
           dict(dice_class_weights=[0.0, 0.0]), dict(dice_class_weights=[1.0, -1.0]), dict(dice_class_weights=[1.0, float("nan")])]
    for kw in bad:
        args = dict(dice_weight=1.0, tversky=(0.5, 0.5), dice_smooth=1.0, dice_class_weights=None)
        args.update(kw)
        with pytest.raises(ValueError):
            model.check_region(args["dice_weight"], args["tversky"], args["dice_smooth"], args["dice_class_weights"], 2)
        with pytest.raises(ValueError):                            # the constructor refuses them before it touches a device
            model.UNet(2, 2, 1, **args)
        if "dice_weight" not in kw:                                # settings are checked even while the term is off
            with pytest.raises(ValueError):
                model.UNet(2, 2, 1, **dict(args, dice_weight=0.0))


class RecordingUNet:
    """what train_model touches of model.UNet; records the keywords it was built with"""
    last_kw = None

    def __init__(self, number_classes, global_batch_size, number_channels, learning_rate, device=None, compute_dtype=None, **kw):
        RecordingUNet.last_kw = kw
        self.parallel = None

    def set_learning_rate(self, lr):
        pass

    def dist_train_step(self, strategy, inputs, **kw):
        inputs[2].update_state(0.5); inputs[3].update_state(1.0, 2.0)
        return pkg("model")._Loss(torch.tensor([0.5]))

    dist_test_step = dist_train_step

    def save_checkpoint(self, path):
        pass


def test_command_line_reaches_the_network(tmp_path, monkeypatch, capsys):
    train, readers = pkg("train"), pkg("readers")
    assert train.region_settings() == {} and train.region_settings(0.0, 0.3, 0.7, 2.0, "1,2", 2) == {}
    assert train.region_settings(0.5, 0.3, 0.7, 2.0, "1,3", 2) == {"dice_weight": 0.5, "tversky": (0.3, 0.7), "dice_smooth": 2.0,
                                                                    "dice_class_weights": [1.0, 3.0]}
    seen = {}
    monkeypatch.setattr(train, "train_model", lambda *a, **kw: seen.update(kw))
    base = ["--output_dir", str(tmp_path / "o"), "--synthetic", "16x16x1", "--number_classes", "3"]
    train.main(base)
    assert seen["region"] is None                                  # nothing set: the network is built as before
    train.main(base + ["--dice_weight", "0.5", "--tversky_alpha", "0.3", "--tversky_beta", "0.7", "--dice_smooth", "0.1",
                       "--dice_class_weights", "0,1,2"])
    assert seen["region"] == {"dice_weight": 0.5, "tversky": (0.3, 0.7), "dice_smooth": 0.1, "dice_class_weights": [0.0, 1.0, 2.0]}
    for args, msg in ((["--dice_weight", "-1"], ">= 0"), (["--dice_weight", "1", "--dice_smooth", "0"], "dice_smooth must be > 0"),
                      (["--dice_weight", "1", "--tversky_beta", "-0.5"], ">= 0"),
                      (["--dice_weight", "1", "--dice_class_weights", "1,2"], "--dice_class_weights has 2 entries but --number_classes is 3"),
                      (["--dice_weight", "1", "--dice_class_weights", "0,0,0"], "must not all be zero")):
        with pytest.raises(SystemExit):
            train.main(base + args)
        assert msg in capsys.readouterr().err
    assert not (tmp_path / "o").exists()
    monkeypatch.undo()
    # train_model hands the settings to the network as keywords, only when the term is on
    run = lambda **kw: train.train_model(str(tmp_path / "t"), 2, 1, None, None, 0, 3, 0, 3e-4, 1, 1,
                                         train_reader=readers.SyntheticReader(8, 16, 16, 1, 3, seed=1),
                                         test_reader=readers.SyntheticReader(4, 16, 16, 1, 3, seed=2),
                                         max_epochs=1, quiet=True, unet_factory=RecordingUNet, **kw)
    run(region={"dice_weight": 0.0})
    assert RecordingUNet.last_kw == {}
    run(region={"dice_weight": 0.5, "tversky": (0.3, 0.7)}, class_metrics=True)
    assert RecordingUNet.last_kw == {"dice_weight": 0.5, "tversky": (0.3, 0.7)}
    with pytest.raises(ValueError, match="dice_smooth"):
        run(region={"dice_weight": 0.5, "dice_smooth": 0.0})
