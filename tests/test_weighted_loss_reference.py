"""The weighted loss without a GPU: the fp64 numpy restatement the kernel tests compare against (weighted_loss_cases.py) is itself checked
against torch autograd in fp64, and the `train` command line / train_model plumbing of --class_weights and --ignore_label is exercised with
a stand-in network."""
import numpy as np
import pytest
import torch

from conftest import pkg
import weighted_loss_cases as wl


def _torch_loss(z, lab, cw, pw, ls, scale, clip):
    """Keras sample_weight semantics in torch fp64: per-pixel cross-entropy x class weight of the truth x pixel weight, unlabeled rows masked,
    summed, times scale -> (loss, d loss / d logits)."""
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    labt = torch.tensor(lab)
    t = labt.argmax(-1)
    cwt, pwt = torch.tensor(cw, dtype=torch.float64), torch.tensor(pw, dtype=torch.float64)
    labeled = labt.max(-1).values > 0
    if clip:
        y = labt.double()
        if ls:
            y = y * (1.0 - ls) + ls / z.shape[1]
        per = -(y * torch.log(torch.clamp(torch.softmax(zt, -1), clip, 1.0 - clip))).sum(-1) * cwt[t] * pwt     # clamp: no gradient outside
    elif ls:
        # (torch's own weight= weights the smoothing term class by class; a sample weight multiplies the whole pixel, so it goes outside)
        per = torch.nn.functional.cross_entropy(zt, t, reduction="none", label_smoothing=ls) * cwt[t] * pwt
    else:
        per = torch.nn.functional.cross_entropy(zt, t, weight=cwt, reduction="none") * pwt
    loss = (per * labeled).sum() * scale
    loss.backward()
    return float(loss.detach()), zt.grad.numpy()


@pytest.mark.parametrize("clip", [0.0, 1e-7])
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("k", [2, 5])
def test_restatement_is_torch_autograd_in_fp64(k, ls, clip):
    P = 257
    z, lab, cw, pw = wl.make_case(P, k, seed=5)
    assert (lab.max(-1) == 0).sum() >= 1 and (cw == 0).sum() == 1 and (pw == 0).sum() >= 1
    pr = wl.weighted_ce(z, lab)["prob"]
    assert ((pr < 1e-17).any(-1)).sum() >= 1                                            # the extreme pixels
    assert not ((np.abs(pr - 1e-7) < 5e-8) | (np.abs(1 - pr - 1e-7) < 5e-8)).any()      # and nothing near a clip edge
    scale = 1.0 / (3 * P)
    ref = wl.weighted_ce(z, lab, cw, pw, True, ls, scale, scale, clip)
    loss_t, grad_t = _torch_loss(z, lab, cw, pw, ls, scale, clip)
    assert abs(ref["loss"] - loss_t) <= 1e-12 * abs(loss_t)
    assert np.abs(ref["dlogits"] - grad_t).max() <= 1e-12 * np.abs(grad_t).max()
    labeled = lab.max(-1) > 0
    assert ref["valid"] == labeled.sum() and (ref["dlogits"][~labeled] == 0).all()
    assert ref["correct"] == (labeled & (lab.argmax(-1) == z.argmax(-1))).sum()
    assert abs(ref["weight_sum"] - (cw.astype(np.float64)[lab.argmax(-1)] * pw.astype(np.float64))[labeled].sum()) < 1e-12 * P


def test_restatement_without_options_is_the_oracle_loss():
    from oracle import unet_numpy as on
    n, h, w, k, G = 2, 4, 8, 3, 4
    z, lab, _, _ = wl.make_case(n * h * w, k, seed=6)
    lab[lab.max(-1) == 0, 0] = 1                                   # the oracle has no unlabeled pixels
    for ls, clip in ((0.0, 0.0), (0.1, 0.0), (0.0, 1e-7)):
        c = on.Contract(ce_from_softmax_logits=(clip == 0.0), ce_clip_eps=clip if clip else 1e-7)
        z4 = z.astype(np.float64).reshape(n, h, w, k)
        loss, p, y = on.ce_loss_fwd(z4, lab.reshape(n, h, w, k), G, ls, c)
        dl = on.ce_loss_bwd(p, y, G, c)
        s = 1.0 / (G * h * w)
        ref = wl.weighted_ce(z, lab, None, None, False, ls, s, s, clip)
        assert abs(ref["loss"] - loss) < 1e-13 * abs(loss) and np.abs(ref["dlogits"] - dl.reshape(-1, k)).max() < 1e-15


# ---- command line and train_model ------------------------------------------------------------------------------------------------------
class RecordingUNet:
    """what train_model touches of model.UNet; records the keywords it was built with"""
    last_kw = None
    built = 0

    def __init__(self, number_classes, global_batch_size, number_channels, learning_rate, device=None, compute_dtype=None, **kw):
        RecordingUNet.last_kw = kw
        RecordingUNet.built += 1
        self.parallel = None
        self.label_rows = []

    def set_learning_rate(self, lr):
        pass

    def dist_train_step(self, strategy, inputs):
        images, labels, lm, am = inputs
        RecordingUNet.labels = labels.clone()
        lm.update_state(0.5); am.update_state(1.0, 2.0)
        return pkg("model")._Loss(torch.tensor([0.5]))

    def dist_test_step(self, strategy, inputs):
        inputs[2].update_state(0.5); inputs[3].update_state(1.0, 2.0)
        return pkg("model")._Loss(torch.tensor([0.5]))

    def save_checkpoint(self, path):
        pass


def _train(tmp_path, use_augmentation=0, **kw):
    readers = pkg("readers")
    tr, te = readers.SyntheticReader(8, 16, 16, 1, 3, seed=1), readers.SyntheticReader(4, 16, 16, 1, 3, seed=2)
    return pkg("train").train_model(str(tmp_path), 2, 1, None, None, use_augmentation, 3, 0, 3e-4, 1, 1, train_reader=tr, test_reader=te,
                                    max_epochs=1, quiet=True, unet_factory=RecordingUNet, **kw)


def test_train_model_hands_the_options_to_the_network_and_the_feeds(tmp_path):
    _train(tmp_path)
    assert RecordingUNet.last_kw == {}                             # nothing set: the network is built as before
    assert (RecordingUNet.labels.sum(-1) == 1).all()
    _train(tmp_path, class_weights=[0.5, 1, 2], ignore_label=2)
    assert RecordingUNet.last_kw == {"class_weights": [0.5, 1.0, 2.0], "ignore_unlabeled": True}
    lab = RecordingUNet.labels                                     # the feed turned class 2 into all-zero rows
    assert lab.dtype == torch.int32 and lab.shape[-1] == 3 and (lab[..., 2] == 0).all() and (lab.sum(-1) == 0).any() and (lab.sum(-1) == 1).any()


def test_class_weights_of_the_wrong_length_are_rejected(tmp_path, capsys):
    train = pkg("train")
    built = RecordingUNet.built
    with pytest.raises(ValueError, match="class_weights"):
        _train(tmp_path / "a", class_weights=[1.0, 2.0])
    for bad in ([1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError, match="finite and >= 0"):
            _train(tmp_path / "a", class_weights=bad)
    assert RecordingUNet.built == built and not (tmp_path / "a").exists()       # refused before anything is opened
    with pytest.raises(SystemExit):
        train.main(["--output_dir", str(tmp_path / "b"), "--synthetic", "16x16x1", "--number_classes", "3", "--class_weights", "1,2"])
    assert "--class_weights has 2 entries but --number_classes is 3" in capsys.readouterr().err
    assert not (tmp_path / "b").exists()
    assert train.parse_class_weights("0.5,1,2", 3) == [0.5, 1.0, 2.0]
    with pytest.raises(ValueError):
        train.parse_class_weights("1,x,2", 3)


def test_ignore_label_with_augmentation_is_refused(tmp_path, capsys):
    train = pkg("train")
    with pytest.raises(ValueError, match="bilinear"):
        _train(tmp_path / "a", use_augmentation=1, ignore_label=2)
    assert not (tmp_path / "a").exists()
    with pytest.raises(SystemExit):
        train.main(["--output_dir", str(tmp_path / "b"), "--synthetic", "16x16x1", "--ignore_label", "255"])      # --use_augmentation defaults to 1
    assert "--ignore_label cannot be combined with --use_augmentation 1" in capsys.readouterr().err
    assert not (tmp_path / "b").exists()


def test_host_feed_marks_the_ignore_label_unlabeled():
    feed = pkg("feed")
    cls = torch.tensor([[[0, 1, 255, 2]]], dtype=torch.uint8)
    f = feed.DeviceFeed(iter([(torch.zeros(1, 1, 1, 4), cls)]), "cpu", classmap=True, number_classes=3, ignore_label=255)
    _, lab = next(f)
    f.close()
    assert lab.tolist() == [[[[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]]]]
    f = feed.DeviceFeed(iter([(torch.zeros(1, 1, 1, 4), cls)]), "cpu", classmap=True, number_classes=3)
    with pytest.raises(IndexError):
        next(f)
    f.close()
    with pytest.raises(ValueError):
        feed.DeviceFeed(iter([]), "cpu", ignore_label=3)


def test_weights_are_validated_on_the_host():
    model = pkg("model")
    assert model.check_weights([0, 1.5], "w", (2,)).dtype == np.float32
    for bad in ([1, -0.5], [np.nan, 1], [np.inf, 1]):
        with pytest.raises(ValueError):
            model.check_weights(bad, "w")
    with pytest.raises(ValueError):
        model.check_weights([1, 2, 3], "w", (2,))
