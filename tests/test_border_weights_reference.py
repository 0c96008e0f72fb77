"""The border-distance weight map without a GPU: the brute-force restatement the kernel tests compare against (border_weight_cases.py) is
checked against an independent separable statement and against hand-written border sets, the library is checked to export the new entry
points, and the `train` command line / train_model plumbing of --border_weight and --border_sigma is exercised with a stand-in network."""
import numpy as np
import pytest
import torch

from conftest import pkg
import border_weight_cases as bw
from fake_segmenter import FakeSegmenter


@pytest.mark.parametrize("name", bw.NAMES)
def test_bruteforce_is_the_separable_transform(name):
    cm, k, m, d2 = bw.case(name)
    assert cm.max() < k and cm.shape == bw.SHAPES[name]
    for c, d in zip(cm, d2):
        assert np.array_equal(d, bw.d2_separable(c))
        assert np.array_equal(d == 0, bw.border_set(c))


def test_the_cases_are_what_their_names_say():
    none = lambda name: (bw.case(name)[3] == bw.NONE).all()
    assert none("one_pixel") and none("two_uniform_images") and none("unlabeled_band_between_classes")
    assert (bw.case("checkerboard")[3] == 0).all()
    d2 = bw.case("border_at_the_left_edge")[3]
    assert d2[0, :, -1].tolist() == [1098 ** 2] * 8                       # the row search runs the whole width
    d2 = bw.case("border_at_the_top_edge")[3]
    assert (d2[0, :, 2] == np.maximum(np.arange(130) - 1, 0) ** 2).all()  # purely vertical
    cm, _, _, d2 = bw.case("blobs_k5")
    b = np.stack([bw.border_set(c) for c in cm])
    assert b.any((1, 2)).all() and not b[:, :, 90:].any() and not b[:, 26:, :].any() and (d2 < bw.NONE).all()
    cm, _, _, d2 = bw.case("unlabeled_blob_beside_a_border")
    assert (d2[cm < 0] > 0).all() and (d2[cm < 0] < bw.NONE).all()        # unlabeled pixels: a finite distance, never a border themselves
    assert len(set(bw.case("blobs_k2_with_pixel_weights")[3].ravel().tolist())) > 20


def test_border_set_rules_on_hand_written_masks():
    U = -1
    masks = [
        # a vertical class edge: both sides are in B, the image edge is not
        ([[0, 0, 1, 1, 1]] * 5, [[0, 1, 1, 0, 0]] * 5),
        # one pixel of another class: itself and its four neighbours, not the diagonal ones
        ([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
         [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]),
        # an unlabeled column between two classes: no border at all
        ([[0, 0, U, 1, 1]] * 5, [[0, 0, 0, 0, 0]] * 5),
        # unlabeled pixels next to a real border are never in B and put no neighbour in it
        ([[0, U, 1, 2, 2], [0, U, 1, 2, 2], [0, 0, 1, 2, 2], [U, U, U, U, U], [3, 3, 3, 3, 3]],
         [[0, 0, 1, 1, 0], [0, 0, 1, 1, 0], [0, 1, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]),
        # a corner pixel of another class
        ([[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 2]],
         [[1, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1], [0, 0, 0, 1, 1]]),
    ]
    for cm, want in masks:
        assert bw.border_set(np.array(cm)).astype(int).tolist() == want
    d2 = bw.d2_bruteforce(np.array(masks[1][0]))
    assert d2.tolist() == [[5, 2, 1, 2, 5], [2, 1, 0, 1, 2], [1, 0, 0, 0, 1], [2, 1, 0, 1, 2], [5, 2, 1, 2, 5]]
    assert (bw.d2_bruteforce(np.array(masks[2][0])) == bw.NONE).all()


def test_weights_restatement():
    d2 = np.array([0, 1, 50, bw.NONE])
    w = bw.weights_fp64(d2, 10.0, 5.0, np.array([1.0, 2.0, 0.5, 3.0]))
    c = float(np.float32(-1.0 / 50.0))
    assert w.tolist() == [11.0, 2.0 * (1.0 + 10.0 * np.exp(c)), 0.5 * (1.0 + 10.0 * np.exp(50 * c)), 3.0]
    assert bw.onehot(np.array([[[0, -1, 2]]]), 3).tolist() == [[[[1, 0, 0], [0, 0, 0], [0, 0, 1]]]]


def test_library_exports_the_entry_points():
    import ctypes
    so = pkg("_build").build_library()
    protos = pkg("_lib").parse_header()
    assert protos["unet_border_weights_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    res, args = protos["unet_border_weights"]
    assert res is ctypes.c_int and len(args) == 13 and args[3] is ctypes.c_float and args[4] is ctypes.c_float and args[11] is ctypes.c_size_t
    exported = open(so, "rb").read()
    assert b"unet_border_weights_workspace\0" in exported and b"unet_border_weights\0" in exported
    assert "border_weights.hip" in pkg("_build").SOURCES
    assert pkg("_lib").header_abi_version() == 10                 # added without a bump: no existing signature changed


# ---- command line and train_model ------------------------------------------------------------------------------------------------------
class RecordingNet(FakeSegmenter):
    """the stand-in segmenter with what train_model touches of model.UNet on top; records the keywords it was built with"""
    last_kw = None

    def __init__(self, number_classes, global_batch_size, number_channels, learning_rate, device=None, compute_dtype=None, **kw):
        super().__init__(radius=96)
        RecordingNet.last_kw = kw
        self.parallel = None

    def set_learning_rate(self, lr):
        pass

    def dist_train_step(self, strategy, inputs):
        inputs[2].update_state(0.5); inputs[3].update_state(1.0, 2.0)
        return pkg("model")._Loss(torch.tensor([0.5]))

    dist_test_step = dist_train_step

    def save_checkpoint(self, path):
        pass


def _main(tmp_path, monkeypatch, *flags):
    train = pkg("train")
    real = train.train_model
    monkeypatch.setattr(train, "train_model", lambda *a, **kw: real(*a, **dict(kw, unet_factory=RecordingNet, quiet=True)))
    RecordingNet.last_kw = None
    train.main(["--output_dir", str(tmp_path), "--synthetic", "16x16x1x8", "--batch_size", "2", "--test_every_n_steps", "1", "--max_epochs", "1",
                "--number_classes", "3", "--use_augmentation", "0", *flags])      # (the device augmentation needs the GPU: test_gpu_border_weights.py)
    return RecordingNet.last_kw


def test_flags_reach_the_network_factory_only_when_set(tmp_path, monkeypatch):
    assert _main(tmp_path, monkeypatch) == {}                                                  # unset: the network is built as before
    assert _main(tmp_path, monkeypatch, "--border_sigma", "3") == {}                           # a sigma alone switches nothing on
    assert _main(tmp_path, monkeypatch, "--border_weight", "10") == {"border_weight": 10.0, "border_sigma": 5.0}
    kw = _main(tmp_path, monkeypatch, "--border_weight", "2.5", "--border_sigma", "3", "--ignore_label", "2",
               "--class_weights", "1,2,3", "--dice_weight", "0.5")
    assert kw["border_weight"] == 2.5 and kw["border_sigma"] == 3.0 and kw["ignore_unlabeled"] is True
    assert kw["class_weights"] == [1.0, 2.0, 3.0] and kw["dice_weight"] == 0.5


def test_the_flags_are_accepted_with_the_augmentation_on(tmp_path, monkeypatch):
    train, seen = pkg("train"), {}
    monkeypatch.setattr(train, "train_model", lambda *a, **kw: seen.update(kw, use_augmentation=a[5]))
    train.main(["--output_dir", str(tmp_path), "--synthetic", "16x16x1", "--border_weight", "10", "--border_sigma", "4"])     # --use_augmentation defaults to 1
    assert seen["use_augmentation"] == 1 and seen["border"] == {"border_weight": 10.0, "border_sigma": 4.0}
    train.main(["--output_dir", str(tmp_path), "--synthetic", "16x16x1"])
    assert seen["border"] is None


@pytest.mark.parametrize("flags, message", [
    (("--border_sigma", "0"), "--border_sigma must be finite and > 0"),
    (("--border_weight", "10", "--border_sigma", "-2"), "--border_sigma must be finite and > 0"),
    (("--border_weight", "-1"), "--border_weight must be finite and >= 0"),
    (("--border_weight", "nan"), "--border_weight must be finite and >= 0"),
    (("--border_weight", "inf"), "--border_weight must be finite and >= 0"),
])
def test_bad_settings_are_parser_errors(tmp_path, capsys, flags, message):
    with pytest.raises(SystemExit):
        pkg("train").main(["--output_dir", str(tmp_path / "a"), "--synthetic", "16x16x1", *flags])
    assert message in capsys.readouterr().err
    assert not (tmp_path / "a").exists()


def test_settings_are_validated_before_the_device():
    model = pkg("model")
    assert model.check_border(0, 5) is None and model.check_border(10, 5) == (10.0, 5.0)
    for bad in ((-1, 5), (float("nan"), 5), (1, 0), (1, float("inf")), ("x", 5)):
        with pytest.raises(ValueError):
            model.check_border(*bad)
    with pytest.raises(ValueError, match="border_sigma"):       # refused before the engine (which needs a GPU) is built
        model.UNet(2, 2, 1, border_weight=1.0, border_sigma=0.0)
