"""CPU checks of the per-class metrics (metrics.py) and of the loops that use them: the arithmetic of `summary()` against values worked by
hand and against Python fractions, int64 counts beyond 2^32, the cross-replica read over two gloo ranks, `train_model(class_metrics=True)`
with a scripted stand-in network, and the inference CLI's --mask_folder check.  Counts are compared for exact equality; the quotients are
single float64 divisions of exactly representable integers, compared for equality with the correctly rounded fraction."""
import math
import os
import socket
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import pkg

NAN = float("nan")


def _same(got, want):
    """equality with NaN == NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


#   truth \ pred   0  1  2      class 1 is predicted (2 pixels) but never true, class 2 never occurs at all
HAND = np.array([[6, 2, 0],
                 [0, 0, 0],
                 [0, 0, 0]], np.int64)


def test_summary_matches_values_worked_by_hand():
    m = pkg("metrics")
    cm = m.ConfusionMatrix(3, device="cpu")
    cm.add_counts(HAND)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = cm.summary()
    assert s["pixel_accuracy"] == 6 / 8
    assert _same(s["recall"], [6 / 8, NAN, NAN])                 # class 1: no true pixel -> recall NaN
    assert _same(s["precision"], [6 / 6, 0 / 2, NAN])            #          predicted twice, never right -> precision 0
    assert _same(s["iou"], [6 / 8, 0 / 2, NAN])                  #          union = 2 -> IoU 0; class 2: union 0 -> NaN
    assert _same(s["dice"], [12 / 14, 0 / 2, NAN])
    assert s["mean_iou"] == (6 / 8 + 0.0) / 2                    # class 2 is excluded from the mean
    assert s["frequency_weighted_iou"] == (8 * (6 / 8) + 0 * 0.0) / 8
    assert all(np.asarray(s[k]).dtype == np.float64 for k in ("recall", "precision", "iou", "dice"))
    # a full 3-class case: every class present on both sides
    c = np.array([[5, 1, 0], [2, 3, 1], [0, 0, 4]], np.int64)
    s = m.summarize(c)
    assert s["pixel_accuracy"] == 12 / 16
    assert _same(s["recall"], [5 / 6, 3 / 6, 4 / 4]) and _same(s["precision"], [5 / 7, 3 / 4, 4 / 5])
    assert _same(s["iou"], [5 / 8, 3 / 7, 4 / 5]) and _same(s["dice"], [10 / 13, 6 / 10, 8 / 9])
    assert s["mean_iou"] == np.mean(np.array([5 / 8, 3 / 7, 4 / 5]))
    assert s["frequency_weighted_iou"] == (6 * (5 / 8) + 6 * (3 / 7) + 4 * (4 / 5)) / 16


def test_empty_matrix_is_nan_without_warnings():
    m = pkg("metrics")
    cm = m.ConfusionMatrix(4, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = cm.summary()
    assert math.isnan(s["pixel_accuracy"]) and math.isnan(s["mean_iou"]) and math.isnan(s["frequency_weighted_iou"])
    for k in ("recall", "precision", "iou", "dice"):
        assert s[k].shape == (4,) and np.isnan(s[k]).all()
    assert cm.result().dtype == np.int64 and not cm.result().any()


def test_add_counts_and_reset_states():
    m = pkg("metrics")
    cm = m.ConfusionMatrix(3, device="cpu", name="x")
    assert cm.name == "x" and cm.number_classes == 3 and cm.matrix.dtype == torch.int64 and tuple(cm.matrix.shape) == (3, 3)
    cm.add_counts(HAND)
    cm.add_counts(torch.from_numpy(HAND.astype(np.int32)))          # a tensor of another integer dtype
    cm.add_counts(HAND.astype(np.uint8).tolist())                   # a nested list
    got = cm.result()
    assert got.dtype == np.int64 and np.array_equal(got, 3 * HAND)
    got[0, 0] = -1                                                   # the result is a copy
    assert np.array_equal(cm.result(), 3 * HAND)
    with pytest.raises(ValueError):
        cm.add_counts(np.zeros((2, 2), np.int64))
    with pytest.raises(TypeError):
        cm.add_counts(np.zeros((3, 3), np.float32))
    cm.reset_states()
    assert not cm.result().any() and int(cm.out_of_range) == 0
    with pytest.raises(ValueError):
        m.ConfusionMatrix(0, device="cpu")
    with pytest.raises(ValueError):
        m.ConfusionMatrix(1025, device="cpu")


def test_counts_above_two_to_the_32_stay_exact():
    m = pkg("metrics")
    big = 2 ** 32 - 1
    c = np.array([[big, 7], [big, big]], np.int64)
    cm = m.ConfusionMatrix(2, device="cpu")
    cm.add_counts(c)
    cm.add_counts(c)
    got = cm.result()
    assert got.dtype == np.int64 and got.tolist() == [[2 * big, 14], [2 * big, 2 * big]] and 2 * big > 2 ** 32
    s = cm.summary()
    C = [[2 * big, 14], [2 * big, 2 * big]]
    tp = [C[0][0], C[1][1]]
    truth = [sum(C[0]), sum(C[1])]
    pred = [C[0][0] + C[1][0], C[0][1] + C[1][1]]
    total = sum(truth)
    rn = lambda a, b: float(Fraction(a, b))                          # the correctly rounded quotient
    assert s["pixel_accuracy"] == rn(sum(tp), total)
    for k in range(2):
        assert s["recall"][k] == rn(tp[k], truth[k]) and s["precision"][k] == rn(tp[k], pred[k])
        assert s["iou"][k] == rn(tp[k], truth[k] + pred[k] - tp[k]) and s["dice"][k] == rn(2 * tp[k], truth[k] + pred[k])


def test_a_host_matrix_refuses_the_kernel_paths():
    cm = pkg("metrics").ConfusionMatrix(2, device="cpu")
    m = torch.zeros((4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        cm.update_from_masks(m, m)
    with pytest.raises(RuntimeError, match="GPU only"):
        cm.update_from_scores(torch.zeros((4, 2)), torch.zeros((4, 2), dtype=torch.int32))


# ---- cross-replica read ------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


class _Reducer:
    """the two members of parallel.DataParallel that ConfusionMatrix.result touches"""

    def __init__(self, world):
        self.world_size, self.calls = world, 0

    def reduce_sum(self, t):
        self.calls += 1
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t


def _rank_matrix(rank):
    return np.array([[1 + rank, 2 ** 33 * rank, 0], [3, 5 * rank, 1], [0, 0, 2 ** 32 - 1]], np.int64)


def _reduce_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cm = pkg("metrics").ConfusionMatrix(3, device="cpu")
        cm.add_counts(_rank_matrix(rank))
        red = _Reducer(world)
        got = cm.result(reduce=red)
        assert red.calls == 1                                              # one all-reduce per read
        assert np.array_equal(cm.result(), _rank_matrix(rank))              # ... of a clone: the accumulator keeps this rank's counts
        out.put((rank, got.tolist()))
    except Exception:
        import traceback
        out.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_result_is_summed_over_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, out)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(out.get(timeout=120) for _ in procs)
    [p.join(30) for p in procs]
    want = (_rank_matrix(0) + _rank_matrix(1)).tolist()
    assert res == {0: want, 1: want}, res


def test_single_replica_read_does_not_reduce():
    class One:
        world_size = 1

        def reduce_sum(self, t):
            raise AssertionError("no collective with one replica")
    cm = pkg("metrics").ConfusionMatrix(3, device="cpu")
    cm.add_counts(HAND)
    assert np.array_equal(cm.result(reduce=One()), HAND)


# ---- train loop ----------------------------------------------------------------------------------------------------------------------
EPOCH_MATRIX = [np.array([[6, 2], [1, 3]], np.int64), np.array([[0, 0], [4, 4]], np.int64), np.array([[0, 0], [0, 5]], np.int64)]


class _ScriptedNet:
    """what train_model touches of model.UNet (the stand-in of tests/test_train_loop.py), with a test step that feeds a known matrix:
    the FIRST test step of epoch e adds EPOCH_MATRIX[e], every later one nothing"""
    last = None
    with_keyword = True

    def __init__(self, number_classes, global_batch_size, number_channels, learning_rate, device=None, compute_dtype=None):
        type(self).last = self
        self.epoch, self._test_n, self.parallel, self.seen_confusion = 0, 0, None, []

    def set_learning_rate(self, lr):
        if self._test_n:
            self.epoch += 1
            self._test_n = 0

    def dist_train_step(self, strategy, inputs):
        inputs[2].update_state(0.5); inputs[3].update_state(1.0, 2.0)
        return pkg("model")._Loss(torch.tensor([0.5]))

    def _test(self, inputs, confusion):
        if confusion is not None and self._test_n == 0:
            confusion.add_counts(EPOCH_MATRIX[self.epoch])
        self.seen_confusion.append(confusion)
        self._test_n += 1
        loss = [0.9, 0.5, 0.7][self.epoch]
        inputs[2].update_state(loss); inputs[3].update_state(1.0, 2.0)
        return pkg("model")._Loss(torch.tensor([loss], dtype=torch.float64))

    def dist_test_step(self, strategy, inputs, confusion=None):
        return self._test(inputs, confusion)

    def save_checkpoint(self, path):
        pass


class _NetWithoutKeyword(_ScriptedNet):
    def dist_test_step(self, strategy, inputs):                              # TypeError if the loop passed confusion=
        return self._test(inputs, None)


def _train(out_dir, factory, **kw):
    readers = pkg("readers")
    tr, te = readers.SyntheticReader(16, 16, 16, 1, 2, seed=1), readers.SyntheticReader(4, 16, 16, 1, 2, seed=2)
    return pkg("train").train_model(str(out_dir), 2, 1, "a", "b", 0, 2, 0, 3e-4, 2, 10, train_reader=tr, test_reader=te, quiet=True,
                                    max_epochs=3, unet_factory=factory, **kw)


def test_train_loop_writes_class_metrics(tmp_path, capsys):
    m = pkg("metrics")
    losses = _train(tmp_path, _ScriptedNet, class_metrics=True)
    assert len(losses) == 3
    net = _ScriptedNet.last
    assert len(net.seen_confusion) == 9 and all(isinstance(c, m.ConfusionMatrix) for c in net.seen_confusion)      # 4 / 2 + 1 test steps x 3
    assert len({id(c) for c in net.seen_confusion}) == 1                     # one accumulator, reset per epoch
    want = ["epoch,pixel_accuracy,mean_iou,iou_0,iou_1,dice_0,dice_1"]
    for e, c in enumerate(EPOCH_MATRIX):
        s = m.summarize(c)
        want.append(",".join([str(e)] + [repr(float(v)) for v in [s["pixel_accuracy"], s["mean_iou"], *s["iou"], *s["dice"]]]))
    text = open(tmp_path / "test_class_metrics.csv").read()
    assert text == "\n".join(want) + "\n"
    # worked by hand: epoch 0 -> accuracy 9/12, IoU 6/9 and 3/6; epoch 1: class 0 is predicted but never true -> IoU 0; epoch 2: class 0
    # occurs on neither side -> NaN, left out of the mean
    rows = text.splitlines()
    assert rows[1] == "0,0.75,%r,%r,0.5,%r,%r" % ((6 / 9 + 0.5) / 2, 6 / 9, 12 / 15, 6 / 9)
    assert rows[2] == "1,0.5,0.25,0.0,0.5,0.0,%r" % (8 / 12)
    assert rows[3] == "2,1.0,1.0,nan,1.0,nan,1.0"
    # the scalars went through the existing writer, after the reference's two
    import json
    tb = [d for d in os.listdir(tmp_path) if d.startswith("tensorboard-")][0]
    recs = [json.loads(l) for l in open(tmp_path / tb / "test" / "scalars.jsonl")]
    assert [r["tag"] for r in recs[:5]] == ["loss", "accuracy", "mean_iou", "iou_class_0", "iou_class_1"]
    assert recs[2]["value"] == (6 / 9 + 0.5) / 2 and recs[2]["step"] == recs[0]["step"]
    # early stopping / checkpointing stay on the loss: test_loss.csv is what it is without the flag
    assert open(tmp_path / "test_loss.csv").read().split() == [str(v) for v in losses] and len(losses) == 3


def test_train_loop_prints_the_iou_line_after_the_reference_line(tmp_path, capsys):
    readers = pkg("readers")
    tr, te = readers.SyntheticReader(16, 16, 16, 1, 2, seed=1), readers.SyntheticReader(4, 16, 16, 1, 2, seed=2)
    pkg("train").train_model(str(tmp_path), 2, 1, "a", "b", 0, 2, 0, 3e-4, 2, 10, train_reader=tr, test_reader=te, max_epochs=1,
                             unet_factory=_ScriptedNet, class_metrics=True)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test Epoch")]
    assert len(lines) == 2 and lines[0].startswith("Test Epoch: 0: Loss = ") and " Accuracy = " in lines[0]
    assert lines[1] == "Test Epoch: 0: mean IoU = {} IoU per class = {}".format((6 / 9 + 0.5) / 2, [6 / 9, 0.5])


def test_train_loop_without_the_flag_is_unchanged(tmp_path):
    _train(tmp_path, _NetWithoutKeyword)                                      # the stand-in never sees the keyword
    assert _NetWithoutKeyword.last.seen_confusion == [None] * 9
    assert not os.path.exists(tmp_path / "test_class_metrics.csv")
    import json
    tb = [d for d in os.listdir(tmp_path) if d.startswith("tensorboard-")][0]
    assert {json.loads(l)["tag"] for l in open(tmp_path / tb / "test" / "scalars.jsonl")} == {"loss", "accuracy"}
    import inspect
    sig = inspect.signature(pkg("train").train_model)
    assert sig.parameters["class_metrics"].default is False


# ---- inference CLI -------------------------------------------------------------------------------------------------------------------
def test_inference_cli_names_a_missing_mask_before_touching_the_gpu(tmp_path):
    inf = pkg("inference")
    imgs, masks = tmp_path / "imgs", tmp_path / "masks"
    imgs.mkdir(); masks.mkdir()
    for n in ("a.npy", "b.npy"):
        np.save(imgs / n, np.zeros((20, 20), np.uint8))
    np.save(masks / "a.npy", np.zeros((20, 20), np.uint8))
    argv = ["--checkpoint_filepath", str(tmp_path / "ckpt"), "--image_folder", str(imgs), "--output_folder", str(tmp_path / "out"),
            "--number_classes", "2", "--number_channels", "1", "--image_format", "npy", "--mask_folder", str(masks), "--ignore_label", "255"]
    with pytest.raises(FileNotFoundError, match="b.npy"):
        inf.main(argv)
    assert not os.path.exists(tmp_path / "out" / "scores.csv")


def test_scoring_checks_shape_and_pairing():
    inf, m = pkg("inference"), pkg("metrics")
    cm = m.ConfusionMatrix(2, device="cpu")
    with pytest.raises(ValueError):
        inf._check_truth(np.zeros((4, 5), np.uint8), cm, 5, 4)               # shape mismatch
    with pytest.raises(ValueError):
        inf._check_truth(np.zeros((4, 5), np.uint8), None, 4, 5)             # truth without a matrix
    with pytest.raises(ValueError):
        inf._check_truth(None, cm, 4, 5)
    assert inf._check_truth(np.zeros((4, 5), np.int64), cm, 4, 5).dtype == np.int32
    assert inf._check_truth(np.zeros((4, 5), np.uint16), cm, 4, 5).dtype == np.uint16
    # the host count: rows = truth, ignore label skipped, out-of-range labels counted apart
    mask = np.array([[0, 1, 1], [1, 0, 1]], np.int32)
    truth = np.array([[0, 1, 0], [7, 9, -1]], np.int32)
    inf._host_confusion(mask, truth, cm, ignore_label=7)
    assert cm.result().tolist() == [[1, 1], [0, 1]] and int(cm.out_of_range) == 2
