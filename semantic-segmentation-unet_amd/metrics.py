"""Per-class segmentation metrics from a K x K confusion matrix kept on the device.

The reference reports pixel accuracy only (tf.keras.metrics.CategoricalAccuracy, UNet/train.py:106,108); on masks with a few percent of
foreground that number says almost nothing.  `ConfusionMatrix` accumulates cm[truth][prediction] where the data already is -- the eval /
train step's logits and one-hot labels (`unet_confusion_scores`), the whole-image mask before its download (`unet_confusion_masks`) --
with no host synchronisation, and derives IoU, Dice, precision, recall and their means on the host when it is read.

Numerical contract: the prediction is the FIRST maximum of the scores, the truth the first maximum of the one-hot row (an all-zero row is
class 0), both by the loops of `unet_softmax_ce`, so `trace(matrix)` equals the engine's count of correctly classified pixels exactly.
Counts are int64 end to end; the quotients are float64 and NaN where the denominator is zero.
"""
import ctypes

import numpy as np
import torch


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class ConfusionMatrix:
    """update / result / reset_states in the shape of model.Mean.  Owns ONE int64 [K, K] tensor (rows = truth, columns = prediction), on the
    device when there is one; the kernels add to it as unsigned 64-bit counts."""

    def __init__(self, number_classes, device=None, name="confusion_matrix"):
        k = int(number_classes)
        if not 1 <= k <= 1024:
            raise ValueError("number_classes must be in [1, 1024]")
        self.name = name
        self.number_classes = k
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.matrix = torch.zeros((k, k), dtype=torch.int64, device=self.device)
        self.out_of_range = torch.zeros(1, dtype=torch.int64, device=self.device)      # pixels update_from_masks left out (label not in [0, K))
        self.device = self.matrix.device                 # with its index ("cuda" -> "cuda:0"): what the tensors handed in are compared with

    # ---- device producers: one launch each, no synchronisation ----------------------------------------------------------------------
    def _lib(self):
        if self.device.type != "cuda":
            raise RuntimeError("the confusion-matrix kernels run on the GPU only; use add_counts() with a host matrix")
        from ._lib import lib
        return lib()

    def _on_device(self, **tensors):
        """the kernels take raw pointers: every tensor must live on this matrix's (GPU) device"""
        for name, t in tensors.items():
            if not torch.is_tensor(t) or t.device != self.device:
                raise ValueError("%s must be a tensor on %s (got %s)" % (name, self.device, t.device if torch.is_tensor(t) else type(t).__name__))

    def update_from_scores(self, scores, labels_onehot, stream=None, ignore_unlabeled=False):
        """scores: fp32 [..., K] device tensor whose last axis may be a channel slice (stride(-2) = leading dimension) -- pass the LOGITS;
        labels_onehot: contiguous int32 [..., K].  stream: a hipStream_t handle (None: the current torch stream).  ignore_unlabeled: pixels
        whose one-hot row has no positive entry are counted nowhere (`unet_confusion_scores_valid`): trace and sum of the added counts are
        the `correct` and `valid` of the weighted loss with ignore_unlabeled on the same tensors, exactly."""
        L = self._lib()
        self._on_device(scores=scores, labels_onehot=labels_onehot)
        k = self.number_classes
        dense_above = scores.dim() <= 2 or all(scores.stride(i) == scores.stride(i + 1) * scores.shape[i + 1] for i in range(scores.dim() - 2))
        if not (scores.dtype == torch.float32 and labels_onehot.dtype == torch.int32 and scores.dim() >= 1 and scores.shape[-1] == k
                and scores.shape == labels_onehot.shape and labels_onehot.is_contiguous() and scores.stride(-1) == 1 and dense_above):
            raise ValueError("scores must be fp32 [..., %d] (a channel slice at most), labels_onehot contiguous int32 of the same shape" % k)
        lds = scores.stride(-2) if scores.dim() > 1 and scores.numel() > k else k
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        fn = L.unet_confusion_scores_valid if ignore_unlabeled else L.unet_confusion_scores
        fn(_ptr(scores), lds, _ptr(labels_onehot), labels_onehot.numel() // k, k, _ptr(self.matrix), stream)

    _PRED_ELEM = {torch.uint8: 1, torch.int32: 4}
    _TRUTH_ELEM = {torch.uint8: 1, torch.int16: 2, torch.int32: 4}          # (+ torch.uint16 where this torch has it)
    if hasattr(torch, "uint16"):
        _TRUTH_ELEM[torch.uint16] = 2

    def update_from_masks(self, pred, truth, ignore_label=-1, stream=None):
        """pred: device class map [H, W], uint8 or int32 (what `unet_argmax_paste` writes); truth: device class map [H, W], uint8, uint16
        (or int16 holding the same bits) or int32.  Rows may be pitched (stride(1) == 1, stride(0) >= W).  truth == ignore_label is skipped
        (-1: nothing is); pixels whose label is out of range are counted in self.out_of_range and left out of the matrix."""
        L = self._lib()
        self._on_device(pred=pred, truth=truth)
        if not (pred.dim() == 2 and pred.shape == truth.shape and pred.numel() > 0 and pred.stride(1) == 1 and truth.stride(1) == 1
                and pred.dtype in self._PRED_ELEM and truth.dtype in self._TRUTH_ELEM):
            raise ValueError("pred must be a uint8 / int32 class map [H, W], truth a uint8 / uint16 / int32 one of the same shape, rows contiguous")
        h, w = pred.shape
        pitch = lambda t: t.stride(0) if h > 1 else w                        # (the stride of a one-row view is arbitrary)
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.unet_confusion_masks(_ptr(pred), self._PRED_ELEM[pred.dtype], pitch(pred), _ptr(truth), self._TRUTH_ELEM[truth.dtype], pitch(truth),
                               h, w, self.number_classes, int(ignore_label), _ptr(self.matrix), _ptr(self.out_of_range), stream)

    # ---- host side -------------------------------------------------------------------------------------------------------------------
    def add_counts(self, matrix):
        """Add a host or device integer matrix [K, K] (the CPU path of the host inference pipeline, of tests, of stand-in networks)."""
        if torch.is_tensor(matrix):
            m = matrix
            if m.is_floating_point() or m.dtype == torch.bool:
                raise TypeError("add_counts needs an integer matrix")
        else:
            a = np.asarray(matrix)
            if a.dtype.kind not in "iu":
                raise TypeError("add_counts needs an integer matrix")
            m = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
        if tuple(m.shape) != (self.number_classes, self.number_classes):
            raise ValueError("add_counts needs a [%d, %d] matrix" % (self.number_classes, self.number_classes))
        self.matrix += m.to(device=self.device, dtype=torch.int64)

    update_state = add_counts

    def result(self, reduce=None):
        """The matrix as a numpy int64 array: one download; with `reduce` (parallel.DataParallel, or anything with reduce_sum and
        world_size) over more than one replica, first one SUM all-reduce of a clone -- the sync-on-read of the reference's metric
        variables under MirroredStrategy.  The accumulator itself is left as it is."""
        m = self.matrix
        if reduce is not None and getattr(reduce, "world_size", 1) > 1:
            m = reduce.reduce_sum(m.clone())
        return m.cpu().numpy().astype(np.int64, copy=True)

    def reset_states(self):
        self.matrix.zero_()
        self.out_of_range.zero_()

    def summary(self, reduce=None):
        return summarize(self.result(reduce))


def summarize(matrix):
    """int64 [K, K] counts (rows = truth) -> dict of float64 metrics; every quotient with a zero denominator is NaN, mean_iou averages the
    classes whose IoU denominator is > 0 (NaN when there is none), frequency_weighted_iou = sum_k truth_k * iou_k / total over the same."""
    c = np.asarray(matrix, dtype=np.int64)
    tp = np.diagonal(c).astype(np.int64)
    truth, pred, total = c.sum(axis=1), c.sum(axis=0), int(c.sum())

    def quot(num, den):
        num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
        out = np.full(den.shape, np.nan, dtype=np.float64)
        np.divide(num, den, out=out, where=den > 0)
        return out

    union = truth + pred - tp
    iou = quot(tp, union)
    ok = union > 0
    return {
        "pixel_accuracy": float(quot(tp.sum(), total)),
        "recall": quot(tp, truth),
        "precision": quot(tp, pred),
        "iou": iou,
        "dice": quot(2 * tp, truth + pred),
        "mean_iou": float(iou[ok].mean()) if ok.any() else float("nan"),
        "frequency_weighted_iou": float((truth[ok].astype(np.float64) * iou[ok]).sum() / total) if ok.any() else float("nan"),
    }


def csv_header(first, number_classes):
    k = number_classes
    return ",".join([first, "pixel_accuracy", "mean_iou"] + ["iou_%d" % i for i in range(k)] + ["dice_%d" % i for i in range(k)])


def csv_row(first, summary):
    """One row of test_class_metrics.csv / scores.csv: repr of every float64 (NaN as `nan`)."""
    vals = [summary["pixel_accuracy"], summary["mean_iou"]] + list(summary["iou"]) + list(summary["dice"])
    return ",".join([str(first)] + [repr(float(v)) for v in vals])
