"""Drop-in for the reference's `UNet/model.py`: same class name, constructor signature, constants and method names
(reference UNet/model.py:19-256), with the TensorFlow graph replaced by the HIP engine (engine.py).

    UNet(number_classes, global_batch_size, number_channels, learning_rate=3e-4, label_smoothing=0)

Callers written against the reference keep working:
  * `train.py` uses get_keras_model()/get_optimizer()/set_learning_rate()/dist_train_step()/dist_test_step()
    (reference UNet/train.py:94-161);
  * `inference.py` uses load_checkpoint(), estimate_radius() and `model(batch_data)` returning softmax [N,H,W,K] that
    np.squeeze/np.argmax accept (reference UNet/inference.py:54,105-107,164-166,191-192).
"""
import numpy as np
import torch

from . import engine as _engine
from .engine import Engine


class Mean:
    """Look-alike of tf.keras.metrics.Mean (reference UNet/train.py:105,107): update_state / result / reset_states."""

    def __init__(self, name="mean"):
        self.name = name
        self.total, self.count = 0.0, 0.0

    def update_state(self, value, sample_weight=None):
        self.total += float(value)
        self.count += 1.0

    def add(self, total, count):
        """(total, count) pair summed over replicas -- tf.keras metrics under MirroredStrategy aggregate their `total` and
        `count` variables with SUM on read."""
        self.total += float(total)
        self.count += float(count)

    def result(self):
        return np.float32(self.total / self.count) if self.count else np.float32(0.0)

    def reset_states(self):
        self.total, self.count = 0.0, 0.0


class CategoricalAccuracy(Mean):
    """Look-alike of tf.keras.metrics.CategoricalAccuracy (reference UNet/train.py:106,108): mean over pixels of
    argmax(labels) == argmax(softmax).  The engine counts matches on the device; update_state(correct, total) adds them."""

    def update_state(self, correct, total):
        self.total += float(correct)
        self.count += float(total)


class _Optimizer:
    """The part of tf.keras.optimizers.Adam the reference touches: `.learning_rate` (UNet/model.py:154-158)."""

    def __init__(self, learning_rate):
        self.learning_rate = learning_rate


class _Loss:
    """What dist_train_step returns: something with .numpy() (reference UNet/train.py:141,159,161)."""

    def __init__(self, tensor):
        self._t = tensor

    def numpy(self):
        return np.float32(self._t.item())

    def __float__(self):
        return float(self._t.item())


def check_weights(values, what, shape=None):
    """Loss weights as an fp32 numpy array: finite and >= 0 (the kernel does not check), of `shape` when given."""
    a = np.asarray(values, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (what, list(shape), list(a.shape)))
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("%s must be finite and >= 0" % what)
    return a


def check_region(dice_weight, tversky, dice_smooth, dice_class_weights, number_classes):
    """The region term's settings, validated on the host (the kernel checks signs only):
    -> None when dice_weight == 0, else (weight, alpha, beta, smooth, class weights as an fp32 numpy array or None)"""
    try:
        alpha, beta = (float(v) for v in tversky)
    except (TypeError, ValueError):
        raise ValueError("tversky must be a pair (alpha, beta)")
    lam, smooth = float(dice_weight), float(dice_smooth)
    if not all(np.isfinite(v) for v in (lam, alpha, beta, smooth)):
        raise ValueError("dice_weight, tversky and dice_smooth must be finite")
    if lam < 0 or alpha < 0 or beta < 0:
        raise ValueError("dice_weight, tversky alpha and beta must be >= 0")
    if smooth <= 0:
        raise ValueError("dice_smooth must be > 0")
    cw = None
    if dice_class_weights is not None:
        cw = check_weights(dice_class_weights, "dice_class_weights", (number_classes,))
        if not (cw > 0).any():
            raise ValueError("dice_class_weights must not all be zero")
    return None if lam == 0 else (lam, alpha, beta, smooth, cw)


def check_border(border_weight, border_sigma):
    """The border-distance weight's settings, validated on the host: -> None when border_weight == 0, else (w0, sigma)"""
    try:
        w0, sigma = float(border_weight), float(border_sigma)
    except (TypeError, ValueError):
        raise ValueError("border_weight and border_sigma must be numbers")
    if not np.isfinite(w0) or w0 < 0:
        raise ValueError("border_weight must be finite and >= 0")
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError("border_sigma must be finite and > 0")
    return None if w0 == 0 else (w0, sigma)


class _KerasLikeModel:
    """`unet.get_keras_model()`: callable as m(x, training=False) with x fp32 [N,C,H,W] (numpy or torch), returning the
    softmax [N,H,W,K] (reference UNet/inference.py:105,164; UNet/model.py:177,209,239)."""

    def __init__(self, owner):
        self._o = owner

    def __call__(self, x, training=False, dropout_masks=None):
        """numpy in -> numpy out (the reference's callers run np.squeeze / np.argmax(...).astype on the result,
        UNet/inference.py:105-107,164-166); torch tensor in -> device tensor out (no host copy)."""
        o = self._o
        if not torch.is_tensor(x):
            xa = np.asarray(x, dtype=np.float32)
            # host arrays are checked where they enter: the fp32 route forms fp32 values as three bf16 pieces (csrc/winograd_x6.hip), which turns an
            # Inf into NaN (Inf - Inf in the split) where TensorFlow's fp32 kernels would carry the Inf -- either way the mask is garbage, so say so
            if not np.isfinite(xa).all():
                raise ValueError("input image contains Inf / NaN")
            xt = torch.as_tensor(xa)
        else:
            xt = x.float()
        prob = o.engine.forward(xt, training=bool(training), dropout_masks=dropout_masks)
        if torch.is_tensor(x):
            return prob.clone()      # engine buffers are reused by the next call
        return prob.cpu().numpy()

    @property
    def trainable_weights(self):
        return [self._o.engine.p[k] for k in self._o.engine.trainable_names()]


class UNet:
    _BASELINE_FEATURE_DEPTH = 64
    _KERNEL_SIZE = 3
    _DECONV_KERNEL_SIZE = 2
    _POOLING_STRIDE = 2

    SIZE_FACTOR = 16
    RADIUS = 96

    def __init__(self, number_classes, global_batch_size, number_channels, learning_rate=3e-4, label_smoothing=0,
                 device="cuda", seed=0, compute_dtype=None, class_weights=None, ignore_unlabeled=False,
                 dice_weight=0.0, tversky=(0.5, 0.5), dice_smooth=1.0, dice_class_weights=None, border_weight=0.0, border_sigma=5.0):
        """border_weight (w0 >= 0), border_sigma (sigma > 0, pixels): every step forms the U-Net recipe's border weight map from its own labels
        on the device, w(p) = 1 + w0 exp(-d(p)^2 / (2 sigma^2)) with d the exact Euclidean distance from p to the nearest pixel that has a
        4-neighbour of another class in the same image (unet_border_weights), and hands it on as the step's pixel_weights, multiplied into the
        caller's where given.  Per image: no new collective, independent of how a batch is split.  Like pixel_weights it does not enter the
        region term.  border_weight = 0: the launches of before.
        dice_weight (lambda >= 0), tversky = (alpha, beta) >= 0, dice_smooth (s > 0), dice_class_weights (length number_classes, >= 0, not
        all zero; normalised to sum 1): the compound loss CE + lambda / G * sum over the local images n and the classes k of c~_k (1 - T_nk),
        T_nk = (I + s) / ((1 - alpha - beta) I + alpha S + beta Y + s) the soft Tversky index of image n (alpha = beta = 0.5: soft Dice) over
        its labeled pixels; class_weights and pixel_weights do not enter it.  Per image and divided by the global batch size, like the
        cross-entropy: independent of how a batch is split over replicas.  dice_weight = 0: the launches of before.
        class_weights (length number_classes, finite, >= 0), ignore_unlabeled, and the steps' pixel_weights: the weighted loss
        loss = sum_p class_weights[truth_p] * pixel_weights[p] * ce_p / (G H W) -- Keras' sample_weight under the reference's reduction, NOT
        divided by the weight sum; with ignore_unlabeled a pixel whose one-hot row is all zero (feed.DeviceFeed(ignore_label=...)) adds no
        loss and no gradient and leaves the accuracy's numerator and denominator.  All unset: the reference's loss, the launches of before."""
        self.number_channels = number_channels
        self.learning_rate = learning_rate
        self.number_classes = number_classes
        self.global_batch_size = global_batch_size
        self.label_smoothing = label_smoothing
        region = check_region(dice_weight, tversky, dice_smooth, dice_class_weights, number_classes)     # before anything touches the device
        self.border = check_border(border_weight, border_sigma)  # None, or (w0, sigma)
        self.engine = Engine(number_classes, number_channels, device=device, seed=seed)
        self.ignore_unlabeled = bool(ignore_unlabeled)
        self.class_weights = None
        if class_weights is not None:                            # validated and uploaded once
            cw = check_weights(class_weights, "class_weights", (number_classes,))
            self.class_weights = torch.as_tensor(cw).to(self.engine.dev)
        self.region = None                                       # Engine.forward(region=...): class weights uploaded once
        if region is not None:
            self.region = region[:4] + (torch.as_tensor(region[4]).to(self.engine.dev) if region[4] is not None else None,)
        if compute_dtype is not None:        # "fp32" (reference arithmetic) | "bf16" (mixed precision the reference leaves commented
            if compute_dtype not in ("fp32", "bf16"):                                  # out, UNet/train.py:52-54)
                raise ValueError("compute_dtype must be 'fp32' or 'bf16'")
            self.engine.compute_dtype = compute_dtype
        self.model = _KerasLikeModel(self)
        self.optimizer = _Optimizer(learning_rate)
        self.parallel = None         # set by parallel.DataParallel

    # -- reference UNet/model.py:81-83: tf.train.Checkpoint's own files (TensorBundle ckpt.index + ckpt.data-*, object-graph keys;
    #    checkpoint.py / tf_checkpoint.py); round-1 .npz files still load
    def load_checkpoint(self, checkpoint_filepath):
        from .checkpoint import load_checkpoint
        load_checkpoint(self, checkpoint_filepath)

    def save_checkpoint(self, checkpoint_filepath):
        from .checkpoint import save_checkpoint
        save_checkpoint(self, checkpoint_filepath)

    def get_keras_model(self):
        return self.model

    def get_optimizer(self):
        return self.optimizer

    def set_learning_rate(self, learning_rate):
        self.optimizer.learning_rate = learning_rate

    def get_learning_rate(self):
        return self.optimizer.learning_rate

    @staticmethod
    def _round_radius(x):
        return int(UNet.SIZE_FACTOR * np.ceil(float(x) / UNet.SIZE_FACTOR))

    def input_gradient(self, img, dprob):
        """d sum(dprob * softmax(img)) / d img with the model in eval mode; img [N,C,H,W], dprob [N,H,W,K]."""
        x = torch.as_tensor(np.asarray(img, dtype=np.float32)) if not torch.is_tensor(img) else img.float()
        self.engine.forward(x, training=False)
        g = torch.as_tensor(np.asarray(dprob, dtype=np.float32)) if not torch.is_tensor(dprob) else dprob.float()
        return self.engine.input_gradient_eval(g)

    def estimate_radius(self, img=None):
        """Effective-receptive-field probe (reference UNet/model.py:165-202): eval-mode forward of a random-normal
        [1,C,192,192] image, mean-absolute-error loss against a copy of the softmax whose centre pixel is flipped
        (1 - p), gradient of that loss w.r.t. the image, extent of |grad| > 1e-8, rounded up to a multiple of 16;
        falls back to the theoretical radius when fewer than 2 rows/columns respond.  (The reference repeats the
        identical forward 10 times and keeps the last tape; one pass is the same result.)"""
        N = 2 * UNet.RADIUS
        if img is None:
            img = np.random.normal(size=(1, self.number_channels, N, N))
        img = np.asarray(img, dtype=np.float32)
        mid = int(img.shape[2] / 2)
        x = torch.as_tensor(img)
        prob = self.engine.forward(x, training=False)
        k = prob.shape[-1]
        # loss[h,w] = mean_k |msk - p| is non-zero only at the centre pixel, where msk = 1 - p.  msk is a CONSTANT of the tape (the
        # reference takes it from softmax.numpy()), so d/dp_k of mean_k |msk_k - p_k| = -sign(msk_k - p_k) / K = -sign(1 - 2 p_k) / K --
        # not the derivative of |1 - 2 p_k|, which is twice that and widens the extent of |grad| > 1e-8
        g = torch.zeros_like(prob)
        pm = prob[0, mid, mid, :]
        g[0, mid, mid, :] = -torch.sign(1.0 - 2.0 * pm) / k
        grad_img = np.abs(self.engine.input_gradient_eval(g)[0].cpu().numpy())      # [C,H,W]
        grad_img = np.average(grad_img, axis=0) if self.number_channels > 1 else grad_img[0]
        print('Theoretical RF: {}'.format(UNet.RADIUS))
        eps = 1e-8
        vec = np.maximum(np.max(grad_img, axis=0), np.max(grad_img, axis=1))
        idx = np.nonzero(vec > eps)[0]
        if len(idx) < 2:
            radius = UNet.RADIUS
            print('ERF based radius detection failed, defaulting to theoretical radius: {}'.format(radius))
        else:
            erf = int((np.max(idx) - np.min(idx)) / 2)
            radius = UNet._round_radius(erf)
            print('computed radius : "{}"'.format(radius))
        return radius

    # -- reference UNet/model.py:204-228
    def _pixel_weights(self, pixel_weights, images):
        """[N,H,W] fp32, numpy (validated here) or device tensor (the caller's to keep finite and >= 0: no host sync) -> device tensor"""
        if pixel_weights is None:
            return None
        n, _, h, w = images.shape
        if torch.is_tensor(pixel_weights):
            if tuple(pixel_weights.shape) != (n, h, w):
                raise ValueError("pixel_weights must have shape %s, got %s" % ([n, h, w], list(pixel_weights.shape)))
            return pixel_weights.to(device=self.engine.dev, dtype=torch.float32).contiguous()
        return torch.as_tensor(check_weights(pixel_weights, "pixel_weights", (n, h, w))).to(self.engine.dev)

    def border_weight_map(self, labels, pixel_weights=None, return_distance=False):
        """The border weight map of a batch of one-hot labels [N,H,W,K] (numpy or tensor), as the steps form it: fp32 [N,H,W] on the device,
        the caller's pixel_weights multiplied in; with return_distance also the int32 squared distances (engine.UNET_BORDER_NONE where an
        image has no class border).  Needs border_weight > 0.  The tensors are the caller's own (copies of the engine's buffers)."""
        if self.border is None:
            raise ValueError("border_weight_map needs a network built with border_weight > 0")
        lab = (labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels, dtype=np.int32))).to(self.engine.dev).contiguous()
        if lab.dim() != 4 or lab.dtype != torch.int32:
            raise ValueError("labels must be int32 one-hot [N,H,W,K]")
        pw = self._pixel_weights(pixel_weights, lab.permute(0, 3, 1, 2))
        out = self.engine.border_weights(lab, self.border[0], self.border[1], pixel_weights=pw, return_d2=return_distance)
        return (out[0].clone(), out[1].clone()) if return_distance else out.clone()

    def _loss_kw(self, pixel_weights, images, labels=None):
        """forward()'s weighted-loss keywords; empty when nothing is set, so the default step calls forward() as it always did"""
        kw = {}
        if self.class_weights is not None:
            kw["class_weights"] = self.class_weights
        if self.border is not None and labels is not None:       # the step's own labels -> the map, the caller's weights multiplied in
            kw["pixel_weights"] = self.engine.border_weights(labels.to(self.engine.dev).contiguous(), self.border[0], self.border[1],
                                                             pixel_weights=self._pixel_weights(pixel_weights, images))
        elif pixel_weights is not None:
            kw["pixel_weights"] = self._pixel_weights(pixel_weights, images)
        if self.ignore_unlabeled:
            kw["ignore_unlabeled"] = True
        if self.region is not None:
            kw["region"] = self.region
        return kw

    def train_step(self, inputs, dropout_masks=None, confusion=None, pixel_weights=None):
        """confusion (metrics.ConfusionMatrix, opt-in): the step's per-class counts are added to it on the device, no host sync;
        pixel_weights ([N,H,W] fp32, opt-in): the per-pixel factor of the weighted loss"""
        (images, labels, loss_metric, accuracy_metric) = inputs
        e = self.engine
        images = torch.as_tensor(np.asarray(images, dtype=np.float32)) if not torch.is_tensor(images) else images
        labels = torch.as_tensor(np.asarray(labels, dtype=np.int32)) if not torch.is_tensor(labels) else labels
        if self.border is not None:
            labels = labels.to(e.dev).contiguous()               # one upload serves the map and the loss
        e.forward(images, training=True, dropout_masks=dropout_masks, labels=labels,
                  global_batch_size=self.global_batch_size, label_smoothing=self.label_smoothing, want_grad=True, confusion=confusion,
                  **self._loss_kw(pixel_weights, images, labels))
        if self.parallel is not None:
            self.parallel.begin_step()
        e.backward()
        if self.parallel is not None:
            self.parallel.finish_step()
        e.adam_step(float(self.optimizer.learning_rate))
        return self._update_metrics(images, loss_metric, accuracy_metric)

    # -- reference UNet/model.py:237-250
    def test_step(self, inputs, confusion=None, pixel_weights=None):
        (images, labels, loss_metric, accuracy_metric) = inputs
        e = self.engine
        images = torch.as_tensor(np.asarray(images, dtype=np.float32)) if not torch.is_tensor(images) else images
        labels = torch.as_tensor(np.asarray(labels, dtype=np.int32)) if not torch.is_tensor(labels) else labels
        if self.border is not None:
            labels = labels.to(e.dev).contiguous()               # one upload serves the map and the loss
        e.forward(images, training=False, labels=labels, global_batch_size=self.global_batch_size,
                  label_smoothing=self.label_smoothing, confusion=confusion, **self._loss_kw(pixel_weights, images, labels))
        return self._update_metrics(images, loss_metric, accuracy_metric)

    def _update_metrics(self, images, loss_metric, accuracy_metric):
        e = self.engine
        # [per-replica loss, correctly classified pixels]; behind the weighted loss also [labeled pixels, weight sum], which travel in the
        # same all-reduce
        vals = e.loss_stats.clone() if e.weighted_loss else e.loss_buf.clone()
        self._reduced = None
        if loss_metric is not None or accuracy_metric is not None:       # forces the per-step host sync the reference has
            world = 1
            if self.parallel is not None and self.parallel.world_size > 1:
                # metric variables are summed over the replicas (X3); the same 8-byte all-reduce serves the loss SUM (X2)
                self._reduced = self.parallel.reduce_sum(vals.clone())
                world = self.parallel.world_size
            lb = (self._reduced if self._reduced is not None else vals).tolist()
            n, _, h, w = images.shape
            if loss_metric is not None:
                loss_metric.add(lb[0], world) if hasattr(loss_metric, "add") else loss_metric.update_state(lb[0] / world)
            if accuracy_metric is not None:
                # unlabeled pixels are in neither count: the denominator is the labeled pixels summed over the replicas
                accuracy_metric.update_state(lb[1], lb[2] if (e.weighted_loss and self.ignore_unlabeled) else n * h * w * world)
        return _Loss(vals[0:1])

    # -- reference UNet/model.py:230-235,252-256: one replica per process here; the cross-replica SUM of the per-replica
    #    losses is an RCCL all-reduce in parallel.DataParallel (reference: dist_strategy.reduce(SUM, ...)).
    def dist_train_step(self, dist_strategy, inputs, dropout_masks=None, confusion=None, pixel_weights=None):
        loss = self.train_step(inputs, dropout_masks=dropout_masks, confusion=confusion, pixel_weights=pixel_weights)
        return self._reduce_loss(dist_strategy, loss)

    def dist_test_step(self, dist_strategy, inputs, confusion=None, pixel_weights=None):
        loss = self.test_step(inputs, confusion=confusion, pixel_weights=pixel_weights)
        return self._reduce_loss(dist_strategy, loss)

    def _reduce_loss(self, dist_strategy, loss):
        strat = dist_strategy if dist_strategy is not None else self.parallel
        if strat is not None and getattr(strat, "world_size", 1) > 1:
            if getattr(self, "_reduced", None) is not None:              # already summed together with the metric pairs
                return _Loss(self._reduced[0:1])
            return _Loss(strat.reduce_sum(loss._t))
        return loss
