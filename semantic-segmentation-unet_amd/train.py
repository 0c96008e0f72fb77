#!/usr/bin/env python3
"""`train_unet` -- the caller of the hot path (reference UNet/train.py), re-hosted on the HIP engine + RCCL.

Flags are the reference's (UNet/train.py:213-233) plus opt-in extras that default to reference behaviour.  Behaviour kept:
global batch = batch_size x replicas (:61); epoch = `test_every_n_steps` optimizer steps, and because the reference breaks
on `step > N` an epoch runs N+1 steps (:137-138); epoch 0 is an Adam warm-up at lr/10 over min(1000, N) steps (:126-132);
the test pass runs while step <= image_count / batch_size (:100,154-156); `test_loss.csv` is rewritten every epoch
(:173-176); the checkpoint `<out>/checkpoint/ckpt` is written only on a new best test loss (:181-184); early stopping
counts epochs since the first loss within 1e-4 of the best (:187-199).  Differences: one process per GPU (launch with
torchrun) instead of MirroredStrategy; scalars go to `<out>/tensorboard-<time>/{train,test}/scalars.jsonl` (TensorBoard
event files only if `tensorboard` is importable); data comes from readers.py unless a compatible reader object is passed.
"""
import argparse
import datetime
import json
import os
import time

LABEL_CHECK_EVERY = 16          # train steps between polls of the device-side out-of-range-label counter (one 4-byte read)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # before HIP initialises: RCCL needs dmabuf IPC on this platform

import numpy as np
import torch
import torch.distributed as dist

from . import model as unet_model_module
from . import readers

CONVERGENCE_TOLERANCE = 1e-4


class _Scalars:
    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.f = open(os.path.join(log_dir, "scalars.jsonl"), "a")
        self.tb = None
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.tb = SummaryWriter(log_dir)
        except Exception:
            pass

    def scalar(self, tag, value, step):
        self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        self.f.flush()
        if self.tb is not None:
            self.tb.add_scalar(tag, float(value), int(step))


def best_epoch_index(test_loss):
    """First epoch whose loss is within the tolerance of the minimum (reference UNet/train.py:187-196)."""
    err = np.abs(np.asarray(test_loss, dtype=np.float64) - np.min(test_loss))
    err[err < CONVERGENCE_TOLERANCE] = 0
    return int(np.where(err == 0)[0][0])


def parse_class_weights(text, number_classes):
    """`--class_weights w0,w1,...`: one finite weight >= 0 per class."""
    try:
        w = [float(v) for v in str(text).split(",")]
    except ValueError:
        raise ValueError("--class_weights must be comma-separated numbers, got %r" % (text,))
    if len(w) != number_classes:
        raise ValueError("--class_weights has %d entries but --number_classes is %d" % (len(w), number_classes))
    return [float(v) for v in unet_model_module.check_weights(w, "--class_weights")]


def region_settings(dice_weight=0.0, tversky_alpha=0.5, tversky_beta=0.5, dice_smooth=1.0, dice_class_weights=None, number_classes=2):
    """`--dice_weight`, `--tversky_alpha`, `--tversky_beta`, `--dice_smooth`, `--dice_class_weights w0,w1,...` -> the keywords of model.UNet
    for the region term ({} when the weight is 0: the network is then built as before); ValueError names the option at fault."""
    cw = dice_class_weights
    if isinstance(cw, str):
        try:
            cw = parse_class_weights(cw, number_classes)
        except ValueError as e:
            raise ValueError(str(e).replace("--class_weights", "--dice_class_weights"))
    if unet_model_module.check_region(dice_weight, (tversky_alpha, tversky_beta), dice_smooth, cw, number_classes) is None:
        return {}
    kw = {"dice_weight": float(dice_weight), "tversky": (float(tversky_alpha), float(tversky_beta)), "dice_smooth": float(dice_smooth)}
    if cw is not None:
        kw["dice_class_weights"] = [float(v) for v in cw]
    return kw


def border_settings(border_weight=0.0, border_sigma=5.0):
    """`--border_weight W0`, `--border_sigma S` -> the keywords of model.UNet for the border-distance weight map ({} when the weight is 0: the
    network is then built as before); ValueError names the option at fault."""
    try:
        b = unet_model_module.check_border(border_weight, border_sigma)
    except ValueError as e:
        raise ValueError(str(e).replace("border_", "--border_"))
    return {} if b is None else {"border_weight": b[0], "border_sigma": b[1]}


def train_model(output_folder, batch_size, reader_count, train_lmdb_filepath, test_lmdb_filepath, use_augmentation,
                number_classes, balance_classes, learning_rate, test_every_n_steps, early_stopping_count,
                train_reader=None, test_reader=None, max_epochs=None, quiet=False, compute_dtype=None, unet_factory=None,
                class_metrics=False, class_weights=None, ignore_label=None, region=None, border=None):
    """unet_factory (tests): callable(number_classes, global_batch_size, number_channels, learning_rate, device=..., compute_dtype=...)
    standing in for model.UNet, so the loop semantics can be checked without a GPU; the default is the HIP-backed class, which
    refuses to run anywhere but on an MI355X.

    class_metrics (opt-in extra): every test epoch accumulates one confusion matrix on the device (metrics.ConfusionMatrix, passed to
    dist_test_step as `confusion=`; no host sync per step), reads it once summed over the replicas, prints mean / per-class IoU behind the
    reference's own line, logs the scalars `mean_iou` and `iou_class_<k>` and rewrites `test_class_metrics.csv` (one row per epoch:
    epoch, pixel_accuracy, mean_iou, iou_0.., dice_0..).  Early stopping and checkpointing stay on the test loss.

    class_weights (opt-in extra, one per class) weight every pixel's loss by its truth class; ignore_label (opt-in extra) is the mask value
    of unlabeled pixels: the feeds turn it into an all-zero one-hot row, and the network (`ignore_unlabeled=True`), the accuracy and the
    test-epoch confusion matrix leave such pixels out.  Both reach the network as keywords only when set.

    region (opt-in extra; region_settings()'s dict): the soft Dice / Tversky term of the loss (model.UNet(dice_weight=, tversky=, dice_smooth=,
    dice_class_weights=)).  Train and test steps then return CE + region, so test_loss.csv, the best checkpoint and early stopping follow
    the compound loss; with class_metrics the test epoch's line also carries the mean soft index per class.

    border (opt-in extra; border_settings()'s dict): the border-distance weight map (model.UNet(border_weight=, border_sigma=)), formed on the
    device from every train and test step's own labels -- behind the device augmentation, so it follows the warped masks; unlabeled pixels
    (ignore_label) are no border.  Combines with class_weights, ignore_label and region."""
    say = (lambda *a: None) if quiet else print
    # the weighted-loss options are checked before anything is opened
    if class_weights is not None:
        class_weights = [float(v) for v in unet_model_module.check_weights(class_weights, "class_weights", (number_classes,))]
    if region:
        region = dict(region)
        if unet_model_module.check_region(region.get("dice_weight", 0.0), region.get("tversky", (0.5, 0.5)), region.get("dice_smooth", 1.0),
                                          region.get("dice_class_weights"), number_classes) is None:
            region = None
    if border:
        border = border_settings(**border)
    if ignore_label is not None:
        ignore_label = int(ignore_label)
        if not 0 <= ignore_label <= 255:
            raise ValueError("--ignore_label must be in [0, 255] (masks travel as uint8 class maps)")
        if use_augmentation and not getattr(train_reader, "augments_itself", False):
            raise ValueError("--ignore_label cannot be combined with --use_augmentation 1: the augmentation warps masks by rounded bilinear "
                             "interpolation (as the reference does), which smears the ignore value into neighbouring class ids; "
                             "pass --use_augmentation 0 (a nearest-neighbour mask warp is not implemented)")
        if os.environ.get("UNET_FEED", "1") == "0":
            raise ValueError("--ignore_label needs the device feed (UNET_FEED=0 hands over the reader's own one-hot labels)")
    for k, v in (("batch_size", batch_size), ("number_classes", number_classes), ("learning_rate", learning_rate),
                 ("test_every_n_steps", test_every_n_steps), ("balance_classes", balance_classes),
                 ("use_augmentation", use_augmentation), ("train_database", train_lmdb_filepath),
                 ("test_database", test_lmdb_filepath), ("output folder", output_folder),
                 ("early_stopping count", early_stopping_count), ("reader_count", reader_count)):
        say("{} = {}".format(k, v))
    os.makedirs(output_folder, exist_ok=True)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    have_gpu = torch.cuda.is_available()
    dev_ = torch.device("cuda", local) if have_gpu else torch.device("cpu")
    if have_gpu:
        torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl", device_id=dev_) if have_gpu else dist.init_process_group("gloo")
    global_batch_size = batch_size * world

    # reader workers: `reader_count` per replica (the reference scales it by the replica count, UNet/train.py:63); worker ids
    # are global, so the non-shuffled test readers of different ranks walk DISJOINT strides of the key list -- each global
    # test batch is split over the replicas like experimental_distribute_dataset does (UNet/train.py:85-90) -- and every
    # training worker draws its own random key stream (UNet/imagereader.py:209-233)
    reader_count = max(1, int(reader_count))
    total_workers = reader_count * world
    worker_ids = [rank * reader_count + w for w in range(reader_count)]
    # a reader with the reference's own surface (per-sample generator(), UNet/imagereader.py:338-355) is batched by an adapter
    train_reader = readers.as_batch_reader(train_reader) if train_reader is not None else None
    test_reader = readers.as_batch_reader(test_reader) if test_reader is not None else None
    if train_reader is None:
        train_reader = readers.TileFolderReader(train_lmdb_filepath, number_classes, shuffle=True, seed=0,
                                                balance_classes=bool(balance_classes), ignore_label=ignore_label)
    elif balance_classes and not getattr(train_reader, "balance_classes", False):
        raise ValueError("--balance_classes 1 needs a reader that implements class-balanced sampling (readers.TileFolderReader); "
                         "the reader passed in does not")
    if test_reader is None:
        test_reader = readers.TileFolderReader(test_lmdb_filepath, number_classes, shuffle=False, ignore_label=ignore_label)

    def worker_batches(reader, **kw):
        import inspect
        if "worker" not in inspect.signature(reader.batches).parameters:       # a caller-supplied reader without worker streams
            if total_workers > 1:
                raise ValueError("reader_count x replicas > 1 needs a reader whose batches() takes worker/num_workers")
            return [reader.batches(batch_size, **kw)]
        return [reader.batches(batch_size, worker=w, num_workers=total_workers, **kw) for w in worker_ids]
    say("Test Reader has {} images".format(test_reader.get_image_count()))
    say("Train Reader has {} images".format(train_reader.get_image_count()))
    feeds = []
    try:
        train_reader.startup()
        test_reader.startup()
        # device feed (feed.py): reader batches are staged and copied on a copy stream while the previous step runs, labels
        # travel as uint8 class maps and become the one-hot on the device; UNET_FEED=0 restores the synchronous hand-over
        use_feed = os.environ.get("UNET_FEED", "1") != "0"
        feed_kw = {"ignore_label": ignore_label} if ignore_label is not None else {}
        if use_feed:
            from .feed import DeviceFeed
            if use_augmentation and not getattr(train_reader, "augments_itself", False):
                # the reference augments inside its reader processes (UNet/imagereader.py:283-301, settings :79-85), ~31 images/s
                # per host core; here the raw tiles go to the device and the same sequence runs as HIP kernels (augment.py)
                from .augment import AugmentingFeed, DeviceAugmenter
                raw_feed = DeviceFeed(worker_batches(train_reader, classmap=True, pin=False, raw=True), dev_, classmap=True,
                                      number_classes=number_classes, onehot=False)
                train_batches = AugmentingFeed(raw_feed, DeviceAugmenter(
                    rotation_flag=True, reflection_flag=True, jitter_augmentation_severity=0.1, noise_augmentation_severity=0.02,
                    scale_augmentation_severity=0.1, blur_augmentation_max_sigma=2, intensity_augmentation_severity=None,
                    seed=rank, device=dev_), number_classes)
            else:
                train_batches = DeviceFeed(worker_batches(train_reader, classmap=True, pin=False), dev_, classmap=True, number_classes=number_classes,
                                           **feed_kw)
            test_batches = DeviceFeed(worker_batches(test_reader, classmap=True, pin=False), dev_, classmap=True, number_classes=number_classes,
                                      **feed_kw)
            feeds = [train_batches, test_batches]
        else:
            train_batches = readers.round_robin(worker_batches(train_reader))
            test_batches = readers.round_robin(worker_batches(test_reader))
        number_channels = train_reader.get_image_size()[2]
        loss_kw = {}                                        # only what is set: a stand-in network need not know the keywords
        if class_weights is not None:
            loss_kw["class_weights"] = class_weights
        if ignore_label is not None:
            loss_kw["ignore_unlabeled"] = True
        if region:
            loss_kw.update(region)
        if border:
            loss_kw.update(border)
        net = (unet_factory or unet_model_module.UNet)(number_classes, global_batch_size, number_channels, learning_rate,
                                                       device=dev_, compute_dtype=compute_dtype, **loss_kw)
        strategy = None
        if world > 1 and unet_factory is None:
            from .parallel import DataParallel
            strategy = net.parallel = DataParallel(net.engine)

        train_epoch_size = test_every_n_steps
        test_epoch_size = test_reader.get_image_count() / batch_size
        test_loss = []
        test_confusion, class_rows, step_kw = None, [], {}
        if class_metrics:
            from . import metrics
            test_confusion = metrics.ConfusionMatrix(number_classes, device=dev_, name="test_confusion")
            # (with ignore_label the network passes ignore_unlabeled on to update_from_scores: unlabeled pixels are in no cell)
            step_kw = {"confusion": test_confusion}        # only with the flag on: a stand-in network need not know the keyword
        train_loss_metric, train_acc_metric = unet_model_module.Mean("train_loss"), unet_model_module.CategoricalAccuracy("train_accuracy")
        test_loss_metric, test_acc_metric = unet_model_module.Mean("test_loss"), unet_model_module.CategoricalAccuracy("test_accuracy")
        stamp = datetime.datetime.now().strftime("%Y%m%dT%H%M%S")
        writers = None
        if rank == 0:
            writers = (_Scalars(os.path.join(output_folder, "tensorboard-" + stamp, "train")),
                       _Scalars(os.path.join(output_folder, "tensorboard-" + stamp, "test")))

        def check_labels():
            """The reference's reader raises IndexError on the first tile with a class id >= number_classes (UNet/imagereader.py:302-312).
            The device feed only COUNTS such pixels (no host sync per batch), so the counter is polled every LABEL_CHECK_EVERY steps and
            before anything is written; with several replicas the verdict is all-reduced (MAX) so that every rank raises on the same
            step instead of one raising and the others waiting in the next collective."""
            bad = sum(f.out_of_range_labels() for f in feeds if hasattr(f, "out_of_range_labels"))
            if world > 1:
                t = torch.tensor([float(bad)], device=dev_)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                bad = int(t.item())
            if bad > 0:
                raise IndexError("Number of classes specified differs from number of observed classes in data")

        epoch = 0
        while True:
            say("---- Epoch: {} ----".format(epoch))
            if epoch == 0:
                steps_this_epoch = min(1000, train_epoch_size)
                say("Performing Adam Optimizer learning rate warmup for {} steps".format(steps_this_epoch))
                net.set_learning_rate(learning_rate / 10)
            else:
                steps_this_epoch = train_epoch_size
                net.set_learning_rate(learning_rate)
            t0 = time.time()
            step = 0
            while step <= steps_this_epoch:                      # N+1 steps, as the reference's `step > N: break`
                images, labels = next(train_batches)
                net.dist_train_step(strategy, (images.to(dev_, non_blocking=True), labels.to(dev_, non_blocking=True),
                                               train_loss_metric, train_acc_metric))
                say("Train Epoch {}: Batch {}/{}: Loss {} Accuracy = {}".format(
                    epoch, step, train_epoch_size, train_loss_metric.result(), train_acc_metric.result()))
                if writers:
                    writers[0].scalar("loss", train_loss_metric.result(), epoch * train_epoch_size + step)
                    writers[0].scalar("accuracy", train_acc_metric.result(), epoch * train_epoch_size + step)
                train_loss_metric.reset_states(); train_acc_metric.reset_states()
                step += 1
                if step % LABEL_CHECK_EVERY == 0:
                    check_labels()
            epoch_test_loss = []
            soft_sum, soft_steps = None, 0                         # region term: the steps' mean soft index per class, summed on the device
            step = 0
            while step <= test_epoch_size:
                images, labels = next(test_batches)
                loss_value = net.dist_test_step(strategy, (images.to(dev_, non_blocking=True), labels.to(dev_, non_blocking=True),
                                                           test_loss_metric, test_acc_metric), **step_kw)
                epoch_test_loss.append(loss_value.numpy())
                rs = getattr(getattr(net, "engine", None), "region_stats", None) if (region and test_confusion is not None) else None
                if rs is not None:
                    soft_sum = rs[1:].clone() if soft_sum is None else soft_sum + rs[1:]
                    soft_steps += 1
                step += 1
            test_loss.append(np.mean(epoch_test_loss))             # (kept as numpy's fp32 scalar: test_loss.csv then carries the reference's text, UNet/train.py:162,173-176)
            check_labels()                                         # before the csv / checkpoint of this epoch are written
            say("Test Epoch: {}: Loss = {} Accuracy = {}".format(epoch, test_loss_metric.result(), test_acc_metric.result()))
            if writers:
                writers[1].scalar("loss", test_loss_metric.result(), (epoch + 1) * train_epoch_size)
                writers[1].scalar("accuracy", test_acc_metric.result(), (epoch + 1) * train_epoch_size)
            test_loss_metric.reset_states(); test_acc_metric.reset_states()
            if test_confusion is not None:
                cls = test_confusion.summary(strategy)             # the epoch's one read: an all-reduce over the replicas, one download
                test_confusion.reset_states()
                if rank == 0:
                    say("Test Epoch: {}: mean IoU = {} IoU per class = {}".format(epoch, cls["mean_iou"], [float(v) for v in cls["iou"]]))
                if soft_sum is not None:                           # (every rank: the sum over the replicas is a collective)
                    if strategy is not None:
                        soft_sum = strategy.reduce_sum(soft_sum)
                    soft = [float(v) / (soft_steps * world) for v in soft_sum.tolist()]
                    if rank == 0:
                        say("Test Epoch: {}: mean soft Tversky index per class = {}".format(epoch, soft))
                if writers:
                    writers[1].scalar("mean_iou", cls["mean_iou"], (epoch + 1) * train_epoch_size)
                    for k, v in enumerate(cls["iou"]):
                        writers[1].scalar("iou_class_%d" % k, v, (epoch + 1) * train_epoch_size)
                class_rows.append(metrics.csv_row(epoch, cls))
            if rank == 0:
                with open(os.path.join(output_folder, "test_loss.csv"), "w") as f:
                    f.writelines(str(v) + "\n" for v in test_loss)
                if test_confusion is not None:
                    with open(os.path.join(output_folder, "test_class_metrics.csv"), "w") as f:
                        f.write(metrics.csv_header("epoch", number_classes) + "\n")
                        f.writelines(r + "\n" for r in class_rows)
            say("Epoch took: {} s".format(time.time() - t0))
            if (len(test_loss) - 1) == int(np.argmin(test_loss)):
                say("Test loss improved: {}, saving checkpoint".format(np.min(test_loss)))
                if strategy is not None:
                    strategy.average_moving_stats()
                if rank == 0:
                    net.save_checkpoint(os.path.join(output_folder, "checkpoint", "ckpt"))
            best = best_epoch_index(test_loss)
            say("Best epoch: {}".format(best))
            if len(test_loss) - best > early_stopping_count:
                break
            epoch += 1
            if max_epochs is not None and epoch >= max_epochs:
                break
        return test_loss
    finally:
        for f in feeds:
            f.close()
        train_reader.shutdown()
        test_reader.shutdown()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="train_unet", description="Script which trains a unet model")
    ap.add_argument("--batch_size", dest="batch_size", type=int, default=4, help="training batch size")
    ap.add_argument("--number_classes", dest="number_classes", type=int, default=2)
    ap.add_argument("--learning_rate", dest="learning_rate", type=float, default=3e-4)
    ap.add_argument("--output_dir", dest="output_folder", type=str, required=True, help="Folder where outputs will be saved (Required)")
    ap.add_argument("--test_every_n_steps", dest="test_every_n_steps", type=int, default=1000)
    ap.add_argument("--balance_classes", dest="balance_classes", type=int, default=0)
    ap.add_argument("--use_augmentation", dest="use_augmentation", type=int, default=1)
    ap.add_argument("--train_database", dest="train_database_filepath", type=str, required=False, default=None,
                    help="training data store (folder of .npy tiles; see readers.py)")
    ap.add_argument("--test_database", dest="test_database_filepath", type=str, required=False, default=None)
    ap.add_argument("--early_stopping", dest="early_stopping_count", type=int, default=10)
    ap.add_argument("--reader_count", dest="reader_count", type=int, default=1)
    # opt-in extras (not in the reference)
    ap.add_argument("--synthetic", type=str, default=None, help="HxWxC[xCOUNT] synthetic tiles instead of databases")
    ap.add_argument("--max_epochs", type=int, default=None)
    ap.add_argument("--compute_dtype", choices=["fp32", "bf16"], default=None,
                    help="bf16: mixed precision (the policy the reference keeps commented out, UNet/train.py:52-54): bf16 "
                         "contractions in the wide 3x3 layers, fp32 accumulation and master weights")
    ap.add_argument("--class_metrics", dest="class_metrics", action="store_true",
                    help="per test epoch: confusion matrix on the device -> mean / per-class IoU printed, logged and written to "
                         "test_class_metrics.csv (pixel accuracy alone says little on masks with a few percent of foreground)")
    ap.add_argument("--class_weights", dest="class_weights", type=str, default=None,
                    help="w0,w1,...: one loss weight per class (finite, >= 0; as many as --number_classes).  Every pixel's cross-entropy is "
                         "multiplied by the weight of its truth class; the reduction stays sum / (batch x H x W), not divided by the weights")
    ap.add_argument("--ignore_label", dest="ignore_label", type=int, default=None,
                    help="mask value of unlabeled pixels: they add no loss and no gradient and are left out of the accuracy and of "
                         "--class_metrics (needs --use_augmentation 0: the augmentation's bilinear mask warp would smear the value)")
    ap.add_argument("--dice_weight", dest="dice_weight", type=float, default=0.0,
                    help="lambda >= 0: adds lambda x the soft Dice / Tversky term (per image, 1 - index averaged over the classes, summed over the "
                         "batch / global batch size) to the cross-entropy; 0 = cross-entropy only")
    ap.add_argument("--tversky_alpha", dest="tversky_alpha", type=float, default=0.5, help="weight of false positives in the index (0.5, 0.5: Dice)")
    ap.add_argument("--tversky_beta", dest="tversky_beta", type=float, default=0.5, help="weight of false negatives in the index")
    ap.add_argument("--dice_smooth", dest="dice_smooth", type=float, default=1.0, help="smoothing constant s > 0 of the index")
    ap.add_argument("--dice_class_weights", dest="dice_class_weights", type=str, default=None,
                    help="w0,w1,...: weight of each class's index in the term (finite, >= 0, not all zero; normalised to sum 1)")
    ap.add_argument("--border_weight", dest="border_weight", type=float, default=0.0,
                    help="w0 >= 0: every pixel's loss is multiplied by 1 + w0 exp(-d^2 / (2 sigma^2)), d = its distance in pixels to the nearest "
                         "class border of its mask, computed on the device from each batch's (augmented) masks; 0 = off")
    ap.add_argument("--border_sigma", dest="border_sigma", type=float, default=5.0, help="sigma > 0 of --border_weight, in pixels")
    a = ap.parse_args(argv)
    try:
        border = border_settings(a.border_weight, a.border_sigma)
    except ValueError as e:
        ap.error(str(e))
    try:
        region = region_settings(a.dice_weight, a.tversky_alpha, a.tversky_beta, a.dice_smooth, a.dice_class_weights, a.number_classes)
    except ValueError as e:
        ap.error(str(e))
    class_weights = None
    if a.class_weights is not None:
        try:
            class_weights = parse_class_weights(a.class_weights, a.number_classes)
        except ValueError as e:
            ap.error(str(e))
    if a.ignore_label is not None and a.use_augmentation:
        ap.error("--ignore_label cannot be combined with --use_augmentation 1: the augmentation warps masks by rounded bilinear interpolation, "
                 "which smears the ignore value into neighbouring class ids; pass --use_augmentation 0")
    tr = te = None
    if a.synthetic:
        parts = [int(v) for v in a.synthetic.lower().split("x")]
        h, w, c = parts[:3]
        count = parts[3] if len(parts) > 3 else 64
        tr = readers.SyntheticReader(count, h, w, c, a.number_classes, seed=1)
        te = readers.SyntheticReader(max(count // 4, a.batch_size), h, w, c, a.number_classes, seed=2)
    elif not (a.train_database_filepath and a.test_database_filepath):
        ap.error("--train_database and --test_database are required unless --synthetic is given")
    train_model(a.output_folder, a.batch_size, a.reader_count, a.train_database_filepath, a.test_database_filepath,
                a.use_augmentation, a.number_classes, a.balance_classes, a.learning_rate, a.test_every_n_steps,
                a.early_stopping_count, train_reader=tr, test_reader=te, max_epochs=a.max_epochs, compute_dtype=a.compute_dtype,
                class_metrics=a.class_metrics, class_weights=class_weights, ignore_label=a.ignore_label, region=region or None,
                border=border or None)


if __name__ == "__main__":
    main()
