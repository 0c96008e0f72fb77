"""GPU: the confusion-matrix kernels (`unet_confusion_scores`, `unet_confusion_masks`, csrc/metrics.hip) through the C ABI, and the three
places that launch them: the eval / train step, `segment_image`, the inference CLI.  The checker is numpy in this file --
np.bincount(t * K + p, minlength=K * K).reshape(K, K) with np.argmax (first maximum) -- and every comparison is exact integer equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

PREFILL = 2 ** 32 - 1


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _count(t, p, k):
    return np.bincount(np.asarray(t, np.int64).ravel() * k + np.asarray(p, np.int64).ravel(), minlength=k * k).reshape(k, k)


def _scores_case(P, k, lds, seed):
    """scores from {-1, 0, 0.5, 1} (ties in most pixels; the slack of lds > K holds 9, which would win if it were read); one-hot labels with
    about 1 % all-zero rows (P >= 64: at least one), which count as class 0"""
    rng = np.random.default_rng(seed)
    z = np.full((P, lds), 9.0, np.float32)
    z[:, :k] = rng.choice(np.array([-1.0, 0.0, 0.5, 1.0], np.float32), size=(P, k))
    cls = rng.integers(0, k, P)
    lab = np.zeros((P, k), np.int32)
    lab[np.arange(P), cls] = 1
    zero = rng.random(P) < 0.01
    if P >= 64:
        zero[rng.integers(0, P)] = True
    lab[zero] = 0
    want = _count(np.argmax(lab, axis=-1), np.argmax(z[:, :k], axis=-1), k)
    return z, lab, want


def _offset_tensor(a, offset_elems, dtype):
    """a device copy of `a` that starts `offset_elems` elements into a 256-byte aligned allocation"""
    buf = torch.zeros(a.size + offset_elems + 8, dtype=dtype, device="cuda")
    view = buf[offset_elems:offset_elems + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    return buf, view


SCORE_PATHS = [   # (K, lds, byte offset of the scores pointer, of the labels pointer)
    (2, 2, 0, 0),          # dense path, 16-byte loads
    (2, 2, 8, 8),          # dense path, 8-byte loads
    (2, 2, 4, 0),          # scores pointer 4 bytes into the allocation: generic path
    (2, 2, 0, 4),          # labels pointer 4 bytes in
    (3, 4, 0, 0),          # padded rows must not be read as classes
    (4, 4, 0, 0),          # K^2 = 16: last of the ballot path, dense
    (4, 6, 0, 0),          # ... with a leading dimension
    (5, 5, 0, 0),          # first of the LDS path
    (64, 64, 0, 0),        # last of the LDS path
    (65, 65, 0, 0),        # first direct path
    (256, 256, 0, 0),      # direct path
]
SCORE_P = [1, 63, 64, 65, 255, 257, 70001]        # 70001: 274 workgroups (137 on the pixel-pair path), one pass each, the last one ends mid-wave;
#                                                   several passes per workgroup: test_confusion_scores_when_the_grid_stride_loop_wraps


@pytest.mark.parametrize("k,lds,zoff,loff", SCORE_PATHS, ids=["K%d_lds%d_z%d_l%d" % c for c in SCORE_PATHS])
def test_confusion_scores_equals_numpy_on_every_path(hip, k, lds, zoff, loff):
    for P in SCORE_P:
        z, lab, want = _scores_case(P, k, lds, seed=k * 1000 + P)
        zb, zt = _offset_tensor(z, zoff // 4, torch.float32)
        lb, lt = _offset_tensor(lab, loff // 4, torch.int32)
        assert zt.data_ptr() % 16 == zoff and lt.data_ptr() % 16 == loff
        cm = torch.zeros((k, k), dtype=torch.int64, device="cuda")
        hip.unet_confusion_scores(_ptr(zt), lds, _ptr(lt), P, k, _ptr(cm), _stream())
        got = cm.cpu().numpy()
        assert got.sum() == P and np.array_equal(got, want), (k, lds, P, int(np.abs(got - want).sum()))


WRAP_P = 3 * 1024 * 256 + 4465     # > 1024 workgroups x 256 threads, also in pixel pairs: workgroups run their grid-stride loop up to 4 times (2 in pairs) and
#                                    the last pass ends mid-wave (790897 = 64 * 12357 + 49; 395449 pairs = 64 * 6178 + 57, the last pair half full)
WRAP_PATHS = [(2, 2, 0, 0), (2, 2, 8, 8), (2, 2, 4, 0), (3, 4, 0, 0), (4, 4, 0, 0), (4, 6, 0, 0), (5, 5, 0, 0), (9, 12, 0, 0)]


@pytest.mark.parametrize("k,lds,zoff,loff", WRAP_PATHS, ids=["K%d_lds%d_z%d_l%d" % c for c in WRAP_PATHS])
def test_confusion_scores_when_the_grid_stride_loop_wraps(hip, k, lds, zoff, loff):
    # the wave-uniform counters (K <= 4) / the LDS histogram carry over several passes of one workgroup, the stride is the whole grid, and
    # the flush comes after the last pass -- the shape of every production launch (config 2: 2M pixels, 4 to 8 passes per workgroup)
    P = WRAP_P
    assert P > 2 * 1024 * 256 and P % 64 != 0 and ((P + 1) // 2) % 64 != 0
    z, lab, want = _scores_case(P, k, lds, seed=7 * k + lds)
    zb, zt = _offset_tensor(z, zoff // 4, torch.float32)
    lb, lt = _offset_tensor(lab, loff // 4, torch.int32)
    assert zt.data_ptr() % 16 == zoff and lt.data_ptr() % 16 == loff
    cm = torch.full((k, k), PREFILL, dtype=torch.int64, device="cuda")
    hip.unet_confusion_scores(_ptr(zt), lds, _ptr(lt), P, k, _ptr(cm), _stream())
    got = cm.cpu().numpy() - PREFILL
    assert got.sum() == P and np.array_equal(got, want), (k, lds, int(np.abs(got - want).sum()))


@pytest.mark.parametrize("k,lds", [(2, 2), (4, 4), (7, 8), (100, 100)])
def test_confusion_scores_accumulates_beyond_32_bits(hip, k, lds):
    cm = torch.full((k, k), PREFILL, dtype=torch.int64, device="cuda")
    total = np.full((k, k), PREFILL, np.int64)
    for P, seed in ((1000, 1), (333, 2)):
        z, lab, want = _scores_case(P, k, lds, seed)
        dz, dl = torch.from_numpy(z).cuda(), torch.from_numpy(lab).cuda()
        hip.unet_confusion_scores(_ptr(dz), lds, _ptr(dl), P, k, _ptr(cm), _stream())
        total += want
    assert np.array_equal(cm.cpu().numpy(), total) and total.max() > 2 ** 32


@pytest.mark.parametrize("k", [2, 3, 5])
def test_trace_is_the_accuracy_count_of_softmax_ce(hip, k):
    P = 5000
    z, lab, want = _scores_case(P, k, k, seed=40 + k)
    dz, dl = torch.from_numpy(z).cuda(), torch.from_numpy(lab).cuda()
    prob = torch.empty((P, k), device="cuda")
    out = torch.zeros(2, device="cuda")
    nb = hip.unet_softmax_ce_workspace(P)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    hip.unet_softmax_ce(_ptr(dz), k, _ptr(dl), _ptr(prob), None, 0, P, k, 0.0, 1.0 / P, 0.0, 0.0, _ptr(out[0:1]), _ptr(out[1:2]), _ptr(ws), nb, _stream())
    cm = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    hip.unet_confusion_scores(_ptr(dz), k, _ptr(dl), P, k, _ptr(cm), _stream())
    got = cm.cpu().numpy()
    assert np.array_equal(got, want)
    assert int(np.trace(got)) == int(out[1].item()) and got.sum() == P
    assert (lab.sum(-1) == 0).any() and 0 < np.trace(got) < P


# ---- class maps ----------------------------------------------------------------------------------------------------------------------
NP_ELEM = {1: np.uint8, 2: np.uint16, 4: np.int32}


def _to_dev(a):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def _mask_case(h, w, pitch, k, pe, te, ignore, seed):
    """pitched pred / truth arrays whose padding holds K - 1 (a kernel that ignores the pitch miscounts), truth with the ignore label,
    values >= K and, for int32, negative values; -> arrays, expected matrix, expected out-of-range count"""
    rng = np.random.default_rng(seed)
    top_p = min(k, 256 if pe == 1 else k)
    pred = np.full((h, pitch), min(k - 1, 255 if pe == 1 else k - 1), NP_ELEM[pe])
    truth = np.full((h, pitch), min(k - 1, 255 if te == 1 else k - 1), NP_ELEM[te])
    p = rng.integers(0, top_p, (h, w))
    t = rng.integers(0, min(k, 256 if te == 1 else k), (h, w))
    r = rng.random((h, w))
    if te > 1 or k < 250:
        t[r < 0.10] = k + rng.integers(0, 5)          # >= K: out of range
    if te == 4:
        t[(r >= 0.10) & (r < 0.18)] = -rng.integers(1, 4, (h, w))[(r >= 0.10) & (r < 0.18)]      # negative, -1 included
    if pe == 4:
        p[r > 0.97] = k + 1                           # a prediction outside the classes
    pred[:, :w] = p.astype(NP_ELEM[pe])
    truth[:, :w] = t.astype(NP_ELEM[te])
    p, t = pred[:, :w].astype(np.int64), truth[:, :w].astype(np.int64)
    keep = np.ones(t.shape, bool) if ignore == -1 else t != ignore
    inside = (t >= 0) & (t < k) & (p >= 0) & (p < k)
    return pred, truth, _count(t[keep & inside], p[keep & inside], k), int((keep & ~inside).sum())


MASK_TYPES = [(pe, te) for pe in (1, 4) for te in (1, 2, 4)]


@pytest.mark.parametrize("k", [2, 5, 300])
@pytest.mark.parametrize("pe,te", MASK_TYPES, ids=["pred%d_truth%d" % c for c in MASK_TYPES])
def test_confusion_masks_equals_numpy(hip, pe, te, k):
    # (K = 300 beside a uint8 map: that map holds classes 0..255 only, which is valid input)
    for w in (1, 5, 64, 67):
        for h, ignore in ((1, -1), (37, 1), (37, -1)):
            pitch = w + 3
            pred, truth, want, bad = _mask_case(h, w, pitch, k, pe, te, ignore, seed=w * 100 + h + k)
            dp, dt = _to_dev(pred), _to_dev(truth)
            cm = torch.zeros((k, k), dtype=torch.int64, device="cuda")
            oor = torch.zeros(1, dtype=torch.int64, device="cuda")
            hip.unet_confusion_masks(_ptr(dp), pe, pitch, _ptr(dt), te, pitch, h, w, k, ignore, _ptr(cm), _ptr(oor), _stream())
            got = cm.cpu().numpy()
            assert np.array_equal(got, want) and int(oor.item()) == bad, (pe, te, k, w, h, ignore, got.sum(), want.sum(), int(oor.item()), bad)
            cm.zero_()
            hip.unet_confusion_masks(_ptr(dp), pe, pitch, _ptr(dt), te, pitch, h, w, k, ignore, _ptr(cm), None, _stream())     # NULL accepted
            assert np.array_equal(cm.cpu().numpy(), want)
    if te > 1:
        assert bad > 0


def test_confusion_masks_large_image_accumulates(hip):
    # 300 x 1031: 303 workgroups, rows that end in a partial vector; the matrix and the counter are pre-filled and two launches add up
    k, h, w, pitch = 3, 300, 1031, 1040
    pred, truth, want, bad = _mask_case(h, w, pitch, k, 1, 1, 2, seed=5)
    cm = torch.full((k, k), PREFILL, dtype=torch.int64, device="cuda")
    oor = torch.full((1,), PREFILL, dtype=torch.int64, device="cuda")
    dp, dt = _to_dev(pred), _to_dev(truth)
    for _ in range(2):
        hip.unet_confusion_masks(_ptr(dp), 1, pitch, _ptr(dt), 1, pitch, h, w, k, 2, _ptr(cm), _ptr(oor), _stream())
    assert np.array_equal(cm.cpu().numpy(), PREFILL + 2 * want) and int(oor.item()) == PREFILL + 2 * bad and want[2].sum() == 0


WRAP_MASKS = [(2, 1, 1), (4, 1, 2), (5, 1, 2), (300, 4, 4)]      # (K, pred_elem, truth_elem): ballot (2- and 4-wide), LDS, direct


@pytest.mark.parametrize("k,pe,te", WRAP_MASKS, ids=["K%d_pred%d_truth%d" % c for c in WRAP_MASKS])
def test_confusion_masks_when_the_grid_stride_loop_wraps(hip, k, pe, te):
    # 1100 x 1031: 283800 four-column items > 1024 x 256, so 21656 threads make a second pass, which ends mid-wave; rows end in a partial vector
    h, w, pitch = 1100, 1031, 1048
    assert h * ((w + 3) // 4) > 1024 * 256 and (h * ((w + 3) // 4)) % 64 != 0
    pred, truth, want, bad = _mask_case(h, w, pitch, k, pe, te, 1, seed=k)
    dp, dt = _to_dev(pred), _to_dev(truth)
    cm = torch.zeros((k, k), dtype=torch.int64, device="cuda")
    oor = torch.zeros(1, dtype=torch.int64, device="cuda")
    hip.unet_confusion_masks(_ptr(dp), pe, pitch, _ptr(dt), te, pitch, h, w, k, 1, _ptr(cm), _ptr(oor), _stream())
    got = cm.cpu().numpy()
    assert np.array_equal(got, want) and int(oor.item()) == bad and bad > 0 and want[1].sum() == 0, (int(np.abs(got - want).sum()), int(oor.item()), bad)


def test_update_from_masks_takes_pitched_views_of_every_dtype(hip):
    # metrics.ConfusionMatrix.update_from_masks (what segment_image calls): the pitch from stride(0), uint16 truth as torch.int16 bits or
    # torch.uint16, a one-row map (whose stride(0) means nothing), accumulation over calls, the out-of-range counter
    metrics = pkg("metrics")
    k = 5
    cm = metrics.ConfusionMatrix(k, device="cuda:%d" % torch.cuda.current_device())
    total, total_bad = np.zeros((k, k), np.int64), 0
    cases = [(37, 67, 80, 1, 1, -1), (37, 67, 72, 4, 4, 2), (37, 64, 64, 1, 2, 2), (1, 53, 60, 4, 2, -1), (1, 1, 4, 1, 4, 0)]
    for n, (h, w, pitch, pe, te, ignore) in enumerate(cases):
        pred, truth, want, bad = _mask_case(h, w, pitch, k, pe, te, ignore, seed=50 + n)
        dp, dt = _to_dev(pred)[:, :w], _to_dev(truth)[:, :w]             # views of the pitched allocations
        assert (h == 1 or dp.stride(0) == pitch) and (pitch == w or not dp.is_contiguous() or h == 1)
        cm.update_from_masks(dp, dt, ignore_label=ignore)
        if te == 2 and hasattr(torch, "uint16"):                          # the same bits under torch's own uint16: counted a second time
            cm.update_from_masks(dp, dt.view(torch.uint16), ignore_label=ignore)
            want, bad = 2 * want, 2 * bad
        total += want
        total_bad += bad
        assert np.array_equal(cm.result(), total) and int(cm.out_of_range.item()) == total_bad, (n, cm.result(), total)
    assert total_bad > 0 and (total > 0).sum() > k
    # host tensors, wrong dtypes and wrong shapes are refused in Python: nothing reaches the kernel
    before = cm.result()
    dp, dt = torch.zeros((4, 4), dtype=torch.uint8, device="cuda"), torch.zeros((4, 4), dtype=torch.uint8, device="cuda")
    for bad_pred, bad_truth in ((dp.cpu(), dt), (dp, dt.cpu()), (dp.to(torch.int16), dt), (dp, dt.float()), (dp[:3], dt), (dp.t(), dt.t()), (np.zeros((4, 4), np.uint8), dt)):
        with pytest.raises(ValueError):
            cm.update_from_masks(bad_pred, bad_truth)
    z, lab = torch.zeros((8, k), device="cuda"), torch.zeros((8, k), dtype=torch.int32, device="cuda")
    for bad_z, bad_lab in ((z.cpu(), lab), (z, lab.cpu()), (z.double(), lab), (z[:, :4], lab[:, :4]), (z, lab[:4])):
        with pytest.raises(ValueError):
            cm.update_from_scores(bad_z, bad_lab)
    assert np.array_equal(cm.result(), before)
    # ... and a leading dimension is read from a channel slice
    wide = torch.full((8, k + 3), 9.0, device="cuda")
    wide[:, :k] = 0.0
    wide[:, 2] = 1.0
    lab[:, 4] = 1
    cm.update_from_scores(wide[:, :k], lab)
    after = cm.result() - before
    assert after[4, 2] == 8 and after.sum() == 8


def test_bad_arguments_are_refused_before_any_launch(hip):
    raw_s, raw_m = hip.cdll.unet_confusion_scores, hip.cdll.unet_confusion_masks
    z = torch.zeros((64, 4), device="cuda")
    lab = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    cmb = torch.zeros(4 * 1025 * 1025 // 4 + 8, dtype=torch.int64, device="cuda")
    m8 = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    st = _stream()
    EINVAL = -1
    assert raw_s(_ptr(z), 4, _ptr(lab), 64, 0, _ptr(cmb), st) == EINVAL                        # K = 0
    assert raw_s(_ptr(z), 4, _ptr(lab), 64, 1025, _ptr(cmb), st) == EINVAL                     # K = 1025
    assert raw_s(_ptr(z), 3, _ptr(lab), 64, 4, _ptr(cmb), st) == EINVAL                        # lds < K
    assert raw_s(_ptr(z), 4, _ptr(lab), 64, 4, ctypes.c_void_p(cmb.data_ptr() + 4), st) == EINVAL      # misaligned cm
    assert raw_s(_ptr(z), 4, _ptr(lab), 0, 4, _ptr(cmb), st) == EINVAL                         # P = 0
    assert raw_s(None, 4, _ptr(lab), 64, 4, _ptr(cmb), st) == EINVAL
    assert raw_m(_ptr(m8), 1, 8, _ptr(m8), 3, 8, 8, 8, 2, -1, _ptr(cmb), None, st) == EINVAL   # truth_elem = 3
    assert raw_m(_ptr(m8), 2, 8, _ptr(m8), 1, 8, 8, 8, 2, -1, _ptr(cmb), None, st) == EINVAL   # pred_elem = 2
    assert raw_m(_ptr(m8), 1, 7, _ptr(m8), 1, 8, 8, 8, 2, -1, _ptr(cmb), None, st) == EINVAL   # pitch < W
    assert raw_m(_ptr(m8), 1, 8, _ptr(m8), 1, 8, 8, 8, 0, -1, _ptr(cmb), None, st) == EINVAL   # K = 0
    assert raw_m(_ptr(m8), 1, 8, _ptr(m8), 1, 8, 8, 8, 2, -1, ctypes.c_void_p(cmb.data_ptr() + 4), None, st) == EINVAL
    assert raw_m(_ptr(m8), 1, 8, _ptr(m8), 1, 8, 8, 8, 2, -1, _ptr(cmb), ctypes.c_void_p(cmb.data_ptr() + 12), st) == EINVAL
    torch.cuda.synchronize()
    assert not cmb.any()                                                                       # nothing was launched
    with pytest.raises(pkg("_lib").UnetHipError, match="bad argument"):
        hip.unet_confusion_scores(_ptr(z), 4, _ptr(lab), 64, 0, _ptr(cmb), st)


# ---- engine --------------------------------------------------------------------------------------------------------------------------
ENGINE_CASES = [(2, 2, 1, 32, 32, None), (2, 2, 1, 32, 32, "bf16"), (3, 1, 3, 16, 48, None), (3, 1, 3, 16, 48, "bf16")]


def _batch(k, n, c, h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((n, c, h, w)).astype(np.float32)
    lab = np.zeros((n, h, w, k), np.int32)
    cls = rng.integers(0, k, (n, h, w))
    np.put_along_axis(lab, cls[..., None], 1, axis=-1)
    lab[0, 0, :3] = 0                                 # three all-zero rows: class 0
    return img, lab


@pytest.mark.parametrize("k,n,c,h,w,cd", ENGINE_CASES, ids=["K%d_%dx%dx%dx%d_%s" % (k, n, c, h, w, cd or "fp32") for k, n, c, h, w, cd in ENGINE_CASES])
def test_test_step_accumulates_the_confusion_matrix(k, n, c, h, w, cd):
    model, metrics = pkg("model"), pkg("metrics")
    net = model.UNet(k, n, c, seed=1, compute_dtype=cd)
    e = net.engine
    cm = metrics.ConfusionMatrix(k, device=e.dev)
    acc = model.CategoricalAccuracy()
    total = np.zeros((k, k), np.int64)
    for step in range(2):
        img, lab = _batch(k, n, c, h, w, seed=10 * k + step)
        net.test_step((img, lab, None, acc), confusion=cm)
        logits = e.bufs["y_logits"].cpu().numpy().reshape(-1, k)
        total += _count(np.argmax(lab.reshape(-1, k), axis=-1), np.argmax(logits, axis=-1), k)
        got = cm.result()
        assert np.array_equal(got, total), (step, got, total)
        assert int(np.trace(got)) == int(acc.total) and got.sum() == (step + 1) * n * h * w
    assert (total > 0).sum() >= 2                     # not one cell
    # the train step takes the keyword too (a training-set matrix)
    tcm = metrics.ConfusionMatrix(k, device=e.dev)
    tacc = model.CategoricalAccuracy()
    img, lab = _batch(k, n, c, h, w, seed=99)
    net.train_step((img, lab, None, tacc), confusion=tcm)
    assert int(np.trace(tcm.result())) == int(tacc.total) and tcm.result().sum() == n * h * w


def test_without_a_matrix_the_step_launches_nothing_new(hip, monkeypatch):
    model, metrics = pkg("model"), pkg("metrics")
    net = model.UNet(2, 2, 1, seed=1)
    e = net.engine
    calls = []
    for name in ("unet_confusion_scores", "unet_confusion_masks"):
        orig = getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _o=orig, _n=name: (calls.append(_n), _o(*a))[1])
    img, lab = _batch(2, 2, 1, 32, 32, seed=3)

    def recorded(**kw):
        e.profile = {}
        try:
            net.test_step((img, lab, None, None), **kw)
            torch.cuda.synchronize()
            return {key: len(v) for key, v in e.profile.items()}
        finally:
            e.profile = None
    plain = recorded()
    assert calls == [] and not any("confusion" in key for key in plain)
    assert recorded(confusion=None) == plain and calls == []
    with_cm = recorded(confusion=metrics.ConfusionMatrix(2, device=e.dev))
    assert calls == ["unet_confusion_scores"]
    assert with_cm == dict(plain, confusion=1)        # the same launches plus exactly one
    net.train_step((img, lab, None, None))
    net.dist_test_step(None, (img, lab, None, None))
    assert calls == ["unet_confusion_scores"]


# ---- inference -----------------------------------------------------------------------------------------------------------------------
def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 0.5 + 0.3 * np.sin(yy / 5.0) * np.cos(xx / 4.0) + 0.1 * rng.standard_normal((h, w))
    return (np.clip(v, 0.0, 1.0) * 60000.0).astype(np.uint16)


_NET = {}


def _net():
    if "n" not in _NET:
        _NET["n"] = pkg("model").UNet(2, 1, 1, seed=0)
    return _NET["n"]


@pytest.mark.parametrize("hw,tdt", [((40, 52), np.uint8), ((80, 1056), np.uint16), ((40, 52), np.int64)], ids=["40x52_u8", "80x1056_u16", "40x52_i64"])
def test_segment_image_scores_its_mask_on_the_device(hw, tdt, monkeypatch):
    inf, metrics = pkg("inference"), pkg("metrics")
    net = _net()
    monkeypatch.setattr(net, "estimate_radius", lambda: 16, raising=False)
    h, w = hw
    tile = 64 if w > 64 else 1024                     # 80 x 1056 at tile 64, radius 16: 3 x 33 tiles; 40 x 52: one tile, reflect-padded to 48 x 64
    raw = _image(h, w, seed=h)
    rng = np.random.default_rng(w)
    truth = rng.integers(0, 2, (h, w)).astype(tdt)
    truth[rng.random((h, w)) < 0.05] = 3              # out of range
    truth[rng.random((h, w)) < 0.05] = 7              # ignored
    plain = inf.segment_image(raw, net, tile_size=tile)
    cm = metrics.ConfusionMatrix(2, device=net.engine.dev)
    got = inf.segment_image(raw, net, tile_size=tile, truth=truth, confusion=cm, ignore_label=7)
    assert np.array_equal(got, plain) and got.dtype == plain.dtype
    assert len(np.unique(plain)) == 2                 # a flat mask would prove little
    t = truth.astype(np.int64)
    ok = (t >= 0) & (t < 2)
    want = _count(t[ok], plain[ok], 2)
    assert np.array_equal(cm.result(), want) and int(cm.out_of_range.item()) == int((t == 3).sum())
    host = metrics.ConfusionMatrix(2, device=net.engine.dev)
    hmask = inf._segment_host_pipeline(raw, net, tile, truth=truth, confusion=host, ignore_label=7)
    assert np.array_equal(hmask, plain)
    assert np.array_equal(host.result(), want) and int(host.out_of_range.item()) == int((t == 3).sum())
    with pytest.raises(ValueError):
        inf.segment_image(raw, net, tile_size=tile, truth=truth[:-1], confusion=cm)
    with pytest.raises(ValueError):
        inf.segment_image(raw, net, tile_size=tile, truth=truth)
    with pytest.raises(ValueError, match="device"):                       # a host matrix would hand the kernel host pointers
        inf.segment_image(raw, net, tile_size=tile, truth=truth, confusion=metrics.ConfusionMatrix(2, device="cpu"))
    with pytest.raises(ValueError, match="classes"):
        inf.segment_image(raw, net, tile_size=tile, truth=truth, confusion=metrics.ConfusionMatrix(3, device=net.engine.dev))
    assert np.array_equal(cm.result(), want)


def test_cli_writes_scores_and_the_summed_matrix(tmp_path):
    inf, metrics = pkg("inference"), pkg("metrics")
    net = _net()
    stem = str(tmp_path / "checkpoint" / "ckpt")
    net.save_checkpoint(stem)
    imgs, masks = tmp_path / "imgs", tmp_path / "masks"
    imgs.mkdir(); masks.mkdir()
    rng = np.random.default_rng(0)
    shapes = {"a.npy": (70, 83), "b.npy": (40, 40)}
    for name, (h, w) in shapes.items():
        np.save(imgs / name, _image(h, w, seed=h))
        np.save(masks / name, rng.integers(0, 2, (h, w)).astype(np.uint8))
    common = ["--checkpoint_filepath", stem, "--image_folder", str(imgs), "--number_classes", "2", "--number_channels", "1", "--image_format", "npy"]
    inf.main(common + ["--output_folder", str(tmp_path / "plain")])
    assert sorted(os.listdir(tmp_path / "plain")) == ["a.npy", "b.npy"]
    for out, extra in (("dev", []), ("host", ["--host_pipeline"])):
        inf.main(common + ["--output_folder", str(tmp_path / out), "--mask_folder", str(masks)] + extra)
        assert sorted(os.listdir(tmp_path / out)) == ["a.npy", "b.npy", "confusion.npy", "scores.csv"]
        total, rows = np.zeros((2, 2), np.int64), [metrics.csv_header("image", 2)]
        for name in sorted(shapes):
            assert open(tmp_path / out / name, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
            c = _count(np.load(masks / name), np.load(tmp_path / out / name), 2)
            total += c
            rows.append(metrics.csv_row(name, metrics.summarize(c)))
        saved = np.load(tmp_path / out / "confusion.npy")
        assert saved.dtype == np.int64 and np.array_equal(saved, total)
        cm = metrics.ConfusionMatrix(2, device="cpu")
        cm.add_counts(total)
        s = cm.summary()
        rows.append(",".join(["total"] + [repr(float(v)) for v in [s["pixel_accuracy"], s["mean_iou"], *s["iou"], *s["dice"]]]))
        assert open(tmp_path / out / "scores.csv").read() == "\n".join(rows) + "\n"
