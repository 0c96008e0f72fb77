"""The weighted training loss in fp64 numpy -- the semantics `unet_softmax_ce_weighted` is held to -- and the seeded cases of its tests.

Per pixel p, with t_p = first maximum of its one-hot row and l_p the unweighted cross-entropy (label smoothing, and with clip_eps > 0
Keras' clipped-probability path):

    w_p  = class_weight[t_p] * pixel_weight[p]          (a missing factor is 1)
    loss = loss_scale * sum_p w_p * l_p
    dlogits[p][k] = (unweighted d l_p / d z_pk) * grad_scale * w_p

With ignore_empty a pixel whose one-hot row has no positive entry is unlabeled: no loss, a zero dlogits row, not counted in `correct` or
`valid`; without it such a row is class 0, as in `unet_softmax_ce`.  The reduction is not divided by the weight sum; `weight_sum` (over the
valid pixels) is reported.  (No GPU here: test_weighted_loss_reference.py checks this file against torch autograd in fp64.)"""
import numpy as np


def weighted_ce(z, lab, class_weight=None, pixel_weight=None, ignore_empty=False, label_smoothing=0.0, loss_scale=1.0, grad_scale=1.0,
                clip_eps=0.0):
    """z [P, K] logits, lab [P, K] one-hot integers -> dict(prob [P, K], dlogits [P, K], loss, correct, valid, weight_sum), all fp64"""
    z = np.asarray(z, dtype=np.float64)
    lab = np.asarray(lab)
    P, K = z.shape
    zs = z - z.max(axis=-1, keepdims=True)
    e = np.exp(zs)
    p = e / e.sum(axis=-1, keepdims=True)
    t = np.argmax(lab, axis=-1)                                  # first maximum
    labeled = (lab.max(axis=-1) > 0) if ignore_empty else np.ones(P, dtype=bool)
    y = lab.astype(np.float64)
    if label_smoothing:
        y = y * (1.0 - label_smoothing) + label_smoothing / K
    if clip_eps:
        ell = -(y * np.log(np.clip(p, clip_eps, 1.0 - clip_eps))).sum(axis=-1)
        gp = np.where((p >= clip_eps) & (p <= 1.0 - clip_eps), -y, 0.0)           # g_k p_k: the clip passes no gradient outside its range
        d = gp - p * gp.sum(axis=-1, keepdims=True)
    else:
        ell = -(y * (zs - np.log(e.sum(axis=-1, keepdims=True)))).sum(axis=-1)
        d = p * y.sum(axis=-1, keepdims=True) - y
    w = np.ones(P)
    if class_weight is not None:
        w = w * np.asarray(class_weight, dtype=np.float64)[t]
    if pixel_weight is not None:
        w = w * np.asarray(pixel_weight, dtype=np.float64)
    w = np.where(labeled, w, 0.0)
    return {"prob": p, "dlogits": d * grad_scale * w[:, None], "loss": float(loss_scale * (w * ell).sum()),
            "correct": int((labeled & (t == np.argmax(z, axis=-1))).sum()), "valid": int(labeled.sum()), "weight_sum": float(w.sum())}


def make_case(P, K, seed):
    """-> z fp32 [P, K], lab int32 [P, K], class_weight fp32 [K], pixel_weight fp32 [P].
    Logits uniform in [-3, 3]: every probability far inside the clip range [1e-7, 1 - 1e-7]; ~2 % EXTREME pixels with a logit gap of 40
    (p < 1e-17, 1 - p rounds to 1) so that the clip path's outside branches run with no pixel near a clip edge; ~10 % unlabeled rows (at least
    one whenever P >= 16); class weights in [0.25, 4] with one exactly 0; pixel weights in [0, 2] with ~5 % exactly 0."""
    rng = np.random.default_rng([seed, P, K])
    z = rng.uniform(-3.0, 3.0, (P, K))
    cls = rng.integers(0, K, P)
    few = lambda frac: rng.choice(P, max(1, int(round(frac * P))), replace=False) if P >= 16 else np.zeros(0, dtype=np.int64)
    ext = few(0.02)
    z[ext] = -20.0
    z[ext, rng.integers(0, K, ext.size)] = 20.0
    lab = (cls[:, None] == np.arange(K)).astype(np.int32)
    lab[few(0.10)] = 0
    cw = rng.uniform(0.25, 4.0, K)
    cw[rng.integers(0, K)] = 0.0
    pw = rng.uniform(0.0, 2.0, P)
    pw[few(0.05)] = 0.0
    return z.astype(np.float32), lab, cw.astype(np.float32), pw.astype(np.float32)


# the option sets of the kernel test: (name, class weights, pixel weights, ignore, label smoothing, clip)
OPTIONS = [("class", True, False, False, 0.0, 0.0), ("pixel", False, True, False, 0.0, 0.0), ("ignore", False, False, True, 0.0, 0.0),
           ("all", True, True, True, 0.0, 0.0), ("all_smooth", True, True, True, 0.1, 0.0), ("all_clip", True, True, True, 0.0, 1e-7)]
