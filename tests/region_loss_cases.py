"""The region term of the training loss in fp64 numpy -- the semantics `unet_region_loss_sums` / `unet_region_loss_bwd` are held to -- the
same in the device's operation order in fp32 (the error budget of the kernel tests), and the seeded cases of its tests.

p = softmax(z); y = the hard one-hot row (first maximum of the label row; an all-zero row is class 0, or with ignore_empty an unlabeled pixel
with m_p = 0).  Per image n and class k, over the pixels of that image:

    I = sum m p_k y_k      S = sum m p_k      Y = sum m y_k
    D = (1 - alpha - beta) I + alpha S + beta Y + s          T = (I + s) / D            (alpha = beta = 0.5: soft Dice)
    region = scale * sum_n sum_k c~_k (1 - T_nk),            c~ = class_weight / sum(class_weight)  (None: 1 / K)
    g_pk = -scale c~_k m_p (A_nk y_pk + B_nk),   A = 1 / D - (I + s)(1 - alpha - beta) / D^2,   B = -alpha (I + s) / D^2
    dz_pj = p_pj (g_pj - sum_k p_pk g_pk)

(No GPU here: test_region_loss_reference.py checks this file against torch autograd in fp64.)"""
import numpy as np


def _masks(lab, ignore_empty):
    lab = np.asarray(lab)
    y = (np.argmax(lab, axis=-1)[:, None] == np.arange(lab.shape[1])).astype(np.float64)        # first maximum
    m = (lab.max(axis=-1) > 0).astype(np.float64) if ignore_empty else np.ones(lab.shape[0])
    return y, m


def _weights(class_weight, K):
    c = np.ones(K) if class_weight is None else np.asarray(class_weight, dtype=np.float64)
    return c / c.sum()


def region_loss(z, lab, N, HW, alpha=0.5, beta=0.5, smooth=1.0, scale=1.0, class_weight=None, ignore_empty=False):
    """z [N * HW, K] logits, lab [N * HW, K] one-hot integers -> dict(prob [P, K], dlogits [P, K] (the region term's share), loss,
    tbar [K] (mean of T over the images), T [N, K]), all fp64"""
    z = np.asarray(z, dtype=np.float64)
    K = z.shape[1]
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    y, m = _masks(lab, ignore_empty)
    ct = _weights(class_weight, K)
    p3, y3, m3 = p.reshape(N, HW, K), y.reshape(N, HW, K), m.reshape(N, HW, 1)
    I, S, Y = (m3 * p3 * y3).sum(1), (m3 * p3).sum(1), (m3 * y3).sum(1)
    r = 1.0 - alpha - beta
    D = r * I + alpha * S + beta * Y + smooth
    T = (I + smooth) / D
    A = 1.0 / D - (I + smooth) * r / D ** 2
    B = -alpha * (I + smooth) / D ** 2
    g = -scale * ct * m3 * (A[:, None, :] * y3 + B[:, None, :])
    dz = p3 * (g - (p3 * g).sum(-1, keepdims=True))
    return {"prob": p, "dlogits": dz.reshape(-1, K), "loss": float(scale * (ct * (1.0 - T)).sum()), "tbar": T.mean(0), "T": T}


def region_loss_device_order(z, lab, N, HW, alpha=0.5, beta=0.5, smooth=1.0, scale=1.0, class_weight=None, ignore_empty=False):
    """The same in the kernels' arithmetic: fp32 softmax, sums / T / coefficients in double FROM the fp32 probabilities and the fp32 settings,
    coefficients rounded to fp32, the backward expression in fp32 operation by operation -> dict(dlogits fp32, loss fp32, tbar fp32)"""
    f = np.float32
    z = np.asarray(z, dtype=f)
    K = z.shape[1]
    e = np.exp(z - z.max(axis=-1, keepdims=True), dtype=f)
    p = (e * (f(1) / e.sum(axis=-1, keepdims=True, dtype=f))).astype(f)
    y, m = _masks(lab, ignore_empty)
    a, b, s, sc = (float(f(v)) for v in (alpha, beta, smooth, scale))
    ct = _weights(None if class_weight is None else np.asarray(class_weight, dtype=f), K)
    p3, y3, m3 = p.astype(np.float64).reshape(N, HW, K), y.reshape(N, HW, K), m.reshape(N, HW, 1)
    I, S, Y = (m3 * p3 * y3).sum(1), (m3 * p3).sum(1), (m3 * y3).sum(1)
    r = 1.0 - a - b
    D = r * I + a * S + b * Y + s
    T = (I + s) / D
    cA = (-sc * ct * (1.0 / D - (I + s) * r / D ** 2)).astype(f)
    cB = (-sc * ct * (-a * (I + s) / D ** 2)).astype(f)
    pf, yf = p.reshape(N, HW, K), y3.astype(f)
    g = np.where(yf > 0, cA[:, None, :] + cB[:, None, :], cB[:, None, :]).astype(f)
    dot = np.zeros((N, HW), f)
    for k in range(K):
        dot = (dot + pf[..., k] * g[..., k]).astype(f)
    dz = (pf * (g - dot[..., None])).astype(f) * m3.astype(f)
    return {"dlogits": dz.reshape(-1, K), "loss": f(sc * (ct * (1.0 - T)).sum()), "tbar": (T.mean(0)).astype(f)}


def make_case(N, HW, K, seed):
    """-> z fp32 [N * HW, K], lab int32 [N * HW, K], class_weight fp32 [K], built like weighted_loss_cases.make_case: logits uniform in
    [-3, 3]; ~2 % extreme pixels with a logit gap of 40; ~10 % unlabeled rows (at least one whenever N * HW >= 16); class weights in
    [0.25, 4] with one exactly 0; and in image 0 the class K - 1 absent from the labels (K >= 2)."""
    P = N * HW
    rng = np.random.default_rng([seed, N, HW, K])
    z = rng.uniform(-3.0, 3.0, (P, K))
    cls = rng.integers(0, K, P)
    if K >= 2:
        first = cls[:HW]
        first[first == K - 1] = rng.integers(0, K - 1, (first == K - 1).sum())
    few = lambda frac: rng.choice(P, max(1, int(round(frac * P))), replace=False) if P >= 16 else np.zeros(0, dtype=np.int64)
    ext = few(0.02)
    z[ext] = -20.0
    z[ext, rng.integers(0, K, ext.size)] = 20.0
    lab = (cls[:, None] == np.arange(K)).astype(np.int32)
    lab[few(0.10)] = 0
    cw = rng.uniform(0.25, 4.0, K)
    if K >= 2:
        cw[rng.integers(0, K)] = 0.0
    return z.astype(np.float32), lab, cw.astype(np.float32)


def f32(v):
    """a setting as the C ABI receives it (a float argument)"""
    return float(np.float32(v))


TVERSKY = [(0.5, 0.5), (0.3, 0.7), (1.0, 1.0)]
