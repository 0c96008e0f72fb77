"""BatchNorm on ill-conditioned channels, every kernel against fp64 (tests/bn_conditioning_cases.py holds the ladder, the references and the
one-pass fp32 floor; tests/test_bn_conditioning_reference.py checks those on the CPU).

Channel c of every tensor here sits on rung c % 8 of the conditioning ladder: relu(randn), mean/sigma = 10, 100, 1000, a constant, a dead
channel, var << eps, raw-pixel scale.  The bounds are derived, none is read off the kernels (u = 2^-24):

  a. unet_bn_train_stats accumulates exact fp32 inputs in fp64: kappa'-independent, 2u / 4u;
  b. statistics finalized from a producer's fp32 partial sums: <= 8 x the one-pass fp32 floor of the SAME stored tensor with the kernel's
     own row count, + (a).  8 = 4 (a row of ~128 terms summed sequentially against pairwise: sqrt(128) / sqrt(7) of a random-walk error)
     x 2 (two samples of that error).  The constant rung's rounding errors do not walk randomly (every lane makes the same ones), so one
     sampled order is no floor for another: it gets the design's a-priori bound once instead (bc.constant_channel_floor);
  c. y = fma(scale, r, shift): 2u (|scale r| + |shift|) per element from the device's own scale / shift;
  d. backward sums: standalone kernels subtract the mean before multiplying -- 4u sum|dy|, 8u invstd sum|dy (r - mean)|; from a data
     gradient's partials <= 8 x floor + that;
  e. dz = A dy + B r + K: (1 + 9 roundings) u (|A dy| + |B r| + |K|) per element from the device's own fp32 per-channel values (the nine
     roundings are listed at bn_conditioning_cases.DZ_ROUNDINGS); dbias 4u sum|dz|.

Every assertion names family, shape, rung, measured error and bound; every check also prints its worst error / bound ratio (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import bn_conditioning_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = bc.U
P_ = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a).astype(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def flat(t):
    """device NHWC (any channel slice) -> [P, C] numpy, the dtype it is stored in"""
    return host(t.reshape(-1, t.shape[-1]))


def ws_bytes(n):
    return torch.empty(int(n) + 256, dtype=torch.uint8, device=DEV)


def check(family, shape, what, err, bound, rungs=None):
    """err <= bound element-wise ([C] or [P, C]); the message names the worst channel's rung."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    assert np.isfinite(err).all(), "%s %s %s: NaN/Inf in the device result" % (family, shape, what)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    c = i[-1]
    rung = (rungs if rungs is not None else bc.rung_of(err.shape[-1]))[c]
    print("RATIO %-34s %-22s %-8s worst err/bound %.3f (rung %d, err %.3e, bound %.3e)" % (family, shape, what, ratio[i], rung, err[i], bound[i]))
    assert ratio[i] <= 1.0, "%s shape %s: %s on rung %d (%s), channel %d: error %.4e > bound %.4e" % (
        family, shape, what, rung, bc.RUNGS[rung][0], c, err[i], bound[i])


class Coef:
    """per-channel device vectors (each its own allocation: 16-byte aligned for the vector kernels)"""

    def __init__(self, C, gamma, beta, mm0, mv0):
        self.C = C
        pad = lambda a: dev(np.concatenate([np.asarray(a, np.float32), np.zeros((-C) % 8, np.float32)]))
        self.gamma, self.beta, self.mm, self.mv = pad(gamma), pad(beta), pad(mm0), pad(mv0)
        self.mean, self.invstd, self.scale, self.shift = (torch.full_like(self.gamma, float("nan")) for _ in range(4))

    def stats(self):
        return {k: host(getattr(self, k))[:self.C] for k in ("mean", "invstd", "scale", "shift", "mm", "mv")}


def bn_stats(hip, rv, ld, P, co):
    nb = hip.unet_bn_workspace(P, co.C); ws = ws_bytes(nb)
    hip.unet_bn_train_stats(P_(rv), ld, P, co.C, P_(co.gamma), P_(co.beta), bc.EPS, bc.MOMENTUM, 1, P_(co.mm), P_(co.mv),
                            P_(co.mean), P_(co.invstd), P_(co.scale), P_(co.shift), P_(ws), nb, ST())
    return co.stats()


def assert_stats(family, shape, got, ref, beta, extra=None, rung0_tight=False, const=None):
    """extra: the sampled one-pass floor (x 8); const: the a-priori floor of the constant channels (x 1), bc.constant_channel_floor"""
    e, bound = bc.stat_errors(got, ref), bc.stat_floor_standalone(ref, beta)
    C = len(ref["mean"])
    k = bc.rung_of(C)
    for key in bc.STAT_KEYS:
        b = bound[key] + (8.0 * extra[key] if extra is not None else 0.0) + (const[key] if const is not None else 0.0)
        check(family, shape, key, e[key], b)
        if rung0_tight:                                          # rung 0: 2e-6 relative whatever the floor says
            scale0 = {"mean": np.abs(ref["mean"]), "shift": np.abs(beta.astype(np.float64)) + np.abs(ref["mean"] * ref["scale"])}.get(key, 1.0)
            check(family, shape, key + "@r0", np.where(k == 0, e[key], 0.0), 2e-6 * scale0)
    # moving mean: 4u relative; from partials + the mean's own floor scaled by (1 - momentum)
    check(family, shape, "mm", np.abs(got["mm"] - ref["mm"]),
          4 * U * np.abs(ref["mm"]) + (1 - bc.MOMENTUM) * ((8.0 * extra["mean"] if extra is not None else 0.0) + (const["mean"] if const is not None else 0.0)))
    # constant and dead rungs: the clamped variance gives invstd <= 1/sqrt(eps), and a dead channel's sums are exactly zero
    top = float(np.float32(1 / np.sqrt(bc.EPS))) * (1 + 2 * U)
    c = int(np.argmax(got["invstd"]))
    assert got["invstd"][c] <= top, "%s shape %s: invstd on rung %d (%s), channel %d: %.9g > 1/sqrt(eps) = %.9g (negative variance not clamped?)" % (
        family, shape, k[c], bc.RUNGS[k[c]][0], c, got["invstd"][c], top)
    assert (got["mean"][k == 5] == 0).all(), "%s %s: dead rung mean not exactly 0" % (family, shape)


# ---- a. / c. / d. / e. standalone kernels ---------------------------------------------------------------------------------------------

N, H, W = 3, 10, 14
STANDALONE = [(64, 0), (6, 0), (72, 0), (64, 16)]         # C, extra leading dimension (r, y, dy, dz as channel slices of wider buffers)


def standalone_case(C, extra):
    P = N * H * W
    r = bc.ladder_tensor(P, C, 100 + C)
    dy = np.random.default_rng(200 + C).standard_normal((P, C)).astype(np.float32)
    gamma, beta, mm0, mv0 = bc.bn_params(C, 300 + C)
    ld = C + extra
    off = 8 if extra else 0

    def sliced(a):
        buf = torch.full((N, H, W, ld), float("nan"), device=DEV)
        buf[..., off:off + C] = dev(a).view(N, H, W, C)
        return buf, buf[..., off:off + C]
    return P, r, dy, gamma, beta, mm0, mv0, ld, sliced


@pytest.mark.parametrize("C,extra", STANDALONE)
def test_standalone_statistics_and_apply(hip, C, extra):
    P, r, dy, gamma, beta, mm0, mv0, ld, sliced = standalone_case(C, extra)
    shape = (N, H, W, C, "ld%d" % ld)
    rbuf, rv = sliced(r)
    co = Coef(C, gamma, beta, mm0, mv0)
    got = bn_stats(hip, rv, ld, P, co)
    ref = bc.ref_forward(r, gamma, beta, mm0, mv0)
    assert_stats("unet_bn_train_stats", shape, got, ref, beta, rung0_tight=True)
    # c. apply, against fp64 from the device's own fp32 scale / shift
    sc, sh = got["scale"].astype(np.float64), got["shift"].astype(np.float64)
    sr = sc * r.astype(np.float64)
    y64, ybound = sr + sh, 2 * U * (np.abs(sr) + np.abs(sh))
    ybuf, yv = sliced(np.zeros_like(r))
    hip.unet_bn_apply(P_(rv), ld, P_(co.scale), P_(co.shift), P_(yv), ld, P, C, ST())
    check("unet_bn_apply", shape, "y", np.abs(flat(yv) - y64), ybound)
    if extra:
        assert torch.isnan(ybuf[..., :8]).all() and torch.isnan(ybuf[..., 8 + C:]).all(), "unet_bn_apply wrote outside its channel slice"
    if C % 4 == 0:                   # unet_bn_apply_any refuses C % 4 != 0 (its argument check in semantic-segmentation-unet_amd/csrc/norm.hip): no C = 6 case
        y2buf, y2v = sliced(np.zeros_like(r))
        hip.unet_bn_apply_any(P_(rv), ld, 0, P_(co.scale), P_(co.shift), P_(y2v), ld, 0, None, 0, None, N, H, W, C, ST())
        check("unet_bn_apply_any", shape, "y", np.abs(flat(y2v) - y64), ybound)
    # the pooled forms need C % 4 == 0 and a lane layout that tiles a 256-thread block (launch_bn_apply, semantic-segmentation-unet_amd/csrc/norm.hip: C / 8 or C / 4
    # lanes per pixel must divide 256, else UNET_EINVAL), which refuses C = 6 and C = 72: C = 64 is the only size of this set they take
    if C == 64:
        for name in ("unet_bn_apply_maxpool", "unet_bn_apply_any+pool"):
            y3buf, y3v = sliced(np.zeros_like(r))
            pooled = torch.full((N, H // 2, W // 2, C), float("nan"), device=DEV)
            idx = torch.full((N, H // 2, W // 2, C), 255, dtype=torch.uint8, device=DEV)
            if name == "unet_bn_apply_maxpool":
                hip.unet_bn_apply_maxpool(P_(rv), ld, P_(co.scale), P_(co.shift), P_(y3v), ld, P_(pooled), C, P_(idx), N, H, W, C, ST())
            else:
                hip.unet_bn_apply_any(P_(rv), ld, 0, P_(co.scale), P_(co.shift), P_(y3v), ld, 0, P_(pooled), C, P_(idx), N, H, W, C, ST())
            yd = flat(y3v)
            check(name, shape, "y", np.abs(yd - y64), ybound)
            # pooled = the max of the device's own y, bit for bit; first-max index; constant / dead rungs tie four ways -> index 0
            win = yd.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)
            assert np.array_equal(host(pooled), win.max(3)), "%s %s: pooled is not the maximum of the stored y" % (name, shape)
            assert np.array_equal(host(idx), win.argmax(3).astype(np.uint8)), "%s %s: index is not the first maximum" % (name, shape)
            k = bc.rung_of(C)
            assert (host(idx)[..., (k == 4) | (k == 5)] == 0).all(), "%s %s: tie on the constant / dead rung not resolved to position 0" % (name, shape)


def assert_backward(family, shape, out, dy, r, gamma, mean, invstd, relu, fsum=None):
    """d. and e. for one backward call: out = (dz [P, C], dgamma, dbeta, dbias) as numpy, mean / invstd the fp32 values the kernel was given"""
    dz, dg, db, dbias = out
    C = r.shape[1]
    k = bc.rung_of(C)
    sums = bc.ref_backward_sums(dy, r, mean, invstd)
    check(family, shape, "dbeta", np.abs(db - sums["dbeta"]), 4 * U * sums["abs_dy"] + (8.0 * fsum["dbeta"] if fsum else 0.0))
    check(family, shape, "dgamma", np.abs(dg - sums["dgamma"]), 8 * U * sums["abs_t"] + (8.0 * fsum["dgamma"] if fsum else 0.0))
    dz64, mag = bc.ref_dz(dy, r, gamma, mean, invstd, dg, db, relu)
    check(family, shape, "dz", np.abs(dz - dz64), bc.DZ_C * U * mag)
    if relu:
        assert (dz[r <= 0] == 0).all(), "%s %s: dz not exactly 0 where r <= 0" % (family, shape)
        assert (dz[:, k == 5] == 0).all(), "%s %s: dead rung dz not exactly 0" % (family, shape)
    d64 = dz.astype(np.float64)
    check(family, shape, "dbias", np.abs(dbias - d64.sum(0)), 4 * U * np.abs(d64).sum(0))


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("C,extra", STANDALONE)
def test_standalone_backward(hip, C, extra, relu):
    P, r, dy, gamma, beta, mm0, mv0, ld, sliced = standalone_case(C, extra)
    shape = (N, H, W, C, "ld%d" % ld, "relu%d" % relu)
    _, rv = sliced(r); _, dyv = sliced(dy)
    co = Coef(C, gamma, beta, mm0, mv0)
    st = bn_stats(hip, rv, ld, P, co)
    nb = hip.unet_bn_workspace(P, C); ws = ws_bytes(nb)
    k = bc.rung_of(C)

    def fresh():
        zbuf, zv = sliced(np.zeros_like(r))
        return zbuf, zv, [torch.full_like(co.gamma, float("nan")) for _ in range(3)]

    zbuf, zv, (dg, db, dbias) = fresh()
    hip.unet_bn_bwd(P_(dyv), ld, P_(rv), ld, P_(co.gamma), P_(co.mean), P_(co.invstd), P, C, relu, P_(zv), ld, P_(dg), P_(db), P_(dbias), P_(ws), nb, ST())
    out = (flat(zv), host(dg)[:C], host(db)[:C], host(dbias)[:C])
    assert_backward("unet_bn_bwd", shape, out, dy, r, gamma, st["mean"], st["invstd"], relu)
    assert (out[1][k == 5] == 0).all(), "unet_bn_bwd %s: dead rung dgamma not exactly 0" % (shape,)
    if extra:
        assert torch.isnan(zbuf[..., :8]).all() and torch.isnan(zbuf[..., 8 + C:]).all(), "unet_bn_bwd wrote outside its channel slice"
    zbuf, zv, (dg, db, dbias) = fresh()
    hip.unet_bn_bwd_any(P_(dyv), ld, None, 0, None, N, H, W, P_(rv), ld, P_(co.gamma), P_(co.mean), P_(co.invstd), C, relu,
                        P_(zv), ld, 0, P_(dg), P_(db), P_(dbias), None, 0, P_(ws), nb, ST(), 0, 0, 0, None)
    assert_backward("unet_bn_bwd_any", shape, (flat(zv), host(dg)[:C], host(db)[:C], host(dbias)[:C]), dy, r, gamma, st["mean"], st["invstd"], relu)
    if True:
        # pooled form (any C: 6 and 72 take the one-channel-per-lane kernels): dy = skip gradient + the pooled gradient routed to each window's first maximum (indices from the ladder's own y)
        y = st["scale"].astype(np.float64) * r.astype(np.float64) + st["shift"].astype(np.float64)
        win = y.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)
        idx = win.argmax(3).astype(np.uint8)
        pdy = np.random.default_rng(400 + C).standard_normal((N, H // 2, W // 2, C)).astype(np.float32)
        pos = (np.arange(H)[:, None] % 2) * 2 + (np.arange(W)[None, :] % 2)                       # [H, W] window position of each pixel
        up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
        dy_tot = (dy.reshape(N, H, W, C) + np.where(up(idx) == pos[None, :, :, None], up(pdy), np.float32(0))).astype(np.float32).reshape(P, C)
        zbuf, zv, (dg, db, dbias) = fresh()
        pdyd, idxd = dev(pdy), dev(idx, np.uint8)
        hip.unet_bn_bwd_pooled(P_(dyv), ld, P_(pdyd), C, P_(idxd), N, H, W, P_(rv), ld, P_(co.gamma), P_(co.mean), P_(co.invstd), C, relu,
                               P_(zv), ld, P_(dg), P_(db), P_(dbias), P_(ws), nb, ST())
        assert_backward("unet_bn_bwd_pooled", shape, (flat(zv), host(dg)[:C], host(db)[:C], host(dbias)[:C]), dy_tot, r, gamma, st["mean"], st["invstd"], relu)


def test_finalize_partials_clamps_a_negative_one_pass_variance(hip):
    """Hand-written partial sums with sum y^2 / P < mean^2 -- what cancellation leaves on a constant channel -- by a lot (var = -1: without
    the clamp sqrt of a negative number) and by a little (var = -1e-4 > -eps: without the clamp a finite invstd above 1/sqrt(eps))."""
    C, rows, P = 64, 3, 96
    family, shape = "unet_bn_train_finalize_partials", ("hand-written", "rows%d" % rows, "P%d" % P)
    var = np.where(np.arange(C) % 2 == 0, -1.0, -1e-4)
    per_row = np.stack([np.full(C, 5.0 * P / rows), (25.0 + var) * P / rows], -1).astype(np.float32)        # [64][2]: mean 5, E[y^2] = 25 + var
    part = dev(np.broadcast_to(per_row, (rows, C, 2)).copy())
    gamma, beta, mm0, mv0 = bc.bn_params(C, 9)
    co = Coef(C, gamma, beta, mm0, mv0)
    hip.unet_bn_train_finalize_partials(P_(part), rows, P, C, P_(co.gamma), P_(co.beta), bc.EPS, bc.MOMENTUM, 1, P_(co.mm), P_(co.mv),
                                        P_(co.mean), P_(co.invstd), P_(co.scale), P_(co.shift), ST())
    got = co.stats()
    ref = bc.finalize64(np.full(C, 5.0 * P), np.full(C, 25.0 * P), P, gamma, beta, mm0, mv0)          # variance exactly 0
    e, bound = bc.stat_errors(got, ref), bc.stat_floor_standalone(ref, beta)
    for key in bc.STAT_KEYS:
        check(family, shape, key, e[key], bound[key], rungs=np.full(C, 4))
    check(family, shape, "mm", np.abs(got["mm"] - ref["mm"]), 4 * U * np.abs(ref["mm"]), rungs=np.full(C, 4))


# ---- b. forward statistics from a producer's partial sums -------------------------------------------------------------------------------

def conv_inputs(shape, seed, taps, transposed=False):
    n, h, w, ci, co = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
    if transposed:
        wt, b = bc.ladder_conv_params(rng.standard_normal((2, 2, co, ci)), np.zeros(co), 2, ci, relu=False)
    else:
        wt, b = bc.ladder_conv_params(rng.standard_normal((3, 3, ci, co)), np.zeros(co), 3, taps * ci)
    return dev(x), dev(wt), dev(b)


def winograd_fused(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_fwd_winograd_fused_stats_rows(n, h, w, ci, co)
    Uc = torch.empty(16 * ci * co, device=DEV)
    hip.unet_winograd_weight_transform(P_(wt), P_(Uc), ci, co, 2, ST())
    r = torch.empty(n, h, w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_fwd_winograd_fused(P_(x), ci, None, P_(Uc), P_(b), P_(r), co, n, h, w, ci, co, 1, P_(part), part.numel() * 4, ST())
    return r, part, rows


def winograd_x6(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_fwd_winograd_fused_stats_rows(n, h, w, ci, co)
    U6 = torch.empty(hip.unet_winograd_x6_weight_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_winograd_weight_transform_x6(P_(wt), P_(U6), ci, co, 0, ST())
    r = torch.empty(n, h, w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_fwd_winograd_x6(P_(x), ci, None, P_(U6), P_(b), P_(r), co, n, h, w, ci, co, 1, P_(part), part.numel() * 4, ST())
    return r, part, rows


def conv_bf16(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_bf16_stats_rows(n, h, w, ci, co)
    wp = ws_bytes(hip.unet_conv3x3_bf16_packed_bytes(ci, co))
    hip.unet_conv3x3_bf16_pack_weights(P_(wt), P_(wp), ci, co, 0, ST())
    r = torch.empty(n, h, w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_fwd_bf16(P_(x), ci, 0, None, None, P_(wp), P_(b), P_(r), co, 0, n, h, w, ci, co, 1, P_(part), part.numel() * 4, ST())
    return r, part, rows


def conv_direct(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_fwd_direct_stats_rows(n, h, w, ci, co)
    r = torch.empty(n, h, w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_fwd_direct_stats(P_(x), ci, P_(wt), P_(b), P_(r), co, 0, n, h, w, ci, co, 1, P_(part), part.numel() * 4, ST())
    return r, part, rows


def convt_stream(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_convT2x2_fwd_stream_stats_rows(n, h, w, ci, co)
    r = torch.empty(n, 2 * h, 2 * w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_convT2x2_fwd_stream_stats(P_(x), ci, P_(wt), P_(b), P_(r), co, n, h, w, ci, co, P_(part), part.numel() * 4, ST())
    return r, part, rows


def convt_x6(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_convT2x2_x6_stats_rows(n, h, w, ci, co)
    W6 = torch.empty(hip.unet_convT2x2_x6_weight_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_convT2x2_weight_transform_x6(P_(wt), P_(W6), ci, co, 0, ST())
    r = torch.empty(n, 2 * h, 2 * w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_convT2x2_fwd_x6(P_(x), ci, P_(W6), P_(b), P_(r), co, n, h, w, ci, co, P_(part), part.numel() * 4, ST())
    return r, part, rows


def convt_bf16(hip, shape, x, wt, b):
    n, h, w, ci, co = shape
    rows = hip.unet_convT2x2_bf16_stats_rows(n, h, w, ci, co, 0)
    wp = ws_bytes(hip.unet_convT2x2_bf16_packed_bytes(ci, co))
    hip.unet_convT2x2_bf16_pack_weights(P_(wt), P_(wp), ci, co, 0, ST())
    r = torch.empty(n, 2 * h, 2 * w, co, device=DEV); part = torch.zeros((co // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_convT2x2_fwd_bf16(P_(x), ci, 0, P_(wp), P_(b), P_(r), co, 0, n, h, w, ci, co, P_(part), part.numel() * 4, ST())
    return r, part, rows


BIG = (5, 104, 136, 64, 64)          # several ragged tiles per persistent workgroup
FORWARD = [  # family, producer, shape (N, H, W, Cin, Cout; transposed convs: INPUT dims), transposed
    ("unet_conv3x3_fwd_winograd_fused", winograd_fused, (2, 16, 16, 64, 64), False),
    ("unet_conv3x3_fwd_winograd_fused", winograd_fused, BIG, False),
    ("unet_conv3x3_fwd_winograd_x6", winograd_x6, (2, 16, 16, 64, 64), False),
    ("unet_conv3x3_fwd_winograd_x6", winograd_x6, BIG, False),
    ("unet_convT2x2_fwd_stream_stats", convt_stream, (1, 16, 16, 64, 64), True),
    ("unet_convT2x2_fwd_x6", convt_x6, (2, 8, 8, 128, 64), True),
    ("unet_conv3x3_fwd_bf16", conv_bf16, (2, 20, 40, 64, 128), False),
    ("unet_convT2x2_fwd_bf16", convt_bf16, (2, 10, 20, 128, 64), True),
    ("unet_conv3x3_fwd_direct_stats", conv_direct, (2, 18, 24, 1, 64), False),
    ("unet_conv3x3_fwd_direct_stats", conv_direct, (2, 18, 24, 3, 64), False),
]


@pytest.mark.parametrize("family,producer,shape,transposed", FORWARD, ids=["%s-%s" % (f[0], "x".join(map(str, f[2]))) for f in FORWARD])
def test_forward_statistics_from_partials(hip, family, producer, shape, transposed):
    n, h, w, ci, co = shape
    x, wt, b = conv_inputs(shape, 7 + ci + h, 9, transposed)
    r, part, rows = producer(hip, shape, x, wt, b)
    assert rows > 0, "%s %s leaves no partial sums" % (family, shape)
    P = r.numel() // co
    gamma, beta, mm0, mv0 = bc.bn_params(co, 300 + co)
    co_ = Coef(co, gamma, beta, mm0, mv0)
    hip.unet_bn_train_finalize_partials(P_(part), rows, P, co, P_(co_.gamma), P_(co_.beta), bc.EPS, bc.MOMENTUM, 1, P_(co_.mm), P_(co_.mv),
                                        P_(co_.mean), P_(co_.invstd), P_(co_.scale), P_(co_.shift), ST())
    got = co_.stats()
    rh = flat(r)
    k = bc.rung_of(co)
    # the producer landed on the ladder: dead rung all zero, constant rung one value, the ill-conditioned rungs where they should be
    assert (rh[:, k == 5] == 0).all() and (rh[:, k == 4] == np.float32(5.1)).all(), "%s %s: ladder inputs did not give the constant / dead rungs" % (family, shape)
    m, s = rh.astype(np.float64).mean(0), rh.astype(np.float64).std(0)
    for rung, what, val, lo, hi in ((3, "mean", m, 99.9, 100.1), (3, "sigma", s, 0.02, 0.3), (2, "mean", m, 29.7, 30.3)):
        bad = (k == rung) & ((val < lo) | (val > hi))
        assert not bad.any(), "%s shape %s: the producer's output is off the ladder on rung %d (%s), channel %d: %s %.4g outside [%g, %g]" % (
            family, shape, rung, bc.RUNGS[rung][0], int(np.argmax(bad)), what, val[int(np.argmax(bad))], lo, hi)
    ref = bc.ref_forward(rh, gamma, beta, mm0, mv0)
    floor = bc.f_stat_forward(rh, rows, gamma, beta, mm0, mv0, ref)
    const = bc.constant_channel_floor(rh, rows, gamma, beta, mm0, mv0, ref)
    assert_stats(family, shape + ("rows%d" % rows,), got, ref, beta, extra=floor, rung0_tight=True, const=const)
    # the standalone pass over the same stored tensor stays kappa'-independent at this shape too
    co2 = Coef(co, gamma, beta, mm0, mv0)
    assert_stats("unet_bn_train_stats", shape, bn_stats(hip, r, co, P, co2), ref, beta)


# ---- d. / e. backward from a data gradient's partial sums -------------------------------------------------------------------------------

def dgrad_winograd(hip, shape, crange, dzin, wt, r_prev):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_fwd_winograd_fused_stats_rows(n, h, w, co, ci)
    Ucd = torch.empty(16 * ci * co, device=DEV)
    hip.unet_winograd_weight_transform(P_(wt), P_(Ucd), ci, co, 3, ST())
    dx = torch.empty(n, h, w, ci, device=DEV); part = torch.zeros((ci // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_dgrad_winograd_fused(P_(dzin), co, P_(Ucd), P_(dx), ci, n, h, w, ci, co, P_(r_prev), r_prev.shape[-1], crange[0], crange[1],
                                          P_(part), part.numel() * 4, ST())
    return dx, part, rows


def dgrad_x6(hip, shape, crange, dzin, wt, r_prev):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_fwd_winograd_fused_stats_rows(n, h, w, co, ci)
    U6d = torch.empty(hip.unet_winograd_x6_weight_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_winograd_weight_transform_x6(P_(wt), P_(U6d), ci, co, 1, ST())
    dx = torch.empty(n, h, w, ci, device=DEV); part = torch.zeros((ci // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_dgrad_winograd_x6(P_(dzin), co, P_(U6d), P_(dx), ci, n, h, w, ci, co, P_(r_prev), r_prev.shape[-1], crange[0], crange[1],
                                       P_(part), part.numel() * 4, ST())
    return dx, part, rows


def dgrad_bf16(hip, shape, crange, dzin, wt, r_prev):
    n, h, w, ci, co = shape
    rows = hip.unet_conv3x3_bf16_stats_rows(n, h, w, co, ci)
    wpd = ws_bytes(hip.unet_conv3x3_bf16_packed_bytes(ci, co))
    hip.unet_conv3x3_bf16_pack_weights(P_(wt), P_(wpd), ci, co, 1, ST())
    dx = torch.empty(n, h, w, ci, device=DEV); part = torch.zeros((ci // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_conv3x3_dgrad_bf16(P_(dzin), co, 0, P_(wpd), P_(dx), ci, 0, n, h, w, ci, co, P_(r_prev), r_prev.shape[-1], 0, crange[0], crange[1],
                                P_(part), part.numel() * 4, ST())
    return dx, part, rows


def dgrad_convt_x6(hip, shape, crange, dzin, wt, r_prev):
    n, h, w, ci, co = shape
    rows = hip.unet_convT2x2_x6_bnbwd_rows(n, h, w, ci, co)
    W6d = torch.empty(hip.unet_convT2x2_x6_weight_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_convT2x2_weight_transform_x6(P_(wt), P_(W6d), ci, co, 1, ST())
    dx = torch.empty(n, h, w, ci, device=DEV); part = torch.zeros((ci // 64) * max(rows, 1) * 128, device=DEV)
    hip.unet_convT2x2_dgrad_x6_sums(P_(dzin), co, P_(W6d), P_(dx), ci, n, h, w, ci, co, P_(r_prev), r_prev.shape[-1], P_(part), part.numel() * 4, ST())
    return dx, part, rows


BACKWARD = [  # family, producer, shape (N, H, W, Cin, Cout of the CONSUMER layer), channel range of dx that is the producer's dy, transposed
    ("unet_conv3x3_dgrad_winograd_fused", dgrad_winograd, (2, 16, 16, 64, 64), (0, 64), False),
    ("unet_conv3x3_dgrad_winograd_fused", dgrad_winograd, (1, 16, 32, 128, 64), (64, 128), False),
    ("unet_conv3x3_dgrad_winograd_fused", dgrad_winograd, BIG, (0, 64), False),
    ("unet_conv3x3_dgrad_winograd_x6", dgrad_x6, (2, 16, 16, 64, 64), (0, 64), False),
    ("unet_conv3x3_dgrad_winograd_x6", dgrad_x6, BIG, (0, 64), False),
    ("unet_convT2x2_dgrad_x6_sums", dgrad_convt_x6, (2, 8, 24, 128, 64), (0, 128), True),
    ("unet_conv3x3_dgrad_bf16", dgrad_bf16, (2, 20, 40, 64, 128), (0, 64), False),
]


@pytest.mark.parametrize("family,producer,shape,crange,transposed", BACKWARD,
                         ids=["%s-%s-c%d" % (f[0], "x".join(map(str, f[2])), f[3][0]) for f in BACKWARD])
def test_backward_from_partials(hip, family, producer, shape, crange, transposed):
    n, h, w, ci, co = shape
    c0, c1 = crange
    cp = c1 - c0
    P = n * h * w
    rng = np.random.default_rng(11 + ci + co + h)
    if transposed:
        dzin = dev(rng.standard_normal((n, 2 * h, 2 * w, co))); wt = dev(rng.standard_normal((2, 2, co, ci)) / np.sqrt(4 * co))
    else:
        dzin = dev(rng.standard_normal((n, h, w, co))); wt = dev(rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * co))
    r = bc.ladder_tensor(P, cp, 500 + cp + h)
    gamma, beta, mm0, mv0 = bc.bn_params(cp, 600 + cp)
    rd = dev(r).view(n, h, w, cp)
    co_ = Coef(cp, gamma, beta, mm0, mv0)
    st = bn_stats(hip, rd, cp, P, co_)
    dx, part, rows = producer(hip, shape, crange, dzin, wt, rd)
    assert rows > 0, "%s %s leaves no partial sums" % (family, shape)
    dyv = dx[..., c0:c1]
    dy = flat(dyv)                                                      # the dy the kernel itself stored
    nb = hip.unet_bn_workspace(P, cp); ws = ws_bytes(nb)
    dz = torch.full((n, h, w, cp), float("nan"), device=DEV)
    dg, db, dbias = [torch.full((cp,), float("nan"), device=DEV) for _ in range(3)]
    sub = ctypes.c_void_p(part.data_ptr() + (c0 // 64) * rows * 128 * 4)
    hip.unet_bn_bwd_from_partials(P_(dyv), ci, P_(rd), cp, P_(co_.gamma), P_(co_.mean), P_(co_.invstd), P, cp, 1, P_(dz), cp, P_(dg), P_(db), P_(dbias),
                                  sub, rows, P_(ws), nb, ST())
    fsum = bc.f_stat_backward(dy, r, rows, st["mean"], st["invstd"])
    out = (flat(dz), host(dg), host(db), host(dbias))
    assert_backward(family, shape + ("c%d:%d" % crange, "rows%d" % rows), out, dy, r, gamma, st["mean"], st["invstd"], 1, fsum)
    k = bc.rung_of(cp)
    assert (out[1][k == 5] == 0).all(), "%s %s: dead rung dgamma not exactly 0" % (family, shape)
