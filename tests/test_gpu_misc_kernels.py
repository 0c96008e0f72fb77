"""The elementwise kernels of semantic-segmentation-unet_amd/csrc/misc.hip, one entry point of the C ABI at a time, against the references of
tests/misc_kernel_cases.py: unet_maxpool2x2_fwd / _bwd, unet_dropout, unet_argmax and unet_nchw_to_nhwc bit for bit, unet_softmax_ce and
unet_adam_keras inside bounds derived from their operation order -- on the 16-byte and the scalar path, dense, strided, misaligned and in
place, fp32 and bf16 storage, at one-pixel and ragged shapes and on the second trip of every grid-stride loop.  Every output buffer is longer
than its tensor and ends in sentinels that must survive, a strided tensor lives in a sentinel-filled buffer whose channels >= C must survive
as well, and every input must come back unchanged unless the call is in place.  NaN inputs are out of contract for all of these kernels and
are not tested.

The unmarked part runs without a GPU: the numpy hash is the C++ one, the fp32 evaluation of every formula stays inside its bound, the clip
cases are what they claim, and each reference tells the near-miss restatement it exists to catch from the truth on the committed cases."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import misc_kernel_cases as mc
from conftest import PKG, ROOT

gpu = pytest.mark.gpu               # the device part; everything else runs anywhere

DEV = "cuda"
F, D, U = mc.F, mc.D, mc.U
PAD = 37                            # sentinels behind every buffer
EINVAL, ENOSPC = -1, -2
_KINDS = {"f32": (np.float32, mc.SENT), "bf16": (np.uint16, mc.bf16_pack(np.asarray([mc.SENT16], F))[0]), "u8": (np.uint8, mc.SENT_U8),
          "i32": (np.int32, mc.SENT_I32)}
_TORCH = {np.float32: torch.float32, np.uint16: torch.int16, np.uint8: torch.uint8, np.int32: torch.int32}


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """rows [P][C] of a device tensor with `ld` elements between rows, `off` elements into a sentinel-filled buffer that ends in PAD sentinels.
    vals None: the rows are sentinels too (an output).  bf16 rows are given and returned as float32 values."""

    def __init__(self, shape, vals=None, ld=None, off=0, kind="f32"):
        self.p, self.c = int(np.prod(shape[:-1])), int(shape[-1])
        self.shape, self.ld, self.off, self.kind = tuple(shape), (ld or self.c), off, kind
        dt, sent = _KINDS[kind]
        self.host = np.full(off + self.p * self.ld + PAD, sent, dt)
        self.rows(self.host)[...] = sent if vals is None else self._pack(np.asarray(vals).reshape(self.p, self.c))
        self.t = torch.as_tensor(self.host.view(np.int16) if dt is np.uint16 else self.host.copy()).to(DEV)
        self.ptr = ctypes.c_void_p(self.t.data_ptr() + off * self.host.itemsize)

    def _pack(self, a):
        return mc.bf16_pack(np.asarray(a, F)) if self.kind == "bf16" else a

    def rows(self, flat):
        return flat[self.off:self.off + self.p * self.ld].reshape(self.p, self.ld)[:, :self.c]

    def read(self):
        """-> the rows in the tensor's shape, and whether every element outside them still holds the sentinel"""
        now = self.t.cpu().numpy().view(self.host.dtype)
        outside = np.ones(now.size, bool)
        self.rows(outside)[...] = False
        vals = self.rows(now).copy()
        vals = mc.bf16_unpack(vals) if self.kind == "bf16" else vals
        return vals.reshape(self.shape), bool((now[outside] == _KINDS[self.kind][1]).all())

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(self.host.dtype).view(np.uint8), self.host.view(np.uint8))


def same_bits(a, b):
    return np.array_equal(mc.bits(a), mc.bits(b))


def where_differs(a, b):
    d = mc.bits(a) != mc.bits(b)
    return int(d.sum()), np.argwhere(d)[:4].tolist()


# ------------------------------------------------------------------------------------------------------------------------------ CPU part
def _unet_hash32_source():
    text = open(os.path.join(ROOT, PKG, "csrc", "common.h")).read()
    m = re.search(r"uint32_t unet_hash32\((uint32_t seed, uint64_t idx)\) (\{.*?\n\})", text, re.S)
    assert m, "unet_hash32 not found in common.h"
    return "static uint32_t unet_hash32(%s) %s" % m.groups()


HASH_POINTS = [(0, 0), (123, 1), (0xFFFFFFFF, 2 ** 33 + 5)]


def test_numpy_hash_is_the_hash_of_common_h(tmp_path):
    # the body of common.h's function, compiled for the host as it stands (plain integer C++), against the numpy restatement
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = "#include <cstdint>\n#include <cstdio>\n%s\nint main() {\n%s    return 0;\n}\n" % (
        _unet_hash32_source(), "".join('    std::printf("%%u\\n", unet_hash32(%du, %dull));\n' % p for p in HASH_POINTS))
    (tmp_path / "hash.cpp").write_text(src)
    subprocess.check_call([cxx, "-O1", "-o", str(tmp_path / "hash"), str(tmp_path / "hash.cpp")])
    want = [int(v) for v in subprocess.check_output([str(tmp_path / "hash")]).split()]
    got = [int(mc.hash32(s, np.uint64(i))) for s, i in HASH_POINTS]
    assert got == want and len(set(want)) == 3, (got, want)
    assert int(mc.hash32(0xFFFFFFFF, np.uint64(7))) == int(mc.hash32(-1, np.uint64(7)))          # seed + 1 wraps to 0
    assert [mc.threshold(r) for r in mc.DROPOUT_RATES] == [0, 2 ** 30, 2 ** 31, int(float(F(0.9)) * 2 ** 32)]
    assert mc.threshold(float(np.nextafter(F(1), F(0)))) == 2 ** 32 - 256


def test_pool_reference_rejects_the_last_maximum_and_accumulate_for_store():
    told = 0
    for n, h, w in mc.POOL_SHAPES:
        for c in (1, 8):
            x = mc.pool_input(n, h, w, c, 3)
            y, idx = mc.pool_fwd_ref(x)
            kinds = mc.pool_window_kinds(n, h // 2, w // 2, c)
            for kind, first in mc.POOL_FIRST.items():
                assert (idx[kinds == kind] == first).all()
            assert np.array_equal(mc.bits(y[kinds == 2]), mc.bits(np.zeros((kinds == 2).sum(), F)))
            for kind in (3, 7):
                assert (mc.bits(y[kinds == kind]) == 0x80000000).all()
            y_last, idx_last = mc.pool_fwd_ref(x, last=True)
            assert idx.size < 8 or not np.array_equal(idx, idx_last)
            told += not same_bits(y, y_last)                                   # (+0 / -0 windows: even the values differ)
            dy, base = mc.pool_grads(n, h // 2, w // 2, c, 4)
            store = mc.pool_bwd_ref(dy, idx, base, 0)
            assert not same_bits(store, mc.pool_bwd_ref(dy, idx, base, 0, always_accumulate=True))
            assert same_bits(mc.windows(store)[np.arange(4) != idx[..., None]], np.zeros(3 * idx.size, F))
            acc = mc.pool_bwd_ref(dy, idx, base, 1)
            assert np.array_equal(mc.windows(acc)[np.arange(4) != idx[..., None]].view(np.uint32),
                                  mc.windows(base)[np.arange(4) != idx[..., None]].view(np.uint32))
    assert told >= 3
    assert [mc.pool_path_is_vector(k) for k in mc.POOL_PATHS] == [True, True, True, False, False, False, False, False, True, True]
    b = mc.bf16_round(np.asarray([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, np.inf, -1.0 - 2.0 ** -9], F))          # ties to even
    assert b.tolist() == [1.0, 1.0 + 2.0 ** -6, np.inf, -1.0]


def test_dropout_reference_rejects_its_three_near_misses():
    p = mc.DROPOUT_P
    for seed in mc.DROPOUT_SEEDS:
        for c in (6, 8):
            for rate in mc.DROPOUT_RATES[1:]:
                keep = mc.dropout_keep(seed, p, c, rate)
                assert abs(keep.mean() - (1 - rate)) < 0.04
                assert not np.array_equal(keep, mc.dropout_keep(seed, p, c, rate, index_ld=2 * c))
                assert not np.array_equal(keep, mc.dropout_keep(seed, p, c, rate, seed_plus=0))
            assert mc.dropout_keep(seed, p, c, 0.0).all()
            if seed == 0xFFFFFFFF:              # seed + 1 wraps to 0 and element 0 hashes to 0: dropped at every rate > 0, kept at rate 0
                assert int(mc.hash32(seed, np.uint64(0))) == 0 and not mc.dropout_keep(seed, p, c, 2.0 ** -32)[0, 0]
                continue
            # the threshold: at the ordinary rates no element of a small case sits on it; the edge rates put one there
            r0, r1, el = mc.dropout_edge_rates(seed, p, c)
            k0, k1 = mc.dropout_keep(seed, p, c, r0), mc.dropout_keep(seed, p, c, r1)
            assert k0.all() and (~k1).sum() == 1 and not k1.reshape(-1)[el]
            assert not mc.dropout_keep(seed, p, c, r0, thr_plus=1).all() and mc.dropout_keep(seed, p, c, r1, thr_plus=-1).all()
    x = mc.dropout_input(p, 8, 1)
    assert np.isposinf(x).any() and np.isneginf(x).any() and (x == -3.0).any()
    out = mc.dropout_ref(x, mc.dropout_keep(1, p, 8, 0.5), 0.5)
    dropped = ~mc.dropout_keep(1, p, 8, 0.5)
    assert not mc.bits(out)[dropped].any() and np.isinf(x[dropped]).any() and (x[dropped] == -3.0).any()
    assert mc.dropout_scale(0.9) == F(1) / F(0.100000024) and mc.dropout_scale(0.0) == 1


def test_argmax_cases_hold_their_ties_and_the_prob_argmax_is_told_apart():
    for k in mc.ARGMAX_KS:
        z = mc.argmax_rows(64, k, k)
        ref = mc.argmax_ref(z)
        if k > 1:
            assert (ref[0::8] == 0).all() and (ref[1::8] == min(k // 2, (k // 2 + 1) % k)).all() and (ref[2::8] == k - 2).all()
            assert (ref[3::8] == k // 2).all() and (mc.bits(z[3::8, k // 2]) == 0x80000000).all() and (ref[4::8] == 0).all()
            assert (ref[5::8] == 0).all() and np.isneginf(z[5::8]).all() and (ref[6::8] == (np.arange(6, 64, 8) // 8) % k).all()
    # unet_softmax_ce's accuracy: first maximum of the logits; the rounded probabilities tie where the logits do not
    for k in mc.CE_KS[1:]:
        z, lab = mc.ce_logits(mc.CE_P, k, "near_ties", k), mc.ce_labels(mc.CE_P, k, k)
        a, b = mc.ce_ref(z, lab), mc.ce_ref(z, lab, argmax_on_prob=True)
        assert a["correct"] != b["correct"], k
        p32 = a["prob"].astype(F)
        assert ((p32 == p32.max(-1, keepdims=True)).sum(-1) == 2).mean() > 0.9
        z, lab = mc.ce_logits(mc.CE_P, k, "ties", k), mc.ce_labels(mc.CE_P, k, k)
        assert ((z == z.max(-1, keepdims=True)).sum(-1) >= 2).all()


CE_CONFIGS = [(0.0, 0.0), (0.1, 0.0), (0.0, 1e-7), (0.1, 1e-7)]                      # label smoothing, clip
CE_SCALES = (1.0 / (4 * 24 * 16), 1.0 / 257)                                          # loss_scale, grad_scale


def _ce_cases():
    for k in mc.CE_KS:
        for regime in mc.CE_REGIMES:
            yield k, regime


def test_fp32_evaluation_of_softmax_ce_stays_inside_the_bounds():
    worst = {"prob": 0.0, "dz": 0.0, "loss": 0.0}
    for k, regime in _ce_cases():
        z, lab = mc.ce_logits(mc.CE_P, k, regime, 10 * k), mc.ce_labels(mc.CE_P, k, k)
        for ls, clip in CE_CONFIGS:
            if clip and regime != "ordinary":
                continue                        # (the clip cases have a generator of their own)
            ref = mc.ce_ref(z, lab, ls, clip, *CE_SCALES)
            prob, dz, loss = mc.ce_fp32(z, lab, ls, clip, *CE_SCALES)
            ex = {"prob": mc.ce_excess(prob, ref["prob"], ref["prob_bound"]), "loss": abs(float(loss) - ref["loss"]) / ref["loss_bound"] if k > 1 else 0.0}
            if not clip:
                ex["dz"] = mc.ce_excess(dz, ref["dz"], ref["dz_bound"])
            for name, v in ex.items():
                assert v <= 1, (k, regime, ls, clip, name, v)
                worst[name] = max(worst[name], v)
            if regime == "gap_90":
                assert k == 1 or ((ref["prob"] > 0) & (ref["prob"] < 2.0 ** -126)).any()            # subnormal probabilities
            if regime == "gap_200":
                assert k == 1 or (prob == 0).any()
            # where the ordinary cases overlap tests/test_gpu_kernels.py, the derived bound is no wider than that test's tolerance
            if regime == "ordinary" and k in (2, 3, 7):
                assert ref["prob_bound"].max() <= 2e-6 * ref["prob"].max()
                assert ref["dz_bound"].max() <= 5e-6 * np.abs(ref["dz"]).max()
                assert ref["loss_bound"] <= (2e-5 if clip else 2e-6) * abs(ref["loss"])
    print("fp32 evaluation / bound:", worst)
    assert worst["prob"] > 0.02 and worst["loss"] > 0.02                 # (the bounds are within two orders of what fp32 really does)


@pytest.mark.parametrize("k,clip", [(2, 1e-7), (3, 1e-7), (7, 1e-7), (3, 1e-3)])
def test_clip_cases_move_few_pixels_and_still_leave_the_clip_range(k, clip):
    z, moved, outside = mc.ce_clip_case(mc.CE_P * 3, k, clip, k)
    assert moved <= mc.CE_CLIP_MOVED_CAP and outside, (moved, outside)
    lab = mc.ce_labels(mc.CE_P * 3, k, k)
    for ls in (0.0, 0.1):
        ref = mc.ce_ref(z, lab, ls, clip, *CE_SCALES)
        prob, dz, loss = mc.ce_fp32(z, lab, ls, clip, *CE_SCALES)
        assert mc.ce_excess(prob, ref["prob"], ref["prob_bound"]) <= 1
        assert mc.ce_excess(dz, ref["dz"], ref["dz_bound"]) <= 1
        assert abs(float(loss) - ref["loss"]) <= ref["loss_bound"] <= 2e-5 * abs(ref["loss"])
        assert ref["dz_bound"].max() <= 5e-6 * np.abs(ref["dz"]).max()


def test_fp32_evaluation_of_adam_stays_inside_the_bounds_and_the_double_beta_does_not():
    for n in mc.ADAM_NS + (7 * 400,):
        th, g, m, v, block = mc.adam_state(n, n)
        for t in (1, 7, 1000):
            alpha = mc.adam_alpha(t)
            ref, bound = mc.adam_ref(th, g, m, v, alpha)
            for name, got, r, b in zip("mvt", mc.adam_fp32(th, g, m, v, alpha), ref, bound):
                assert (np.abs(got.astype(D) - r) <= b).all(), (n, t, name, float((np.abs(got.astype(D) - r) / b).max()))
            zg = block == mc.ADAM_STATES.index("zero_gradient")
            assert np.array_equal(ref[2][zg], th[zg].astype(D)) and not ref[0][zg].any() and not ref[1][zg].any()
            # 1 - 0.9 formed in double is 2^-22 away from the kernel's constant: outside the bound of m' on the first step
            wrong, _ = mc.adam_ref(th, g, m, v, alpha, beta_in_double=True)
            first = block == mc.ADAM_STATES.index("first_step")
            if first.any():
                assert (np.abs(wrong[0] - ref[0]) > bound[0])[first].all()
    assert float(F(1) - F(0.9)) == 1 - float(F(0.9)) and float(F(1) - F(0.999)) == 1 - float(F(0.999))          # exact in fp32
    th, g, m, v, block = mc.adam_state(2800, 1)
    under = block == mc.ADAM_STATES.index("g_1e-25")
    assert not (g[under] * g[under]).any() and (g[under] != 0).all()
    big = block == mc.ADAM_STATES.index("m_large")
    assert (np.abs(m[big]) > 1e5 * np.sqrt(v[big])).all()


def test_second_trip_sizes():
    for kind, cap in mc.CAPS.items():
        total = mc.second_trip(kind, 133)
        assert cap * 256 < total < (cap + 1) * 256 and total % 256
    assert 3 * 699095 == mc.second_trip("permute", 133)


# ------------------------------------------------------------------------------------------------------------------------------ max pool
def _pool_case(shape, path, seed=0):
    n, h, w = shape
    c, ex, ey, off, b16 = mc.POOL_PATHS[path]
    return n, h, w, c, c + ex, c + ey, off, b16, mc.pool_input(n, h, w, c, seed + 7 * c + h, bool(b16))


def _run_pool_fwd(hip, x, n, h, w, c, ldx, ldy, off, b16):
    kind = "bf16" if b16 else "f32"
    xb = Buf((n, h, w, c), x, ldx, off, kind)
    yb, ib = Buf((n, h // 2, w // 2, c), None, ldy, 0, kind), Buf((n, h // 2, w // 2, c), None, None, 0, "u8")
    hip.unet_maxpool2x2_fwd(xb.ptr, ldx, yb.ptr, ldy, ib.ptr, n, h, w, c, b16, ST())
    (y, y_ok), (idx, i_ok) = yb.read(), ib.read()
    assert y_ok and i_ok and xb.unchanged()
    return y, idx


def _run_pool_bwd(hip, dy, idx, base, n, h, w, c, lddy, lddx, off, b16, accumulate):
    kind = "bf16" if b16 else "f32"
    gb, ib = Buf(dy.shape, dy, lddy, 0, kind), Buf(idx.shape, idx, None, 0, "u8")
    # accumulate = 0: the kernel must not read dx -- it holds the sentinel, which no sum with dy reproduces
    db = Buf((n, h, w, c), base if accumulate else None, lddx, off, kind)
    hip.unet_maxpool2x2_bwd(gb.ptr, lddy, ib.ptr, db.ptr, lddx, n, h, w, c, accumulate, b16, ST())
    dx, ok = db.read()
    assert ok and gb.unchanged() and ib.unchanged()
    return dx


@gpu
@pytest.mark.parametrize("path", list(mc.POOL_PATHS))
@pytest.mark.parametrize("shape", mc.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_forward_and_backward_are_the_reference_bit_for_bit(hip, shape, path):
    n, h, w, c, ldx, ldy, off, b16, x = _pool_case(shape, path)
    y, idx = _run_pool_fwd(hip, x, n, h, w, c, ldx, ldy, off, b16)
    y_ref, idx_ref = mc.pool_fwd_ref(x)
    assert np.array_equal(idx, idx_ref), np.argwhere(idx != idx_ref)[:4].tolist()
    assert same_bits(y, y_ref), where_differs(y, y_ref)
    dy, base = mc.pool_grads(n, h // 2, w // 2, c, 5, bool(b16))
    for accumulate in (0, 1):
        # (the forward's strides the other way round: dy has the pooled tensor's, dx the input's)
        dx = _run_pool_bwd(hip, dy, idx_ref, base, n, h, w, c, ldy, ldx, off, b16, accumulate)
        ref = mc.pool_bwd_ref(dy, idx_ref, base, accumulate, bool(b16))
        assert same_bits(dx, ref), (accumulate,) + where_differs(dx, ref)
        if not accumulate:
            assert not mc.bits(mc.windows(dx)[np.arange(4) != idx_ref[..., None]]).any()            # every other position: +0.0, written


@gpu
@pytest.mark.parametrize("c,b16", [(1, 0), (4, 0), (4, 1)], ids=["scalar_c1", "vec_c4", "bf16_c4"])
def test_maxpool_grid_stride_loops_wrap(hip, c, b16):
    # one row of windows: cap * 256 + 133 work items (one channel each on the scalar path, four on the 16-byte path)
    n, h, w2 = 1, 2, mc.second_trip("pool", 133)
    rng = np.random.RandomState(c)
    x = np.round(rng.randn(n, h, 2 * w2, c) * 2).astype(F)
    y, idx = _run_pool_fwd(hip, x, n, h, 2 * w2, c, c, c, 0, b16)
    y_ref, idx_ref = mc.pool_fwd_ref(x)
    assert np.array_equal(idx, idx_ref) and same_bits(y, y_ref)
    assert len(np.unique(idx_ref[0, 0, mc.CAPS["pool"] * 256:])) == 4
    dy = np.round(rng.randn(n, 1, w2, c) * 4).astype(F) + 0.5
    base = np.round(rng.randn(n, h, 2 * w2, c) * 4).astype(F)
    for accumulate in (0, 1):
        dx = _run_pool_bwd(hip, dy, idx_ref, base, n, h, 2 * w2, c, c, c, 0, b16, accumulate)
        assert same_bits(dx, mc.pool_bwd_ref(dy, idx_ref, base, accumulate, bool(b16))), accumulate


# ------------------------------------------------------------------------------------------------------------------------------- dropout
def _run_dropout(hip, x, form, seed, rate, mask=None):
    """-> the output rows; asserts the sentinels, the channels >= C and the inputs"""
    c, ex, off, in_place, b16 = mc.DROPOUT_FORMS[form] if isinstance(form, str) else form
    kind, p = "bf16" if b16 else "f32", x.shape[0]
    xb = Buf((p, c), x, c + ex, off, kind)
    ob = xb if in_place else Buf((p, c), None, c + ex, off, kind)
    mb = None if mask is None else Buf((p, c), mask, None, 0, "u8")
    hip.unet_dropout(xb.ptr, c + ex, ob.ptr, c + ex, p, c, None if mb is None else mb.ptr, seed, rate, b16, ST())
    out, ok = ob.read()
    assert ok and (in_place or xb.unchanged()) and (mb is None or mb.unchanged())
    return out


@gpu
@pytest.mark.parametrize("form", list(mc.DROPOUT_FORMS))
def test_dropout_kept_set_and_values_are_the_restatement_exactly(hip, form):
    c, b16 = mc.DROPOUT_FORMS[form][0], bool(mc.DROPOUT_FORMS[form][4])
    p = mc.DROPOUT_P
    x = mc.dropout_input(p, c, 2, b16)
    for seed in mc.DROPOUT_SEEDS:
        for rate in mc.DROPOUT_RATES:
            keep = mc.dropout_keep(seed, p, c, rate)
            out = _run_dropout(hip, x, form, seed, rate)
            assert np.array_equal(out != 0, keep), (seed, rate, int(((out != 0) != keep).sum()))
            ref = mc.dropout_ref(x, keep, rate, b16)
            assert same_bits(out, ref), (seed, rate) + where_differs(out, ref)
            assert rate or same_bits(out, x)


@gpu
@pytest.mark.parametrize("form", ["dense", "in_place_slice", "scalar_c6", "bf16"])
def test_dropout_threshold_is_inclusive(hip, form):
    # thresholds exactly on, and one above, the smallest hash of the case: that element is kept at the first rate and alone dropped at the second
    c, b16 = mc.DROPOUT_FORMS[form][0], bool(mc.DROPOUT_FORMS[form][4])
    p, seed = mc.DROPOUT_P, 1
    x = mc.dropout_input(p, c, 3, b16)
    r0, r1, el = mc.dropout_edge_rates(seed, p, c)
    o0, o1 = _run_dropout(hip, x, form, seed, r0), _run_dropout(hip, x, form, seed, r1)
    assert (o0 != 0).all() and np.argwhere(o1.reshape(-1) == 0).reshape(-1).tolist() == [el]
    for out, rate in ((o0, r0), (o1, r1)):
        assert same_bits(out, mc.dropout_ref(x, mc.dropout_keep(seed, p, c, rate), rate, b16))


@gpu
def test_dropout_backward_regenerates_the_forward_mask(hip):
    # the engine's pair: forward in place on a channel slice of the concat buffer (ld = 2C), backward on the dense gradient, same seed
    p, c, seed = mc.DROPOUT_P, 8, 20240
    x, g = mc.dropout_input(p, c, 4), mc.dropout_input(p, c, 5)
    keep = mc.dropout_keep(seed, p, c, 0.5)
    for b16 in (0, 1):
        xs, gs = (mc.bf16_round(x), mc.bf16_round(g)) if b16 else (x, g)
        fwd = _run_dropout(hip, xs, (c, c, c, 1, b16), seed, 0.5)
        bwd = _run_dropout(hip, gs, (c, 0, 0, 1, b16), seed, 0.5)
        assert np.array_equal(fwd == 0, bwd == 0) and np.array_equal(fwd != 0, keep)
        assert same_bits(bwd, mc.dropout_ref(gs, keep, 0.5, bool(b16)))


@gpu
@pytest.mark.parametrize("form", ["in_place_slice", "scalar_c8_ld10_in_place", "scalar_c6_slice", "bf16_in_place_slice"])
def test_dropout_explicit_mask_is_indexed_without_the_stride(hip, form):
    c, b16 = mc.DROPOUT_FORMS[form][0], bool(mc.DROPOUT_FORMS[form][4])
    p = mc.DROPOUT_P
    x = mc.dropout_input(p, c, 6, b16)
    mask = np.random.RandomState(7).choice(np.asarray([0, 0, 1, 2, 255], np.uint8), (p, c))
    out = _run_dropout(hip, x, form, 9, 0.25, mask)
    assert same_bits(out, mc.dropout_ref(x, mask != 0, 0.25, b16))


@gpu
@pytest.mark.parametrize("c", [1, 4])
def test_dropout_grid_stride_loop_wraps(hip, c):
    p, seed = mc.second_trip("dropout", 133), 0xFFFFFFFF
    x = (np.random.RandomState(c).rand(p, c) + 0.5).astype(F)
    out = _run_dropout(hip, x, (c, 0, 0, 0, 0), seed, 0.5)
    keep = mc.dropout_keep(seed, p, c, 0.5)
    assert same_bits(out, mc.dropout_ref(x, keep, 0.5))
    tail = keep[mc.CAPS["dropout"] * 256:]
    assert tail.any() and not tail.all()


# -------------------------------------------------------------------------------------------------------------------------------- argmax
def _run_argmax(hip, z, ldp):
    p, k = z.shape
    zb, ob = Buf((p, k), z, ldp), Buf((p, 1), None, None, 0, "i32")
    hip.unet_argmax(zb.ptr, ldp, ob.ptr, p, k, ST())
    out, ok = ob.read()
    assert ok and zb.unchanged()
    return out[:, 0]


@gpu
@pytest.mark.parametrize("extra", [0, 2], ids=["dense", "ld_k_plus_2"])
@pytest.mark.parametrize("p", [1, 301])
@pytest.mark.parametrize("k", mc.ARGMAX_KS)
def test_argmax_is_the_first_maximum(hip, k, p, extra):
    z = mc.argmax_rows(p, k, k + p)
    got = _run_argmax(hip, z, k + extra)
    assert np.array_equal(got, mc.argmax_ref(z)), np.argwhere(got != mc.argmax_ref(z))[:4].tolist()


@gpu
def test_argmax_grid_stride_loop_wraps(hip):
    p = mc.second_trip("argmax", 77)
    z = np.round(np.random.RandomState(0).randn(p, 2)).astype(F)
    got = _run_argmax(hip, z, 2)
    ref = mc.argmax_ref(z)
    assert np.array_equal(got, ref) and len(np.unique(ref[mc.CAPS["argmax"] * 256:])) == 2


# ---------------------------------------------------------------------------------------------------------------------------- NCHW -> NHWC
def _run_permute(hip, x):
    n, c, h, w = x.shape
    xb, yb = Buf((n * c * h * w, 1), x), Buf((n, h, w, c), None)
    hip.unet_nchw_to_nhwc(xb.ptr, yb.ptr, n, c, h, w, ST())
    y, ok = yb.read()
    assert ok and xb.unchanged()
    return y


@gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", mc.PERMUTE_HW, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", mc.PERMUTE_CS)
def test_nchw_to_nhwc_is_the_transpose(hip, c, hw, n):
    x = mc.permute_input(n, c, hw[0], hw[1], c + n)
    assert same_bits(_run_permute(hip, x), mc.permute_ref(x))


@gpu
def test_nchw_to_nhwc_grid_stride_loop_wraps(hip):
    x = np.random.RandomState(1).randn(1, 3, 699095, 1).astype(F)
    assert x.size == mc.second_trip("permute", 133)
    assert same_bits(_run_permute(hip, x), mc.permute_ref(x))


# ---------------------------------------------------------------------------------------------------------------------- unet_softmax_ce
def _run_ce(hip, z, lab, ls, clip, ldz=None, lddz=None, want=("prob", "dz", "loss", "correct"), scales=CE_SCALES):
    """-> dict of the requested outputs (prob, dz float32 arrays; loss, correct floats); asserts sentinels and inputs"""
    p, k = z.shape
    zb = Buf((p, k), z, ldz)
    lb = Buf((p, k), lab, None, 0, "i32") if lab is not None else None
    pb = Buf((p, k), None) if "prob" in want else None
    db = Buf((p, k), None, lddz) if "dz" in want else None
    res = Buf((2, 1), None, 3)                                                        # loss and count three floats apart
    nb = hip.unet_softmax_ce_workspace(p)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    ptr = lambda b: None if b is None else b.ptr
    loss_ptr = res.ptr if "loss" in want else None
    corr_ptr = ctypes.c_void_p(res.ptr.value + 12) if "correct" in want else None
    hip.unet_softmax_ce(zb.ptr, zb.ld, ptr(lb), ptr(pb), ptr(db), db.ld if db else k, p, k, ls, scales[0], scales[1], clip, loss_ptr, corr_ptr,
                        ctypes.c_void_p(ws.data_ptr()), nb, ST())
    out = {}
    assert zb.unchanged() and (lb is None or lb.unchanged())
    for name, b in (("prob", pb), ("dz", db)):
        if b is not None:
            out[name], ok = b.read()
            assert ok, name
    r, ok = res.read()
    assert ok
    for i, name in enumerate(("loss", "correct")):
        if name in want:
            out[name] = float(r[i, 0])
        else:
            assert r[i, 0] == F(mc.SENT)
    return out


FIGURES = {}                         # worst error / bound per kernel and output, printed by the last test of this file


def _note(name, value):
    FIGURES[name] = max(FIGURES.get(name, 0.0), float(value))


def _check_ce(got, ref, k, tag):
    ex_p = mc.ce_excess(got["prob"], ref["prob"], ref["prob_bound"])
    ex_d = mc.ce_excess(got["dz"], ref["dz"], ref["dz_bound"])
    ex_l = abs(got["loss"] - ref["loss"]) / ref["loss_bound"] if ref["loss_bound"] > 0 else float(got["loss"] != 0)
    print("softmax_ce", tag, "error / bound: prob %.3f, dlogits %.3f, loss %.3f" % (ex_p, ex_d, ex_l))
    _note("softmax_ce prob", ex_p), _note("softmax_ce dlogits", ex_d), _note("softmax_ce loss", ex_l)
    assert got["correct"] == ref["correct"], (got["correct"], ref["correct"])
    assert ex_p <= 1 and ex_d <= 1 and ex_l <= 1, (ex_p, ex_d, ex_l)


@gpu
@pytest.mark.parametrize("strided", [0, 1], ids=["dense", "ldz_k3_lddz_k1"])
@pytest.mark.parametrize("regime", mc.CE_REGIMES)
@pytest.mark.parametrize("k", mc.CE_KS)
def test_softmax_ce_matches_fp64_inside_the_derived_bounds(hip, k, regime, strided):
    z, lab = mc.ce_logits(mc.CE_P, k, regime, 10 * k), mc.ce_labels(mc.CE_P, k, k)
    assert (lab.sum(-1) == 0).any()
    for ls in (0.0, 0.1):
        got = _run_ce(hip, z, lab, ls, 0.0, k + 3 if strided else None, k + 1 if strided else None)
        ref = mc.ce_ref(z, lab, ls, 0.0, *CE_SCALES)
        _check_ce(got, ref, k, (k, regime, ls))
        if regime == "gap_200" and k > 1:
            assert (got["prob"] == 0).any() and (got["prob"].max(-1) == 1).all()
        if ls == 0.0:                            # an all-zero label row: no loss term, so no gradient either (ysum = 0)
            assert not got["dz"][lab.sum(-1) == 0].any()


@gpu
@pytest.mark.parametrize("k,clip", [(2, 1e-7), (3, 1e-7), (7, 1e-7), (3, 1e-3)])
def test_softmax_ce_clip_path_matches_fp64_inside_the_derived_bounds(hip, k, clip):
    p = mc.CE_P * 3
    z, moved, outside = mc.ce_clip_case(p, k, clip, k)
    assert moved <= mc.CE_CLIP_MOVED_CAP and outside
    lab = mc.ce_labels(p, k, k)
    for ls in (0.0, 0.1):
        for strided in (0, 1):
            got = _run_ce(hip, z, lab, ls, clip, k + 3 if strided else None, k + 1 if strided else None)
            ref = mc.ce_ref(z, lab, ls, clip, *CE_SCALES)
            _check_ce(got, ref, k, (k, "clip", clip, ls))


@gpu
def test_softmax_ce_single_pixel(hip):
    for k in mc.CE_KS:
        z, lab = mc.ce_logits(1, k, "ordinary", k), mc.ce_labels(1, k, k, empty_every=0)
        for ls, clip in CE_CONFIGS:
            _check_ce(_run_ce(hip, z, lab, ls, clip), mc.ce_ref(z, lab, ls, clip, *CE_SCALES), k, (k, "P = 1", ls, clip))


@gpu
@pytest.mark.parametrize("ls,clip", CE_CONFIGS)
def test_softmax_ce_null_forms_equal_the_full_call_bit_for_bit(hip, ls, clip):
    k = 7
    z, lab = mc.ce_logits(mc.CE_P, k, "ordinary", 3), mc.ce_labels(mc.CE_P, k, 3)
    full = _run_ce(hip, z, lab, ls, clip, k + 3, k + 1)
    forms = [(("prob",), False), (("loss", "correct"), True), (("prob", "loss", "correct"), True), (("dz",), True), (("dz", "loss"), True),
             (("prob", "dz", "correct"), True), (("prob", "loss"), True), (("correct",), True)]
    for want, with_labels in forms:
        got = _run_ce(hip, z, lab if with_labels else None, ls, clip, k + 3, k + 1, want)
        assert set(got) == set(want)
        for name in want:
            if name in ("prob", "dz"):
                assert same_bits(got[name], full[name]), (want, name)
            else:
                assert got[name] == full[name], (want, name)


@gpu
def test_softmax_ce_grid_stride_loop_wraps(hip):
    p, k = mc.second_trip("softmax_ce", 201), 2
    z, lab = mc.ce_logits(p, k, "ordinary", 5), mc.ce_labels(p, k, 5)
    scales = (1.0 / p, 1.0 / p)
    got = _run_ce(hip, z, lab, 0.0, 0.0, scales=scales)
    ref = mc.ce_ref(z, lab, 0.0, 0.0, *scales)
    _check_ce(got, ref, k, "second trip")
    first = mc.ce_ref(z[:mc.CAPS["softmax_ce"] * 256], lab[:mc.CAPS["softmax_ce"] * 256], 0.0, 0.0, *scales)
    assert abs(first["loss"] - ref["loss"]) > 4 * ref["loss_bound"] and first["correct"] < ref["correct"]          # the tail counts


# ---------------------------------------------------------------------------------------------------------------------- unet_adam_keras
def _run_adam(hip, th, g, m, v, alpha):
    n = th.size
    bufs = [Buf((n, 1), a) for a in (th, g, m, v)]
    hip.unet_adam_keras(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, alpha, mc.ADAM_HYPER["beta1"], mc.ADAM_HYPER["beta2"],
                        mc.ADAM_HYPER["eps"], ST())
    outs = [b.read() for b in (bufs[2], bufs[3], bufs[0])]
    assert all(ok for _, ok in outs) and bufs[1].unchanged()
    return [a[:, 0] for a, _ in outs]


def _check_adam(got, th, g, m, v, alpha, tag):
    ref, bound = mc.adam_ref(th, g, m, v, alpha)
    for name, a, r, b in zip(("m", "v", "theta"), got, ref, bound):
        ex = float((np.abs(a.astype(D) - r) / b).max())
        print("adam", tag, name, "error / bound = %.3f" % ex)
        _note("adam " + name, ex)
        assert ex <= 1, (tag, name, ex, int(np.argmax(np.abs(a.astype(D) - r) / b)))


@gpu
@pytest.mark.parametrize("t", [1, 7, 1000])
@pytest.mark.parametrize("n", mc.ADAM_NS)
def test_adam_single_step_matches_fp64_on_m_v_and_theta(hip, n, t):
    th, g, m, v, block = mc.adam_state(n, n)
    alpha = mc.adam_alpha(t)
    got = _run_adam(hip, th, g, m, v, alpha)
    _check_adam(got, th, g, m, v, alpha, (n, t))
    zg = block == mc.ADAM_STATES.index("zero_gradient")
    assert same_bits(got[2][zg], th[zg]) and not mc.bits(got[0][zg]).any() and not mc.bits(got[1][zg]).any()


@gpu
def test_adam_grid_stride_loop_wraps(hip):
    n = 4 * mc.second_trip("adam", 77)
    th, g, m, v, _ = mc.adam_state(n, 3)
    alpha = mc.adam_alpha(2)
    got = _run_adam(hip, th, g, m, v, alpha)
    _check_adam(got, th, g, m, v, alpha, "second trip")
    tail = slice(4 * mc.CAPS["adam"] * 256, None)                  # (the last block: theta large against the update, so look at m)
    assert (got[0][tail] != m[tail]).all() and (got[1][tail] != v[tail]).any()


# ------------------------------------------------------------------------------------------------------------------------- bad arguments
def _raw(hip, name):
    return getattr(hip.cdll, name)             # the bound function itself: returns the status instead of raising


@gpu
def test_bad_arguments_are_refused_and_leave_the_outputs_alone(hip):
    n, h, w, c = 1, 4, 4, 8
    f32 = lambda shape, ld=None, off=0: Buf(shape, np.ones(shape, F), ld, off)
    out = lambda shape, ld=None, kind="f32": Buf(shape, None, ld, 0, kind)
    checked = []

    def refused(rc, want, *outs):
        torch.cuda.synchronize()
        assert rc == want, (rc, want, len(checked))
        for b in outs:
            assert b.unchanged(), len(checked)
        checked.append(rc)

    fwd, bwd, drop = _raw(hip, "unet_maxpool2x2_fwd"), _raw(hip, "unet_maxpool2x2_bwd"), _raw(hip, "unet_dropout")
    for hh, ww, cc, ldx, ldy, b16 in [(3, 4, 8, 8, 8, 0), (4, 5, 8, 8, 8, 0), (4, 4, 8, 7, 8, 0), (4, 4, 8, 8, 7, 0), (4, 4, 6, 6, 6, 1), (4, 4, 8, 10, 8, 1)]:
        x, y, idx = f32((n, 4, 5, 8), 10), out((n, 2, 2, 8), 10), out((n, 2, 2, 8), None, "u8")
        refused(fwd(x.ptr, ldx, y.ptr, ldy, idx.ptr, n, hh, ww, cc, b16, ST()), EINVAL, y, idx)
        dy, ib, dx = f32((n, 2, 2, 8), 10), Buf((n, 2, 2, 8), np.zeros((n, 2, 2, 8), np.uint8), None, 0, "u8"), out((n, 4, 5, 8), 10)
        refused(bwd(dy.ptr, ldy, ib.ptr, dx.ptr, ldx, n, hh, ww, cc, 0, b16, ST()), EINVAL, dx)
    for cc, ldx, ldo, rate, b16 in [(8, 7, 8, 0.5, 0), (8, 8, 7, 0.5, 0), (8, 8, 8, 1.0, 0), (8, 8, 8, -0.25, 0), (6, 6, 6, 0.5, 1), (8, 8, 10, 0.5, 1)]:
        x, o = f32((16, 8), 10), out((16, 8), 10)
        refused(drop(x.ptr, ldx, o.ptr, ldo, 16, cc, None, 1, rate, b16, ST()), EINVAL, o)
    # Adam: n % 4 != 0, and each of the four pointers off the 16-byte grid
    adam = _raw(hip, "unet_adam_keras")
    bufs = [Buf((16, 1), np.ones(16, F), None, 4) for _ in range(4)]
    refused(adam(*[b.ptr for b in bufs], 6, 1e-3, 0.9, 0.999, 1e-7, ST()), EINVAL, *bufs)
    for bad in range(4):
        ptrs = [ctypes.c_void_p(b.ptr.value + (4 if i == bad else 0)) for i, b in enumerate(bufs)]
        refused(adam(*ptrs, 8, 1e-3, 0.9, 0.999, 1e-7, ST()), EINVAL, *bufs)
    # softmax + cross-entropy
    ce, k, p = _raw(hip, "unet_softmax_ce"), 3, 300
    z, lab = f32((p, k)), Buf((p, k), np.zeros((p, k), np.int32), None, 0, "i32")
    nb = hip.unet_softmax_ce_workspace(p)
    assert nb == 2 * 16 and hip.unet_softmax_ce_workspace(mc.second_trip("softmax_ce", 1)) == 1024 * 16
    ws = Buf((nb, 1), None, None, 0, "u8")
    for clip, labels, ldz, lddz, wsb, want in [(0.5, True, k, k, nb, EINVAL), (0.75, True, k, k, nb, EINVAL), (-1e-7, True, k, k, nb, EINVAL),
                                               (0.0, False, k, k, nb, EINVAL), (0.0, True, k - 1, k, nb, EINVAL), (0.0, True, k, k - 1, nb, EINVAL),
                                               (0.0, True, k, k, nb - 1, ENOSPC), (0.0, True, k, k, 16, ENOSPC)]:
        prob, dz, res = out((p, k)), out((p, k)), out((2, 1))
        rc = ce(z.ptr, ldz, lab.ptr if labels else None, prob.ptr, dz.ptr, lddz, p, k, 0.0, 1.0, 1.0, clip, res.ptr, ctypes.c_void_p(res.ptr.value + 4),
                ws.ptr, wsb, ST())
        refused(rc, want, prob, dz, res, ws)
    prob, res = out((p, k)), out((2, 1))                  # a loss or a count without labels
    refused(ce(z.ptr, k, None, prob.ptr, None, k, p, k, 0.0, 1.0, 1.0, 0.0, res.ptr, None, ws.ptr, nb, ST()), EINVAL, prob, res, ws)
    refused(ce(z.ptr, k, None, prob.ptr, None, k, p, k, 0.0, 1.0, 1.0, 0.0, None, res.ptr, ws.ptr, nb, ST()), EINVAL, prob, res, ws)
    o = out((p, 1), None, "i32")
    refused(_raw(hip, "unet_argmax")(z.ptr, k - 1, o.ptr, p, k, ST()), EINVAL, o)
    refused(_raw(hip, "unet_argmax")(z.ptr, k, o.ptr, 0, k, ST()), EINVAL, o)
    y = out((p, k))
    refused(_raw(hip, "unet_nchw_to_nhwc")(z.ptr, y.ptr, 1, 0, p, 1, ST()), EINVAL, y)
    assert len(checked) == 12 + 6 + 5 + 8 + 2 + 3


@gpu
def test_print_the_worst_error_over_bound_figures(hip):
    # (runs last in this file: the figures DESIGN.md quotes)
    for name in sorted(FIGURES):
        print("worst error / bound: %-20s %.3f" % (name, FIGURES[name]))
    assert all(v <= 1 for v in FIGURES.values())
