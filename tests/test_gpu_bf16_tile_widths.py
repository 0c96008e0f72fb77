"""The 128-channel-tile (128-column-tile) bf16 kernels of semantic-segmentation-unet_amd/csrc/conv_bf16.hip against the fp64 oracle.

The launchers take the wide tile only when it still gives every compute unit a workgroup, so the small-shape oracle tests of
tests/test_gpu_kernels.py run the 64-wide kernels.  Here every case is sized from the device's CU count to sit exactly at that threshold
(tests/bf16_tile_cases.py), asserts the launcher's own answer (unet_conv3x3_bf16_tile_channels / unet_convT2x2_bf16_tile_columns) before it runs,
and holds the fp32-output per-tile kernel to the oracle on the bf16-valued operands twice: the family's 2e-5 of the output range, and a
per-element bound derived from the operation.  Every other variant the launcher can choose (bf16-stored input, bf16-stored output = the persistent
form for 3x3, fused BatchNorm sums forward and backward, BatchNorm-apply on load, LDS-DMA staging of the transposed conv) is tied to that result
bit for bit wherever tests/test_gpu_kernels.py promises bit identity, and to the oracle otherwise.  Outputs land in the upper channel half of a
sentinel-filled concat buffer with a sentinel tail; inputs have padded leading dimensions and must come back unchanged.  With the full-size
bit-identity tests (persistent == per-tile, DMA == register staging) this closes the chain from the fp64 oracle to the kernels the benchmark runs.

Two weight-gradient cases cover the branches of the CU-sized plans that no other oracle case reaches (see bf16_tile_cases.wgrad3_walk_case,
convt_wgrad_direct_case).  The unmarked part runs without a GPU: the bound is neither vacuous nor too tight on the committed cases."""
import ctypes

import numpy as np
import pytest
import torch

import bf16_tile_cases as bc
from conftest import pkg
from oracle import unet_numpy as on

gpu = pytest.mark.gpu               # the device part; everything else runs anywhere

DEV = "cuda"
F, D = bc.F, bc.D
BF = torch.bfloat16


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


# ------------------------------------------------------------------------------------------------------------------------------ CPU part
def test_threshold_shapes_are_the_smallest_wide_ones():
    # on 256 compute units: the N column of the issue's table; one image fewer falls below the threshold for any CU count
    assert [bc.images_at_threshold(256, *bc.RAGGED, c) for c in (128, 256, 512)] == [64, 32, 16]
    assert bc.images_at_threshold(256, *bc.ALIGNED, 256) == 128 and bc.pixel_tiles(*bc.RAGGED) == 4 and bc.pixel_tiles(*bc.ALIGNED) == 1
    for c in (96, 256, 304):
        for hw, cols in ((bc.RAGGED, 128), (bc.RAGGED, 512), (bc.ALIGNED, 256)):
            n = bc.images_at_threshold(c, *hw, cols)
            assert n * bc.pixel_tiles(*hw) * (cols // 128) >= c > (n - 1) * bc.pixel_tiles(*hw) * (cols // 128)
    s = bc.channel_scale(128)
    assert s.max() / s.min() == 4096 and not (s[:64] == s[64:]).any()          # channel c and c ^ 64 never share a scale


def test_dispatch_queries_follow_the_launch_rule():
    # host-only queries; the CU count is the device's (256 where there is none)
    L, c = pkg("_lib").lib(), cus()
    for (hw, ci, co, below, want) in bc.CONV_FWD.values():
        n = bc.images_at_threshold(c, *hw, co) - below
        assert L.unet_conv3x3_bf16_tile_channels(n, *hw, ci, co) == want
    assert L.unet_conv3x3_bf16_tile_channels(4 * c, 16, 32, 64, 192) == 64        # Cout % 128 != 0: never wide
    assert L.unet_conv3x3_bf16_tile_channels(1, 16, 32, 48, 128) == 0             # unsupported
    n = bc.images_at_threshold(c, *bc.RAGGED, 128)
    assert L.unet_conv3x3_bf16_tile_channels(n, *bc.RAGGED, 256, 128) == 128 and L.unet_conv3x3_bf16_tile_channels(n, *bc.RAGGED, 128, 64) == 64
    for (ci, co, w32, w16) in bc.CONVT_FWD.values():
        n = bc.convt_fwd_images(c, co)
        assert L.unet_convT2x2_bf16_tile_columns(n, *bc.RAGGED, ci, co, 0, 0) == w32 and L.unet_convT2x2_bf16_tile_columns(n, *bc.RAGGED, ci, co, 0, 1) == w16
        assert L.unet_convT2x2_bf16_tile_columns(n - 1, *bc.RAGGED, ci, co, 0, 0) == 64
    n = bc.images_at_threshold(c, *bc.RAGGED, 256)
    assert [L.unet_convT2x2_bf16_tile_columns(n - d, *bc.RAGGED, 256, 64, 1, s) for d in (0, 1) for s in (0, 1)] == [128, 128, 64, 64]
    assert L.unet_convT2x2_bf16_tile_columns(1, 4, 4, 96, 64, 0, 0) == 0


@pytest.mark.parametrize("name", ["fwd_64_128", "fwd_128_256", "fwd_64_256_aligned"])
def test_bound_holds_for_fp32_orders_and_rejects_near_misses(name):
    # the committed case shrunk to one image: fp32 evaluations in three summation orders stay inside both bounds (not too tight) ...
    (h, w), ci, co, _, _ = bc.CONV_FWD[name]
    x, wt, b = bc.conv_fwd_inputs(name, 1)
    ref, bound = bc.conv_fwd_ref(x, wt, b)
    worst = 0.0
    for order in ("chunks", "taps", "reverse"):
        got = bc.conv_fwd_fp32(x, wt, b, order)
        assert bc.violations(got, ref, bound) == 0 and bc.family_bound_ok(got, ref), order
        assert bc.violations(np.maximum(got, 0), np.maximum(ref, 0), bound) == 0
        worst = max(worst, float((np.abs(got.astype(D) - ref) / bound).max()))
    assert 1e-4 < worst < 1.0                       # ... and reach a visible fraction of it: the bound is a bound on this arithmetic, not on air
    # ... and is not vacuous: every element's allowance is below 2^-12 of that element's own magnitude sum, and each near miss leaves it
    assert (9 * ci + 1) * bc.ULP < 2.0 ** -12
    if w % 32:                                      # one tap dropped at the last column of the ragged tile (the tap that reaches back across the tile edge)
        bad = bc.conv_fwd_fp32(x, wt, b, "chunks", drop_tap_at=(w - 1, 3))
        assert bc.violations(bad, ref, bound) > 0
        only = np.abs(bad.astype(D) - ref) > bound
        assert only[:, :, :w - 1].sum() == 0 and only[:, :, w - 1].mean() > 0.9
    bad = bc.conv_fwd_fp32(x, wt, b, "chunks", bias_from=np.arange(co) ^ 64)          # the bias of channel c taken from channel c ^ 64
    assert (np.abs(bad.astype(D) - ref) > bound).mean() > 0.95                           # all over the tensor
    # a wrong SMALL channel passes the family's max-based bound and only the per-element one sees it
    small = int(np.argmin(bc.channel_scale(co)))
    bad = bc.conv_fwd_fp32(x, wt, b, "chunks").astype(D)
    bad[..., small] = ref[..., small] * (1 + 2.0 ** -9)
    assert bc.family_bound_ok(bad, ref) and bc.violations(bad, ref, bound) > 0


def test_apply_on_load_reference_and_the_padding_near_miss():
    name = "fwd_128_256"
    x, wt, b = bc.conv_fwd_inputs(name, 1)
    r, sc, sh = bc.norm_inputs(name, 1)
    y = bc.norm_operand(r, sc, sh)
    assert bc.is_bf16(y) and (y[..., 5] == sh[5]).all()                                 # the zero scale leaves the shift alone
    ref, bound = bc.conv_fwd_ref(y, wt, b)
    assert bc.violations(bc.conv_fwd_fp32(y, wt, b, "chunks"), ref, bound) == 0
    pad0 = np.zeros((1, y.shape[1] + 2, y.shape[2] + 2, y.shape[3]), F); pad0[:, 1:-1, 1:-1] = y
    assert bc.violations(bc.conv_valid_fp64(pad0, wt, b), ref, bound) == 0                # the helper is the same convolution
    for half in (0, 1):                             # the padding value an unmasked apply forms, kept for one 64-channel half of the input
        bad = bc.conv_valid_fp64(bc.norm_operand_padded_wrong(r, sc, sh, half), wt, b)
        wrong = np.abs(bad - ref) > bound
        assert wrong[:, 1:-1, 1:-1].sum() == 0 and wrong[:, 0].mean() > 0.9 and wrong[:, :, -1].mean() > 0.9      # the border pixels, only them


def test_statistics_check_tells_swapped_halves():
    name = "fwd_128_256"
    (h, w), ci, co, _, _ = bc.CONV_FWD[name]
    x, wt, b = bc.conv_fwd_inputs(name, 1)
    y = np.maximum(bc.conv_fwd_fp32(x, wt, b, "chunks"), 0)
    part, rows = bc.tile_partials(y, y, 1, h, w)
    assert rows == bc.pixel_tiles(h, w) and bc.stats_ok(part, rows, y, y)
    assert bc.stats_ok(part.astype(F), rows, y, y)                                      # rows rounded to fp32: inside
    assert not bc.stats_ok(bc.swap_halves(part, co), rows, y, y)                        # the two halves of every 128-tile exchanged
    one = part.copy(); one[1, 2] = part[0, 2]                                           # ONE row of the second half written from the first
    assert not bc.stats_ok(one, rows, y, y)


def test_data_gradient_and_transposed_references_hold_fp32_orders():
    dz, wt, _ = bc.conv_dgrad_inputs("dgrad_64_128", 1)
    ref, bound = bc.conv_dgrad_ref(dz, wt)
    wr = np.ascontiguousarray(wt[::-1, ::-1].transpose(0, 1, 3, 2))                       # the data gradient is the forward of the flipped kernel
    for order in ("chunks", "taps"):
        assert bc.violations(bc.conv_fwd_fp32(dz, wr, np.zeros(wt.shape[2], F), order), ref, bound) == 0
    x, wt, b = bc.convt_fwd_inputs("convt_fwd_128_64", 1)
    ref, bound = bc.convt_fwd_ref(x, wt, b)
    n, h, w, ci = x.shape
    for ks in (32, 128):                             # chunks of 32 reduce channels (the kernel's) and one sum
        acc = np.zeros((n, h, 2, w, 2, wt.shape[2]), F) + b
        for k in range(0, ci, ks):
            acc = (acc + np.einsum("nijc,abdc->niajbd", x[..., k:k + ks], wt[..., k:k + ks]).astype(F)).astype(F)
        assert bc.violations(acc.reshape(ref.shape), ref, bound) == 0
    dz, wt, _ = bc.convt_dgrad_inputs("convt_dgrad_256_64", 1)
    ref, bound = bc.convt_dgrad_ref(dz, wt)
    got = np.einsum("niajbd,abdc->nijc", dz.reshape(1, h, 2, w, 2, -1), wt).astype(F)
    assert bc.violations(got, ref, bound) == 0


def test_weight_gradient_plans_and_the_branches_the_oracle_cases_reach():
    # the audit in executable form: the restated plan gives the library's workspace for every existing oracle case and for the new one, and
    # says which branch each reaches (on 256 CUs: splits 2, 12, 8, 32, 1, 45 -- all == strip-chunks or 1, two-row chunks)
    L, c = pkg("_lib").lib(), cus()
    old = [(1, 4, 32, 64, 64), (2, 6, 40, 64, 128), (1, 7, 33, 128, 64), (1, 64, 32, 64, 64), (2, 4, 32, 1024, 1024), (3, 10, 70, 192, 64)]
    new = bc.wgrad3_walk_case(c)
    for s in old + ([new] if new else []):
        splits, n_sc, rpc, cps = bc.wgrad3_plan(c, *s)
        assert L.unet_conv3x3_wgrad_bf16_workspace(*s) == (splits * 9 * s[3] * s[4] * 4 if splits > 1 else 16), s
        if c == 256 and s in old:
            assert splits in (1, n_sc) and (rpc == 2 or cps == 1)
    if c == 256:
        assert new is not None
    for s, want in (((1, 4, 32, 128, 64), 4), ((2, 6, 40, 128, 128), 24), ((1, 8, 16, 256, 128), 8), ((3, 5, 70, 128, 64), 45), ((2, 4, 8, 1024, 512), 4)):
        if c == 256:
            assert L.unet_convT2x2_wgrad_bf16_workspace(*s) == want * 4 * s[3] * s[4] * 4
    assert L.unet_convT2x2_wgrad_bf16_workspace(*bc.convt_wgrad_direct_case(c)) == 16


# --------------------------------------------------------------------------------------------------------------------------- device part
class In:
    """an input tensor [pixels][C] with a padded leading dimension, the padding filled with sentinels; fp32 or bf16 storage of the same values"""

    def __init__(self, vals, bf16=False, pad=8):
        v = np.asarray(vals, F).reshape(-1, vals.shape[-1])
        self.bf16, self.c, self.ld = int(bf16), v.shape[1], v.shape[1] + pad
        host = np.full((v.shape[0], self.ld), bc.SENT16 if bf16 else bc.SENT, F)
        host[:, :self.c] = v
        self.t = torch.as_tensor(host).to(DEV)
        if bf16:
            self.t = self.t.to(BF)
            assert torch.equal(self.t.float()[:, :self.c].cpu(), torch.as_tensor(v))     # the values are bf16-representable
        self.keep = self.t.clone()
        self.ptr = P(self.t)

    def unchanged(self):
        return torch.equal(self.t.view(torch.int16 if self.bf16 else torch.int32), self.keep.view(torch.int16 if self.bf16 else torch.int32))


class Out:
    """the upper channel half of a sentinel-filled concat buffer [pixels][2 C], followed by a sentinel tail"""

    def __init__(self, npix, c, bf16=False):
        self.bf16, self.c, self.ld, self.npix = int(bf16), c, 2 * c, npix
        self.sent = bc.SENT16 if bf16 else bc.SENT
        self.flat = torch.full((npix * self.ld + bc.TAIL,), self.sent, dtype=BF if bf16 else torch.float32, device=DEV)
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + c * self.flat.element_size())

    def vals(self):
        return self.flat[:self.npix * self.ld].view(self.npix, self.ld)[:, self.c:]

    def intact(self):
        body = self.flat[:self.npix * self.ld].view(self.npix, self.ld)
        return bool((body[:, :self.c] == self.sent).all()) and bool((self.flat[self.npix * self.ld:] == self.sent).all()) and bool((self.vals() != self.sent).all())


class Ref:
    def __init__(self, ref, bound):
        self.ref = torch.as_tensor(ref.reshape(-1, ref.shape[-1])).to(DEV)
        self.bound = torch.as_tensor(bound.reshape(-1, ref.shape[-1])).to(DEV)

    def check(self, got, relu=0, what=""):
        """both bounds of the family for an fp32 output: 2e-5 of the output range, and the per-element bound"""
        ref = self.ref.clamp_min(0) if relu else self.ref
        d = (got.double() - ref).abs()
        fam, per = d.max().item() / ref.abs().max().item(), (d / self.bound.clamp_min(1e-300)).max().item()
        print("%s relu %d: max|err| / max|ref| = %.3g (< 2e-5), max err / bound = %.3g (<= 1)" % (what, relu, fam, per))
        assert fam < 2e-5, what
        assert not bool((d > self.bound).any()), what


def parts(blocks, rows):
    return torch.full((blocks * rows * 128,), float("nan"), device=DEV)


def nbytes(t):
    return t.numel() * t.element_size() if t is not None else 0


def stats_check(part, rows, y, second, slope2=0.0):
    assert not bool(torch.isnan(part).any())                                            # every row of every block written
    assert bc.stats_ok(part.cpu().numpy(), rows, y.float().cpu().numpy(), second if isinstance(second, np.ndarray) else second.float().cpu().numpy(), slope2)


def skip_unless_fits(n, elems_per_image):
    if n < 1 or n * elems_per_image * 4 >= bc.OPERAND_LIMIT:
        pytest.skip("%d compute units: no %d-image operand below the 2 GiB limit sits at the tile-width threshold" % (cus(), n))


@gpu
@pytest.mark.parametrize("name", list(bc.CONV_FWD))
def test_conv3x3_fwd_wide_tiles_match_oracle(hip, name):
    # reaches conv_bf16_kernel_128, _stats_kernel_128, _norm_kernel_128, _norm_stats_kernel_128, _stream_kernel_128, _stream_stats_kernel_128
    # (ragged cases) and _stream_in_kernel_128, _stream_in_stats_kernel_128 (aligned case); "_below" the same forms of the 64-channel tiles
    (h, w), ci, co, below, want = bc.CONV_FWD[name]
    n = bc.images_at_threshold(cus(), h, w, co) - below
    skip_unless_fits(n, h * w * max(ci + 8, 2 * co))
    assert hip.unet_conv3x3_bf16_supported(n, h, w, ci, co) == 1
    assert hip.unet_conv3x3_bf16_tile_channels(n, h, w, ci, co) == want
    npix, rows = n * h * w, hip.unet_conv3x3_bf16_stats_rows(n, h, w, ci, co)
    assert rows == n * bc.pixel_tiles(h, w)
    x, wt, b = bc.conv_fwd_inputs(name, n)
    wd, bd = torch.as_tensor(wt).to(DEV), torch.as_tensor(b).to(DEV)
    wp = torch.empty(hip.unet_conv3x3_bf16_packed_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_conv3x3_bf16_pack_weights(P(wd), P(wp), ci, co, 0, ST())

    def call(xin, out, relu, part=None, sc=None, sh=None):
        hip.unet_conv3x3_fwd_bf16(xin.ptr, xin.ld, xin.bf16, P(sc) if sc is not None else None, P(sh) if sh is not None else None, P(wp), P(bd),
                                  out.ptr, out.ld, out.bf16, n, h, w, ci, co, relu, P(part) if part is not None else None, nbytes(part), ST())
        return out

    def variants(R, x32, x16, sc, sh, what):
        for relu in (0, 1):
            base = call(x32, Out(npix, co), relu, None, sc, sh)                         # fp32 in / fp32 out, per tile: the one held to the oracle
            R.check(base.vals(), relu, what + " fp32->fp32")
            assert base.intact()
            part = parts(co // 64, rows)
            o = call(x32, Out(npix, co), relu, part, sc, sh)                            # + forward sums: same tensor, bit for bit
            assert torch.equal(o.vals(), base.vals()) and o.intact()
            stats_check(part, rows, base.vals(), base.vals())
            o = call(x16, Out(npix, co), relu, None, sc, sh)                            # bf16-stored input == the same values as fp32
            assert torch.equal(o.vals(), base.vals()) and o.intact()
            want16 = base.vals().to(BF)                                                 # bf16-stored output == the fp32 output rounded to nearest even
            for xin in (x32, x16):                                                      # (x16 without scale / shift: the persistent form)
                for stats in (0, 1):
                    p2 = parts(co // 64, rows) if stats else None
                    o = call(xin, Out(npix, co, bf16=True), relu, p2, sc, sh)
                    assert torch.equal(o.vals(), want16) and o.intact(), (what, relu, xin.bf16, stats)
                    assert p2 is None or torch.equal(p2, part), (what, relu, xin.bf16, stats)     # sums taken before the rounding, persistent == per tile
        return base

    x32, x16 = In(x), In(x, bf16=True)
    variants(Ref(*bc.conv_fwd_ref(x, wt, b)), x32, x16, None, None, name)
    assert x32.unchanged() and x16.unchanged()
    # BatchNorm-apply on load: its own reference on the operand the contract names, bf16(scale * r + shift) inside the image, 0 at the padding
    r, sc, sh = bc.norm_inputs(name, n)
    y = bc.norm_operand(r, sc, sh)
    r32, r16, scd, shd = In(r), In(r, bf16=True), torch.as_tensor(sc).to(DEV), torch.as_tensor(sh).to(DEV)
    base = variants(Ref(*bc.conv_fwd_ref(y, wt, b)), r32, r16, scd, shd, name + " on load")
    two = call(In(y, bf16=True), Out(npix, co), 1)                                     # == the BatchNorm output materialised as bf16, then the plain kernel
    assert torch.equal(two.vals(), base.vals())
    assert r32.unchanged() and r16.unchanged() and torch.equal(scd.cpu(), torch.as_tensor(sc)) and torch.equal(shd.cpu(), torch.as_tensor(sh))


@gpu
@pytest.mark.parametrize("name", list(bc.CONV_DGRAD))
def test_conv3x3_dgrad_wide_tiles_match_oracle(hip, name):
    # reaches conv_bf16_kernel_128 (no bias), _bnbwd_kernel_128, _stream_kernel_128, _stream_bnbwd_kernel_128 (ragged) and
    # _stream_in_kernel_128, _stream_in_bnbwd_kernel_128 (aligned)
    (h, w), ci, co, slices = bc.CONV_DGRAD[name]
    n = bc.images_at_threshold(cus(), h, w, ci)
    skip_unless_fits(n, h * w * max(co + 8, 2 * ci))
    assert hip.unet_conv3x3_bf16_tile_channels(n, h, w, co, ci) == 128 and (n == 1 or hip.unet_conv3x3_bf16_tile_channels(n - 1, h, w, co, ci) == 64)
    npix, rows = n * h * w, hip.unet_conv3x3_bf16_stats_rows(n, h, w, co, ci)
    assert rows == n * bc.pixel_tiles(h, w)
    dz, wt, rp = bc.conv_dgrad_inputs(name, n)
    wd = torch.as_tensor(wt).to(DEV)
    wpd = torch.empty(hip.unet_conv3x3_bf16_packed_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_conv3x3_bf16_pack_weights(P(wd), P(wpd), ci, co, 1, ST())
    R = Ref(*bc.conv_dgrad_ref(dz, wt))

    def call(zin, out, rin=None, c0=0, c1=0, part=None):
        hip.unet_conv3x3_dgrad_bf16(zin.ptr, zin.ld, zin.bf16, P(wpd), out.ptr, out.ld, out.bf16, n, h, w, ci, co,
                                    rin.ptr if rin else None, rin.ld if rin else 0, rin.bf16 if rin else 0, c0, c1,
                                    P(part) if part is not None else None, nbytes(part), ST())
        return out

    z32, z16 = In(dz), In(dz, bf16=True)
    base = call(z32, Out(npix, ci))
    R.check(base.vals(), 0, name + " fp32->fp32")
    assert base.intact()
    o = call(z16, Out(npix, ci))
    assert torch.equal(o.vals(), base.vals()) and o.intact()
    want16 = base.vals().to(BF)
    for zin in (z32, z16):                                                              # z16: the persistent form
        o = call(zin, Out(npix, ci, bf16=True))
        assert torch.equal(o.vals(), want16) and o.intact()
    for c0, c1 in slices:                                                               # the producer's BatchNorm-backward sums over dx[..., c0:c1)
        rs = np.ascontiguousarray(rp[..., c0:c1])
        rfull = np.zeros((npix, ci), F); rfull[:, c0:c1] = rs.reshape(npix, -1)         # channels outside the slice: sum dx * 0
        rp32, rp16 = In(rs), In(rs, bf16=True)
        part = parts(ci // 64, rows)
        o = call(z32, Out(npix, ci), rp32, c0, c1, part)
        assert torch.equal(o.vals(), base.vals()) and o.intact()
        stats_check(part, rows, base.vals(), rfull, 1e-3)
        for zin, rin, out16 in ((z32, rp16, 0), (z16, rp32, 0), (z32, rp16, 1), (z16, rp16, 1)):      # last: the persistent form
            p2 = parts(ci // 64, rows)
            o = call(zin, Out(npix, ci, bf16=bool(out16)), rin, c0, c1, p2)
            assert torch.equal(o.vals(), want16 if out16 else base.vals()) and o.intact(), (c0, c1, zin.bf16, rin.bf16, out16)
            assert torch.equal(p2, part), (c0, c1, zin.bf16, rin.bf16, out16)
        assert rp32.unchanged() and rp16.unchanged()
    assert z32.unchanged() and z16.unchanged()


@gpu
@pytest.mark.parametrize("name", list(bc.CONVT_FWD))
def test_convT2x2_fwd_wide_tiles_match_oracle(hip, name):
    # reaches convt_bf16_fwd_kernel_128, _fwd_stats_kernel_128 (fp32 input) and, where K > 256, _fwd_dma_kernel_128, _fwd_stats_dma_kernel_128;
    # with K <= 256 a bf16 input must take the 64-column tiles, two workgroups per CU
    ci, co, want32, want16 = bc.CONVT_FWD[name]
    h, w = bc.RAGGED
    n = bc.convt_fwd_images(cus(), co)
    skip_unless_fits(n, 4 * h * w * 2 * co)
    assert hip.unet_convT2x2_bf16_supported(n, h, w, ci, co) == 1
    assert hip.unet_convT2x2_bf16_tile_columns(n, h, w, ci, co, 0, 0) == want32 and hip.unet_convT2x2_bf16_tile_columns(n, h, w, ci, co, 0, 1) == want16
    npix, rows = 4 * n * h * w, hip.unet_convT2x2_bf16_stats_rows(n, h, w, ci, co, 0)
    assert rows == 4 * n * bc.pixel_tiles(h, w)
    x, wt, b = bc.convt_fwd_inputs(name, n)
    wd, bd = torch.as_tensor(wt).to(DEV), torch.as_tensor(b).to(DEV)
    wp = torch.empty(hip.unet_convT2x2_bf16_packed_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_convT2x2_bf16_pack_weights(P(wd), P(wp), ci, co, 0, ST())
    R = Ref(*bc.convt_fwd_ref(x, wt, b))

    def call(xin, out, part=None):
        hip.unet_convT2x2_fwd_bf16(xin.ptr, xin.ld, xin.bf16, P(wp), P(bd), out.ptr, out.ld, out.bf16, n, h, w, ci, co,
                                   P(part) if part is not None else None, nbytes(part), ST())
        return out

    x32, x16 = In(x), In(x, bf16=True)
    first = None
    for xin in (x32, x16):
        base = call(xin, Out(npix, co))
        R.check(base.vals(), 0, "%s input bf16 %d" % (name, xin.bf16))
        assert base.intact()
        part = parts(co // 64, rows)
        o = call(xin, Out(npix, co), part)
        assert torch.equal(o.vals(), base.vals()) and o.intact()
        stats_check(part, rows, base.vals(), base.vals())
        p2 = parts(co // 64, rows)
        o = call(xin, Out(npix, co, bf16=True), p2)
        assert torch.equal(o.vals(), base.vals().to(BF)) and o.intact() and torch.equal(p2, part)
        o = call(xin, Out(npix, co, bf16=True))
        assert torch.equal(o.vals(), base.vals().to(BF)) and o.intact()
        if first is None:
            first = (base, part)
        elif want16 == want32:                       # LDS-DMA staging == register staging, bit for bit (same tile width)
            assert torch.equal(base.vals(), first[0].vals()) and torch.equal(part, first[1])
    assert x32.unchanged() and x16.unchanged()


@gpu
@pytest.mark.parametrize("name", list(bc.CONVT_DGRAD))
def test_convT2x2_dgrad_wide_tiles_match_oracle(hip, name):
    # reaches convt_bf16_dgrad_kernel_128, _dgrad_bnbwd_kernel_128, _dgrad_dma_kernel_128, _dgrad_bnbwd_dma_kernel_128
    ci, co = bc.CONVT_DGRAD[name]
    h, w = bc.RAGGED
    n = bc.images_at_threshold(cus(), h, w, ci)
    skip_unless_fits(n, 4 * h * w * (co + 8))
    for s in (0, 1):
        assert hip.unet_convT2x2_bf16_tile_columns(n, h, w, ci, co, 1, s) == 128 and hip.unet_convT2x2_bf16_tile_columns(n - 1, h, w, ci, co, 1, s) == 64
    npix, rows = n * h * w, hip.unet_convT2x2_bf16_stats_rows(n, h, w, ci, co, 1)
    assert rows == n * bc.pixel_tiles(h, w)
    dz, wt, rp = bc.convt_dgrad_inputs(name, n)
    wd = torch.as_tensor(wt).to(DEV)
    wpd = torch.empty(hip.unet_convT2x2_bf16_packed_bytes(ci, co), dtype=torch.uint8, device=DEV)
    hip.unet_convT2x2_bf16_pack_weights(P(wd), P(wpd), ci, co, 1, ST())
    R = Ref(*bc.convt_dgrad_ref(dz, wt))

    def call(zin, out, rin=None, part=None):
        hip.unet_convT2x2_dgrad_bf16(zin.ptr, zin.ld, zin.bf16, P(wpd), out.ptr, out.ld, out.bf16, n, h, w, ci, co,
                                     rin.ptr if rin else None, rin.ld if rin else 0, rin.bf16 if rin else 0,
                                     P(part) if part is not None else None, nbytes(part), ST())
        return out

    z32, z16, rp32, rp16 = In(dz), In(dz, bf16=True), In(rp), In(rp, bf16=True)
    base = call(z32, Out(npix, ci))
    R.check(base.vals(), 0, name + " fp32->fp32")
    assert base.intact()
    part = parts(ci // 64, rows)
    o = call(z32, Out(npix, ci), rp32, part)
    assert torch.equal(o.vals(), base.vals()) and o.intact()
    stats_check(part, rows, base.vals(), rp.reshape(npix, ci), 1e-3)
    want16 = base.vals().to(BF)
    for zin in (z32, z16):                                                              # z16: LDS-DMA staging
        for out16 in (0, 1):
            o = call(zin, Out(npix, ci, bf16=bool(out16)))
            assert torch.equal(o.vals(), want16 if out16 else base.vals()) and o.intact(), (zin.bf16, out16)
            for rin in (rp32, rp16):
                p2 = parts(ci // 64, rows)
                o = call(zin, Out(npix, ci, bf16=bool(out16)), rin, p2)
                assert torch.equal(o.vals(), want16 if out16 else base.vals()) and o.intact(), (zin.bf16, out16, rin.bf16)
                assert torch.equal(p2, part), (zin.bf16, out16, rin.bf16)
    assert z32.unchanged() and z16.unchanged() and rp32.unchanged() and rp16.unchanged()


def _relerr(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@gpu
def test_conv3x3_wgrad_walk_with_partial_sums_matches_oracle(hip):
    # 1 < splits < strip-chunks, several steps per chunk, several chunks per strip: the branch of wgrad_bf16_plan no other oracle case reaches
    case = bc.wgrad3_walk_case(cus())
    if case is None:
        pytest.skip("%d compute units: no small 256 -> 256 shape with 1 < splits < strip-chunks" % cus())
    n, h, w, ci, co = case
    splits, n_sc, rpc, cps = bc.wgrad3_plan(cus(), *case)
    nb = hip.unet_conv3x3_wgrad_bf16_workspace(*case)
    assert nb == splits * 9 * ci * co * 4 and 1 < splits < n_sc and rpc >= 4 and cps >= 2
    rng = np.random.default_rng(7)
    x, dz = bc.bf16_round(rng.standard_normal((n, h, w, ci)).astype(F)), bc.bf16_round(rng.standard_normal((n, h, w, co)).astype(F))
    t = lambda a: np.ascontiguousarray(a.astype(D).transpose(0, 3, 1, 2))
    ref = on.conv_same_bwd(t(x), np.zeros((3, 3, ci, co)), t(dz))[1]
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    outs = []
    for bf16 in (False, True):                       # register staging, LDS-DMA staging
        xi, zi = In(x, bf16), In(dz, bf16)
        dw = torch.full((3, 3, ci, co), float("nan"), device=DEV)
        hip.unet_conv3x3_wgrad_bf16(xi.ptr, xi.ld, xi.bf16, zi.ptr, zi.ld, zi.bf16, P(dw), n, h, w, ci, co, P(ws), nb, ST())
        assert _relerr(dw.cpu().numpy().astype(D), ref) < 2e-5 and xi.unchanged() and zi.unchanged()
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])


@gpu
def test_convT2x2_wgrad_without_partial_sums_matches_oracle(hip):
    # more channel tiles than half the compute units: splits == 1, the kernel writes dw itself and no reduction pass runs
    n, h, w, ci, co = case = bc.convt_wgrad_direct_case(cus())
    assert hip.unet_convT2x2_wgrad_bf16_supported(*case) == 1
    nb = hip.unet_convT2x2_wgrad_bf16_workspace(*case)
    assert nb == 16
    rng = np.random.default_rng(8)
    x, dz = bc.bf16_round(rng.standard_normal((n, h, w, ci)).astype(F)), bc.bf16_round(rng.standard_normal((n, 2 * h, 2 * w, co)).astype(F))
    t = lambda a: np.ascontiguousarray(a.astype(D).transpose(0, 3, 1, 2))
    ref = on.deconv2x2_bwd(t(x), np.zeros((2, 2, co, ci)), t(dz))[1]
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    outs = []
    for bf16 in (False, True):
        xi, zi = In(x, bf16), In(dz, bf16)
        dw = torch.full((2, 2, co, ci), float("nan"), device=DEV)
        hip.unet_convT2x2_wgrad_bf16(xi.ptr, xi.ld, xi.bf16, zi.ptr, zi.ld, zi.bf16, P(dw), n, h, w, ci, co, P(ws), nb, ST())
        assert _relerr(dw.cpu().numpy().astype(D), ref) < 2e-5 and xi.unchanged() and zi.unchanged()
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])
