"""The references of the BatchNorm conditioning tests, checked on the CPU before a GPU is involved (tests/bn_conditioning_cases.py):
the fp64 references are the oracle's, the one-pass fp32 floor reproduces the error table it was introduced with, and a numpy fp32
restatement of the kernels' formulas (semantic-segmentation-unet_amd/csrc/norm.hip, ends_inline.h) stays inside every derived bound of
tests/test_gpu_bn_conditioning.py on every rung."""
import numpy as np
import pytest

import bn_conditioning_cases as bc
from oracle import unet_numpy as on

U = bc.U
N, H, W = 3, 10, 14


def nchw(a, n=N, h=H, w=W):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(n, h, w, -1).transpose(0, 3, 1, 2))


def flat(a):
    return a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1])


def test_fp64_references_equal_the_oracle_on_well_conditioned_data():
    P, C = N * H * W, 16
    rng = np.random.default_rng(3)
    r = np.maximum(rng.standard_normal((P, C)) + 0.3, 0).astype(np.float32)          # rung-0 data in every channel
    dy = rng.standard_normal((P, C)).astype(np.float32)
    gamma, beta, mm0, mv0 = bc.bn_params(C, 4)
    ref = bc.ref_forward(r, gamma, beta, mm0, mv0)
    y_o, cache = on.bn_train_fwd(nchw(r), gamma.astype(np.float64), beta.astype(np.float64), bc.EPS)
    _, inv_o, mu_o, var_o = cache
    for got, want in ((ref["mean"], mu_o), (ref["var"], var_o), (ref["invstd"], inv_o)):
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    y = ref["scale"] * r.astype(np.float64) + ref["shift"]
    assert np.abs(y - flat(y_o)).max() <= 1e-13 * np.abs(y_o).max()
    assert np.allclose(ref["mm"], bc.MOMENTUM * mm0.astype(np.float64) + (1 - bc.MOMENTUM) * mu_o, rtol=1e-13, atol=0)
    assert np.allclose(ref["mv"], bc.MOMENTUM * mv0.astype(np.float64) + (1 - bc.MOMENTUM) * var_o * P / (P - 1), rtol=1e-13, atol=0)
    # the one-pass formula in fp64 agrees with the two-pass reference while the channel is well conditioned
    r64 = r.astype(np.float64)
    one = bc.finalize64(r64.sum(0), (r64 * r64).sum(0), P, gamma, beta, mm0, mv0)
    for k in bc.STAT_KEYS:
        assert np.allclose(one[k], ref[k], rtol=1e-12, atol=1e-13)
    dr_o, dg_o, db_o = on.bn_train_bwd(nchw(dy), gamma.astype(np.float64), cache)
    sums = bc.ref_backward_sums(dy, r, ref["mean"], ref["invstd"])
    assert np.abs(sums["dbeta"] - db_o).max() <= 1e-13 * np.abs(db_o).max()
    assert np.abs(sums["dgamma"] - dg_o).max() <= 1e-12 * np.abs(dg_o).max()
    dz, _ = bc.ref_dz(dy, r, gamma, ref["mean"], ref["invstd"], sums["dgamma"], sums["dbeta"], relu=True)
    dz_o = flat(dr_o * (nchw(r) > 0))
    assert np.abs(dz - dz_o).max() <= 1e-12 * np.abs(dz_o).max()


# the table the floor emulation was introduced with: P = 3072, fp32 sums over 128-pixel rows combined in fp64; relative error of invstd
TABLE = [(0.5, 1.0, 7e-9), (10.0, 1.0, 8e-7), (30.0, 0.3, 3e-5), (100.0, 1.0, 1.1e-4), (100.0, 0.1, 8e-3)]


@pytest.mark.parametrize("mean,sigma,expected", TABLE)
def test_floor_emulation_reproduces_the_error_table(mean, sigma, expected):
    """The table's entries are taken as TYPICAL errors of a channel (the rms over 64 channels and both product forms is compared), not as
    the maximum over a rung that F_stat is: this checks the emulation, no kernel is held to it."""
    P, C, rows = 3072, 64, 24
    rng = np.random.default_rng(int(mean * 10 + sigma * 100))
    r = (mean + sigma * rng.standard_normal((P, C))).astype(np.float32)
    ones, zeros = np.ones(C, np.float32), np.zeros(C, np.float32)
    ref = bc.ref_forward(r, ones, zeros, zeros, ones)
    errs = []
    for s, ss in bc.floor_forward_sums(r, rows):
        emu = bc.finalize64(s, ss, P, ones, zeros, zeros, ones)
        errs.append(np.abs(emu["invstd"] - ref["invstd"]) / ref["invstd"])
    typical = float(np.sqrt(np.mean(np.square(errs))))                      # rms over 64 channels and both product forms
    print("mean %g sigma %g: rms relative error of invstd %.2e (table %.1e)" % (mean, sigma, typical, expected))
    assert expected / 3 <= typical <= expected * 3, (mean, sigma, typical, expected)


def test_dead_and_constant_channels_are_exact_or_clamped_in_the_floor():
    P, C, rows = N * H * W, 16, 4
    r = bc.ladder_tensor(P, C, 5)
    gamma, beta, mm0, mv0 = bc.bn_params(C, 6)
    k = bc.rung_of(C)
    assert (r[:, k == 5] == 0).all() and (r[:, k == 4] == np.float32(5.1)).all() and (r[:, k == 6] < 0).any()
    for s, ss in bc.floor_forward_sums(r, rows):
        assert (s[k == 5] == 0).all() and (ss[k == 5] == 0).all()
        emu = bc.finalize64(s, ss, P, gamma, beta, mm0, mv0)
        assert (emu["var"] >= 0).all() and np.isfinite(emu["invstd"]).all()
        assert np.allclose(emu["invstd"][k == 5], 1 / np.sqrt(bc.EPS), rtol=1e-15)


@pytest.mark.parametrize("C", [64, 6, 72])
def test_fp32_restatement_of_the_kernels_formulas_meets_every_derived_bound(C):
    P = N * H * W
    r = bc.ladder_tensor(P, C, 100 + C)
    dy = np.random.default_rng(200 + C).standard_normal((P, C)).astype(np.float32)
    gamma, beta, mm0, mv0 = bc.bn_params(C, 300 + C)
    k = bc.rung_of(C)
    ref = bc.ref_forward(r, gamma, beta, mm0, mv0)
    # a. standalone statistics
    st = bc.restate_stats(r, gamma, beta, mm0, mv0)
    assert all(np.isfinite(v).all() for v in st.values())
    e, bound = bc.stat_errors(st, ref), bc.stat_floor_standalone(ref, beta)
    for key in bc.STAT_KEYS:
        assert (e[key] <= bound[key]).all(), (key, k[np.argmax(e[key] / np.maximum(bound[key], 1e-300))], e[key].max())
    e_mm = np.abs(st["mm"].astype(np.float64) - ref["mm"])
    assert (e_mm <= 4 * U * np.abs(ref["mm"])).all()
    # c. apply, from the restatement's own fp32 scale / shift
    y = bc.restate_apply(r, st["scale"], st["shift"])
    sr = st["scale"].astype(np.float64) * r.astype(np.float64)
    y64 = sr + st["shift"].astype(np.float64)
    assert (np.abs(y - y64) <= 2 * U * (np.abs(sr) + np.abs(st["shift"].astype(np.float64)))).all()
    for relu in (1, 0):
        # d. backward sums, references at the restatement's fp32 mean / invstd
        db, dg = bc.restate_backward_sums(dy, r, st["mean"], st["invstd"])
        sums = bc.ref_backward_sums(dy, r, st["mean"], st["invstd"])
        assert (np.abs(db - sums["dbeta"]) <= 4 * U * sums["abs_dy"]).all()
        assert (np.abs(dg - sums["dgamma"]) <= 8 * U * sums["abs_t"]).all()
        assert (dg[k == 5] == 0).all()                                   # dead rung: r - mean == 0 exactly (dbeta = sum dy is not zero)
        # e. dz and the bias gradient, references at the restatement's own fp32 per-channel values
        dz, dbias = bc.restate_dz(dy, r, gamma, st["mean"], st["invstd"], dg, db, relu)
        dz64, mag = bc.ref_dz(dy, r, gamma, st["mean"], st["invstd"], dg, db, relu)
        ratio = np.abs(dz - dz64) / (U * mag + 1e-300)
        assert ratio.max() <= bc.DZ_C, (relu, k[np.unravel_index(np.argmax(ratio), ratio.shape)[1]], ratio.max())
        if relu:
            assert (dz[r <= 0] == 0).all() and (dz[:, k == 5] == 0).all()
        d64 = dz.astype(np.float64)
        assert (np.abs(dbias - d64.sum(0)) <= 4 * U * np.abs(d64).sum(0)).all()
