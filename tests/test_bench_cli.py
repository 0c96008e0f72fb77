"""bench.py's command line: a plain run measures the headline figure only and can write what its last timed step computed
(`--dump-outputs`); the other measurements sit behind `--full`."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench


def test_synthetic_inputs_are_seeded():
    a = bench.synthetic(2, 3, 4, 32, 1234, "cpu")
    b = bench.synthetic(2, 3, 4, 32, 1234, "cpu")
    c = bench.synthetic(2, 3, 4, 32, 1235, "cpu")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])
    assert tuple(a[0].shape) == (2, 3, 32, 32) and tuple(a[1].shape) == (2, 32, 32, 4)
    assert (a[1].sum(-1) == 1).all()


def test_dump_sample_is_fixed_and_capped():
    small = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert bench.dump_sample(small, max_elems=12) is small                       # at the cap: the array itself, shape kept
    big = np.arange(1000, dtype=np.float32).reshape(10, 100)
    s1, s2 = bench.dump_sample(big, max_elems=64), bench.dump_sample(big.copy(), max_elems=64)
    assert s1.shape == (64,) and np.array_equal(s1, s2)                          # same positions in every call
    assert (np.diff(s1) >= 0).all() and len(np.unique(s1)) > 32                  # ascending positions spread over the array
    assert 4 * 4 * bench.DUMP_MAX_ELEMS <= 64 * 1024 * 1024                      # four float32 arrays: within 64 MB


def _run_bench(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, monkeypatch, capsys):
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "64", "--batch", "2"]
    d = _run_bench(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert d["metric"] == "training images/sec" and d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["value"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 0.01 * d["value"]
    # nothing but the headline was measured: no kernel events, no CPU leg, no other configuration
    assert d["roofline"] is None and d["kernels"] == {} and d["sampled_steps"] == 0
    assert d["cpu_baseline"] is None and "extra_configs" not in d and len(d["configs"]) == 1
    out = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "softmax", "theta", "grad")}
    assert sorted(os.listdir(tmp_path / "a")) == ["grad.npy", "loss.npy", "softmax.npy", "theta.npy"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 * 1024 * 1024
    assert out["softmax"].shape == (2, 64, 64, 2) and np.abs(out["softmax"].sum(-1) - 1).max() < 1e-5
    assert out["theta"].shape == out["grad"].shape == (bench.DUMP_MAX_ELEMS,) and np.abs(out["grad"]).max() > 0
    assert float(out["loss"][0]) == pytest.approx(d["final_loss"], abs=1e-6)
    # the same arguments again: same inputs, same parameters, same dropout masks -> the same three steps.  fp32 sums whose order is not
    # fixed (atomics in the reductions) move a value by a few ulp per step; 1e-3 of the largest magnitude is orders above that and far below
    # what another input, seed or step count gives
    _run_bench(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    for n, v in out.items():
        w = np.load(tmp_path / "b" / (n + ".npy"))
        print("run-to-run %s: max|diff| %.3e, max|value| %.3e" % (n, np.abs(w - v).max(), np.abs(v).max()))
        assert w.shape == v.shape and np.abs(w - v).max() <= 1e-3 * np.abs(v).max(), n
