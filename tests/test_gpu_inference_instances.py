"""Instance labels through the inference pipeline: `segment_image(instances=True, min_object_area=A)` against the CPU restatement
(component_cases.py) applied to the plain mask of the same run, on the device and with the host pipeline; TTA and confidence unchanged
beside it; scoring of the filtered mask; the default path untouched; the command line.  Networks and images as test_gpu_inference_tta.py."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg
import component_cases as cc
from test_gpu_inference_tta import _net, _uint16_image, _raw_image, _Recorder, TILE, RADIUS

pytestmark = pytest.mark.gpu
AREA, ROWS = 6, 48
IMAGES = [((48, 40), "one_tile"), ((100, 75), "tiled")]


def _restated(plain, connectivity, background, area, rows):
    labels, count, objects, filtered = cc.label_reference(plain[None].astype(np.int64), connectivity, background, area, rows)
    return labels[0], int(count[0]), objects[0], filtered[0]


@pytest.mark.parametrize("hw", [i[0] for i in IMAGES], ids=[i[1] for i in IMAGES])
def test_instances_are_the_restatement_of_the_plain_mask(hw, monkeypatch):
    inf = pkg("inference")
    net = _net(1, 2)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    h, w = hw
    raw = _uint16_image(h, w, 1, seed=h + 1)
    plain = inf.segment_image(raw, net, tile_size=TILE)
    assert len(inf.tile_plan(h + (-h) % 16, w + (-w) % 16, TILE, RADIUS)) > 1 or hw == (48, 40)
    for connectivity, background, area in ((8, 0, AREA), (4, 1, AREA), (4, None, 0), (8, 0, 0)):
        labels, count, objects, filtered = _restated(plain, connectivity, background, area, ROWS)
        print(hw, connectivity, background, area, "objects:", count, "pixels removed:", int((filtered != plain).sum()))
        kw = dict(tile_size=TILE, instances=True, connectivity=connectivity, background=background, min_object_area=area, max_objects=ROWS)
        dev = inf.segment_image(raw, net, **kw)
        host = inf._segment_host_pipeline(raw, net, TILE, **{k: v for k, v in kw.items() if k != "tile_size"})
        for res in (dev, host):
            assert isinstance(res, inf.InstanceResult) and res.confidence is None and res.probabilities is None
            assert res.labels.dtype == np.int32 and res.objects.dtype == np.int64 and res.objects.shape == (ROWS, 8) and isinstance(res.count, int)
            assert res.count == count and np.array_equal(res.labels, labels) and np.array_equal(res.objects, objects)
            assert np.array_equal(res.mask, filtered)
        assert dev.mask.dtype == np.uint8
    # what keeps this honest: the mask holds several objects and the filter removes some but not all of them
    labels, count, _, filtered = _restated(plain, 8, 0, AREA, ROWS)
    assert count >= 2 and (filtered != plain).any()
    only_filter = inf.segment_image(raw, net, tile_size=TILE, min_object_area=AREA)                 # the filter alone: the same stage
    assert isinstance(only_filter, inf.InstanceResult) and np.array_equal(only_filter.mask, filtered) and np.array_equal(only_filter.labels, labels)
    with pytest.raises(ValueError):
        inf.segment_image(raw, net, tile_size=TILE, instances=True, connectivity=5)
    with pytest.raises(ValueError):
        inf.segment_image(raw, net, tile_size=TILE, min_object_area=3, background=None)


def test_one_pixel_axis_takes_the_host_route_with_the_same_options(monkeypatch):
    """a 1 x W image has no reflection to pad it with on the device: segment_image hands it, options and all, to the host pipeline"""
    inf = pkg("inference")
    net = _net(1, 2)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    rec = _Recorder(pkg("_lib").lib())
    monkeypatch.setattr(inf, "lib", lambda: rec)
    for shape in ((1, 40), (37, 1)):
        raw = _uint16_image(shape[0], shape[1], 1, seed=7)
        plain = inf.segment_image(raw, net, tile_size=TILE)
        for area in (0, 2):
            labels, count, objects, filtered = _restated(plain, 4, 0, area, ROWS)
            res = inf.segment_image(raw, net, tile_size=TILE, instances=True, connectivity=4, min_object_area=area, max_objects=ROWS)
            assert isinstance(res, inf.InstanceResult) and res.count == count and np.array_equal(res.labels, labels)
            assert np.array_equal(res.objects, objects) and np.array_equal(res.mask, filtered) and res.labels.shape == shape
    assert "unet_label_components" not in rec.calls and "unet_image_tile_gather" not in rec.calls


def test_tta_and_confidence_are_unchanged_beside_the_instances(monkeypatch):
    inf = pkg("inference")
    net = _net(1, 2)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    raw = _uint16_image(100, 75, 1, seed=101)
    base = inf.segment_image(raw, net, tile_size=TILE, tta=4, return_confidence=True)
    res = inf.segment_image(raw, net, tile_size=TILE, tta=4, return_confidence=True, instances=True, max_objects=ROWS)
    assert isinstance(res, inf.InstanceResult) and res[:3][2] is None and base.probabilities is None
    assert np.array_equal(res.mask, base.mask) and np.array_equal(res.confidence, base.confidence)
    labels, count, objects, _ = _restated(base.mask, 8, 0, 0, ROWS)
    assert res.count == count and np.array_equal(res.labels, labels) and np.array_equal(res.objects, objects)


def test_scoring_counts_the_filtered_mask(monkeypatch):
    inf, metrics = pkg("inference"), pkg("metrics")
    net = _net(1, 2)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    raw = _uint16_image(100, 75, 1, seed=101)
    truth = np.random.default_rng(3).integers(0, 2, (100, 75)).astype(np.uint8)
    plain = inf.segment_image(raw, net, tile_size=TILE)
    _, _, _, filtered = _restated(plain, 8, 0, AREA, ROWS)
    assert (filtered != plain).any()
    want = metrics.ConfusionMatrix(2, device="cpu")
    inf._host_confusion(filtered, truth, want)
    for host in (False, True):
        cm = metrics.ConfusionMatrix(2, device="cpu" if host else net.engine.dev)
        fn = (lambda *a, **k: inf._segment_host_pipeline(a[0], a[1], TILE, **k)) if host else (lambda *a, **k: inf.segment_image(*a, tile_size=TILE, **k))
        res = fn(raw, net, truth=truth, confusion=cm, min_object_area=AREA, max_objects=ROWS)
        assert np.array_equal(res.mask, filtered) and np.array_equal(cm.result(), want.result()), host


def test_default_path_is_untouched(monkeypatch):
    inf = pkg("inference")
    net = _net(1, 2)
    monkeypatch.setattr(net, "estimate_radius", lambda: RADIUS, raising=False)
    rec = _Recorder(pkg("_lib").lib())
    monkeypatch.setattr(inf, "lib", lambda: rec)
    raw = _uint16_image(100, 75, 1, seed=101)
    never = inf.segment_image(raw, net, tile_size=TILE)
    calls_never = list(rec.calls)
    del rec.calls[:]
    off = inf.segment_image(raw, net, tile_size=TILE, instances=False, min_object_area=0)
    assert rec.calls == calls_never and "unet_label_components" not in calls_never
    assert isinstance(off, np.ndarray) and off.dtype == never.dtype and np.array_equal(off, never)
    del rec.calls[:]
    on = inf.segment_image(raw, net, tile_size=TILE, instances=True)
    extra = [c for c in rec.calls if c not in ("unet_image_tile_gather", "unet_argmax_paste")]
    assert extra == ["unet_label_components"] and rec.calls[-1] == "unet_label_components"            # one call, after the last paste
    assert np.array_equal(on.mask, never)


def test_cli_writes_label_maps_and_tables(tmp_path):
    inf, comp = pkg("inference"), pkg("components")
    net = _net(1, 2)
    stem = str(tmp_path / "checkpoint" / "ckpt")
    net.save_checkpoint(stem)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    images = {"a.npy": _uint16_image(70, 83, 1, 1)[:, :, 0], "b.npy": _raw_image(40, 40, 1, np.uint8, 2, None)[:, :, 0]}
    for name, im in images.items():
        np.save(imgs / name, im)
    common = ["--checkpoint_filepath", stem, "--image_folder", str(imgs), "--number_classes", "2", "--number_channels", "1", "--image_format", "npy"]
    inf.main(common + ["--output_folder", str(tmp_path / "plain")])
    assert sorted(os.listdir(tmp_path / "plain")) == ["a.npy", "b.npy"]                             # what the folder holds today
    flags = ["--connectivity", "4", "--min_object_area", "4", "--max_objects", "500"]
    inf.main(common + flags + ["--output_folder", str(tmp_path / "dev"), "--instance_folder", str(tmp_path / "inst")])
    inf.main(common + flags + ["--output_folder", str(tmp_path / "host"), "--instance_folder", str(tmp_path / "inst2"), "--host_pipeline"])
    inf.main(common + flags + ["--output_folder", str(tmp_path / "filtered")])                      # the filter alone: masks only
    assert sorted(os.listdir(tmp_path / "filtered")) == ["a.npy", "b.npy"]
    assert sorted(os.listdir(tmp_path / "dev")) == ["a.npy", "b.npy", "object_counts.csv", "objects.csv"]
    assert sorted(os.listdir(tmp_path / "inst")) == ["a.npy", "b.npy"]
    rows = [r.split(",") for r in open(tmp_path / "dev" / "objects.csv").read().splitlines()]
    assert rows[0] == ["image", "label", "class", "area", "y0", "x0", "y1", "x1", "centroid_y", "centroid_x"]
    counts = dict(r.split(",") for r in open(tmp_path / "dev" / "object_counts.csv").read().splitlines()[1:])
    for name in images:
        plain = np.load(tmp_path / "plain" / name)
        labels, count, objects, filtered = _restated(plain, 4, 0, 4, 500)
        for folder in ("dev", "host", "filtered"):
            assert np.array_equal(np.load(tmp_path / folder / name), filtered), (folder, name)
        for folder in ("inst", "inst2"):
            written = np.load(tmp_path / folder / name)
            assert written.dtype == np.uint16 and np.array_equal(written, labels), (folder, name)
        assert int(counts[name]) == count
        mine = [r for r in rows[1:] if r[0] == name]
        assert [[int(v) for v in r[1:8]] for r in mine] == [[i + 1] + objects[i, :6].tolist() for i in range(count)]
        t = comp.objects_table(count, objects)
        assert [float(r[8]) for r in mine] == t["centroid_y"].tolist() and [float(r[9]) for r in mine] == t["centroid_x"].tolist()
    for f in ("objects.csv", "object_counts.csv"):
        assert open(tmp_path / "dev" / f).read() == open(tmp_path / "host" / f).read()
