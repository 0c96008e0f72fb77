"""`inference.tile_plan` -- the host-only list of (tile, zone) rectangles the device pipeline walks -- against the reference's own record
(tests/golden/inference_driver.npz: the tile shapes UNet/inference.py handed its model, and the digests of the masks it stitched) and,
rectangle by rectangle, against what `_inference_tiling` hands its `predict` hook."""
import os

import numpy as np
import pytest

import fake_segmenter as fs
from conftest import pkg

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inference_driver.npz"))
SMALL = [(100, 75), (64, 64), (65, 200), (5, 40)]          # tile_size 64, radius 16: several edge shapes; two that fit in one tile; H < 16


def _pad16(img):
    img = img[:, :, None] if img.ndim == 2 else img
    h, w = img.shape[:2]
    return np.pad(img, ((0, (-h) % 16), (0, (-w) % 16), (0, 0)), mode="reflect"), h, w


def _replay(inf, img, plan, fake):
    """pad-reflect, cut, predict, paste the zone, crop: what the device pipeline does with a plan"""
    p, h, w = _pad16(img)
    predict = fs.predict_with(fake)
    mask = np.full(p.shape[:2], -1, np.int32)
    for (ty, tx, th, tw), (zy, zx, zh, zw) in plan:
        pred = predict(None, p[ty:ty + th, tx:tx + tw])
        mask[zy:zy + zh, zx:zx + zw] = pred[zy - ty:zy - ty + zh, zx - tx:zx - tx + zw]
    return mask[:h, :w]


@pytest.mark.parametrize("case", fs.INFERENCE_CASES, ids=["%dx%dx%d r%d" % c[:4] for c in fs.INFERENCE_CASES])
def test_tile_plan_reproduces_the_reference_record(case):
    inf = pkg("inference")
    h, w, c, radius, seed = case
    key = "%dx%dx%d_r%d_s%d" % case
    img = fs.synthetic_image(h, w, c, seed)
    hp, wp = h + (-h) % 16, w + (-w) % 16
    cc = max(c, 1)
    fits = hp <= inf.TILE_SIZE and wp <= inf.TILE_SIZE
    plan = inf.tile_plan(hp, wp, inf.TILE_SIZE, radius, tiled=True)
    assert np.array_equal(np.array([(1, cc, t[2], t[3]) for t, _ in plan], dtype=np.int32), G["calls_" + key])
    fake = fs.FakeSegmenter(radius)
    m = _replay(inf, img, plan, fake)
    assert np.array_equal(np.array(fake.calls, dtype=np.int32), G["calls_" + key])
    rows, cols = fs.mask_digest(m)
    assert m.shape == (h, w) and np.array_equal(rows, G["tiled_rows_" + key]) and np.array_equal(cols, G["tiled_cols_" + key])
    # the default is the dispatch of inference(): the whole-image entry when the image fits, else the same loop
    default = inf.tile_plan(hp, wp, inf.TILE_SIZE, radius)
    if fits:
        assert default == inf.tile_plan(hp, wp, inf.TILE_SIZE, None) == [((0, 0, hp, wp), (0, 0, hp, wp))]
        rows, cols = fs.mask_digest(_replay(inf, img, default, fs.FakeSegmenter(radius)))
        assert np.array_equal(rows, G["whole_rows_" + key]) and np.array_equal(cols, G["whole_cols_" + key])
    else:
        assert default == plan


@pytest.mark.parametrize("hw", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_tile_plan_rectangles_are_the_ones_inference_tiling_visits(hw):
    inf = pkg("inference")
    h, w = hw
    tile, radius = 64, 16
    img = fs.synthetic_image(h, w, 1, 11)
    p, _, _ = _pad16(img)
    hp, wp = p.shape[:2]
    seen = []

    def predict(_unet, tile_hwc):
        # the tile is a view of the padded image: its rectangle is where its first element lies in it
        off = (tile_hwc.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // base.itemsize
        seen.append((off // base.shape[1], off % base.shape[1], tile_hwc.shape[0], tile_hwc.shape[1]))
        return np.zeros(tile_hwc.shape[:2], np.int32)

    base = np.ascontiguousarray(p)                     # already a multiple of 16: _pad_to_factor hands it on unchanged
    assert base.shape[2] == 1
    inf._inference_tiling(base, fs.FakeSegmenter(radius), tile, predict=predict)
    plan = inf.tile_plan(hp, wp, tile, radius, tiled=True)
    assert [t for t, _ in plan] == seen and len(seen) >= 1
    # zones: a partition of the padded image, each inside its tile, in row-major order of the zone grid
    cover = np.zeros((hp, wp), np.int32)
    for (ty, tx, th, tw), (zy, zx, zh, zw) in plan:
        assert ty <= zy and tx <= zx and zy + zh <= ty + th and zx + zw <= tx + tw and th % 16 == 0 and tw % 16 == 0 and th <= tile and tw <= tile
        cover[zy:zy + zh, zx:zx + zw] += 1
    assert (cover == 1).all()
    # ... and the masks: the replay of the plan == _inference_tiling, the replay of the default plan == what inference() dispatches to
    fake = fs.FakeSegmenter(radius)
    want = inf._inference_tiling(img.copy(), fake, tile, predict=fs.predict_with(fake))
    assert np.array_equal(_replay(inf, img, plan, fs.FakeSegmenter(radius)), want)
    default = inf.tile_plan(hp, wp, tile, radius)
    if hp > tile or wp > tile:
        assert default == plan
    else:
        assert default == [((0, 0, hp, wp), (0, 0, hp, wp))]
        whole = inf._inference(img.copy(), None, predict=fs.predict_with(fs.FakeSegmenter(radius)))
        assert np.array_equal(_replay(inf, img, default, fs.FakeSegmenter(radius)), whole)
