"""Test-time augmentation and confidence maps, the host side: the numpy statement of the eight transforms (`tta_apply` / `tta_invert`),
the three new C-ABI symbols, the argument checks that must fail before any device work, and the float32 BigTIFF the confidence map
is written as.  No GPU is needed."""
import ctypes
import hashlib
import struct
import zlib

import numpy as np
import pytest

from conftest import pkg

inf = pkg("inference")

SYMBOLS = ("unet_image_tile_gather_tta", "unet_prob_accumulate", "unet_argmax_paste_conf")


def test_the_eight_transforms_are_distinct_and_invert_undoes_them():
    x = np.arange(3 * 5 * 7, dtype=np.float32).reshape(3, 5, 7)              # [C, th, tw], non-square: every element its own value
    p = np.arange(5 * 7 * 4, dtype=np.float32).reshape(5, 7, 4)              # [th', tw', K]
    applied = [np.ascontiguousarray(inf.tta_apply(x, t)) for t in range(8)]
    inverted = [np.ascontiguousarray(inf.tta_invert(p, t)) for t in range(8)]
    for t in range(8):
        swapped = (7, 5) if t & 4 else (5, 7)
        assert applied[t].shape == (3,) + swapped, t                          # codes 4..7 swap the spatial shape
        assert inverted[t].shape == swapped + (4,), t
        for u in range(t):
            assert applied[t].shape != applied[u].shape or not np.array_equal(applied[t], applied[u]), (t, u)
            assert inverted[t].shape != inverted[u].shape or not np.array_equal(inverted[t], inverted[u]), (t, u)
        # the inverse, on the NHWC side of the network, brings every pixel back to where the tile has it
        assert np.array_equal(inf.tta_invert(applied[t].transpose(1, 2, 0), t), x.transpose(1, 2, 0)), t
    assert np.array_equal(applied[0], x) and np.array_equal(inverted[0], p)   # 0 is the identity
    # the documented order: transpose, then flip rows, then flip columns
    assert np.array_equal(applied[1], x[:, :, ::-1]) and np.array_equal(applied[2], x[:, ::-1, :])
    assert np.array_equal(applied[4], x.transpose(0, 2, 1)) and np.array_equal(applied[7], x.transpose(0, 2, 1)[:, ::-1, ::-1])
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            inf.tta_apply(x, bad)
        with pytest.raises(ValueError):
            inf.tta_invert(p, bad)


def test_header_declares_and_library_exports_the_three_symbols():
    protos = pkg("_lib").parse_header()
    cdll = ctypes.CDLL(pkg("_build").build_library())
    for name in SYMBOLS:
        assert name in protos, "include/unet_hip.h does not declare " + name
        assert hasattr(cdll, name), "the library does not export " + name
    assert len(protos["unet_image_tile_gather_tta"][1]) == 14
    assert len(protos["unet_prob_accumulate"][1]) == 10
    args = protos["unet_argmax_paste_conf"][1]
    assert len(args) == 21 and args[5] is ctypes.c_float and args[12] is ctypes.c_long and args[18] is ctypes.c_long


@pytest.mark.parametrize("tta", [3, 0, 16, -2, 2.5, True, None])
def test_a_tta_outside_1_2_4_8_is_refused_before_any_device_work(tta):
    img = np.zeros((32, 32), np.uint8)
    with pytest.raises(ValueError, match="tta"):
        inf.segment_image(img, None, tta=tta)                                 # (no network: nothing but the argument is looked at)
    with pytest.raises(ValueError, match="tta"):
        inf._segment_host_pipeline(img, None, tta=tta)


def test_the_cli_refuses_tta_3(tmp_path, capsys):
    argv = ["--checkpoint_filepath", str(tmp_path / "none"), "--image_folder", str(tmp_path), "--output_folder", str(tmp_path / "out"),
            "--number_classes", "2", "--number_channels", "1", "--image_format", "npy"]
    with pytest.raises(SystemExit) as ei:
        inf.main(argv + ["--tta", "3"])
    assert ei.value.code != 0 and "--tta" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="tta"):                              # the function behind the CLI checks it as well, first
        inf.inference(str(tmp_path / "none"), str(tmp_path), str(tmp_path / "out"), 2, 1, "npy", tta=3)
    with pytest.raises(ValueError, match="confidence_folder"):                # a float32 map has no PNG
        inf.inference(str(tmp_path / "none"), str(tmp_path), str(tmp_path / "out"), 2, 1, "png", confidence_folder=str(tmp_path / "conf"))
    assert not (tmp_path / "out").exists() and not (tmp_path / "conf").exists()


def _parse_bigtiff(path):
    b = open(path, "rb").read()
    order, magic, offsize, zero, ifd = struct.unpack_from("<2sHHHQ", b, 0)
    assert (order, magic, offsize, zero) == (b"II", 43, 8, 0)
    (n,) = struct.unpack_from("<Q", b, ifd)
    tags = {}
    for i in range(n):
        tag, typ, cnt, val = struct.unpack_from("<HHQQ", b, ifd + 8 + 20 * i)
        tags[tag] = (typ, cnt, val)
    assert list(tags) == sorted(tags)
    return b, tags


@pytest.mark.parametrize("shape,tile", [((70, 83), 32), ((40, 40), 1024), ((1030, 5), 1024)])
def test_float32_bigtiff_round_trips(tmp_path, shape, tile):
    rng = np.random.default_rng(shape[0])
    conf = (0.5 + 0.5 * rng.random(shape)).astype(np.float32)                 # confidences of a two-class network: [1/2, 1]
    conf[0, 0], conf[-1, -1] = np.float32(1.0), np.float32(0.5)
    path = str(tmp_path / "c.tif")
    inf._write_bigtiff_tiled(path, conf, tile, 6)
    b, tags = _parse_bigtiff(path)
    assert tags[256][2] == shape[1] and tags[257][2] == shape[0]
    assert tags[258][2] == 32 and tags[339][2] == 3                           # 32 bits per sample, SampleFormat 3 = IEEE floating point
    assert tags[259][2] == 8 and tags[322][2] == tile and tags[323][2] == tile
    ty, tx = (shape[0] + tile - 1) // tile, (shape[1] + tile - 1) // tile
    n = ty * tx
    assert tags[324][1] == n and tags[325][1] == n
    offs = [tags[324][2]] if n == 1 else struct.unpack_from("<%dQ" % n, b, tags[324][2])
    cnts = [tags[325][2]] if n == 1 else struct.unpack_from("<%dQ" % n, b, tags[325][2])
    out = np.zeros((ty * tile, tx * tile), np.float32)
    for t, (o, c) in enumerate(zip(offs, cnts)):
        blk = np.frombuffer(zlib.decompress(b[o:o + c]), dtype="<f4").reshape(tile, tile)
        out[(t // tx) * tile:(t // tx + 1) * tile, (t % tx) * tile:(t % tx + 1) * tile] = blk
    assert np.array_equal(out[:shape[0], :shape[1]], conf) and not out[shape[0]:].any() and not out[:, shape[1]:].any()
    try:                                                                      # an independent reader, where it opens the file at all
        from PIL import Image
        back = np.array(Image.open(path))
    except Exception as exc:                                                  # noqa: BLE001 -- no Pillow, or a libtiff without this layout
        print("Pillow does not read the float32 BigTIFF here:", repr(exc))
    else:
        assert back.dtype == np.float32 and np.array_equal(back, conf)
    # the driver's writer takes a float32 map for 'tif' and for .npy
    inf._write(str(tmp_path / "n.npy"), conf, "npy")
    got = np.load(str(tmp_path / "n.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, conf)


# sha256 of the file the writer produced for these masks BEFORE it learnt float32 (computed from that version of the function)
INTEGER_DIGESTS = {
    ((70, 83), 32): ("67380b0569284678ee43a6e890cf51857ef47b8938ffc4c16ced6f26bb77abeb", 2724),
    ((40, 40), 1024): ("c816fbee325ad059d85092b5d54928d4d799d9bf82eb9f4e19ce8c01ca95abd1", 2184),
}


def test_integer_mask_files_did_not_change_by_a_byte(tmp_path):
    rng = np.random.default_rng(20)
    for (shape, tile), (digest, size) in INTEGER_DIGESTS.items():             # (dict order = the order the generator was drawn in)
        mask = rng.integers(0, 4, shape).astype(np.uint8)
        path = str(tmp_path / "m.tif")
        inf._write_bigtiff_tiled(path, mask, tile, 6)
        data = open(path, "rb").read()
        assert len(data) == size and hashlib.sha256(data).hexdigest() == digest, (shape, tile)
        _, tags = _parse_bigtiff(path)
        assert tags[339][2] == 1 and tags[258][2] == 8
