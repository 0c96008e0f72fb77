"""The CPU restatement of connected components (component_cases.py) against hand-written arrays, against scipy where it is installed,
against the package's own host route (components.label_components_host), its filter and object table against direct reductions, and
the two new ABI symbols against the header."""
import ctypes
import os

import numpy as np
import pytest

from conftest import pkg, ROOT, PKG
import component_cases as cc


def one(mask, connectivity, background=0):
    labels, count, _, _ = cc.label_reference(np.asarray(mask)[None], connectivity, background)
    return labels[0].tolist(), int(count[0])


def test_six_tiny_masks_by_hand():
    diag = [[1, 0],
            [0, 1]]
    assert one(diag, 4) == ([[1, 0], [0, 2]], 2)
    assert one(diag, 8) == ([[1, 0], [0, 1]], 1)
    u = [[1, 0, 1],
         [1, 0, 1],
         [1, 1, 1]]
    assert one(u, 4) == (u, 1)                                       # the arms meet only in the last row: ONE object, numbered from its first pixel
    two = [[1, 1, 2, 2],
           [1, 1, 2, 2]]
    assert one(two, 8) == ([[1, 1, 2, 2], [1, 1, 2, 2]], 2)          # classes never merge
    assert one(two, 8, background=1) == ([[0, 0, 1, 1], [0, 0, 1, 1]], 1)
    assert one(np.zeros((3, 4), int), 8) == ([[0] * 4] * 3, 0)
    assert one(np.ones((3, 4), int), 4) == ([[1] * 4] * 3, 1)
    assert one(np.zeros((3, 4), int), 4, background=None) == ([[1] * 4] * 3, 1)
    # numbering is by FIRST pixel in row-major order, not by discovery along a column
    assert one([[0, 0, 1], [1, 0, 1], [1, 0, 0]], 4) == ([[0, 0, 1], [2, 0, 1], [2, 0, 0]], 2)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_against_scipy_per_class(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for h, w in ((17, 33), (65, 129)):
        for name in ("blobs", "percolation_1", "percolation_2", "nested_rings", "comb"):
            m, labels, count, _, _ = cc.reference(name, h, w, connectivity)
            merged, offset = np.zeros((h, w), np.int64), 0
            for cls in np.unique(m[0]):
                if cls == 0:
                    continue
                lab, k = ndi.label(m[0] == cls, structure=structure)
                merged += np.where(lab > 0, lab + offset, 0)
                offset += k
            assert offset == int(count[0]) and np.array_equal(cc.canonical(merged), labels[0]), (name, h, w)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_package_host_route_is_the_restatement(connectivity):
    comp = pkg("components")
    for h, w in cc.SHAPES[:6]:
        for name in cc.CONTENTS + ["percolation_1"]:
            m, labels, count, objects, _ = cc.reference(name, h, w, connectivity)
            got = comp.label_components_host(m, connectivity, 0, 0, 64)
            rows = min(int(count[0]), 64)
            assert np.array_equal(got[0], labels) and np.array_equal(got[1], count), (name, h, w)
            assert np.array_equal(got[2][0, :rows], objects[0, :rows]) and not got[2][0, rows:].any() and np.array_equal(got[3], m)
    m3 = np.array(cc.batch3(65, 129))
    for bg, area in ((0, 0), (0, 7), (None, 0), (2, 3)):
        want = cc.label_reference(m3, connectivity, bg, area, 16)
        got = comp.label_components_host(m3.astype(np.uint8), connectivity, bg, area, 16)
        assert got[3].dtype == np.uint8 and all(np.array_equal(a, b) for a, b in zip(got, want)), (bg, area)
    two_d = comp.label_components_host(m3[0], connectivity)
    assert two_d[0].shape == (65, 129) and isinstance(two_d[1], int) and two_d[2].shape == (65536, 8)


def test_filter_keeps_order_and_the_table_is_the_direct_reduction():
    m = cc.filter_image()[None]
    full = cc.label_reference(m, 8, 0, 0, 16)
    assert full[1].tolist() == [6] and full[2][0, :6, 1].tolist() == [8, 80, 9, 10, 9, 1]          # A - 1, A, A + 1 for A = 9 among them
    labels, count, objects, out = cc.label_reference(m, 8, 0, 9, 16)
    assert count.tolist() == [4] and objects[0, :4, 1].tolist() == [80, 9, 10, 9] and objects[0, :4, 0].tolist() == [2, 1, 1, 2]
    removed = (full[0] > 0) & (labels == 0)
    assert removed.sum() == 9 and (out[removed] == 0).all() and np.array_equal(out[~removed], m[~removed])
    assert np.array_equal(cc.canonical(np.where(labels > 0, full[0], 0)[0]), labels[0])            # survivors keep their relative order
    for i in range(1, 5):
        ys, xs = np.nonzero(labels[0] == i)
        assert objects[0, i - 1].tolist() == [m[0, ys[0], xs[0]], len(ys), ys.min(), xs.min(), ys.max(), xs.max(), ys.sum(), xs.sum()]
    assert not objects[0, 4:].any()
    gone = cc.label_reference(m, 8, 0, 81, 16)                                                      # every object removed
    assert gone[1].tolist() == [0] and not gone[0].any() and not gone[3].any() and not gone[2].any()
    few = cc.label_reference(m, 8, 0, 0, 2, fill=-5)                                                # a short table: true count, first rows only
    assert few[1].tolist() == [6] and np.array_equal(few[2][0], full[2][0, :2]) and few[0].max() == 6
    with pytest.raises(ValueError):
        cc.label_reference(m, 8, None, 3)
    comp = pkg("components")
    t = comp.objects_table(int(count[0]), objects[0])
    assert t["label"].tolist() == [1, 2, 3, 4] and t["class"].tolist() == [2, 1, 1, 2] and t["bbox"][0].tolist() == [1, 20, 8, 29]
    assert t["centroid_y"][0] == 4.5 and t["centroid_x"][0] == 24.5
    assert len(comp.objects_table(6, few[2][0])) == 2
    with pytest.raises(ValueError):
        comp.label_components_host(m, 8, None, 3)


def test_abi_has_the_two_symbols_with_the_header_prototypes():
    lib_mod = pkg("_lib")
    assert lib_mod.header_abi_version() == 10
    protos = lib_mod.parse_header()
    i, p, lng, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_size_t
    assert protos["unet_label_components_workspace"] == (sz, [i, i, i])
    assert protos["unet_label_components"] == (i, [p, i, lng, i, i, i, i, i, i, p, p, p, p, i, p, sz, p])
    assert "components.hip" in pkg("_build").SOURCES
    so = os.path.join(ROOT, PKG, "csrc", "libunet_hip.so")
    if os.path.exists(so):                                           # (built: the binary exports both)
        names = open(so, "rb").read()
        assert b"unet_label_components_workspace" in names and b"unet_label_components" in names
