"""Connected components on the device: `unet_label_components` against the CPU restatement (component_cases.py), exact in every output --
labels, count, object table, filtered mask -- with the outputs in sentinel frames, the workspace's neighbours and the input checked
untouched; two closed-form large cases checked through the object table; the refusals; and `components.label_components`."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
import component_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -777
PAD = 64
EINVAL, ENOSPC = -1, -2


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ST():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def framed(n, dtype, fill):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def run(hip, mask, connectivity=8, background=0, min_area=0, max_objects=64, elem=1, pitch=None, want_mask=True, alias=False, want_objects=True):
    """mask int [N,H,W] (numpy) -> (labels, count, objects or None, filtered mask or None) as numpy, after checking that the frames around
    every output and the workspace still hold their sentinel and that the input is unchanged (unless aliased)"""
    mask = np.asarray(mask)
    n, h, w = mask.shape
    npix = n * h * w
    dt = torch.uint8 if elem == 1 else torch.int32
    pitch = w if pitch is None else pitch
    mbuf = torch.full((n * h * pitch + 2 * PAD,), 99, dtype=dt, device=DEV)
    mview = mbuf[PAD:PAD + n * h * pitch].view(n, h, pitch)
    mview[:, :, :w] = torch.from_numpy(np.array(mask)).to(dt).to(DEV)
    before = mbuf.clone()
    lbuf, lv = framed(npix, torch.int32, SENT)
    cbuf, cv = framed(n, torch.int32, SENT)
    obuf, ov = framed(n * max_objects * 8, torch.int64, SENT) if want_objects else (None, None)
    if alias:
        assert pitch == w
        fbuf, fv = mbuf, mbuf[PAD:PAD + npix]
    else:
        fbuf, fv = framed(npix, dt, 77) if want_mask else (None, None)
    nb = hip.unet_label_components_workspace(n, h, w)
    assert nb > 0
    wsbuf, ws = framed(nb, torch.uint8, 0x5A)
    hip.unet_label_components(P(mview), elem, pitch, n, h, w, connectivity, -1 if background is None else background, min_area, P(lv), P(cv), P(fv),
                              P(ov), max_objects, P(ws), nb, ST())
    torch.cuda.synchronize()
    assert (lbuf[:PAD] == SENT).all() and (lbuf[PAD + npix:] == SENT).all()
    assert (cbuf[:PAD] == SENT).all() and (cbuf[PAD + n:] == SENT).all()
    assert (wsbuf[:PAD] == 0x5A).all() and (wsbuf[PAD + nb:] == 0x5A).all()
    if want_objects:
        assert (obuf[:PAD] == SENT).all() and (obuf[PAD + n * max_objects * 8:] == SENT).all()
    if alias:
        assert torch.equal(mbuf[:PAD], before[:PAD]) and torch.equal(mbuf[PAD + npix:], before[PAD + npix:])
    else:
        assert torch.equal(mbuf, before)
        if want_mask:
            assert (fbuf[:PAD] == 77).all() and (fbuf[PAD + npix:] == 77).all()
    return (lv.cpu().numpy().reshape(n, h, w), cv.cpu().numpy(), ov.cpu().numpy().reshape(n, max_objects, 8) if want_objects else None,
            fv.cpu().numpy().reshape(n, h, w).astype(np.int64) if fv is not None else None)


def check(got, want, what):
    labels, count, objects, fmask = got
    rl, rc, ro, rf = want
    assert np.array_equal(count, rc), (what, count, rc)
    assert labels.dtype == np.int32 and np.array_equal(labels, rl), (what, int((labels != rl).sum()))
    if objects is not None:
        assert np.array_equal(objects, ro), (what, np.argwhere(objects != ro)[:4])
    if fmask is not None:
        assert np.array_equal(fmask, rf), what


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("hw", cc.SHAPES, ids=["%dx%d" % s for s in cc.SHAPES])
def test_every_content_at_every_shape_is_the_restatement(hip, hw, connectivity):
    h, w = hw
    for name in cc.CONTENTS + ["percolation_1", "percolation_2", "percolation_3"]:
        ref = cc.reference(name, h, w, connectivity)
        check(run(hip, ref[0], connectivity), ref[1:], (name, hw, connectivity))
    board = cc.reference("checkerboard", h, w, connectivity)
    assert int(board[2][0]) == ((h * w + 1) // 2 if connectivity == 4 or min(h, w) == 1 else 1)
    assert int(cc.reference("background", h, w, connectivity)[2][0]) == 0 and not cc.reference("background", h, w, connectivity)[1].any()
    assert int(cc.reference("serpentine", h, w, connectivity)[2][0]) == 1


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("hw", [(17, 33), (65, 129), (130, 257)], ids=lambda s: "%dx%d" % s)
def test_pitched_rows_both_element_sizes_and_three_images_in_one_call(hip, hw, connectivity):
    h, w = hw
    m = cc.batch3(h, w)
    want = cc.label_reference(m, connectivity, 0, 0, 64, fill=SENT)
    assert len(set(want[1].tolist())) == 3 and want[1].min() >= 1                # three different images; numbering restarts in each
    for elem, pitch in ((1, w), (1, w + 13), (4, w), (4, w + 5)):
        check(run(hip, m, connectivity, elem=elem, pitch=pitch), want, (hw, connectivity, elem, pitch))
    none = cc.label_reference(m, connectivity, None, 0, 64, fill=SENT)           # no background class: class 0 is labelled too
    assert (none[0] > 0).all()
    check(run(hip, m, connectivity, background=None, elem=4, pitch=w + 5), none, (hw, connectivity, "no background"))
    big = np.where(m > 0, m + 70000, 0)                                          # int32 classes beyond a byte
    got = run(hip, big, connectivity, elem=4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2][..., 1:], want[2][..., 1:])
    assert np.array_equal(got[2][0, :want[1][0], 0], want[2][0, :want[1][0], 0] + 70000)


def test_stripes_2048_in_closed_form(hip):
    """2048 x 2048, vertical stripes of period 3: columns 3k and 3k + 1 class 1, column 3k + 2 background -> 683 components of width 2
    (the last one, columns 2046 and 2047, too); every row of the table is known"""
    h = w = 2048
    x = np.arange(w)
    m = np.broadcast_to((x % 3 != 2).astype(np.int64), (1, h, w))
    count = 683
    labels, cnt, objects, _ = run(hip, m, 4, max_objects=700, want_mask=False)
    assert cnt.tolist() == [count]
    k = np.arange(count)
    want = np.stack([np.ones(count, np.int64), np.full(count, 2 * h), np.zeros(count, np.int64), 3 * k, np.full(count, h - 1), 3 * k + 1,
                     np.full(count, 2 * (h * (h - 1) // 2)), h * (6 * k + 1)], 1)
    assert np.array_equal(objects[0, :count], want) and (objects[0, count:] == SENT).all()
    assert np.array_equal(labels[0], np.broadcast_to(np.where(x % 3 != 2, x // 3 + 1, 0), (h, w)))


def test_frame_around_a_grid_of_squares_in_closed_form(hip):
    """1536 x 2560: 5 x 5 squares of class 2 at every multiple of 8 (rows and columns 8i + 2 .. 8i + 6) on a ground of class 1 that is one
    frame-shaped component around all of them; no background class"""
    h, w = 1536, 2560
    yy, xx = np.mgrid[0:h, 0:w]
    sq = ((yy % 8 >= 2) & (yy % 8 <= 6) & (xx % 8 >= 2) & (xx % 8 <= 6))
    m = np.where(sq, 2, 1)[None]
    ny, nx = h // 8, w // 8
    count = 1 + ny * nx
    labels, cnt, objects, _ = run(hip, m, 8, background=None, max_objects=count + 3, want_mask=False)
    assert cnt.tolist() == [count]
    ground = h * w - 25 * ny * nx
    sum_y_all, sum_x_all = w * (h * (h - 1) // 2), h * (w * (w - 1) // 2)
    i, j = np.divmod(np.arange(ny * nx), nx)
    sq_rows = np.stack([np.full(ny * nx, 2), np.full(ny * nx, 25), 8 * i + 2, 8 * j + 2, 8 * i + 6, 8 * j + 6, 25 * (8 * i + 4), 25 * (8 * j + 4)], 1)
    assert objects[0, 0].tolist() == [1, ground, 0, 0, h - 1, w - 1, sum_y_all - sq_rows[:, 6].sum(), sum_x_all - sq_rows[:, 7].sum()]
    assert np.array_equal(objects[0, 1:count], sq_rows) and (objects[0, count:] == SENT).all()
    assert np.array_equal(labels[0], np.where(sq, 2 + (yy // 8) * nx + xx // 8, 1))


@pytest.mark.parametrize("alias", [False, True], ids=["own_mask_out", "aliased"])
def test_filter_and_table(hip, alias):
    m = cc.filter_image()[None]
    for connectivity in (4, 8):
        for a in (0, 1, 9, 10, 81):
            want = cc.label_reference(m, connectivity, 0, a, 16, fill=SENT)
            for elem in (1, 4):
                check(run(hip, m, connectivity, min_area=a, max_objects=16, elem=elem, alias=alias), want, (connectivity, a, elem, alias))
    assert cc.label_reference(m, 8, 0, 9, 16)[1].tolist() == [4] and cc.label_reference(m, 8, 0, 81, 16)[1].tolist() == [0]     # every object removed
    big = np.array(cc.batch3(130, 257))
    for a in (2, 30):
        want = cc.label_reference(big, 8, 0, a, 64, fill=SENT)
        check(run(hip, big, 8, min_area=a, alias=alias), want, ("batch3", a, alias))


def test_more_objects_than_rows_and_no_table(hip):
    m = cc.batch3(65, 129)
    full = cc.label_reference(m, 4, 0, 0, 64, fill=SENT)
    assert full[1].max() > 64 > 5 > full[1].min() >= 1                    # more objects than rows, fewer, and fewer than the short table's 5
    check(run(hip, m, 4), full, "64 rows")                                        # (the true count, the first 64 rows, sentinel beyond)
    assert sorted(full[1].tolist())[1] > 5
    five = cc.label_reference(m, 4, 0, 0, 5, fill=SENT)
    check(run(hip, m, 4, max_objects=5), five, "5 rows")
    labels, count, objects, fmask = run(hip, m, 4, want_objects=False, want_mask=False)
    assert objects is None and fmask is None and np.array_equal(labels, full[0]) and np.array_equal(count, full[1])


def test_two_calls_with_another_shape_between_give_the_same_bits(hip):
    ref = cc.reference("percolation_2", 130, 257, 8, 0, 3, 64)
    first = run(hip, ref[0], 8, min_area=3)
    run(hip, cc.batch3(65, 129), 4)
    second = run(hip, ref[0], 8, min_area=3)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    check(first, ref[1:], "percolation, filtered")


def test_refusals_launch_nothing(hip):
    raw = hip.cdll.unet_label_components
    n, h, w, mo = 1, 8, 8, 4
    mask = torch.ones((n, h, w), dtype=torch.uint8, device=DEV)
    mask4 = torch.ones((n, h, w), dtype=torch.int32, device=DEV)
    lbuf, lv = framed(n * h * w, torch.int32, SENT)
    cbuf, cv = framed(n, torch.int32, SENT)
    obuf, ov = framed(n * mo * 8, torch.int64, SENT)
    fbuf, fv = framed(n * h * w, torch.uint8, 77)
    nb = hip.unet_label_components_workspace(n, h, w)
    ws = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off) if t is not None else None

    def status(m=mask, elem=1, pitch=w, N=n, H=h, W=w, conn=8, bg=0, area=0, lab=lv, cnt=cv, out=fv, obj=ov, maxo=mo, wsp=ptr(ws), nbytes=nb):
        return raw(ptr(m), elem, pitch, N, H, W, conn, bg, area, ptr(lab) if torch.is_tensor(lab) else lab, ptr(cnt), ptr(out) if torch.is_tensor(out) else out,
                   ptr(obj), maxo, wsp, nbytes, ST())

    assert status(conn=6) == EINVAL and status(conn=0) == EINVAL
    assert status(elem=2) == EINVAL and status(elem=0) == EINVAL
    assert status(N=0) == EINVAL and status(H=0) == EINVAL and status(W=-1) == EINVAL
    assert status(N=1 << 11, H=1 << 10, W=1 << 10) == EINVAL and hip.unet_label_components_workspace(1 << 11, 1 << 10, 1 << 10) == 0
    assert hip.unet_label_components_workspace(0, 8, 8) == 0
    assert status(area=3, bg=-1) == EINVAL
    assert status(maxo=0) == EINVAL and status(maxo=0, obj=None) == 0        # no table: max_objects is not looked at
    torch.cuda.synchronize()
    lv.fill_(SENT); cv.fill_(SENT); fv.fill_(77); ws.fill_(0x5A)                        # (the accepted call above wrote its outputs and the workspace)
    assert status(m=None) == EINVAL and status(lab=None) == EINVAL and status(cnt=None) == EINVAL and status(wsp=None) == EINVAL
    assert status(wsp=ptr(ws, 4)) == EINVAL                                             # misaligned workspace
    assert status(pitch=w - 1) == EINVAL
    assert status(out=ctypes.c_void_p(mask.data_ptr() + 8)) == EINVAL                   # an output half over the input
    assert status(m=mask4, elem=4, out=None, lab=ctypes.c_void_p(mask4.data_ptr())) == EINVAL      # labels over the input
    assert status(m=mask, pitch=w + 8, out=ptr(mask)) == EINVAL                         # the alias is for dense rows only (and the buffer is too short: refused first)
    assert status(lab=ctypes.c_void_p(ws.data_ptr() + 16)) == EINVAL                    # an output inside the workspace
    assert status(nbytes=nb - 1) == ENOSPC
    torch.cuda.synchronize()
    assert (lbuf == SENT).all() and (cbuf == SENT).all() and (obuf == SENT).all() and (fbuf == 77).all() and (ws == 0x5A).all()
    assert (mask == 1).all() and (mask4 == 1).all()
    assert status() == 0
    torch.cuda.synchronize()
    assert (lv == 1).all() and cv.item() == 1 and ov[:8].tolist() == [1, 64, 0, 0, 7, 7, 28 * 8, 28 * 8] and (ov[8:] == SENT).all() and (fv == 1).all()


def test_label_components_enqueues_without_a_synchronise(monkeypatch):
    comp = pkg("components")
    m3 = cc.batch3(65, 129)
    want = cc.label_reference(m3, 8, 0, 4, 32)
    dev = torch.as_tensor(np.array(m3)).to(torch.uint8).to(DEV)
    comp.label_components(dev, min_area=4, max_objects=32)                              # (the workspace of this shape now exists)
    torch.cuda.synchronize()
    calls = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: calls.append("stream.synchronize"))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: calls.append("event.synchronize"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: calls.append("item"))
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self: calls.append("cpu"))
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: calls.append("tolist"))
    res = comp.label_components(dev, min_area=4, max_objects=32)
    two = comp.label_components(dev[1].to(torch.int32), connectivity=4, background=None, want_objects=False)
    monkeypatch.undo()
    assert calls == []
    assert isinstance(res, comp.Components) and all(t.is_cuda for t in res)
    got = tuple(t.cpu().numpy() for t in res)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int64 and got[3].dtype == np.uint8
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    one = cc.label_reference(m3[1:2], 4, None, 0, 8)
    assert two.objects is None and two.mask is None and two.labels.shape == (65, 129) and two.count.dim() == 0
    assert np.array_equal(two.labels.cpu().numpy(), one[0][0]) and int(two.count) == int(one[1][0])
    tables = comp.objects_table(got[1], got[2])
    assert len(tables) == 3
    for n, t in enumerate(tables):
        rows = min(int(want[1][n]), 32)
        assert len(t) == rows and t["label"].tolist() == list(range(1, rows + 1))
        assert np.array_equal(t["area"], want[2][n, :rows, 1]) and np.array_equal(t["bbox"], want[2][n, :rows, 2:6])
        assert np.array_equal(t["centroid_y"], want[2][n, :rows, 6] / want[2][n, :rows, 1])
    with pytest.raises(ValueError):
        comp.label_components(dev, connectivity=6)
    with pytest.raises(ValueError):
        comp.label_components(dev, background=None, min_area=2)
    with pytest.raises(ValueError):
        comp.label_components(dev.to(torch.int64))
