"""GPU: the PNG unfilter kernel (rr_png_unfilter) and the readers built on it
(imgproc.read_png / read_images / ImageFolder) against the source arrays the
files were made from.  Everything is compared bit for bit; tests/pngcraft.py
builds the files (pinned to Pillow in test_png_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import parity
import pngcraft as P

pytestmark = pytest.mark.gpu

# no left neighbour (w = 1), no row above (h = 1), band boundaries at rows
# 63/64/65 and 128/129, images narrower than the 64-step skew with more than
# one band, images wider than a wave
SIZES = [(1, 1), (1, 7), (7, 1), (26, 9), (63, 5), (64, 64), (65, 3), (65, 1), (129, 2), (130, 70),
         (66, 130), (2, 250)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _table(recs):
    """(src, dst, h, w, channels, kind) records -> [n, 32] uint8 host tensor"""
    from roadrestore.imgproc import _PNG_RECORD
    arr = np.array(recs, dtype=_PNG_RECORD)
    return torch.from_numpy(arr.view(np.uint8).reshape(len(recs), 32).copy())


def _pack(images, filters=None, kinds=None):
    """source arrays -> (input bytes, records, expected RGB arrays): the
    filtered streams (kind 1) or raw rows (kind 0) back to back, so offsets
    are odd and unaligned"""
    blobs, recs, src, dst = [], [], 0, 0
    for i, img in enumerate(images):
        h, w, c = img.shape
        kind = 1 if kinds is None else kinds[i]
        blob = P.filter_stream(img, P.cycle_filters(h) if filters is None else filters[i]) if kind else img.tobytes()
        blobs.append(blob)
        recs.append((src, dst, h, w, c, kind))
        src += len(blob)
        dst += h * w * 3
    return b"".join(blobs), recs, [P.to_rgb(im) for im in images]


def _unfilter(dev, data, recs, out_bytes, max_hw=None, fill=0xFF):
    """ops.png_unfilter into a guarded 0xFF buffer -> (host bytes, guards intact)"""
    from roadrestore import ops
    if max_hw is None:
        max_hw = (max(r[2] for r in recs), max(r[3] for r in recs))
    buf, view = parity.guarded((out_bytes,), torch.uint8, dev)
    assert int(view[0]) == fill
    d = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    got = ops.png_unfilter(d, _table(recs).to(dev), max_hw, out_bytes, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr()
    return got.cpu().numpy(), parity.intact(buf)


def _compare(out, recs, want):
    for i, (r, w) in enumerate(zip(recs, want)):
        got = out[r[1]:r[1] + w.size].reshape(w.shape)
        if not np.array_equal(got, w):
            bad = np.argwhere(got != w)
            raise AssertionError(f"image {i} {r[2]} x {r[3]} x {r[4]}: {len(bad)} bytes differ, first at "
                                 f"(row, col, ch) {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_every_filter_pair(dev, c):
    """the 26-row cycle holds all 25 (previous, current) filter pairs; half
    the images uniform random, half from the values that give Paeth ties and
    9-bit Average sums"""
    pairs = set(zip(P.CYCLE[:-1], P.CYCLE[1:]))
    assert len(P.CYCLE) == 26 and len(pairs) == 25
    images = [P.pixels(h, w, c, 100 * c + i, edge=bool(i & 1)) for i, (h, w) in enumerate(SIZES)]
    data, recs, want = _pack(images)
    assert any(r[0] & 3 for r in recs)
    out, ok = _unfilter(dev, data, recs, sum(w.size for w in want))
    _compare(out, recs, want)
    assert ok


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4])
def test_one_filter_for_the_whole_image(dev, ft):
    """all-Paeth and all-Average are the long dependent chains; 130 rows cross
    two band boundaries"""
    shapes = [(130, 70, 3), (130, 3, 4), (1, 70, 3), (70, 1, 3)]
    images = [P.pixels(h, w, c, 7 * ft + i, edge=bool(i & 1)) for i, (h, w, c) in enumerate(shapes)]
    data, recs, want = _pack(images, filters=[[ft] * im.shape[0] for im in images])
    out, ok = _unfilter(dev, data, recs, sum(w.size for w in want))
    _compare(out, recs, want)
    assert ok


def _batch_images(batch):
    data = batch.data.cpu().numpy()
    out = []
    for r, (h, w) in zip(batch.records, batch.sizes):
        assert (int(r["h"]), int(r["w"])) == (h, w)
        o = int(r["offset"])
        out.append(data[o:o + h * w * 3].reshape(h, w, 3))
    return out


def test_round_trip_through_the_writer(dev, tmp_path):
    from roadrestore import imgproc
    a = np.stack([P.smooth(224, 224, 3, 40 + i, k=3 + 2 * (i % 3)) for i in range(8)])
    a[1, ::2] = P.pixels(112, 224, 3, 5)                    # noisy rows between smooth ones
    a[2, :, 100:] = 200                                     # a flat half
    paths = [tmp_path / "a" / f"{i}.png" for i in range(8)]
    imgproc.write_png(torch.from_numpy(a).to(dev), paths)
    seen = set()
    for p in paths:
        seen |= set(P.filter_bytes(p.read_bytes()))
    assert seen == {0, 1, 2, 3, 4}, seen                    # not None rows alone
    batch = imgproc.read_png(paths, dev)
    assert isinstance(batch, imgproc.RaggedBatch) and batch.channels == 3 and batch.data.is_cuda
    assert batch.sizes == [(224, 224)] * 8
    for i, got in enumerate(_batch_images(batch)):
        assert np.array_equal(got, a[i]), i
    # batch B: a one-pixel RGB image and a grey one, which comes back replicated
    rgb, grey = P.pixels(1, 1, 3, 1), P.pixels(25, 31, 1, 2)
    pb = [tmp_path / "b" / "rgb.png", tmp_path / "b" / "grey.png"]
    imgproc.write_png(torch.from_numpy(rgb[None]), pb[:1])
    imgproc.write_png(torch.from_numpy(grey[None]), pb[1:])
    for threads in (0, 1):
        batch = imgproc.read_png(pb, dev, threads=threads)
        assert batch.sizes == [(1, 1), (25, 31)] and batch.channels == 3
        got = _batch_images(batch)
        assert np.array_equal(got[0], rgb) and np.array_equal(got[1], np.repeat(grey, 3, axis=2))


def _ppm(path, img):
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    return str(path)


def _png(path, img, **kw):
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(P.make(img, **kw)[0])
    return str(path)


def test_mixed_list(dev, tmp_path):
    from roadrestore import imgproc
    shapes = [("ppm", 5, 7, 3), ("png", 66, 3, 4), ("png", 9, 31, 1), ("ppm", 1, 1, 3), ("png", 65, 130, 3),
              ("ppm", 70, 2, 3), ("png", 3, 3, 2)]
    paths, want = [], []
    for i, (kind, h, w, c) in enumerate(shapes):
        img = P.pixels(h, w, c, 300 + i)
        want.append(P.to_rgb(img))
        p = tmp_path / f"{i}.{kind}"
        paths.append(_ppm(p, img) if kind == "ppm" else _png(p, img, splits=(1, 7)))
    batch = imgproc.read_images(paths, dev, threads=2)
    assert batch.sizes == [(h, w) for _, h, w, _ in shapes] and batch.channels == 3
    for i, (got, w) in enumerate(zip(_batch_images(batch), want)):
        assert np.array_equal(got, w), (i, shapes[i])
    # an all-PPM list is read_ppm's result: same records, same buffer bytes
    ppms = [p for p in paths if p.endswith(".ppm")]
    x, y = imgproc.read_images(ppms, dev), imgproc.read_ppm(ppms, dev)
    assert np.array_equal(x.records, y.records) and torch.equal(x.data, y.data) and torch.equal(x.table, y.table)


def test_files_to_the_first_tensor(dev, tmp_path):
    from roadrestore import imgproc
    files = [("00000/a.png", 40, 31, 3), ("00000/b.ppm", 17, 50, 3), ("00000/c.png", 65, 20, 1),
             ("00001/a.ppm", 33, 33, 3), ("00001/sub/z.png", 20, 70, 4), ("00002/x.png", 31, 64, 2)]
    sources = []
    for rel, h, w, c in files:
        img = P.pixels(h, w, c, len(rel) + h)
        sources.append(P.to_rgb(img))
        (_ppm if rel.endswith(".ppm") else _png)(tmp_path / rel, img)
    ds = imgproc.ImageFolder(tmp_path, extensions=(".ppm", ".png"), device=dev)
    assert [os.path.relpath(p, tmp_path).replace(os.sep, "/") for p, _ in ds.samples] == [f[0] for f in files]
    tf = imgproc.Compose([imgproc.Resize((32, 32)), imgproc.ToTensor(), imgproc.Normalize(MEAN, STD)])
    ref = tf(imgproc.RaggedBatch.from_arrays(sources, dev))
    got, labels = [], []
    for batch, y in ds.batches(4):
        got.append(tf(batch))
        labels.append(y)
    got = torch.cat(got)
    assert got.shape == (6, 3, 32, 32) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    assert torch.equal(torch.cat(labels).cpu(), torch.tensor([0, 0, 0, 1, 1, 2]))


def test_bad_records_are_skipped(dev):
    """one record past the input buffer and one past the output buffer between
    two good ones: the good images exact, the bad ones' bytes untouched"""
    images = [P.pixels(66, 5, 3, 1), P.pixels(4, 6, 3, 2), P.pixels(5, 4, 3, 3), P.pixels(7, 70, 4, 4)]
    data, recs, want = _pack(images)
    out_bytes = sum(w.size for w in want)
    recs[1] = (len(data) - 4 * 19 + 1, recs[1][1], 4, 6, 3, 1)          # ends one byte past the input
    recs[2] = (recs[2][0], out_bytes - 5 * 4 * 3 + 1, 5, 4, 3, 1)       # ends one byte past the output
    import ctypes as C
    import roadrestore
    from roadrestore._lib import PngImage
    tab = (PngImage * 4)(*[PngImage(*r) for r in recs])
    assert roadrestore.lib().rr_png_table_check(4, len(data), out_bytes, C.cast(tab, C.c_void_p), 66, 70) == -1
    out, ok = _unfilter(dev, data, recs, out_bytes, max_hw=(66, 70))
    _compare(out, [recs[0], recs[3]], [want[0], want[3]])
    lo, hi = recs[0][1] + want[0].size, recs[3][1]
    assert (out[lo:hi] == 0xFF).all()
    assert ok
    # sizes outside the bound the launch was given are skipped too
    data, recs, want = _pack(images[:2])
    out, ok = _unfilter(dev, data, recs, sum(w.size for w in want), max_hw=(65, 70))
    assert (out[:want[0].size] == 0xFF).all() and ok
    _compare(out, recs[1:], want[1:])
