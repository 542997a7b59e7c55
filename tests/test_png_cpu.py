"""CPU: the host side of the PNG reader (files -> inflated scanlines -> table):
the C ABI of rr_png_probe / rr_png_inflate / rr_png_table_check, the errors
read_png raises before any launch, ImageFolder's listing of both kinds, and
the pin of tests/pngcraft.py to Pillow.  No launch anywhere."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import pngcraft as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
SIZES = [(1, 1), (1, 7), (7, 1), (63, 5), (64, 64), (65, 3), (129, 2), (130, 70), (66, 130)]
# rr_png_reason
EOPEN, ESIGNATURE, ETRUNCATED, ECRC, EHEADER, EKIND, ECHUNK, EZLIB, ESIZE, EFILTER, ESLOT = range(1, 12)


def _paths(paths):
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    return arr, C.cast(arr, C.c_void_p)


def _probe(paths):
    import roadrestore
    from roadrestore._lib import PngInfo
    info = (PngInfo * len(paths))()
    keep, arr = _paths(paths)
    rc = roadrestore.lib().rr_png_probe(len(paths), arr, C.cast(info, C.c_void_p), 2)
    return rc, [(i.h, i.w, i.channels, i.status, i.reason) for i in info]


def _inflate(path, h, w, c, slot_at=3, tail=5, kind=1):
    """rr_png_inflate of one file into a 0xEE buffer: -> (rc, status, reason,
    the slot's bytes, True if nothing outside the slot changed)"""
    import roadrestore
    from roadrestore._lib import PngImage, PngInfo
    need = h * (1 + w * c)
    buf = np.full(slot_at + need + tail, 0xEE, dtype=np.uint8)
    rec = (PngImage * 1)(PngImage(slot_at, 0, h, w, c, kind))
    info = (PngInfo * 1)()
    keep, arr = _paths([path])
    rc = roadrestore.lib().rr_png_inflate(1, arr, C.cast(rec, C.c_void_p), buf.ctypes.data, buf.size,
                                          C.cast(info, C.c_void_p), 1)
    outside = bool((buf[:slot_at] == 0xEE).all() and (buf[slot_at + need:] == 0xEE).all())
    return rc, info[0].status, info[0].reason, buf[slot_at:slot_at + need].tobytes(), outside


def _write(path, blob):
    with open(path, "wb") as f:
        f.write(blob)
    return str(path)


def test_symbols_exported_and_declared():
    import roadrestore
    lib = roadrestore.lib()
    hdr = open(os.path.join(REPO, "include", "roadrestore.h")).read()
    for name in ("rr_png_probe", "rr_png_inflate", "rr_png_table_check", "rr_png_unfilter"):
        assert hasattr(lib.dll, name), name
        assert name in roadrestore.EXPORTED
        assert name + "(" in hdr
    assert "png_unfilter" in roadrestore.ops.__all__
    for name in ("read_png", "read_images"):
        assert name in roadrestore.imgproc.__all__ and callable(getattr(roadrestore.imgproc, name))


def test_png_record_layouts(tmp_path):
    """the ctypes mirrors of rr_png_image (32 bytes) and rr_png_info (20) have
    gcc's layout of the header's structs"""
    from roadrestore._lib import PngImage, PngInfo
    assert C.sizeof(PngImage) == 32 and C.sizeof(PngInfo) == 20
    img_f = ["src", "dst", "h", "w", "channels", "kind"]
    inf_f = ["h", "w", "channels", "status", "reason"]
    assert [getattr(PngImage, f).offset for f in img_f] == [0, 8, 16, 20, 24, 28]
    assert [getattr(PngInfo, f).offset for f in inf_f] == [0, 4, 8, 12, 16]
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "roadrestore.h"', "int main(void) {",
             '  printf("%zu %zu\\n", sizeof(rr_png_image), sizeof(rr_png_info));']
    lines += [f'  printf("%zu\\n", offsetof(rr_png_image, {f}));' for f in img_f]
    lines += [f'  printf("%zu\\n", offsetof(rr_png_info, {f}));' for f in inf_f]
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 20] + [getattr(PngImage, f).offset for f in img_f] + \
        [getattr(PngInfo, f).offset for f in inf_f]


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_probe_and_inflate_give_the_filtered_stream(tmp_path, c):
    """multi-IDAT (1-byte chunks included), ancillary chunks in front: the
    inflated bytes are the helper's filtered scanlines, nothing else touched"""
    anc = [(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Comment\0by hand")]
    cases = [((1, 1), (), ()), ((26, 9), (1, 2, 50), anc), ((65, 3), (1,), ()), ((7, 1), tuple(range(1, 400)), anc),
             ((64, 64), (2,), anc)]
    paths, want = [], []
    for k, ((h, w), splits, extra) in enumerate(cases):
        blob, stream = P.make(P.pixels(h, w, c, 10 * c + k), splits=splits, ancillary=extra)
        paths.append(_write(tmp_path / f"{k}.png", blob))
        want.append((h, w, stream))
    rc, info = _probe(paths)
    assert rc == OK
    assert info == [(h, w, c, OK, 0) for h, w, _ in want]
    for p, (h, w, stream) in zip(paths, want):
        rc, st, why, got, outside = _inflate(p, h, w, c)
        assert (rc, st, why) == (OK, OK, 0), p
        assert got == stream and outside, p


def _header_only(colour, depth=8, interlace=0, w=4, h=4):
    return P.assemble(w, h, colour, zlib.compress(bytes(h * (1 + w))), depth=depth, interlace=interlace)


def _bad_files(tmp_path):
    """name -> (path, status, reason, (h, w, c) to inflate with)"""
    img = P.pixels(6, 5, 3, 99)
    good, stream = P.make(img)
    z = zlib.compress(stream)
    five = bytearray(stream)
    five[2 * 16] = 5                                         # row 2's filter byte
    crc_bad = bytearray(good)
    crc_bad[-13] ^= 1                                        # last byte of the IDAT CRC
    anc_crc = P.assemble(5, 6, 2, z, ancillary=[(b"tEXt", b"k\0v")])
    anc_crc = bytearray(anc_crc)
    anc_crc[8 + 25 + 8] ^= 0x40                              # first data byte of tEXt
    files = {
        "palette.png": (_header_only(3), EUNSUPPORTED, EKIND),
        "deep.png": (_header_only(2, depth=16), EUNSUPPORTED, EKIND),
        "deepgrey.png": (_header_only(0, depth=16), EUNSUPPORTED, EKIND),
        "onebit.png": (_header_only(0, depth=1), EUNSUPPORTED, EKIND),
        "adam7.png": (_header_only(2, interlace=1), EUNSUPPORTED, EKIND),
        "signature.png": (b"\x89PNG\r\n\x1a\r" + good[8:], EINVAL, ESIGNATURE),
        "crc.png": (bytes(crc_bad), EINVAL, ECRC),
        "anccrc.png": (bytes(anc_crc), EINVAL, ECRC),
        "truncated.png": (good[:len(good) - 20], EINVAL, ETRUNCATED),
        "noiend.png": (P.assemble(5, 6, 2, z, iend=False), EINVAL, ETRUNCATED),
        "short.png": (P.assemble(5, 6, 2, zlib.compress(stream[:-1])), EINVAL, ESIZE),
        "long.png": (P.assemble(5, 6, 2, zlib.compress(stream + b"\0")), EINVAL, ESIZE),
        "five.png": (P.assemble(5, 6, 2, zlib.compress(bytes(five))), EINVAL, EFILTER),
        "zerow.png": (P.assemble(0, 6, 2, z), EINVAL, EHEADER),
        "zeroh.png": (P.assemble(5, 0, 2, z), EINVAL, EHEADER),
        "cutzlib.png": (P.assemble(5, 6, 2, z[:-6]), EINVAL, EZLIB),
        "badtype.png": (P.assemble(5, 6, 5, z), EINVAL, EHEADER),
        "empty.png": (b"", EINVAL, ETRUNCATED),
    }
    return good, {k: (_write(tmp_path / k, v[0]), v[1], v[2]) for k, v in files.items()}


# detected from the first 33 bytes already
HEAD_ERRORS = {"palette.png", "deep.png", "deepgrey.png", "onebit.png", "adam7.png", "signature.png",
               "zerow.png", "zeroh.png", "badtype.png", "empty.png"}


def test_probe_and_inflate_refuse_bad_files(tmp_path):
    _, bad = _bad_files(tmp_path)
    for name, (path, status, reason) in bad.items():
        rc, info = _probe([path])
        if name in HEAD_ERRORS:
            assert (rc, info[0][3], info[0][4]) == (status, status, reason), name
        else:
            assert (rc, info[0]) == (OK, (6, 5, 3, OK, 0)), name
        rc, st, why, _, outside = _inflate(path, 6, 5, 3)
        assert (rc, st, why) == (status, status, reason), name
        assert outside, name
    rc, info = _probe([str(tmp_path / "missing.png")])
    assert (rc, info[0][3], info[0][4]) == (EINVAL, EINVAL, EOPEN)


def test_inflate_holds_the_record_to_the_file(tmp_path):
    """a record of another size or channel count, or a slot that leaves the
    buffer by one byte: refused, nothing written"""
    import roadrestore
    from roadrestore._lib import PngImage, PngInfo
    blob, stream = P.make(P.pixels(6, 5, 3, 1))
    path = _write(tmp_path / "a.png", blob)
    for h, w, c in ((5, 5, 3), (6, 4, 3), (6, 5, 4), (6, 5, 1)):
        rc, st, why, _, outside = _inflate(path, h, w, c)
        assert (rc, st, why, outside) == (EINVAL, EINVAL, ESLOT, True), (h, w, c)
    need = len(stream)
    keep, arr = _paths([path])
    for src, size, want in ((0, need, OK), (1, need, EINVAL), (0, need - 1, EINVAL), (-1, need + 8, EINVAL),
                            (2 ** 62, need, EINVAL)):
        buf = np.full(need + 8, 0xEE, dtype=np.uint8)
        rec = (PngImage * 1)(PngImage(src, 0, 6, 5, 3, 1))
        info = (PngInfo * 1)()
        rc = roadrestore.lib().rr_png_inflate(1, arr, C.cast(rec, C.c_void_p), buf.ctypes.data, size,
                                              C.cast(info, C.c_void_p), 1)
        assert rc == want and info[0].status == want, (src, size)
        if want == OK:
            assert buf[:need].tobytes() == stream and (buf[need:] == 0xEE).all()
        else:
            assert info[0].reason == ESLOT and (buf == 0xEE).all()


def test_read_png_raises_value_error_naming_the_file(tmp_path, monkeypatch):
    """every refusal surfaces from read_png / read_images as ValueError with
    the path, before the launch wrapper is reached"""
    from roadrestore import imgproc, ops

    def no_launch(*a, **k):
        raise AssertionError("png_unfilter reached for a bad file")
    monkeypatch.setattr(ops, "png_unfilter", no_launch)
    good_blob, bad = _bad_files(tmp_path)
    good = _write(tmp_path / "good.png", good_blob)
    words = {EKIND: "unsupported", ESIGNATURE: "signature", ECRC: "CRC", ETRUNCATED: "truncated",
             ESIZE: "inflated size", EFILTER: "filter byte", EHEADER: "IHDR", EZLIB: "zlib"}
    for name, (path, _, reason) in bad.items():
        for paths in ([path], [good, path, good]):
            with pytest.raises(ValueError, match=name.replace(".", r"\.")) as e:
                imgproc.read_png(paths, "cpu")
            assert words[reason] in str(e.value), (name, str(e.value))
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            imgproc.read_images([good, path], "cpu")
    with pytest.raises(ValueError, match="missing"):
        imgproc.read_png([good, str(tmp_path / "missing.png")], "cpu")
    with pytest.raises(ValueError):
        imgproc.read_png([], "cpu")
    with pytest.raises(ValueError, match=r"x\.jpg"):
        imgproc.read_images([good, str(tmp_path / "x.jpg")], "cpu")
    # a good file reaches the launch; and the real wrapper takes no host tensor
    with pytest.raises(AssertionError, match="reached"):
        imgproc.read_png([good], "cpu")
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="device"):
        imgproc.read_png([good], "cpu")


def _table(*recs):
    from roadrestore._lib import PngImage
    return (PngImage * len(recs))(*[PngImage(*r) for r in recs])


def _check(tab, in_bytes, out_bytes, max_h=250, max_w=250, n=None):
    import roadrestore
    return roadrestore.lib().rr_png_table_check(len(tab) if n is None else n, in_bytes, out_bytes,
                                                C.cast(tab, C.c_void_p), max_h, max_w)


def test_table_check_exact_fit_and_one_byte_out():
    # (src, dst, h, w, channels, kind): a PNG record then a raw one, back to back
    a_in, a_out = 10 * (1 + 7 * 4), 10 * 7 * 3
    b_in, b_out = 3 * 5 * 3, 3 * 5 * 3
    tab = _table((0, 0, 10, 7, 4, 1), (a_in, a_out, 3, 5, 3, 0))
    assert _check(tab, a_in + b_in, a_out + b_out) == OK
    assert _check(tab, a_in + b_in - 1, a_out + b_out) == EINVAL          # source one byte out
    assert _check(tab, a_in + b_in, a_out + b_out - 1) == EINVAL          # destination one byte out
    assert _check(_table((1, 0, 10, 7, 4, 1)), a_in, a_out) == EINVAL
    assert _check(_table((0, 1, 10, 7, 4, 1)), a_in, a_out) == EINVAL
    assert _check(_table((0, 0, 10, 7, 4, 0)), a_in - 10, a_out) == OK    # raw: no filter bytes
    assert _check(_table((0, 0, 10, 7, 4, 0)), a_in - 11, a_out) == EINVAL
    for bad in ((-1, 0, 10, 7, 4, 1), (0, -1, 10, 7, 4, 1), (0, 0, 0, 7, 4, 1), (0, 0, 10, 0, 4, 1),
                (0, 0, 10, 7, 0, 1), (0, 0, 10, 7, 5, 1), (0, 0, 10, 7, 4, 2), (0, 0, 10, 7, 4, -1),
                (2 ** 62, 0, 10, 7, 4, 1), (0, 2 ** 62, 10, 7, 4, 1), (-2 ** 63, 0, 10, 7, 4, 1)):
        assert _check(_table((0, 0, 10, 7, 4, 1), bad), 10 ** 6, 10 ** 6) == EINVAL, bad
    assert _check(_table((0, 0, 251, 7, 4, 1)), 10 ** 6, 10 ** 6) == EINVAL          # h > max_h
    assert _check(_table((0, 0, 10, 251, 4, 1)), 10 ** 6, 10 ** 6) == EINVAL         # w > max_w
    big = 2 ** 31 - 1
    assert _check(_table((0, 0, big, 8192, 4, 1)), 10 ** 6, 10 ** 6, max_h=big, max_w=8192) == EINVAL
    assert _check(_table((0, 0, 10, 7, 4, 1)), 10 ** 6, 10 ** 6, max_w=8193) == EUNSUPPORTED
    assert _check(tab, 10 ** 6, 10 ** 6, n=0) == EINVAL
    import roadrestore
    assert roadrestore.lib().rr_png_table_check(1, 100, 100, None, 10, 10) == EINVAL


def test_unfilter_validates_before_any_launch():
    import roadrestore
    L = roadrestore.lib()
    assert L.rr_png_unfilter(1, 10, 10, None, 100, 1, 1, 100, None) == EINVAL
    assert L.rr_png_unfilter(1, 10, 10, 1, 100, None, 1, 100, None) == EINVAL
    assert L.rr_png_unfilter(1, 10, 10, 1, 100, 1, None, 100, None) == EINVAL
    assert L.rr_png_unfilter(0, 10, 10, 1, 100, 1, 1, 100, None) == EINVAL
    assert L.rr_png_unfilter(1, 10, 10, 1, 0, 1, 1, 100, None) == EINVAL
    assert L.rr_png_unfilter(1, 10, 8193, 1, 100, 1, 1, 100, None) == EUNSUPPORTED


def test_pngcraft_matches_pillow(tmp_path):
    """the helper's files decode in Pillow to the source arrays (grey
    replicated, alpha dropped): the GPU tests then need no Pillow"""
    Image = pytest.importorskip("PIL.Image")
    anc = [(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Comment\0by hand")]
    k = 0
    for c in (1, 2, 3, 4):
        for h, w in SIZES:
            img = P.pixels(h, w, c, 1000 + k, edge=bool(k & 1))
            blob, _ = P.make(img, filters=P.cycle_filters(h, start=k), splits=(1, 2, 50) if k % 3 else (),
                             ancillary=anc if k % 2 else ())
            p = _write(tmp_path / f"{k}.png", blob)
            with Image.open(p) as im:
                assert im.mode == {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[c]
                got = np.asarray(im.convert("RGB"))
            assert np.array_equal(got, P.to_rgb(img)), (c, h, w)
            k += 1


def test_image_folder_lists_both_kinds(tmp_path):
    from roadrestore import imgproc
    blob, _ = P.make(P.pixels(2, 3, 3, 0))
    ppm = b"P6\n3 2\n255\n" + P.pixels(2, 3, 3, 1).tobytes()
    files = {"00001/b.png": blob, "00001/a.ppm": ppm, "00001/c.PNG": blob, "00001/notes.txt": b"x",
             "00000/z.png": blob, "00000/sub/a.ppm": ppm, "00000/m.jpg": b"x"}
    for rel, data in files.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)
    both = imgproc.ImageFolder(tmp_path, extensions=(".ppm", ".png"), device="cpu")
    want = [("00000/z.png", 0), ("00000/sub/a.ppm", 0), ("00001/a.ppm", 1), ("00001/b.png", 1), ("00001/c.PNG", 1)]
    assert both.samples == [(os.path.join(str(tmp_path), *rel.split("/")), i) for rel, i in want]
    only_png = imgproc.ImageFolder(tmp_path, extensions=(".png",), device="cpu")
    assert [os.path.basename(p) for p, _ in only_png.samples] == ["z.png", "b.png", "c.PNG"]
    default = imgproc.ImageFolder(tmp_path, device="cpu")
    assert [os.path.basename(p) for p, _ in default.samples] == ["a.ppm", "a.ppm"]
    # the default folder still loads through read_ppm, on the host
    batch, y = default.load([0, 1])
    assert batch.sizes == [(2, 3), (2, 3)] and y.tolist() == [0, 1] and batch.data.device.type == "cpu"
