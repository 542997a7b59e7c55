"""CPU: the host side of the ragged-batch path (files of unequal size -> the
first tensor): the C ABI of rr_resize_ragged_u8 and its table check, the PPM
header parser, and ImageFolder's torchvision ordering.  No launch anywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4


def _table(*recs):
    from roadrestore._lib import RaggedImage
    return (RaggedImage * len(recs))(*[RaggedImage(o, h, w) for o, h, w in recs])


def _check(tab, n=None, c=3, in_bytes=0, max_h=250, max_w=250, oh=32, ow=32):
    import roadrestore
    return roadrestore.lib().rr_ragged_check(len(tab) if n is None else n, c, in_bytes,
                                             C.cast(tab, C.c_void_p), max_h, max_w, oh, ow)


def test_symbols_exported_and_declared():
    import roadrestore
    lib = roadrestore.lib()
    hdr = open(os.path.join(REPO, "include", "roadrestore.h")).read()
    for name in ("rr_ragged_check", "rr_resize_ragged_workspace", "rr_resize_ragged_u8"):
        assert hasattr(lib.dll, name), name
        assert name in roadrestore.EXPORTED
        assert name + "(" in hdr
    assert "resize_ragged_u8" in roadrestore.ops.__all__


def test_ragged_image_layout(tmp_path):
    """the ctypes mirror of rr_ragged_image has gcc's layout of the header's
    struct (16 bytes: int64 offset, int32 h, int32 w)"""
    from roadrestore._lib import RaggedImage
    assert C.sizeof(RaggedImage) == 16
    assert (RaggedImage.offset.offset, RaggedImage.h.offset, RaggedImage.w.offset) == (0, 8, 12)
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "roadrestore.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(rr_ragged_image), offsetof(rr_ragged_image, offset),\n'
                   '         offsetof(rr_ragged_image, h), offsetof(rr_ragged_image, w));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(RaggedImage), RaggedImage.offset.offset, RaggedImage.h.offset,
                   RaggedImage.w.offset]


def test_ragged_check_accepts_exact_fit():
    # three images back to back, the last one ending on the buffer's last byte
    sizes = [(1, 1), (250, 15), (2, 250)]
    off, recs = 7, []
    for h, w in sizes:
        recs.append((off, h, w))
        off += h * w * 3
    assert _check(_table(*recs), in_bytes=off) == 0
    assert _check(_table((0, 250, 250)), in_bytes=250 * 250 * 3) == 0
    assert _check(_table((0, 250, 250)), c=1, in_bytes=250 * 250) == 0


def test_ragged_check_rejects_bad_tables():
    ok = (0, 10, 10)
    nb = 10 * 10 * 3
    assert _check(_table(ok), in_bytes=nb) == 0
    assert _check(_table(ok, (0, 0, 10)), in_bytes=nb) == EINVAL               # h = 0
    assert _check(_table(ok, (0, 10, 0)), in_bytes=nb) == EINVAL               # w = 0
    assert _check(_table((0, 1, 251)), in_bytes=10 ** 6) == EINVAL             # w > max_w
    assert _check(_table((0, 251, 1)), in_bytes=10 ** 6) == EINVAL             # h > max_h
    assert _check(_table(ok, (1, 10, 10)), in_bytes=nb) == EINVAL              # ends one byte past
    assert _check(_table(ok, (-1, 10, 10)), in_bytes=nb) == EINVAL             # negative offset
    assert _check(_table(ok, (-2 ** 63, 10, 10)), in_bytes=nb) == EINVAL
    assert _check(_table(ok, (2 ** 62, 10, 10)), in_bytes=nb) == EINVAL
    assert _check(_table(ok), c=5, in_bytes=10 ** 6) == EINVAL                 # c = 5
    assert _check(_table(ok), c=0, in_bytes=10 ** 6) == EINVAL
    assert _check(_table(ok), n=0, in_bytes=nb) == EINVAL
    import roadrestore
    assert roadrestore.lib().rr_ragged_check(1, 3, nb, None, 250, 250, 32, 32) == EINVAL
    # more than 255 taps: max_w / ow > 127 (ksize = 2 * ceil(scale) + 1)
    assert _check(_table(ok), in_bytes=nb, max_w=128 * 32 + 1, ow=32) == EUNSUPPORTED
    assert _check(_table(ok), in_bytes=nb, max_h=128 * 32 + 1, oh=32) == EUNSUPPORTED
    assert _check(_table(ok), in_bytes=nb, max_w=127 * 32, ow=32) == 0         # 255 taps: the last accepted


def test_resize_ragged_validates_before_any_launch():
    """a null table, a short workspace, bad arguments: status codes, no GPU"""
    import roadrestore
    L = roadrestore.lib()
    need = L.rr_resize_ragged_workspace(4, 3, 250, 250, 224, 224)
    assert need > 0
    args = (4, 3, 250, 250, 224, 224)
    assert L.rr_resize_ragged_u8(*args, 1, 1000, None, 0, None, None, 1, 1, need, None) == EINVAL
    assert L.rr_resize_ragged_u8(*args, 1, 1000, 1, 0, None, None, 1, 1, need - 1, None) == EWORKSPACE
    assert L.rr_resize_ragged_u8(*args, None, 1000, 1, 0, None, None, 1, 1, need, None) == EINVAL
    assert L.rr_resize_ragged_u8(*args, 1, 1000, 1, 2, None, None, 1, 1, need, None) == EINVAL    # out_kind
    assert L.rr_resize_ragged_u8(4, 5, 250, 250, 224, 224, 1, 1000, 1, 0, None, None, 1, 1, need,
                                 None) == EINVAL
    assert L.rr_resize_ragged_u8(4, 3, 128 * 224 + 1, 250, 224, 224, 1, 1000, 1, 0, None, None, 1, 1,
                                 1 << 40, None) == EUNSUPPORTED
    mean = (C.c_float * 3)(0.5, 0.5, 0.5)
    # Normalize needs the fp32 output, and mean with std
    assert L.rr_resize_ragged_u8(*args, 1, 1000, 1, 0, C.cast(mean, C.c_void_p), C.cast(mean, C.c_void_p),
                                 1, 1, need, None) == EINVAL
    assert L.rr_resize_ragged_u8(*args, 1, 1000, 1, 1, C.cast(mean, C.c_void_p), None,
                                 1, 1, need, None) == EINVAL
    assert L.rr_resize_ragged_workspace(0, 3, 250, 250, 224, 224) == 0
    assert L.rr_resize_ragged_workspace(4, 3, 128 * 224 + 1, 250, 224, 224) == 0


def test_ragged_workspace_monotonic():
    import roadrestore
    ws = roadrestore.lib().rr_resize_ragged_workspace
    for oh, ow in ((32, 32), (24, 40), (224, 224)):
        prev = 0
        for n in (1, 2, 3, 10, 64, 65):
            cur = ws(n, 3, 250, 250, oh, ow)
            assert cur >= prev > -1 and cur > 0
            prev = cur
        for axis in (0, 1):
            prev = 0
            for m in (1, 2, 15, 31, 32, 33, 64, 65, 224, 225, 250, 449, 1000, 3000):
                hw = (m, 250) if axis == 0 else (250, m)
                cur = ws(8, 3, hw[0], hw[1], oh, ow)
                assert cur >= prev and cur > 0, (oh, ow, axis, m)
                prev = cur


# ---------------------------------------------------------------- PPM ----

def _write(path, header, pixels):
    with open(path, "wb") as f:
        f.write(header + pixels.tobytes())
    return str(path)


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _unpack(batch):
    """the images of a host RaggedBatch, through its table"""
    assert batch.data.device.type == "cpu" and batch.table.device.type == "cpu"
    from roadrestore._lib import RaggedImage
    raw = batch.table.numpy().tobytes()
    recs = (RaggedImage * len(batch)).from_buffer_copy(raw)
    data = batch.data.numpy()
    out = []
    for r, (h, w) in zip(recs, batch.sizes):
        assert (r.h, r.w) == (h, w)
        out.append(data[r.offset:r.offset + h * w * batch.channels].reshape(h, w, batch.channels))
    return out


def test_read_ppm_header_grammar(tmp_path):
    """comments, CR/LF and runs of blanks between the tokens; exactly one
    whitespace byte after maxval, whatever the first pixel bytes look like"""
    from roadrestore import imgproc
    a, b, c_, d = _img(5, 7, 1), _img(3, 2, 2), _img(4, 4, 3), _img(2, 3, 4)
    c_.reshape(-1)[:6] = np.frombuffer(b"12 \n#3", dtype=np.uint8)     # pixels that look like a header
    d.reshape(-1)[:3] = np.frombuffer(b"\n\n ", dtype=np.uint8)        # pixels that look like whitespace
    paths = [
        _write(tmp_path / "a.ppm", b"P6\n# made by hand\n7 5\n255\n", a),
        _write(tmp_path / "b.ppm", b"P6\r\n2   \t 3\r\n#c1\r\n# c2\n  255\r", b),
        _write(tmp_path / "c.ppm", b"P6 4 4 255 ", c_),
        _write(tmp_path / "d.ppm", b"P6#x\n3#w\n2\n200\n", d),
    ]
    for threads in (0, 1, 3):
        batch = imgproc.read_ppm(paths, "cpu", threads=threads)
        assert isinstance(batch, imgproc.RaggedBatch) and len(batch) == 4 and batch.channels == 3
        assert batch.sizes == [(5, 7), (3, 2), (4, 4), (2, 3)]
        assert batch.max_hw == (5, 7)
        assert batch.table.dtype == torch.uint8 and tuple(batch.table.shape) == (4, 16)
        for got, want in zip(_unpack(batch), (a, b, c_, d)):
            assert np.array_equal(got, want)


def test_read_ppm_matches_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from roadrestore import imgproc
    paths = []
    for i, (h, w) in enumerate([(1, 1), (15, 17), (61, 32), (10, 49)]):
        p = tmp_path / f"{i}.ppm"
        Image.fromarray(_img(h, w, 10 + i)).save(p)
        paths.append(str(p))
    batch = imgproc.read_ppm(paths, "cpu")
    for got, p in zip(_unpack(batch), paths):
        assert np.array_equal(got, np.asarray(Image.open(p)))


def test_read_ppm_rejects_other_files(tmp_path):
    from roadrestore import imgproc
    good = _write(tmp_path / "good.ppm", b"P6\n2 2\n255\n", _img(2, 2, 0))
    bad = {
        "gray.ppm": b"P5\n2 2\n255\n" + bytes(4),
        "ascii.ppm": b"P3\n1 1\n255\n1 2 3\n",
        "deep.ppm": b"P6\n2 2\n65535\n" + bytes(24),
        "short.ppm": b"P6\n2 2\n255\n" + bytes(11),
        "nohdr.ppm": b"P6\n2 2\n",
        "empty.ppm": b"",
        "glued.ppm": b"P62 2 255\n" + bytes(12),
    }
    for name, blob in bad.items():
        p = tmp_path / name
        p.write_bytes(blob)
        for paths in ([str(p)], [good, str(p), good]):
            with pytest.raises(ValueError, match=name.replace(".", r"\.")):
                imgproc.read_ppm(paths, "cpu")
    assert len(imgproc.read_ppm([good, good], "cpu")) == 2


def test_ragged_batch_constructor_checks_on_host():
    from roadrestore import imgproc
    imgs = [_img(3, 5, 0), _img(1, 1, 1), _img(6, 2, 2)]
    b = imgproc.RaggedBatch.from_arrays(imgs + [torch.from_numpy(_img(2, 2, 3))], "cpu")
    assert len(b) == 4 and b.channels == 3 and b.sizes == [(3, 5), (1, 1), (6, 2), (2, 2)]
    assert b.max_hw == (6, 5) and b.data.numel() == (15 + 1 + 12 + 4) * 3
    for got, want in zip(_unpack(b), imgs):
        assert np.array_equal(got, want)
    data = torch.zeros(100, dtype=torch.uint8)
    imgproc.RaggedBatch(data, [(1, 3, 11)], 3)                         # ends on the last byte
    for rec in [(2, 3, 11), (-1, 3, 11), (0, 0, 11), (0, 3, 0)]:
        with pytest.raises(ValueError, match="image 1"):
            imgproc.RaggedBatch(data, [(0, 1, 1), rec], 3)
    with pytest.raises(ValueError):
        imgproc.RaggedBatch(data, [(0, 1, 1)], 5)
    with pytest.raises(ValueError):
        imgproc.RaggedBatch(data, [(0, 3, 11)], 3, max_hw=(3, 10))     # w > max_w
    with pytest.raises(ValueError):
        imgproc.RaggedBatch(data, [], 3)
    with pytest.raises(ValueError):
        imgproc.RaggedBatch.from_arrays([_img(2, 2, 0), _img(2, 2, 0)[..., :1]], "cpu")
    # a ragged batch has no dense shape; the device ops take no host tensors
    with pytest.raises(TypeError):
        imgproc.ToTensor()(b)
    with pytest.raises(RuntimeError, match="device"):
        imgproc.Resize((4, 4))(b)


# -------------------------------------------------------- ImageFolder ----

def test_image_folder_order_is_torchvisions(tmp_path):
    from roadrestore import imgproc
    files = {
        "00010/b.ppm": (3, 4), "00010/a.PPM": (2, 2), "00010/notes.txt": None,
        "00002/z.ppm": (5, 1), "00002/sub/a.ppm": (1, 6), "00002/sub/deep/c.Ppm": (2, 3),
        "00002/a_dir/y.ppm": (4, 4), "00002/readme.txt": None,
        "00001/10.ppm": (2, 5), "00001/9.ppm": (3, 3), "00001/1.ppm": (7, 2), "00001/GT-00001.csv": None,
        "top.ppm": (1, 1),
    }
    for rel, hw in files.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        if hw is None:
            p.write_text("x")
        else:
            _write(p, b"P6\n%d %d\n255\n" % (hw[1], hw[0]), _img(hw[0], hw[1], len(rel)))
    (tmp_path / "00005").mkdir()                                        # a class with no image
    ds = imgproc.ImageFolder(tmp_path, device="cpu")
    assert ds.classes == ["00001", "00002", "00005", "00010"]
    assert ds.class_to_idx == {"00001": 0, "00002": 1, "00005": 2, "00010": 3}
    want = [("00001/1.ppm", 0), ("00001/10.ppm", 0), ("00001/9.ppm", 0),
            ("00002/z.ppm", 1), ("00002/a_dir/y.ppm", 1), ("00002/sub/a.ppm", 1),
            ("00002/sub/deep/c.Ppm", 1),
            ("00010/a.PPM", 3), ("00010/b.ppm", 3)]
    # one more for ten samples
    _write(tmp_path / "00010" / "c.ppm", b"P6\n1 1\n255\n", _img(1, 1, 0))
    want.append(("00010/c.ppm", 3))
    ds = imgproc.ImageFolder(tmp_path, device="cpu")
    assert ds.samples == [(os.path.join(str(tmp_path), *rel.split("/")), i) for rel, i in want]
    assert len(ds) == 10 and ds.targets == [i for _, i in want]

    got = list(ds.batches(4))
    assert [len(b) for b, _ in got] == [4, 4, 2]
    assert torch.cat([y for _, y in got]).tolist() == ds.targets
    assert all(y.dtype == torch.int64 for _, y in got)
    sizes = [s for b, _ in got for s in b.sizes]
    assert sizes == [files.get(rel, (1, 1)) for rel, _ in want]

    g = torch.Generator().manual_seed(3)
    order = torch.randperm(10, generator=torch.Generator().manual_seed(3)).tolist()
    shuf = list(ds.batches(4, shuffle=True, generator=g))
    assert [len(b) for b, _ in shuf] == [4, 4, 2]
    assert torch.cat([y for _, y in shuf]).tolist() == [ds.targets[i] for i in order]

    batch, y = ds.load([9, 0])
    assert batch.sizes == [(1, 1), (7, 2)] and y.tolist() == [3, 0]
    assert imgproc.find_images(tmp_path) == sorted(tmp_path.glob("*/*.ppm"))
    assert [p.name for p in imgproc.find_images(tmp_path / "00001")] == []
    assert [p.name for p in imgproc.find_images(tmp_path, "00001/*.ppm")] == ["1.ppm", "10.ppm", "9.ppm"]
    with pytest.raises(FileNotFoundError):
        imgproc.ImageFolder(tmp_path / "00005")
