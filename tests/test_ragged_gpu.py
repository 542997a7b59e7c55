"""GPU parity of the ragged resize (rr_resize_ragged_u8: images of unequal size
in one buffer -> one dense batch) against the CPU oracle's per-image PIL
resample (oracle/imgproc_cpu.py, pinned to Pillow in test_imgproc_cpu.py).
Everything is compared bit for bit: the arithmetic is integer up to the final
fp32 division, as for the dense path (test_imgproc_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import imgproc_cpu as I

pytestmark = pytest.mark.gpu

# up- and downscale on each axis independently, the same-size image (32, 32),
# one axis equal, 3 to 23 taps, a one-pixel image first in the buffer
SIZES = [(1, 1), (15, 17), (25, 25), (32, 32), (32, 61), (61, 32), (31, 33), (243, 225), (250, 15),
         (2, 250)]
TARGETS = [(32, 32), (24, 40)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

_CACHE = {}


def _images(sizes, c=3, seed=0):
    key = ("img", tuple(sizes), c, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        _CACHE[key] = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]
    return _CACHE[key]


def _resized(sizes, c, seed, oh, ow):
    """the oracle's per-image results, computed once and shared (read-only)"""
    key = ("ref", tuple(sizes), c, seed, oh, ow)
    if key not in _CACHE:
        ref = [I.pil_resize_bilinear(im, oh, ow) for im in _images(sizes, c, seed)]
        for r in ref:
            r.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _want(ref_u8, kind, c=3):
    if kind == "u8":
        return ref_u8
    if kind == "f32":
        return I.to_tensor_normalize(ref_u8)
    return I.to_tensor_normalize(ref_u8, MEAN[:c], STD[:c])


def _run(batch, oh, ow, kind, c=3):
    if kind == "u8":
        return batch.resize(oh, ow).cpu().numpy()
    if kind == "f32":
        return batch.resize(oh, ow, out="f32").cpu().numpy()
    return batch.resize(oh, ow, out="f32", mean=MEAN[:c], std=STD[:c]).cpu().numpy()


@pytest.mark.parametrize("kind", ["u8", "f32", "f32norm"])
@pytest.mark.parametrize("oh,ow", TARGETS)
def test_ragged_batch_matches_oracle_per_image(dev, oh, ow, kind):
    from roadrestore import imgproc
    batch = imgproc.RaggedBatch.from_arrays(_images(SIZES), dev)
    assert len(batch) == 10 and batch.max_hw == (250, 250) and batch.table.is_cuda
    y = _run(batch, oh, ow, kind)
    assert y.shape == ((10, oh, ow, 3) if kind == "u8" else (10, 3, oh, ow))
    assert y.dtype == (np.uint8 if kind == "u8" else np.float32)
    ref = _resized(SIZES, 3, 0, oh, ow)
    for i, size in enumerate(SIZES):
        assert np.array_equal(y[i], _want(ref[i], kind)), (i, size)
    # the same-size image comes back as it went in (Pillow copies it)
    if (oh, ow) == (32, 32):
        assert np.array_equal(ref[3], _images(SIZES)[3])


@pytest.mark.parametrize("c", [3, 1])
def test_ragged_to_the_reference_target(dev, c):
    """17:66 / 18:28-32: Resize((224, 224)), an upscale and a downscale in one batch"""
    from roadrestore import imgproc
    sizes = [(25, 25), (243, 225)]
    batch = imgproc.RaggedBatch.from_arrays(_images(sizes, c, seed=5), dev)
    ref = _resized(sizes, c, 5, 224, 224)
    for kind in ("u8", "f32norm"):
        y = _run(batch, 224, 224, kind, c)
        for i in range(2):
            assert np.array_equal(y[i], _want(ref[i], kind, c)), (kind, i)


def test_ragged_one_channel_all_sizes(dev):
    from roadrestore import imgproc
    batch = imgproc.RaggedBatch.from_arrays(_images(SIZES, 1, seed=2), dev)
    assert batch.channels == 1
    ref = _resized(SIZES, 1, 2, 24, 40)
    for kind in ("u8", "f32"):
        y = _run(batch, 24, 40, kind, 1)
        for i in range(len(SIZES)):
            assert np.array_equal(y[i], _want(ref[i], kind, 1)), (kind, i)


@pytest.mark.parametrize("oh,ow", [(24, 40), (31, 33)])
def test_uniform_ragged_batch_equals_dense_resize(dev, oh, ow):
    """images that all share one size: byte for byte the dense op on the
    stacked tensor -- also at the same size, where the dense op copies"""
    from roadrestore import imgproc, ops
    imgs = _images([(31, 33)] * 5, seed=7)
    batch = imgproc.RaggedBatch.from_arrays(imgs, dev)
    dense = torch.from_numpy(np.stack(imgs)).to(dev)
    assert torch.equal(batch.resize(oh, ow), ops.resize_bilinear_u8(dense, oh, ow))
    a = batch.resize(oh, ow, out="f32", mean=MEAN, std=STD)
    b = ops.resize_bilinear_u8(dense, oh, ow, out="f32", mean=MEAN, std=STD)
    assert torch.equal(a, b)
    assert torch.equal(imgproc.Resize((oh, ow))(batch), imgproc.Resize((oh, ow))(dense))


def test_files_to_normalised_batch(dev, tmp_path):
    """05:24-32 / 18:28-36: ImageFolder + Compose([Resize, ToTensor, Normalize])
    on PPM files the test writes"""
    from roadrestore import imgproc as T
    sizes = [(15, 17), (40, 32), (32, 61), (7, 90)]
    imgs = _images(sizes, seed=11)
    for i, im in enumerate(imgs):
        d = tmp_path / f"{i % 2:05d}"
        d.mkdir(exist_ok=True)
        hdr = b"P6\n# sign %d\n%d %d\n255\n" % (i, im.shape[1], im.shape[0])
        (d / f"{i}.ppm").write_bytes(hdr + im.tobytes())
    ds = T.ImageFolder(tmp_path)
    assert ds.classes == ["00000", "00001"] and ds.device.type == "cuda"
    order = [0, 2, 1, 3]                                   # class 0: images 0, 2; class 1: 1, 3
    batch, labels = ds.load(range(4), dev)
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.tolist() == [0, 0, 1, 1]
    assert batch.data.is_cuda and batch.sizes == [sizes[i] for i in order]
    tf = T.Compose([T.Resize((32, 32)), T.ToTensor(), T.Normalize(T.IMAGENET_MEAN, T.IMAGENET_STD)])
    y = tf(batch).cpu().numpy()
    assert y.shape == (4, 3, 32, 32) and y.dtype == np.float32
    for j, i in enumerate(order):
        ref = I.to_tensor_normalize(I.pil_resize_bilinear(imgs[i], 32, 32), T.IMAGENET_MEAN, T.IMAGENET_STD)
        assert np.array_equal(y[j], ref), (j, i)
    # read_ppm directly, Resize + ToTensor only (17:66), and Resize alone
    paths = [p for p, _ in ds.samples]
    batch2 = T.read_ppm(paths, dev, threads=2)
    y2 = T.Compose([T.Resize((32, 32)), T.ToTensor()])(batch2).cpu().numpy()
    y3 = T.Resize((32, 32))(batch2).cpu().numpy()
    for j, i in enumerate(order):
        ref = I.pil_resize_bilinear(imgs[i], 32, 32)
        assert np.array_equal(y2[j], I.to_tensor_normalize(ref)) and np.array_equal(y3[j], ref)
    with pytest.raises(TypeError):
        T.Compose([T.ToTensor()])(batch2)


def _packed(imgs, nbytes, max_hw, dev):
    """a RaggedBatch over a buffer of nbytes with the images back to back"""
    from roadrestore import imgproc
    buf = np.zeros(nbytes, np.uint8)
    recs, off = [], 0
    for im in imgs:
        buf[off:off + im.size] = im.reshape(-1)
        recs.append((off, im.shape[0], im.shape[1]))
        off += im.size
    return imgproc.RaggedBatch(torch.from_numpy(buf).to(dev), recs, 3, max_hw=max_hw)


def test_ragged_resize_is_graph_capturable(dev):
    """capture one resize; replay after overwriting data and table in place
    with another batch of the same n and max_hw: the table is read on the
    device, the host holds nothing per image"""
    sa, sb = [(25, 25), (40, 30), (10, 50)], [(50, 10), (33, 33), (40, 50)]
    ia, ib = _images(sa, seed=21), _images(sb, seed=22)
    nbytes = max(sum(im.size for im in ia), sum(im.size for im in ib))
    a, b = _packed(ia, nbytes, (50, 50), dev), _packed(ib, nbytes, (50, 50), dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.resize(32, 32, out="f32", mean=MEAN, std=STD)                  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g):
        out = a.resize(32, 32, out="f32", mean=MEAN, std=STD)
    for imgs, sizes, seed, src in ((ia, sa, 21, None), (ib, sb, 22, b), (ia, sa, 21, _packed(ia, nbytes, (50, 50), dev))):
        if src is not None:
            a.data.copy_(src.data)
            a.table.copy_(src.table)
        out.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        y = out.cpu().numpy()
        ref = _resized(sizes, 3, seed, 32, 32)
        for i in range(3):
            assert np.array_equal(y[i], I.to_tensor_normalize(ref[i], MEAN, STD)), (seed, i)
