"""GPU parity of the ragged cv2.resize (rr_cv_resize_ragged_u8) and of the
fused evaluation (rr_eval_ragged_u8: PSNR and SSIM of every resized clean image
against a restored batch, 08:118-125) against the CPU oracle
(oracle/imgproc_cpu.py: cv_resize_linear, ssim) and against the dense ops.

The resize is compared bit for bit.  PSNR is compared bit for bit with the
dense route (ragged resize, then rr_psnr_u8): the squared error is an exact
integer and the closing expression the same, so a pixel counted twice or
missed by the tile ownership shows there.  SSIM is held to 1e-10 of the
oracle, the bound rr_ssim_u8 is held to: the window sums are exact integers,
one S term's fp64 error is about ulp(65025) / C2 = 2.5e-13 relative, and the
mean of at most 47,524 terms of magnitude at most 1 adds at most about 1e-11;
a window dropped or counted twice moves the mean by far more on noisy images.

The target sizes are the smallest at which the tiling can go wrong: one
window, one window row, and the sizes at, one below and one above T + 6 for
both tile sides the kernel may be built with (16 and 32)."""
import numpy as np
import pytest
import torch

from oracle import imgproc_cpu as I

pytestmark = pytest.mark.gpu

# a one-pixel image first in the buffer, a two-row and a 15-column image (both
# axes clamp), up- and downscales, the same-size image of the (32, 32) target
SIZES = [(1, 1), (2, 250), (250, 15), (25, 25), (32, 32), (31, 33), (41, 47), (243, 225)]
# the six clean images of the fused runs; 2: restored = the resized clean image,
# 3: clean and restored all 255, 4: clean all 0, restored all 255
EVAL_SIZES = [(1, 1), (2, 250), (250, 15), (25, 25), (31, 33), (243, 225)]
EVAL_TARGETS = [(7, 7), (7, 40), (22, 23), (21, 39), (38, 37), (39, 70)]

_CACHE = {}


def _images(sizes, c=3, seed=0):
    key = ("img", tuple(sizes), c, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        _CACHE[key] = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]
    return _CACHE[key]


def _cv_ref(sizes, c, seed, oh, ow):
    """the oracle's per-image cv2.resize results, computed once (read-only)"""
    key = ("cv", tuple(sizes), c, seed, oh, ow)
    if key not in _CACHE:
        ref = [I.cv_resize_linear(im, oh, ow) for im in _images(sizes, c, seed)]
        for r in ref:
            r.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _eval_case(oh, ow, c=3, sizes=EVAL_SIZES, seed=3, special=True):
    """clean images, the oracle's resized clean images, restored = clip(ref +
    integers(-30, 31)), and the oracle's PSNR / SSIM per image; computed once"""
    key = ("eval", oh, ow, c, tuple(sizes), seed, special)
    if key not in _CACHE:
        rng = np.random.default_rng(seed + 1000 * oh + ow)
        clean = [im.copy() for im in _images(sizes, c, seed)]
        if special:
            clean[3][:] = 255
            clean[4][:] = 0
        ref = [I.cv_resize_linear(im, oh, ow) for im in clean]
        rst = [np.clip(r.astype(np.int64) + rng.integers(-30, 31, r.shape), 0, 255).astype(np.uint8) for r in ref]
        if special:
            rst[2] = ref[2].copy()
            rst[3][:] = 255
            rst[4][:] = 255
        mse = [np.mean((r.astype(np.float64) - s.astype(np.float64)) ** 2) for r, s in zip(ref, rst)]
        psnr = np.array([np.inf if m == 0 else 10.0 * np.log10(255.0 ** 2 / m) for m in mse])
        ssim = np.array([I.ssim(r, s) for r, s in zip(ref, rst)])
        for a in clean + ref + rst + [psnr, ssim]:
            a.setflags(write=False)
        _CACHE[key] = (clean, ref, np.stack(rst), psnr, ssim)
    return _CACHE[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _check_against_oracle(psnr, ssim, want_psnr, want_ssim):
    psnr, ssim = psnr.cpu().numpy(), ssim.cpu().numpy()
    print("psnr", psnr, "oracle", want_psnr, "\nssim", ssim, "oracle", want_ssim,
          "max|d ssim|", np.abs(ssim - want_ssim).max())
    fin = np.isfinite(want_psnr)
    assert np.array_equal(np.isposinf(psnr), ~fin)
    assert np.abs(psnr[fin] - want_psnr[fin]).max() < 1e-9
    assert np.abs(ssim - want_ssim).max() < 1e-10


# ----------------------------------------------------------- 1. the resize ----
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("oh,ow", [(32, 32), (24, 40)])
def test_ragged_cv_resize_matches_oracle_per_image(dev, oh, ow, c):
    """(32, 32): the (32, 32) image is the copy case; (24, 40): ow * c = 120
    leaves an 8-element scalar tail at c = 3"""
    from roadrestore import imgproc
    batch = imgproc.RaggedBatch.from_arrays(_images(SIZES, c), dev)
    y = batch.cv_resize((ow, oh))
    assert y.shape == (len(SIZES), oh, ow, c) and y.dtype == torch.uint8 and y.is_cuda
    y = y.cpu().numpy()
    ref = _cv_ref(SIZES, c, 0, oh, ow)
    for i, size in enumerate(SIZES):
        assert np.array_equal(y[i], ref[i]), (i, size)
    if (oh, ow) == (32, 32):
        assert np.array_equal(y[4], _images(SIZES, c)[4])
    assert torch.equal(imgproc.cv_resize(batch, (ow, oh)).cpu(), torch.from_numpy(y))


def test_ragged_cv_resize_all_scalar_row(dev):
    """a 4-element row: shorter than half a vector, every element on the
    22-bit scalar path"""
    from roadrestore import imgproc
    batch = imgproc.RaggedBatch.from_arrays(_images(SIZES, 1), dev)
    y = batch.cv_resize((4, 5)).cpu().numpy()
    ref = _cv_ref(SIZES, 1, 0, 5, 4)
    for i, size in enumerate(SIZES):
        assert np.array_equal(y[i], ref[i]), (i, size)


def test_ragged_cv_resize_to_the_reference_target(dev):
    """08:119: (224, 224), an upscale and a downscale in one batch"""
    from roadrestore import imgproc
    sizes = [(25, 25), (243, 225)]
    batch = imgproc.RaggedBatch.from_arrays(_images(sizes, 3, seed=5), dev)
    y = batch.cv_resize((224, 224)).cpu().numpy()
    ref = _cv_ref(sizes, 3, 5, 224, 224)
    for i in range(2):
        assert np.array_equal(y[i], ref[i]), i


# ------------------------------------------------ 2. uniform batch = dense ----
@pytest.mark.parametrize("oh,ow", [(47, 33), (31, 33)])
def test_uniform_ragged_batch_equals_dense_cv_resize(dev, oh, ow):
    """five (31, 33) images: byte for byte the dense op on the stacked tensor,
    also at the same size, where both copy"""
    from roadrestore import imgproc
    imgs = _images([(31, 33)] * 5, seed=7)
    batch = imgproc.RaggedBatch.from_arrays(imgs, dev)
    dense = torch.from_numpy(np.stack(imgs)).to(dev)
    assert torch.equal(batch.cv_resize((ow, oh)), imgproc.cv_resize(dense, (ow, oh)))
    if (oh, ow) == (31, 33):
        assert torch.equal(batch.cv_resize((ow, oh)), dense)


# ------------------------------------------------ 3. bad records and bounds ----
BAD = 2                                     # the record overwritten with h = 0


def test_ragged_cv_resize_bad_record_and_guard_bands(dev):
    from roadrestore import imgproc, ops
    oh, ow, c, band = 24, 40, 3, 4096
    batch = imgproc.RaggedBatch.from_arrays(_images(SIZES, c), dev)
    batch.table[BAD, 8:12] = 0                                        # h = 0, in place on the device
    n, per = len(SIZES), oh * ow * c
    buf = torch.full((band + n * per + band,), 0xA5, dtype=torch.uint8, device=dev)
    L = ops.lib()
    L.check(L.rr_cv_resize_ragged_u8(n, c, batch.max_hw[0], batch.max_hw[1], oh, ow, batch.data.data_ptr(),
                                     batch.data.numel(), batch.table.data_ptr(), buf.data_ptr() + band, 0,
                                     ops.stream()), "rr_cv_resize_ragged_u8")
    torch.cuda.synchronize(dev)
    host = buf.cpu().numpy()
    assert np.all(host[:band] == 0xA5) and np.all(host[band + n * per:] == 0xA5)
    y = host[band:band + n * per].reshape(n, oh, ow, c)
    ref = _cv_ref(SIZES, c, 0, oh, ow)
    for i, size in enumerate(SIZES):
        if i == BAD:
            assert not y[i].any()
        else:
            assert np.array_equal(y[i], ref[i]), (i, size)


def test_fused_eval_bad_record_is_nan_and_leaves_the_rest(dev):
    from roadrestore import imgproc
    oh, ow = 38, 37
    clean, _, rst, _, _ = _eval_case(oh, ow)
    restored = torch.from_numpy(rst).to(dev)
    batch = imgproc.RaggedBatch.from_arrays(clean, dev)
    p0, s0 = imgproc.restoration_quality(batch, restored)
    batch.table[BAD, 8:12] = 0
    p1, s1 = imgproc.restoration_quality(batch, restored)
    torch.cuda.synchronize(dev)
    assert torch.isnan(p1[BAD]) and torch.isnan(s1[BAD])
    keep = [i for i in range(len(clean)) if i != BAD]
    assert torch.equal(_bits(p0)[keep], _bits(p1)[keep]) and torch.equal(_bits(s0)[keep], _bits(s1)[keep])
    assert not torch.isnan(p0).any() and not torch.isnan(s0).any()


# ----------------------------------------- 4. fused metrics against the oracle ----
def _fused_and_checks(dev, oh, ow, c, sizes, special):
    from roadrestore import imgproc
    clean, ref, rst, want_psnr, want_ssim = _eval_case(oh, ow, c, sizes, special=special)
    batch = imgproc.RaggedBatch.from_arrays(clean, dev)
    restored = torch.from_numpy(rst).to(dev)
    psnr, ssim = imgproc.restoration_quality(batch, restored)
    assert psnr.shape == ssim.shape == (len(clean),) and psnr.dtype == ssim.dtype == torch.float64
    resized = batch.cv_resize((ow, oh))
    assert torch.equal(resized.cpu(), torch.from_numpy(np.stack(ref)))
    # the exact integer squared error, the same closing expression: bit for bit
    assert torch.equal(_bits(psnr), _bits(imgproc.psnr(resized, restored)))
    _check_against_oracle(psnr, ssim, want_psnr, want_ssim)
    return psnr.cpu().numpy(), ssim.cpu().numpy()


@pytest.mark.parametrize("oh,ow", EVAL_TARGETS)
def test_fused_eval_matches_oracle(dev, oh, ow):
    psnr, ssim = _fused_and_checks(dev, oh, ow, 3, EVAL_SIZES, True)
    assert np.isposinf(psnr[2]) and psnr[4] == 0.0
    assert abs(ssim[2] - 1.0) < 1e-12 and abs(ssim[3] - 1.0) < 1e-12


def test_fused_eval_one_channel(dev):
    psnr, ssim = _fused_and_checks(dev, 22, 23, 1, EVAL_SIZES, True)
    assert np.isposinf(psnr[2]) and psnr[4] == 0.0
    assert abs(ssim[2] - 1.0) < 1e-12 and abs(ssim[3] - 1.0) < 1e-12


def test_fused_eval_at_the_reference_target(dev):
    _fused_and_checks(dev, 224, 224, 3, [(25, 25), (243, 225)], False)


def test_restoration_quality_dense_and_mismatches(dev):
    """a dense clean batch goes through psnr and ssim; counts that differ raise"""
    from roadrestore import imgproc
    clean, ref, rst, _, _ = _eval_case(22, 23)
    restored = torch.from_numpy(rst).to(dev)
    dense = torch.from_numpy(np.stack(ref)).to(dev)
    p, s = imgproc.restoration_quality(dense, restored)
    assert torch.equal(_bits(p), _bits(imgproc.psnr(dense, restored)))
    assert torch.equal(_bits(s), _bits(imgproc.ssim(dense, restored)))
    batch = imgproc.RaggedBatch.from_arrays(clean, dev)
    with pytest.raises(ValueError):
        imgproc.restoration_quality(batch, restored[:5])
    with pytest.raises(ValueError):
        imgproc.restoration_quality(batch, restored[..., :2])
    with pytest.raises(ValueError):
        imgproc.restoration_quality(batch, restored[:, :6])           # oh = 6 < win_size
    with pytest.raises(TypeError):
        imgproc.restoration_quality(dense[:, :20], restored)


# ------------------------------------------------------------ 5. determinism ----
def test_fused_eval_is_deterministic(dev):
    from roadrestore import imgproc
    clean, _, rst, _, _ = _eval_case(39, 70)
    batch = imgproc.RaggedBatch.from_arrays(clean, dev)
    restored = torch.from_numpy(rst).to(dev)
    p0, s0 = imgproc.restoration_quality(batch, restored)
    p1, s1 = imgproc.restoration_quality(batch, restored)
    assert torch.equal(_bits(p0), _bits(p1)) and torch.equal(_bits(s0), _bits(s1))


# ------------------------------------------------------------ 6. graph replay ----
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


def test_restoration_quality_is_graph_capturable(dev):
    """capture one call; replay after overwriting data, table and restored in
    place with another batch of the same n and max_hw: the table is read on the
    device, the host holds nothing per image"""
    from roadrestore import imgproc
    oh, ow = 38, 37
    sa, sb = [(25, 25), (40, 30), (10, 50)], [(50, 10), (33, 33), (40, 50)]
    ia, ib = _images(sa, seed=21), _images(sb, seed=22)
    rng = np.random.default_rng(23)
    ra, rb = (torch.from_numpy(rng.integers(0, 256, (3, oh, ow, 3), dtype=np.uint8)).to(dev) for _ in range(2))
    nbytes = max(sum(im.size for im in ia), sum(im.size for im in ib))
    a, b = _packed(ia, nbytes, (50, 50), dev), _packed(ib, nbytes, (50, 50), dev)
    want_p, want_s = imgproc.restoration_quality(b, rb)               # eager, the second batch
    restored = ra.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        imgproc.restoration_quality(a, restored)                      # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g):
        psnr, ssim = imgproc.restoration_quality(a, restored)
    a.data.copy_(b.data)
    a.table.copy_(b.table)
    restored.copy_(rb)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(_bits(psnr), _bits(want_p)) and torch.equal(_bits(ssim), _bits(want_s))
    assert torch.isfinite(psnr).all() and torch.isfinite(ssim).all()


# ------------------------------------------------------- 7. through the files ----
def test_files_to_restoration_quality(dev, tmp_path):
    """08:84-125 without the network: PPM files of unequal size -> read_ppm ->
    restoration_quality against a (224, 224) restored batch"""
    from roadrestore import imgproc as T
    sizes = [(15, 17), (40, 32), (32, 61), (7, 90)]
    clean, ref, rst, want_psnr, want_ssim = _eval_case(224, 224, 3, sizes, seed=11, special=False)
    paths = []
    for i, im in enumerate(clean):
        hdr = b"P6\n# sign %d\n%d %d\n255\n" % (i, im.shape[1], im.shape[0])
        paths.append(tmp_path / f"{i}.ppm")
        paths[-1].write_bytes(hdr + im.tobytes())
    batch = T.read_ppm(paths, dev, threads=2)
    assert batch.sizes == sizes
    psnr, ssim = T.restoration_quality(batch, torch.from_numpy(rst).to(dev))
    _check_against_oracle(psnr, ssim, want_psnr, want_ssim)
