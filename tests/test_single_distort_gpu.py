"""GPU parity of the single distortions (rr_distort_single_ragged_u8: the
noise, blur and fog of 02_gen_noise / 03_gen_blur / 04_gen_fog and of 13:33-56,
ragged batches at native size) against the numpy restatement of the
reference's text (tests/single_distort_ref.py).  Everything is compared byte
for byte.

The sizes are the smallest at which the kernels can go wrong: images below the
12-tap kernel (several reflections), sides one pixel either side of the 32-pixel
tile, several tiles along an axis."""
import random

import numpy as np
import pytest
import torch

import single_distort_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (7, 1), (5, 5), (11, 13), (31, 33), (33, 31), (32, 32), (33, 65), (70, 37)]
NOISE, BLUR, FOG = 0, 1, 2
SENTINEL = 0xA5

_CACHE = {}


def _images(sizes, c=3, seed=0):
    key = ("img", tuple(sizes), c, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        _CACHE[key] = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]
    return _CACHE[key]


def _taps(degree, angle=45):
    from roadrestore import ops
    key = ("taps", degree, angle)
    if key not in _CACHE:
        _CACHE[key] = ops.motion_blur_kernel(degree, angle)
    return _CACHE[key]


def _blur_ref(sizes, c, seed, degree, stretch):
    """the restatement's blur of _images(sizes, c, seed): computed once, shared, read-only"""
    key = ("blur", tuple(sizes), c, seed, degree, stretch)
    if key not in _CACHE:
        out = [R.blur(im, degree, 45, stretch=stretch) for im in _images(sizes, c, seed)]
        for r in out:
            r.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _layout(imgs, order=None, gaps=None, head=0, tail=0):
    """one byte buffer holding the images in ``order`` with ``gaps[j]`` bytes in
    front of the j-th placed one -> (buffer, records in TABLE order, mask of
    the bytes that belong to an image)"""
    n = len(imgs)
    order = list(range(n)) if order is None else order
    gaps = [0] * n if gaps is None else gaps
    off, pos = [0] * n, head
    for j, i in enumerate(order):
        pos += gaps[j]
        off[i] = pos
        pos += imgs[i].size
    buf = np.random.default_rng(7).integers(0, 256, pos + tail, dtype=np.uint8)
    mask = np.zeros(pos + tail, bool)
    for i, im in enumerate(imgs):
        buf[off[i]:off[i] + im.size] = im.reshape(-1)
        mask[off[i]:off[i] + im.size] = True
    return buf, [(off[i], im.shape[0], im.shape[1]) for i, im in enumerate(imgs)], mask


def _table(recs, dev):
    from roadrestore import imgproc
    rec = np.asarray(recs, dtype=imgproc._RECORD).reshape(-1)
    return torch.from_numpy(rec.view(np.uint8).reshape(len(recs), 16).copy()).to(dev)


def _unpack(out, recs, c):
    return [out[o:o + h * w * c].reshape(h, w, c) for o, h, w in recs]


def _max_hw(imgs):
    return max(im.shape[0] for im in imgs), max(im.shape[1] for im in imgs)


def _P(a=0.0, b=0.0, ksize=0, stretch=0):
    from roadrestore._lib import SingleParam
    return SingleParam(a, b, ksize, stretch)


def _run(dev, imgs, kind, params, taps=None, noise=None, seed=0, max_hw=None, **lay):
    """the images packed back to back (or as ``lay`` says) through one call -> the per-image results"""
    from roadrestore import ops
    c = imgs[0].shape[2]
    buf, recs, _ = _layout(imgs, **lay)
    if noise is not None:
        noise = torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise]))
    y = ops.distort_single_ragged_u8(torch.from_numpy(buf).to(dev), _table(recs, dev), max_hw or _max_hw(imgs), c,
                                     kind, params, taps=taps, noise=noise, seed=seed).cpu().numpy()
    return _unpack(y, recs, c)


def _same_taps(degree, n):
    return _taps(degree).unsqueeze(0).expand(n, -1, -1).contiguous()


# ------------------------------------------------------------------ blur ----
@pytest.mark.parametrize("stretch", [1, 0])
@pytest.mark.parametrize("c", [3, 1, 4])
def test_blur_matches_restatement(dev, c, stretch):
    """03:17-30 (stretch) and 13:40-48's form at degree 12, angle 45"""
    imgs = _images(SIZES, c, seed=1)
    ref = _blur_ref(SIZES, c, 1, 12, bool(stretch))
    got = _run(dev, imgs, BLUR, [_P(ksize=12, stretch=stretch)] * len(imgs), taps=_same_taps(12, len(imgs)))
    for i, g in enumerate(got):
        assert np.array_equal(g, ref[i]), (i, SIZES[i])
    if stretch:                                              # an image spans 0..255, a flat one is black
        assert all((g.min(), g.max()) in ((0, 255), (0, 0)) for g in got)
        assert (got[0].max() == 0) == (c == 1)               # 1 x 1: the range is over the channels


def test_blur_extremes_in_different_tiles(dev):
    """a (33, 65) image, constant but for a dark patch in its first tile and a
    bright one in its last: the range spans tiles, so a stretch by one tile's
    own range differs"""
    img = np.full((33, 65, 3), 120, np.uint8)
    img[2:9, 3:10] = 10
    img[20:33, 50:65] = 250                                  # reaches the last tile, the one pixel (32, 64)
    plain = R.blur(img, 12, 45, stretch=False)
    tiles = [plain[y:y + 32, x:x + 32] for y in (0, 32) for x in (0, 32, 64)]
    assert plain.min() == tiles[0].min() < min(t.min() for t in tiles[1:])
    assert plain.max() == tiles[-1].max() > tiles[0].max()
    want = R.normalize(plain)
    assert not np.array_equal(want[:32, :32], R.normalize(tiles[0]))
    got = _run(dev, [img], BLUR, [_P(ksize=12, stretch=1)], taps=_same_taps(12, 1))[0]
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 255


def test_blur_flat_and_range_one(dev):
    """03:29 on a flat image gives zeros; a blurred range of 1 gives only 0 and 255"""
    flat = np.full((40, 35, 3), 77, np.uint8)
    step = np.full((40, 35, 3), 100, np.uint8)
    step[:, 17:] = 101
    plain = R.blur(step, 12, 45, stretch=False)
    assert int(plain.max()) - int(plain.min()) == 1
    got = _run(dev, [flat, step], BLUR, [_P(ksize=12, stretch=1)] * 2, taps=_same_taps(12, 2))
    assert not got[0].any()
    assert set(np.unique(got[1]).tolist()) == {0, 255}
    assert np.array_equal(got[1], R.normalize(plain))


def test_blur_ranges_are_per_image(dev):
    """stretch and ksize differ per image, neighbours have very different
    ranges: each image is the restatement of itself, and permuting the table
    permutes the results without changing a byte"""
    sizes = [(33, 65), (31, 33), (70, 37), (5, 5), (32, 32), (11, 13)]
    rng = np.random.default_rng(5)
    imgs = [rng.integers(lo, hi + 1, (h, w, 3), dtype=np.uint8)
            for (h, w), (lo, hi) in zip(sizes, [(100, 110), (0, 255), (200, 203), (0, 255), (7, 7), (30, 230)])]
    cfg = [(12, 1), (5, 0), (15, 1), (12, 1), (6, 1), (15, 0)]              # (ksize, stretch)
    params = [_P(ksize=k, stretch=s) for k, s in cfg]
    taps = torch.stack([_taps(k) for k, _ in cfg])
    want = [R.blur(im, k, 45, stretch=bool(s)) for im, (k, s) in zip(imgs, cfg)]
    got = _run(dev, imgs, BLUR, params, taps=taps)
    for i, g in enumerate(got):
        assert np.array_equal(g, want[i]), (i, sizes[i], cfg[i])
    perm = [3, 0, 5, 1, 4, 2]
    got_p = _run(dev, [imgs[i] for i in perm], BLUR, [params[i] for i in perm], taps=taps[perm])
    for j, i in enumerate(perm):
        assert np.array_equal(got_p[j], want[i]), (j, i)


# ----------------------------------------------------------------- noise ----
@pytest.mark.parametrize("low", [-1.0, 0.0])
def test_noise_explicit_field(dev, low):
    """02:18-26 (low -1: the wrap of the negatives) and 13:33-38 (low 0) on a
    field that puts x + nz below -1, inside (-1, -1/255), inside (-1/255, 0),
    at exactly 0, at exactly 1 and above 1"""
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((9, 8), (33, 31), (1, 7))]
    noise = [rng.normal(0, 0.02 ** 0.5, im.shape) for im in imgs]
    flat, nz = imgs[0].reshape(-1), noise[0].reshape(-1)
    flat[:8] = [0, 0, 0, 0, 255, 0, 255, 51]
    nz[:8] = [-1.5, -0.5, -0.002, 0.0, -1.0, 1.0, 0.0, 2.0]
    v = flat[:8] / 255 + nz[:8]
    assert v[0] < -1 and -1 < v[1] < -1 / 255 and -1 / 255 < v[2] < 0
    assert v[3] == 0 and v[4] == 0 and v[5] == 1 and v[6] == 1 and v[7] > 1
    want = [R.noise(im, z, low=low) for im, z in zip(imgs, noise)]
    if low < 0:
        assert want[0].reshape(-1)[:3].tolist() == [1, 129, 0]          # -255 -> 1, -127.5 -> 129, -0.51 -> 0
        assert sum(int(((im / 255 + z) < -1 / 255).sum()) for im, z in zip(imgs, noise)) > 20
    got = _run(dev, imgs, NOISE, [_P(0.02 ** 0.5, low)] * 3, noise=noise, gaps=[3, 0, 5], tail=4)
    for i, g in enumerate(got):
        assert np.array_equal(g, want[i]), i


def test_noise_philox_key_and_scale(dev):
    """the draw is keyed by (seed, packed element index): the same seed gives
    the same bytes whatever the buffer layout, another seed other bytes; the
    field has the sigma it is asked for"""
    sizes = [(7, 1), (33, 31), (1, 1), (40, 70), (5, 5)]
    imgs = _images(sizes, 3, seed=6)
    p = [_P(0.02 ** 0.5, -1.0)] * len(imgs)
    a = _run(dev, imgs, NOISE, p, seed=987654321)
    b = _run(dev, imgs, NOISE, p, seed=987654321, order=[3, 0, 4, 2, 1], gaps=[13, 0, 1, 40, 7], head=11, tail=9)
    other = _run(dev, imgs, NOISE, p, seed=987654322)
    for i in range(len(imgs)):
        assert np.array_equal(a[i], b[i]), i
    assert not np.array_equal(a[3], other[3]) and not np.array_equal(a[3], imgs[3])
    # flat 128: 12,288 samples, standard error of the estimate 0.64 %; under 0.1 % of them reach a clip
    sigma = 0.02 ** 0.5
    flat = np.full((64, 64, 3), 128, np.uint8)
    y = _run(dev, [flat], NOISE, [_P(sigma, -1.0)], seed=5)[0]
    d = (y.astype(np.float64) - 128) / 255
    assert ((y == 255) | (y == 0)).mean() < 1e-3
    assert abs(d.std(ddof=1) / sigma - 1) < 0.03
    assert abs(d.mean()) < 4 * sigma / 12288 ** 0.5 + 1 / 255            # four standard errors and one level of truncation


# ------------------------------------------------------------------- fog ----
def test_fog_all_levels(dev):
    """04:17-30 in fp64 on all 256 levels, t over drawn values, both clip ends
    of 04:25 and 13:54's fixed value"""
    from roadrestore import imgproc
    levels = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2).copy()
    levels[:, :, 1] = levels[::-1, ::-1, 0]
    ts = imgproc.fog_transmissions(12, 0.8, random.Random(3)) + [0.1, 0.9, 1.0 - 0.1]
    assert 0.1 in ts[:12] and any(t > 0.1 for t in ts[:12])
    imgs = [levels] * len(ts)
    got = _run(dev, imgs, FOG, [_P(t, R.A_FOG * (1 - t)) for t in ts])
    for t, g in zip(ts, got):
        assert np.array_equal(g, R.fog(levels, t)), t
    # the public entry point draws the same t from the same rng
    x = torch.from_numpy(np.stack(imgs[:12])).to(dev)
    y = imgproc.add_fog(x, 0.8, rng=random.Random(3))
    assert y.shape == x.shape and torch.equal(y.cpu(), torch.from_numpy(np.stack(got[:12])))
    y13 = imgproc.add_fog(x[:2], 0.1, jitter=False)
    assert np.array_equal(y13[1].cpu().numpy(), R.fog(levels, 0.9))


# ------------------------------------------------- layout and bad records ----
def _kind_case(kind, n):
    """(params, taps, explicit noise or None) of n images under ``kind``"""
    if kind == BLUR:
        return [_P(ksize=12, stretch=i % 2) for i in range(n)], _same_taps(12, n)
    if kind == FOG:
        return [_P(0.3 + 0.05 * i, R.A_FOG * (1 - (0.3 + 0.05 * i))) for i in range(n)], None
    return [_P(0.02 ** 0.5, -1.0)] * n, None


def _kind_ref(kind, imgs, params, noise, skip=()):
    """the restatement of every image but those in ``skip`` (None there)"""
    def one(im, p, z):
        if kind == BLUR:
            return R.blur(im, p.ksize, 45, stretch=bool(p.stretch))
        return R.fog(im, p.a) if kind == FOG else R.noise(im, z, low=p.b)
    return [None if i in skip else one(im, p, z) for i, (im, p, z) in enumerate(zip(imgs, params, noise))]


@pytest.mark.parametrize("kind", [NOISE, BLUR, FOG])
def test_layout_and_containment(dev, kind):
    """images in another order than the table, gaps, a head and a tail: every
    image right, no byte of out outside the images written, in unchanged"""
    from roadrestore import ops
    sizes = [(5, 5), (31, 33), (33, 65), (1, 7), (32, 32), (11, 13)]
    imgs = _images(sizes, 3, seed=8)
    n = len(imgs)
    params, taps = _kind_case(kind, n)
    noise = [np.random.default_rng(80 + i).normal(0, 0.02 ** 0.5, im.shape) for i, im in enumerate(imgs)]
    buf, recs, mask = _layout(imgs, order=[4, 1, 5, 0, 3, 2], gaps=[9, 0, 33, 1, 17, 4], head=5, tail=64)
    data = torch.from_numpy(buf).to(dev)
    out = torch.full_like(data, SENTINEL)
    field = torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise])) if kind == NOISE else None
    got = ops.distort_single_ragged_u8(data, _table(recs, dev), _max_hw(imgs), 3, kind, params, taps=taps,
                                       noise=field, out=out)
    assert got is out
    y = out.cpu().numpy()
    want = _kind_ref(kind, imgs, params, noise)
    for i, g in enumerate(_unpack(y, recs, 3)):
        assert np.array_equal(g, want[i]), (i, sizes[i])
    assert (~mask).sum() >= 64 + 5 and np.all(y[~mask] == SENTINEL)
    assert np.array_equal(data.cpu().numpy(), buf)


@pytest.mark.parametrize("kind", [NOISE, BLUR, FOG])
def test_invalid_records_are_skipped(dev, kind):
    """a record with h = 0, one whose offset lies past the buffer and, under
    the blur, one with ksize 16: their bytes keep the sentinel, the others are
    right, the element count skips them"""
    from roadrestore import ops
    sizes = [(33, 31), (9, 30), (5, 5), (17, 16), (12, 12), (31, 33)]
    imgs = _images(sizes, 3, seed=9)
    n = len(imgs)
    params, taps = _kind_case(kind, n)
    noise = [np.random.default_rng(90 + i).normal(0, 0.02 ** 0.5, im.shape) for i, im in enumerate(imgs)]
    buf, recs, _ = _layout(imgs, gaps=[3] * n, tail=32)
    recs[1] = (recs[1][0], 0, 30)                            # record 1: h = 0
    recs[2] = (len(buf) + 1, 5, 5)                           # record 2: starts past the buffer
    bad = {1, 2}
    if kind == BLUR:
        params = list(params)
        params[4] = _P(ksize=16, stretch=1)                  # record 4: a 16-tap side
        bad.add(4)
    data = torch.from_numpy(buf).to(dev)
    out = torch.full_like(data, SENTINEL)
    field = None
    if kind == NOISE:
        field = torch.from_numpy(np.concatenate([noise[i].reshape(-1) for i in range(n) if i not in bad]))
    ops.distort_single_ragged_u8(data, _table(recs, dev), (33, 33), 3, kind, params, taps=taps, noise=field, out=out)
    y = out.cpu().numpy()
    want = _kind_ref(kind, imgs, params, noise, skip=bad)
    written = np.zeros(len(buf), bool)
    for i, (o, h, w) in enumerate(recs):
        if i in bad:
            continue
        assert np.array_equal(y[o:o + h * w * 3].reshape(h, w, 3), want[i]), (i, sizes[i])
        written[o:o + h * w * 3] = True
    assert np.all(y[~written] == SENTINEL)
    assert np.array_equal(data.cpu().numpy(), buf)


# ------------------------------------------------- workspace and replays ----
def test_stale_workspace_is_never_read(dev):
    """one stretch call on large images, then the same workspace under smaller
    ones: the result is that of a zeroed workspace and of one filled with 0xFF"""
    from roadrestore import ops
    big = _images([(70, 65), (65, 70), (70, 70)], 3, seed=12)
    small = [np.random.default_rng(13).integers(90, 140, (h, w, 3), dtype=np.uint8)
             for h, w in ((33, 31), (20, 40), (5, 5))]
    max_hw, n = (70, 70), 3
    params, taps = [_P(ksize=12, stretch=1)] * n, _same_taps(12, n)
    ws = torch.empty(ops.single_workspace(n, 3, max_hw), dtype=torch.uint8, device=dev)

    def run(imgs, w):
        buf, recs, _ = _layout(imgs)
        y = ops.distort_single_ragged_u8(torch.from_numpy(buf).to(dev), _table(recs, dev), max_hw, 3, BLUR,
                                         params, taps=taps, ws=w)
        return _unpack(y.cpu().numpy(), recs, 3)
    run(big, ws)
    got = run(small, ws)
    zero, ones = run(small, torch.zeros_like(ws)), run(small, torch.full_like(ws, 0xFF))
    for i, im in enumerate(small):
        want = R.blur(im, 12, 45)
        assert np.array_equal(got[i], want) and np.array_equal(zero[i], want) and np.array_equal(ones[i], want), i


def test_stretch_call_is_graph_capturable(dev):
    """a captured stretch call, replayed after the input bytes were overwritten
    in place under the same table, matches the restatement of the new bytes"""
    from roadrestore import ops
    sizes = [(33, 65), (31, 33), (5, 5), (40, 40)]
    ia, ib = _images(sizes, 3, seed=21), _images(sizes, 3, seed=22)
    n = len(sizes)
    buf_a, recs, _ = _layout(ia, gaps=[2] * n)
    buf_b, _, _ = _layout(ib, gaps=[2] * n)
    data, tab = torch.from_numpy(buf_a).to(dev), _table(recs, dev)
    max_hw = _max_hw(ia)
    from roadrestore._lib import SingleParam
    prm = torch.frombuffer(bytearray((SingleParam * n)(*[_P(ksize=12, stretch=1)] * n)), dtype=torch.uint8)
    prm = prm.view(n, 24).to(dev)
    taps = _same_taps(12, n).to(dev)
    ws = torch.empty(ops.single_workspace(n, 3, max_hw), dtype=torch.uint8, device=dev)
    out = torch.full_like(data, SENTINEL)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.distort_single_ragged_u8(data, tab, max_hw, 3, BLUR, prm, taps=taps, ws=ws, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g):
        ops.distort_single_ragged_u8(data, tab, max_hw, 3, BLUR, prm, taps=taps, ws=ws, out=out)
    for imgs, buf in ((ia, buf_a), (ib, buf_b)):
        data.copy_(torch.from_numpy(buf))
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize(dev)
        for i, got in enumerate(_unpack(out.cpu().numpy(), recs, 3)):
            assert np.array_equal(got, R.blur(imgs[i], 12, 45)), i


# -------------------------------------------------------- public surface ----
def test_chain_of_13(dev):
    """13:33-56: blur(5, 45, no stretch) -> fog(0.1, fixed) -> noise(var 0.01, clipped at 0), three calls"""
    from roadrestore import imgproc
    imgs = _images([(5, 5), (33, 31), (40, 70)], 3, seed=4)
    noise = [np.random.default_rng(40 + i).normal(0, 0.01 ** 0.5, im.shape) for i, im in enumerate(imgs)]
    b = imgproc.RaggedBatch.from_arrays(imgs, dev)
    y = imgproc.apply_motion_blur(b, degree=5, angle=45, normalize=False)
    y = imgproc.add_fog(y, fog_intensity=0.1, jitter=False)
    y = imgproc.add_gaussian_noise(y, var=0.01, low_clip=0.0,
                                   noise=torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise])))
    assert isinstance(y, imgproc.RaggedBatch) and y.table is b.table and y.sizes == b.sizes
    for i, got in enumerate(_unpack(y.data.cpu().numpy(), [tuple(r) for r in b.records], 3)):
        assert np.array_equal(got, R.chain13(imgs[i], noise[i])), i


def test_dense_batch_goes_through_a_uniform_table(dev):
    from roadrestore import imgproc
    x = np.stack(_images([(31, 33)] * 3, 3, seed=14))
    y = imgproc.apply_motion_blur(torch.from_numpy(x).to(dev))            # 03's defaults: 10, 45, stretch
    assert y.shape == x.shape and y.dtype == torch.uint8
    for i in range(3):
        assert np.array_equal(y[i].cpu().numpy(), R.blur(x[i], 10, 45)), i
    a = imgproc.add_gaussian_noise(torch.from_numpy(x).to(dev), seed=3)
    assert torch.equal(a, imgproc.add_gaussian_noise(torch.from_numpy(x).to(dev), seed=3))
    assert not torch.equal(a, imgproc.add_gaussian_noise(torch.from_numpy(x).to(dev), seed=4))


def _tree(root):
    sizes = {"00000/00000_00000.ppm": (30, 29), "00000/00000_00001.ppm": (33, 35), "00001/00003_00002.ppm": (64, 61),
             "00001/00000_00000.ppm": (25, 27), "00002/00000_00007.ppm": (1, 5)}
    for i, (rel, (h, w)) in enumerate(sizes.items()):
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        px = np.random.default_rng(60 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        p.write_bytes(b"P6\n# GTSRB-like\n%d %d\n255\n" % (w, h) + px.tobytes())
    return sorted(root.glob('*/*.ppm'))


@pytest.mark.parametrize("task", ["Noise", "Blur", "Fog"])
def test_single_distortion_dataset(dev, tmp_path, task):
    """02-04's sets made on the fly: (bad, clean) in 07:72's order through 07's transform"""
    from roadrestore import imgproc
    files = _tree(tmp_path)
    tf = imgproc.Compose([imgproc.Resize((224, 224)), imgproc.ToTensor()])
    ds = imgproc.SingleDistortionDataset(tmp_path, task, tf, device=dev, seed=3)
    assert ds.clean_files == files and len(ds) == 5
    bad, clean = ds.load(range(5))
    for t in (bad, clean):
        assert tuple(t.shape) == (5, 3, 224, 224) and t.dtype == torch.float32 and t.is_cuda
    src = imgproc.read_ppm(files, dev)
    assert torch.equal(clean, tf(src))
    assert not torch.equal(bad, clean)
    if task == "Blur":
        host = src.data.cpu().numpy()
        want = [R.blur(host[o:o + h * w * 3].reshape(h, w, 3), 12, 45) for o, h, w in [tuple(r) for r in src.records]]
        assert torch.equal(bad, tf(imgproc.RaggedBatch.from_arrays(want, dev)))
    got = list(ds.batches(2))
    assert [tuple(c_.shape) for _, c_ in got] == [(2, 3, 224, 224), (2, 3, 224, 224), (1, 3, 224, 224)]
    assert torch.equal(torch.cat([c_ for _, c_ in got]), clean)
    raw_bad, raw_clean = imgproc.SingleDistortionDataset(tmp_path, task, device=dev).load([0, 1])
    assert isinstance(raw_bad, imgproc.RaggedBatch) and raw_bad.table is raw_clean.table


def test_written_set_reads_back_as_pairs(dev, tmp_path):
    """write_ppm -> read_ppm round-trips a ragged batch; PairedDataset over a
    set written where 03:43-46 writes it returns the written pairs"""
    from roadrestore import imgproc
    clean_root, blur_root = tmp_path / "Training", tmp_path / "processed" / "Blur"
    files = _tree(clean_root)
    clean = imgproc.read_ppm(files, dev)
    bad = imgproc.apply_motion_blur(clean, degree=12, angle=45)
    paths = [blur_root / f.relative_to(clean_root) for f in files]
    imgproc.write_ppm(bad, paths)
    back = imgproc.read_ppm(paths, dev)
    assert back.sizes == bad.sizes
    bh, yh = back.data.cpu().numpy(), bad.data.cpu().numpy()
    for rb, ry in zip(back.records, bad.records):
        nb = int(ry["h"]) * int(ry["w"]) * 3
        assert np.array_equal(bh[int(rb["offset"]):int(rb["offset"]) + nb], yh[int(ry["offset"]):int(ry["offset"]) + nb])
    paths[3].unlink()                                        # one file missing: that pair is dropped
    ds = imgproc.PairedDataset(clean_root, blur_root, device=dev)
    assert len(ds) == 4 and [c for _, c in ds.data_pairs] == files[:3] + files[4:]
    got_bad, got_clean = ds.load(range(4))
    keep = [0, 1, 2, 4]
    assert got_bad.sizes == [bad.sizes[i] for i in keep] == got_clean.sizes
    gb, gc, ch = got_bad.data.cpu().numpy(), got_clean.data.cpu().numpy(), clean.data.cpu().numpy()
    for j, i in enumerate(keep):
        nb = bad.sizes[i][0] * bad.sizes[i][1] * 3
        ob, oc = int(got_bad.records["offset"][j]), int(got_clean.records["offset"][j])
        assert np.array_equal(gb[ob:ob + nb], yh[int(bad.records["offset"][i]):int(bad.records["offset"][i]) + nb])
        assert np.array_equal(gc[oc:oc + nb], ch[int(clean.records["offset"][i]):int(clean.records["offset"][i]) + nb])
    tf = imgproc.Compose([imgproc.Resize((224, 224)), imgproc.ToTensor()])
    tb, tc = next(imgproc.PairedDataset(clean_root, blur_root, tf, device=dev).batches(3))
    assert tuple(tb.shape) == tuple(tc.shape) == (3, 3, 224, 224)
