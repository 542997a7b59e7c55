"""GPU parity of the ragged distortion (rr_distort_ragged_u8 and its random
variant: images of unequal size distorted at native size, the blur input kept
on chip) against the CPU oracle's per-image restatement of 14:31-64 / 16:14-37
(oracle/imgproc_cpu.py) and against the dense op.  Everything is compared byte
for byte: the arithmetic is the dense kernels' own device functions.

The sizes are the smallest at which the tile kernel can go wrong: images
smaller than any blur kernel (several reflections), sides one pixel either
side of each tile side the library can be told to use (16, 32, 64), more than
two tiles along an axis."""
import random

import numpy as np
import pytest
import torch

from oracle import imgproc_cpu as I
from rrpath import set_path  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 5), (14, 15), (15, 14), (17, 16), (31, 33), (33, 31),
         (33, 64), (64, 64), (70, 37), (63, 65), (65, 63), (16, 17), (32, 32)]
BLURS = [(5, 0), (6, 45), (15, 137), (15, 90)]           # (degree, angle); 6: even side, anchor k / 2
SENTINEL = 0xA5
A_FOG = 0.9

_CACHE = {}


def _images(sizes, c=3, seed=0):
    key = ("img", tuple(sizes), c, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        _CACHE[key] = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]
    return _CACHE[key]


def _taps(degree, angle):
    from roadrestore import ops
    key = ("taps", degree, angle)
    if key not in _CACHE:
        _CACHE[key] = ops.motion_blur_kernel(degree, angle)
    return _CACHE[key]


def _case(sizes, c, rot, seed=0):
    """Images with parameters cycled over all 8 flag combinations (image i in
    rotation ``rot`` has flags (i + 4 rot) % 8, so two rotations blur every
    image once), an fp64 noise field per image, and the oracle's results --
    computed once, shared, read-only."""
    from roadrestore._lib import DistortParam
    key = ("case", tuple(sizes), c, rot, seed)
    if key in _CACHE:
        return _CACHE[key]
    imgs = _images(sizes, c, seed)
    rng = random.Random(100 * seed + rot)
    nrng = np.random.default_rng(1000 + 10 * seed + rot)
    params, taps, noise, ref, kinds = [], [], [], [], set()
    for i, im in enumerate(imgs):
        flags = (i + 4 * rot) % 8
        t = 1.0 - rng.uniform(0.3, 0.7) * rng.uniform(0.8, 1.2)
        sigma = rng.uniform(0.01, 0.03) ** 0.5
        deg, ang = BLURS[(i + rot) % 4]
        nz = nrng.normal(0, 1, im.shape) * sigma
        p = DistortParam(0.0, 1.0, 0.0, flags, 0)
        kw = {}
        if flags & 1:
            p.fog_mul, p.fog_add = t, A_FOG * (1 - t)
            kw["fog_t"] = t
        if flags & 2:
            p.sigma = sigma
            kw["noise"] = nz
        if flags & 4:
            p.ksize = deg
            kw["blur"] = (deg, ang)
        params.append(p)
        taps.append(_taps(deg, ang) if flags & 4 else torch.zeros(15, 15))
        noise.append(nz)
        r = I.distort(im, **kw)
        r.setflags(write=False)
        ref.append(r)
        kinds.add(flags)
    _CACHE[key] = (imgs, params, torch.stack(taps), noise, ref, kinds)
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


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("c", [3, 1, 4])
def test_mode0_matches_oracle_given_noise(dev, c, rot):
    """14:31-64 per image at native size, explicit fp64 noise in packed order"""
    from roadrestore import ops
    imgs, params, taps, noise, ref, kinds = _case(SIZES, c, rot)
    assert len(kinds) == 8                                   # every flag combination occurs
    buf, recs, _ = _layout(imgs)
    field = torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise]))
    y = ops.distort_ragged_u8(torch.from_numpy(buf).to(dev), _table(recs, dev), _max_hw(imgs), c, params,
                              taps, mode=0, noise=field).cpu().numpy()
    for i, got in enumerate(_unpack(y, recs, c)):
        assert np.array_equal(got, ref[i]), (i, SIZES[i], params[i].flags, params[i].ksize)


@pytest.mark.parametrize("degree,angle", [(10, 45), (15, 137)])
def test_mode1_matches_compound(dev, degree, angle):
    """16:14-37 (blur -> fog -> noise) per image at native size"""
    from roadrestore import ops
    from roadrestore._lib import DistortParam
    c = 3
    imgs = _images(SIZES, c, seed=3)
    t, sigma = 1.0 - 0.5, 0.02 ** 0.5
    nrng = np.random.default_rng(31 + degree)
    noise = [nrng.normal(0, sigma, im.shape) for im in imgs]
    p = DistortParam(sigma, t, A_FOG * (1 - t), 7, degree)
    taps = _taps(degree, angle).unsqueeze(0).expand(len(imgs), -1, -1).contiguous()
    buf, recs, _ = _layout(imgs)
    field = torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise]))
    y = ops.distort_ragged_u8(torch.from_numpy(buf).to(dev), _table(recs, dev), _max_hw(imgs), c,
                              [p] * len(imgs), taps, mode=1, noise=field).cpu().numpy()
    for i, got in enumerate(_unpack(y, recs, c)):
        assert np.array_equal(got, I.compound(imgs[i], noise[i], degree, angle)), (i, SIZES[i])


def test_compound_entry_point_on_a_ragged_batch(dev):
    from roadrestore import imgproc
    imgs = _images([(5, 5), (33, 31), (40, 70)], 3, seed=4)
    nrng = np.random.default_rng(41)
    noise = [nrng.normal(0, 0.02 ** 0.5, im.shape) for im in imgs]
    b = imgproc.RaggedBatch.from_arrays(imgs, dev)
    y = imgproc.apply_compound_distortion(
        b, noise=torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise])))
    assert isinstance(y, imgproc.RaggedBatch) and y.table is b.table and y.max_hw == b.max_hw
    assert y.records is b.records and y.data.data_ptr() != b.data.data_ptr()
    for i, got in enumerate(_unpack(y.data.cpu().numpy(), [tuple(r) for r in b.records], 3)):
        assert np.array_equal(got, I.compound(imgs[i], noise[i]))


def _mixed_params(n, seed):
    from roadrestore._lib import DistortParam
    rng = random.Random(seed)
    params, taps = [], []
    for i in range(n):
        flags = (i * 3 + 1) % 8
        t = 1.0 - rng.uniform(0.3, 0.7) * rng.uniform(0.8, 1.2)
        deg, ang = BLURS[i % 4]
        params.append(DistortParam(rng.uniform(0.01, 0.03) ** 0.5 if flags & 2 else 0.0,
                                   t if flags & 1 else 1.0, A_FOG * (1 - t) if flags & 1 else 0.0, flags,
                                   deg if flags & 4 else 0))
        taps.append(_taps(deg, ang) if flags & 4 else torch.zeros(15, 15))
    return params, torch.stack(taps)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h,w", [(64, 64), (31, 33)])
def test_uniform_ragged_batch_equals_dense_op(dev, h, w, mode, monkeypatch):
    """images of one size back to back: the dense op's element indices, so the
    Philox noise and every byte agree with rr_distort_u8"""
    from roadrestore import ops
    n, c, seed = 6, 3, 0xC0FFEE1234
    imgs = _images([(h, w)] * n, c, seed=5)
    params, taps = _mixed_params(n, 50 + mode)
    assert len({p.flags for p in params}) >= 6
    buf, recs, _ = _layout(imgs)
    data = torch.from_numpy(buf).to(dev)
    y = ops.distort_ragged_u8(data, _table(recs, dev), (h, w), c, params, taps, mode=mode, seed=seed)
    x = data.view(n, h, w, c)
    want = ops.distort_u8(x, params, taps, mode=mode, seed=seed)
    assert torch.equal(y.view(n, h, w, c), want)
    if (h, w) == (64, 64):                                  # the dense per-pixel blur as well
        set_path(monkeypatch, "blur_tiled", "0")
        assert torch.equal(y.view(n, h, w, c), ops.distort_u8(x, params, taps, mode=mode, seed=seed))


@pytest.mark.parametrize("c", [3, 1])
def test_noise_key_is_the_packed_element_index(dev, c):
    """noise only, one sigma: whatever gaps the buffer holds, image i's noise
    is the dense op's on the same bytes packed as one [1, 1, sum h w, c] image"""
    from roadrestore import ops
    from roadrestore._lib import RR_DISTORT_NOISE, DistortParam
    sizes = [(7, 1), (33, 31), (1, 1), (40, 70), (16, 17)]
    imgs = _images(sizes, c, seed=6)
    buf, recs, _ = _layout(imgs, gaps=[13, 0, 1, 40, 7], tail=9)
    p = DistortParam(0.15, 1.0, 0.0, RR_DISTORT_NOISE, 0)
    seed = 987654321
    y = ops.distort_ragged_u8(torch.from_numpy(buf).to(dev), _table(recs, dev), _max_hw(imgs), c,
                              [p] * len(imgs), torch.zeros(len(imgs), 15, 15), seed=seed).cpu().numpy()
    packed = np.concatenate([im.reshape(-1) for im in imgs])
    want = ops.distort_u8(torch.from_numpy(packed).to(dev).view(1, 1, -1, c), [p], torch.zeros(1, 15, 15),
                          seed=seed).cpu().numpy().reshape(-1)
    assert np.array_equal(np.concatenate([g.reshape(-1) for g in _unpack(y, recs, c)]), want)
    assert not np.array_equal(want, packed)


def test_layout_and_containment(dev):
    """images in another order than the table, gaps and a tail: every image
    right, no byte of out outside the images written, in unchanged"""
    from roadrestore import ops
    c = 3
    imgs, params, taps, noise, ref, _ = _case(SIZES, c, 1)
    n = len(imgs)
    order = list(np.random.default_rng(8).permutation(n))
    assert order != sorted(order)
    gaps = [int(g) for g in np.random.default_rng(9).integers(0, 41, n)]
    buf, recs, mask = _layout(imgs, order=order, gaps=gaps, head=5, tail=64)
    data = torch.from_numpy(buf).to(dev)
    out = torch.full_like(data, SENTINEL)
    field = torch.from_numpy(np.concatenate([z.reshape(-1) for z in noise]))      # table order
    got = ops.distort_ragged_u8(data, _table(recs, dev), _max_hw(imgs), c, params, taps, mode=0,
                                noise=field, out=out)
    assert got is out
    y = out.cpu().numpy()
    for i, g in enumerate(_unpack(y, recs, c)):
        assert np.array_equal(g, ref[i]), (i, SIZES[i])
    assert (~mask).sum() >= 64 + 5 and np.all(y[~mask] == SENTINEL)
    assert np.array_equal(data.cpu().numpy(), buf)


def test_invalid_records_are_skipped(dev):
    """a record taller than max_h, one past the buffer, one with ksize 16 and
    the blur flag: nothing written for them, the others right, status OK"""
    from roadrestore import ops
    from roadrestore._lib import RR_DISTORT_BLUR, DistortParam
    c = 3
    sizes = [(33, 31), (40, 20), (5, 5), (17, 16), (9, 30), (31, 33)]
    imgs, params, taps, noise, ref, _ = _case(sizes, c, 1, seed=2)
    params = [DistortParam(p.sigma, p.fog_mul, p.fog_add, p.flags, p.ksize) for p in params]
    buf, recs, mask = _layout(imgs, gaps=[3] * len(imgs), tail=32)
    max_hw = (33, 33)
    assert sizes[1][0] > max_hw[0]                           # record 1: h > max_h
    recs[2] = (len(buf) - 5 * 5 * c + 1, 5, 5)               # record 2: ends one byte past the buffer
    params[4].flags |= RR_DISTORT_BLUR                       # record 4: a 16-tap side
    params[4].ksize = 16
    bad = {1, 2, 4}
    data = torch.from_numpy(buf).to(dev)
    out = torch.full_like(data, SENTINEL)
    field = torch.from_numpy(np.concatenate([noise[i].reshape(-1) for i in range(len(imgs)) if i not in bad]))
    ops.distort_ragged_u8(data, _table(recs, dev), max_hw, c, params, taps, mode=0, noise=field, out=out)
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    written = np.zeros(len(buf), bool)
    for i, (o, h, w) in enumerate(recs):
        if i in bad:
            continue
        assert np.array_equal(y[o:o + h * w * c].reshape(h, w, c), ref[i]), (i, sizes[i])
        written[o:o + h * w * c] = True
    assert np.all(y[~written] == SENTINEL)
    assert np.array_equal(data.cpu().numpy(), buf)


@pytest.mark.parametrize("tile", [16, 64])
def test_other_tile_shapes_agree(dev, tile, monkeypatch):
    """the library ships three tile shapes (RR_PATH rdist_tile=16 / 64 beside
    the default 32): the same bytes from each, Philox noise included"""
    from roadrestore import ops
    c = 3
    imgs, params, taps, _, _, _ = _case(SIZES, c, 1)
    buf, recs, _ = _layout(imgs, gaps=[2] * len(imgs))
    data, tab = torch.from_numpy(buf).to(dev), _table(recs, dev)
    for mode in (0, 1):
        outs = []
        for t in (32, tile):
            set_path(monkeypatch, "rdist_tile", str(t))
            out = torch.full_like(data, SENTINEL)
            outs.append(ops.distort_ragged_u8(data, tab, _max_hw(imgs), c, params, taps, mode=mode, seed=77,
                                              out=out))
        assert torch.equal(outs[0], outs[1]), mode


def _rebuilt(batch, rd, dev):
    """the eager result from a RandomDistortion's last draws"""
    from roadrestore import imgproc, ops
    params, idx, seed = rd.last_draws()
    table = imgproc.motion_blur_table(dev).view(-1, 15, 15)
    return ops.distort_ragged_u8(batch.data, batch.table, batch.max_hw, batch.channels, params,
                                 table[idx.to(dev).long()], mode=0, seed=seed), (params, idx, seed)


def test_device_draws_on_a_ragged_batch(dev):
    """image i of (seed, step) draws what the dense generator draws, whatever
    its size; the pixels are rr_distort_ragged_u8's given those draws"""
    from roadrestore import imgproc
    sizes = (SIZES * 2)[:32]
    imgs = _images(sizes, 3, seed=9)
    n = len(imgs)
    b = imgproc.RaggedBatch.from_arrays(imgs, dev)
    rd = imgproc.RandomDistortion(dev, seed=1234)
    dense = imgproc.RandomDistortion(dev, seed=1234)
    x8 = torch.zeros(n, 8, 8, 3, dtype=torch.uint8, device=dev)
    seen = []
    for step in (1, 2):
        y = rd(b)
        assert isinstance(y, imgproc.RaggedBatch) and y.table is b.table and y.sizes == b.sizes
        want, (p, idx, seed) = _rebuilt(b, rd, dev)
        assert rd.step.item() == step
        assert torch.equal(y.data[_mask(b, dev)], want[_mask(b, dev)])
        dense(x8)
        dp, didx, dseed = dense.last_draws()
        assert seed == dseed and torch.equal(idx, didx)
        assert [bytes(q) for q in p] == [bytes(q) for q in dp]
        seen.append(([bytes(q) for q in p], seed, y.data.clone()))
    assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]
    assert not torch.equal(seen[0][2], seen[1][2])
    assert len({q.flags for q in rd.last_draws()[0]}) >= 4


def _mask(batch, dev):
    m = np.zeros(batch.data.numel(), bool)
    for (o, h, w) in [tuple(r) for r in batch.records]:
        m[o:o + h * w * batch.channels] = True
    return torch.from_numpy(m).to(dev)


def _packed(imgs, nbytes, max_hw, dev):
    from roadrestore import imgproc
    buf, recs, _ = _layout(imgs, tail=nbytes - sum(im.size for im in imgs))
    return imgproc.RaggedBatch(torch.from_numpy(buf).to(dev), recs, 3, max_hw=max_hw)


def test_ragged_distortion_is_graph_capturable(dev):
    """capture RandomDistortion + resize on one stream; every replay re-draws
    and equals the eager result rebuilt from its draws; after the table and
    the data are overwritten in place the replay follows the new table"""
    from roadrestore import ops
    sa, sb = [(25, 25), (40, 30), (10, 50), (33, 31)], [(50, 10), (33, 33), (40, 50), (7, 1)]
    ia, ib = _images(sa, seed=21), _images(sb, seed=22)
    nbytes = max(sum(im.size for im in ia), sum(im.size for im in ib))
    a, b = _packed(ia, nbytes, (50, 50), dev), _packed(ib, nbytes, (50, 50), dev)
    from roadrestore import imgproc
    rd = imgproc.RandomDistortion(dev, seed=7)
    mid = torch.full_like(a.data, SENTINEL)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rd(a, out=mid).resize(32, 32)                        # warm-up: workspace allocated
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(g):
        out = rd(a, out=mid).resize(32, 32)
    draws = []
    for k, src in enumerate((None, None, None, b)):
        if src is not None:
            a.data.copy_(src.data)
            a.table.copy_(src.table)
        out.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert rd.step.item() == 2 + k                      # the warm-up, then one per replay
        want, (p, idx, seed) = _rebuilt(a, rd, dev)
        want = ops.resize_ragged_u8(want, a.table, a.max_hw, 3, 32, 32)
        assert torch.equal(out, want), k
        draws.append(([bytes(q) for q in p], seed))
    assert len({d[1] for d in draws}) == 4
    # the last replay read the NEW table: it equals the other batch run eagerly with those draws
    want_b, _ = _rebuilt(b, rd, dev)
    assert torch.equal(out, ops.resize_ragged_u8(want_b, b.table, b.max_hw, 3, 32, 32))


def test_dataset_pairs_from_files(dev, tmp_path):
    """14:66-93: files -> (bad, clean), the distortion at native size before
    the resize, both through the reference's transform (14:202-205)"""
    from roadrestore import imgproc, ops
    sizes = {"00000/00000_00000.ppm": (30, 29), "00000/00000_00001.ppm": (33, 35),
             "00001/00003_00002.ppm": (64, 61), "00001/00000_00000.ppm": (25, 27),
             "00002/00001_00029.ppm": (90, 97), "00002/00001_00000.ppm": (41, 40),
             "00002/00000_00007.ppm": (1, 5)}
    for i, (rel, (h, w)) in enumerate(sizes.items()):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        px = np.random.default_rng(60 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
        p.write_bytes(b"P6\n# GTSRB-like\n%d %d\n255\n" % (w, h) + px.tobytes())
    tf = imgproc.Compose([imgproc.Resize((224, 224)), imgproc.ToTensor()])
    ds = imgproc.DynamicDistortionDataset(tmp_path, tf, device=dev, seed=3)
    files = sorted(tmp_path.glob('*/*.ppm'))
    assert ds.clean_files == files and len(ds) == 7
    bad, clean = ds.load(range(7))
    for t in (bad, clean):
        assert tuple(t.shape) == (7, 3, 224, 224) and t.dtype == torch.float32 and t.is_cuda
    src = imgproc.read_ppm(files, dev)
    want_clean = src.resize(224, 224, out="f32")
    assert torch.equal(clean, want_clean)
    params, idx, seed = ds.last_draws()
    table = imgproc.motion_blur_table(dev).view(-1, 15, 15)
    y = ops.distort_ragged_u8(src.data, src.table, src.max_hw, 3, params, table[idx.to(dev).long()], seed=seed)
    assert torch.equal(bad, ops.resize_ragged_u8(y, src.table, src.max_hw, 3, 224, 224, out="f32"))
    assert any(p.flags for p in params) and not torch.equal(bad, clean)
    got = list(ds.batches(4))
    assert [tuple(c_.shape) for _, c_ in got] == [(4, 3, 224, 224), (3, 3, 224, 224)]
    assert torch.equal(torch.cat([c_ for _, c_ in got]), want_clean)         # every file once, sorted order
    assert all(b_.shape == c_.shape and b_.dtype == torch.float32 for b_, c_ in got)
    # without a transform: two ragged batches under one table
    raw_bad, raw_clean = imgproc.DynamicDistortionDataset(tmp_path, device=dev, seed=3).load([0, 1])
    assert isinstance(raw_bad, imgproc.RaggedBatch) and raw_bad.table is raw_clean.table
    assert raw_bad.sizes == [(30, 29), (33, 35)]
