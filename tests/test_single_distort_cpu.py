"""CPU: the host side of the single distortions (rr_distort_single_ragged_u8:
02_gen_noise / 03_gen_blur / 04_gen_fog and 13:33-56 in their own spelling):
the restatement against the reference's literal noise text, add_fog's draws,
PairedDataset's pairing, the workspace query, the argument checks that come
before any launch.  No launch anywhere."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import single_distort_ref as R

EINVAL, EWORKSPACE = -1, -4
NOISE, BLUR, FOG = 0, 1, 2


def _L():
    import roadrestore
    return roadrestore.lib()


def test_branch_free_noise_is_the_literal_text():
    """02:21-25 picks low_clip from out.min() < 0; clip(out, -1, 1) gives the
    same bytes for every image: with negatives it IS the branch taken, without
    them the lower clip is inert.  The literal text uses np.uint8, the
    restatement writes the wrap out."""
    rng = np.random.default_rng(0)
    sigma = 0.02 ** 0.5
    saw_negative = saw_wrap = False
    for i, (h, w) in enumerate([(30, 27), (5, 5), (64, 61), (1, 7)]):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        nz = rng.normal(0, sigma, img.shape)
        lit = R.noise_literal(img, nz)
        assert np.array_equal(lit, R.noise(img, nz, low=-1.0)), (h, w)
        neg = (img / 255 + nz) < 0
        saw_negative |= bool(neg.any())
        saw_wrap |= bool((lit[neg] > 128).any())
    assert saw_negative and saw_wrap                       # the reference bug is in the data
    # no negatives: an all-255 image under a non-negative field takes 02:24's branch
    img = np.full((9, 11, 3), 255, np.uint8)
    nz = np.abs(rng.normal(0, sigma, img.shape))
    assert (img / 255 + nz).min() >= 0
    assert np.array_equal(R.noise_literal(img, nz), R.noise(img, nz, low=-1.0))
    # and under a field too small to reach zero
    nz = rng.normal(0, 0.01, img.shape)
    assert (img / 255 + nz).min() >= 0
    assert np.array_equal(R.noise_literal(img, nz), R.noise(img, nz, low=-1.0))
    assert np.array_equal(R.noise_literal(img, nz), R.noise(img, nz, low=0.0))


def test_wrap_is_truncation_then_modulo():
    v = np.array([-3.7, -255.0, -0.5, 0.0, 0.99, 254.9, 255.0, -1.0, -254.2])
    assert R.wrap_u8(v).tolist() == [253, 1, 0, 0, 0, 254, 255, 255, 2]


def test_normalize_restatement():
    """03:29 on small cases worked by hand: a flat image comes out black, a
    range of 1 gives 0 and 255, the extremes go to 0 and 255"""
    assert not R.normalize(np.full((4, 5, 3), 77, np.uint8)).any()
    img = np.array([[[10, 11, 10]], [[11, 10, 11]]], np.uint8)
    assert R.normalize(img).tolist() == [[[0, 255, 0]], [[255, 0, 255]]]
    img = np.array([[[39, 138, 100]]], np.uint8)
    out = R.normalize(img)
    assert out[0, 0, 0] == 0 and out[0, 0, 1] == 255
    assert out[0, 0, 2] == int(np.rint(np.float32(100) * np.float32(255.0 / 99) + np.float32(-39 * (255.0 / 99))))


@pytest.mark.parametrize("seed", [0, 7])
def test_add_fog_draws_are_randoms(seed):
    """04:24-25: one uniform(0.8, 1.2) per image in batch order, then the clip"""
    from roadrestore import imgproc
    got = imgproc.fog_transmissions(9, 0.8, random.Random(seed))
    rng = random.Random(seed)
    want = []
    for _ in range(9):
        t = 1.0 - 0.8 * rng.uniform(0.8, 1.2)
        want.append(float(np.clip(t, 0.1, 0.9)))
    assert got == want
    assert all(0.1 <= t <= 0.9 for t in got) and len(set(got)) > 1
    assert imgproc.fog_transmissions(3, 1.5, random.Random(seed)) == [0.1] * 3       # the lower end of 04:25
    assert imgproc.fog_transmissions(3, 0.05, random.Random(seed)) == [0.9] * 3      # the upper end
    assert imgproc.fog_transmissions(2, 0.1, random.Random(seed), jitter=False) == [0.9, 0.9]   # 13:54
    r = random.Random(seed)
    imgproc.fog_transmissions(2, 0.1, r, jitter=False)
    assert r.random() == random.Random(seed).random()       # no draw without the jitter


def _ppm(path, h, w, seed):
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + px.tobytes())


def test_paired_dataset_pairing(tmp_path):
    """07:42-55: sorted clean files, the same relative path, .png only if the
    first does not exist, unmatched files dropped; no device touched"""
    from roadrestore import imgproc
    clean, bad = tmp_path / "clean", tmp_path / "Noise"
    for i, rel in enumerate(["00001/b.ppm", "00001/a.ppm", "00002/c.ppm", "00002/orphan.ppm", "00000/both.ppm"]):
        _ppm(clean / rel, 3 + i, 4, i)
    _ppm(bad / "00001/a.ppm", 3, 4, 10)                     # a .ppm twin
    _ppm(bad / "00001/b.ppm", 3, 4, 11)
    (bad / "00002").mkdir(parents=True)
    (bad / "00002/c.png").write_bytes(b"png")               # a .png-only twin (never opened here)
    _ppm(bad / "00000/both.ppm", 3, 4, 12)                  # both exist: the .ppm wins
    (bad / "00000/both.png").write_bytes(b"png")
    _ppm(bad / "00003/extra.ppm", 3, 4, 13)                 # no clean file: not listed
    ds = imgproc.PairedDataset(clean, bad, device="cuda:0")
    assert ds.data_pairs == [(bad / "00000/both.ppm", clean / "00000/both.ppm"),
                             (bad / "00001/a.ppm", clean / "00001/a.ppm"),
                             (bad / "00001/b.ppm", clean / "00001/b.ppm"),
                             (bad / "00002/c.png", clean / "00002/c.ppm")]
    assert len(ds) == 4 and len(ds.clean_files) == 5 and ds.transform is None
    assert len(imgproc.PairedDataset(clean, tmp_path / "nowhere")) == 0


def test_single_dataset_lists_files_only(tmp_path):
    from roadrestore import imgproc
    for i, rel in enumerate(["00002/b.ppm", "00002/a.ppm", "00001/9.ppm", "top.ppm", "00001/skip.png"]):
        _ppm(tmp_path / rel, 2 + i, 3, i)
    for task in ("Noise", "Blur", "Fog"):
        ds = imgproc.SingleDistortionDataset(tmp_path, task, device="cuda:0")
        assert ds.clean_files == sorted(tmp_path.glob('*/*.ppm')) and len(ds) == 3
    with pytest.raises(ValueError):
        imgproc.SingleDistortionDataset(tmp_path, "Rain")


def test_workspace_query():
    """elem_base[n] (16-byte aligned) plus one 8-byte (min, max) record per
    32 x 32 tile of n max_h x max_w images"""
    ws = _L().rr_distort_single_ragged_workspace
    for n in (1, 3, 64):
        for m, tiles in ((32, 1), (33, 2), (250, 8)):
            base = (n * 8 + 15) & ~15
            assert ws(n, 3, m, m) == base + n * tiles * tiles * 8, (n, m)
            assert ws(n, 3, m, 32) == base + n * tiles * 8
            assert ws(n, 3, 1, m) == base + n * tiles * 8
            assert ws(n, 1, m, m) == ws(n, 4, m, m) == ws(n, 3, m, m)
    for bad in ((0, 3, 250, 250), (-1, 3, 250, 250), (4, 0, 250, 250), (4, 5, 250, 250),
                (4, 3, 0, 250), (4, 3, 250, 0), (4, 3, -5, 250)):
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("kind", [NOISE, BLUR, FOG])
def test_validates_before_any_launch(kind):
    """every RR_EINVAL / RR_EWORKSPACE case returns without a device: the
    pointers below are never dereferenced"""
    L = _L()
    need = L.rr_distort_single_ragged_workspace(4, 3, 250, 250)
    buf = C.create_string_buffer(1024)
    base = C.addressof(buf)
    IN, OUT, TAB, PRM, TAPS, WS = (base + 64 * i for i in range(1, 7))

    def call(n=4, c=3, kind=kind, max_h=250, max_w=250, inp=IN, in_bytes=1000, tab=TAB, out=OUT, prm=PRM,
             taps=TAPS, noise=None, ws=WS, wsb=need):
        return L.rr_distort_single_ragged_u8(n, c, kind, max_h, max_w, inp, in_bytes, tab, out, prm, taps,
                                             noise, 0, ws, wsb, None)
    for kw in (dict(inp=None), dict(tab=None), dict(out=None), dict(prm=None), dict(ws=None),
               dict(n=0), dict(n=-3), dict(c=0), dict(c=5), dict(kind=3), dict(kind=-1),
               dict(max_h=0), dict(max_w=0), dict(max_h=-1), dict(in_bytes=0), dict(out=IN)):
        assert call(**kw) == EINVAL, kw
    if kind == BLUR:
        assert call(taps=None) == EINVAL
    assert call(wsb=need - 1) == EWORKSPACE
    assert call(wsb=0) == EWORKSPACE
    assert call(n=0, wsb=0) == EINVAL                       # the arguments come first
    assert bytes(buf) == bytes(1024)                        # nothing written through the dummies


def test_param_layout_matches_the_header():
    from roadrestore._lib import SingleParam
    assert C.sizeof(SingleParam) == 24
    assert (SingleParam.a.offset, SingleParam.b.offset, SingleParam.ksize.offset,
            SingleParam.stretch.offset) == (0, 8, 16, 20)


def test_no_cpu_fallback():
    from roadrestore import imgproc
    b = imgproc.RaggedBatch.from_arrays([np.zeros((3, 5, 3), np.uint8), np.zeros((4, 2, 3), np.uint8)], "cpu")
    for fn in (imgproc.add_gaussian_noise, imgproc.apply_motion_blur, imgproc.add_fog):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(b)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros(2, 4, 4, 3, dtype=torch.uint8))


def test_write_ppm_round_trips_on_the_host(tmp_path):
    """P6 as cv2.imwrite writes it; read_ppm reads the same bytes back"""
    from roadrestore import imgproc
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (5, 7), (33, 31))]
    b = imgproc.RaggedBatch.from_arrays(imgs, "cpu")
    paths = [tmp_path / "a" / f"{i}.ppm" for i in range(3)]
    imgproc.write_ppm(b, paths, threads=2)
    assert paths[1].read_bytes() == b"P6\n7 5\n255\n" + imgs[1].tobytes()
    back = imgproc.read_ppm(paths, "cpu")
    assert back.sizes == b.sizes
    for (o, h, w), im in zip([tuple(r) for r in back.records], imgs):
        assert np.array_equal(back.data.numpy()[o:o + h * w * 3].reshape(h, w, 3), im)
    dense = torch.from_numpy(rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8))
    imgproc.write_ppm(dense, [tmp_path / "d0.ppm", tmp_path / "d1.ppm"])
    assert (tmp_path / "d1.ppm").read_bytes() == b"P6\n6 4\n255\n" + dense[1].numpy().tobytes()
    with pytest.raises(ValueError):
        imgproc.write_ppm(dense, [tmp_path / "x.ppm"])
