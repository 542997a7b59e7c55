"""CPU: the host side of the ragged distortion (rr_distort_ragged_u8 and its
random variant): the workspace query, the argument checks that come before
any launch, the draw offsets, the dataset's file rule.  No launch anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

EINVAL, EWORKSPACE = -1, -4


def _L():
    import roadrestore
    return roadrestore.lib()


def test_workspace_has_no_image_term():
    """the blur input never reaches memory: the workspace holds the prefix
    sums and the draws, so it grows with n alone"""
    ws = _L().rr_distort_ragged_workspace
    prev = 0
    for n in (1, 2, 3, 15, 16, 17, 64, 65, 256, 257, 1000):
        cur = ws(n, 3, 250, 250)
        assert cur > 0 and cur >= prev
        # n prefix sums (int64), n rr_distort_param (24 bytes), n int32, one seed
        assert cur >= n * (8 + 24 + 4) + 8
        assert cur == ws(n, 3, 16, 16) == ws(n, 1, 250, 250) == ws(n, 4, 1, 100000)
        prev = cur
    assert ws(64, 3, 250, 250) < 64 * 64                 # far below one 250 x 250 x 3 image
    for bad in ((0, 3, 250, 250), (-1, 3, 250, 250), (4, 0, 250, 250), (4, 5, 250, 250),
                (4, 3, 0, 250), (4, 3, 250, 0), (4, 3, -5, 250)):
        assert ws(*bad) == 0, bad


def test_distort_ragged_validates_before_any_launch():
    """every RR_EINVAL / RR_EWORKSPACE case returns without a device: the
    pointers below are never dereferenced"""
    L = _L()
    need = L.rr_distort_ragged_workspace(4, 3, 250, 250)

    def call(n=4, c=3, mode=0, max_h=250, max_w=250, inp=0x1000, in_bytes=1000, tab=0x2000, out=0x3000,
             prm=0x4000, taps=0x5000, idx=None, noise=None, ws=0x6000, wsb=need):
        return L.rr_distort_ragged_u8(n, c, mode, max_h, max_w, inp, in_bytes, tab, out, prm, taps, idx,
                                      noise, 0, ws, wsb, None)
    for kw in (dict(inp=None), dict(tab=None), dict(out=None), dict(prm=None), dict(taps=None),
               dict(ws=None), dict(n=0), dict(n=-3), dict(c=0), dict(c=5), dict(mode=2), dict(mode=-1),
               dict(max_h=0), dict(max_w=0), dict(max_h=-1), dict(in_bytes=0),
               dict(out=0x1000)):                              # in == out: the halo reads forbid it
        assert call(**kw) == EINVAL, kw
    assert call(wsb=need - 1) == EWORKSPACE
    assert call(wsb=0) == EWORKSPACE


def test_distort_random_ragged_validates_before_any_launch():
    L = _L()
    need = L.rr_distort_ragged_workspace(4, 3, 250, 250)

    def call(n=4, c=3, max_h=250, max_w=250, inp=0x1000, in_bytes=1000, tab=0x2000, out=0x3000,
             step=0x4000, table=0x5000, ws=0x6000, wsb=need):
        return L.rr_distort_random_ragged_u8(n, c, max_h, max_w, inp, in_bytes, tab, out, 7, step, table,
                                             ws, wsb, None)
    for kw in (dict(inp=None), dict(tab=None), dict(out=None), dict(step=None), dict(table=None),
               dict(ws=None), dict(n=0), dict(c=0), dict(c=5), dict(max_h=0), dict(max_w=0),
               dict(in_bytes=0), dict(out=0x1000)):
        assert call(**kw) == EINVAL, kw
    assert call(wsb=need - 1) == EWORKSPACE


def test_draw_offsets_lie_inside_the_workspace_and_apart():
    from roadrestore._lib import DistortParam
    L = _L()
    for n in (1, 3, 4, 5, 64, 1001):
        total = L.rr_distort_ragged_workspace(n, 3, 250, 250)
        po, io, so = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert L.rr_distort_random_ragged_draws(n, 3, 250, 250, 0x1000, C.byref(po), C.byref(io),
                                                C.byref(so)) == 0
        spans = sorted([(0, 8 * n), (po.value, po.value + C.sizeof(DistortParam) * n),
                        (io.value, io.value + 4 * n), (so.value, so.value + 8)])
        assert spans[0][0] == 0 and spans[-1][1] <= total
        for (_, e0), (b1, _) in zip(spans, spans[1:]):
            assert e0 <= b1, (n, spans)                        # prefix, params, indices, seed: disjoint
        assert po.value % 8 == 0 and io.value % 4 == 0 and so.value % 8 == 0
    po = C.c_size_t()
    assert L.rr_distort_random_ragged_draws(4, 3, 250, 250, None, C.byref(po), C.byref(po),
                                            C.byref(po)) == EINVAL
    assert L.rr_distort_random_ragged_draws(0, 3, 250, 250, 0x1000, C.byref(po), C.byref(po),
                                            C.byref(po)) == EINVAL
    assert L.rr_distort_random_ragged_draws(4, 3, 250, 250, 0x1000, None, C.byref(po),
                                            C.byref(po)) == EINVAL


def _ppm(path, h, w, seed):
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + px.tobytes())


def test_dataset_file_rule_is_the_references(tmp_path):
    """14:66-73: sorted(clean_root.glob('*/*.ppm')), len() its length; the
    constructor lists files and touches no device"""
    from roadrestore import imgproc
    for i, rel in enumerate(["00002/b.ppm", "00002/a.ppm", "00010/x.ppm", "00001/9.ppm", "00001/10.ppm",
                             "00001/deep/no.ppm", "top.ppm", "00001/skip.png", "00003/UP.PPM"]):
        _ppm(tmp_path / rel, 2 + i, 3, i)
    ds = imgproc.DynamicDistortionDataset(tmp_path, device="cuda:0", seed=3)   # no GPU needed to list
    assert ds.clean_files == sorted(tmp_path.glob('*/*.ppm'))
    assert len(ds) == len(ds.clean_files) >= 5
    assert [p.name for p in ds.clean_files[:2]] == ["10.ppm", "9.ppm"]
    assert all(p.parent.parent == tmp_path for p in ds.clean_files)
    assert ds.transform is None
    assert len(imgproc.DynamicDistortionDataset(tmp_path / "00005")) == 0


def test_no_cpu_fallback():
    """a host RaggedBatch is refused by every ragged distortion entry point"""
    import random
    from roadrestore import imgproc, ops
    from roadrestore._lib import DistortParam
    imgs = [np.zeros((3, 5, 3), np.uint8), np.zeros((4, 2, 3), np.uint8)]
    b = imgproc.RaggedBatch.from_arrays(imgs, "cpu")
    rd = imgproc.RandomDistortion("cpu", seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rd(b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imgproc.apply_random_distortions(b, rng=random.Random(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imgproc.apply_compound_distortion(b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distort_ragged_u8(b.data, b.table, b.max_hw, 3, [DistortParam(0.0, 1.0, 0.0, 0, 0)] * 2,
                              torch.zeros(2, 15, 15))
    # the records travel with the result; with_data shares them
    y = b.with_data(torch.zeros_like(b.data))
    assert y.table is b.table and y.records is b.records and y.max_hw == b.max_hw and y.sizes == b.sizes
    with pytest.raises(TypeError):
        b.with_data(torch.zeros(3, dtype=torch.uint8))
