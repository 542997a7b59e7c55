"""GPU: the Python wrappers of the ragged image ops (roadrestore/ops.py,
imgproc.RandomDistortion) refuse each kind of bad argument with the exception
type they have always raised, and the three ops functions that took over the
C calls of imgproc.cv_resize and RandomDistortion return what those return,
byte for byte.

The batch is the smallest that is ragged: an 8 x 8 and a 9 x 7 image of three
channels.  Every refusal happens in Python or in the library's argument
checks, before any launch."""
import numpy as np
import pytest
import torch

from oracle import imgproc_cpu as I

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 7)]
N, C_ = len(SIZES), 3
K = 15                                      # RR_DISTORT_KMAX


@pytest.fixture(scope="module")
def batch(dev):
    from roadrestore import imgproc
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, (h, w, C_), dtype=np.uint8) for h, w in SIZES]
    return imgs, imgproc.RaggedBatch.from_arrays(imgs, dev)


def _variant(b, **kw):
    """the batch's (data, table) with one of them replaced"""
    return kw.get("data", b.data), kw.get("table", b.table)


def _ops(b, dev):
    """name -> f(data, table, **kw): one valid call of each ragged op, with keyword overrides"""
    from roadrestore import imgproc, ops
    from roadrestore._lib import DistortParam
    params = [DistortParam(0.1, 0.8, 0.18, 7, 5), DistortParam(0.0, 1.0, 0.0, 0, 0)]
    taps = torch.stack([ops.motion_blur_kernel(5, 30), torch.zeros(K, K)])
    restored = torch.zeros((N, 8, 8, C_), dtype=torch.uint8, device=dev)

    def distort(d, t, **kw):
        kw = dict(dict(params=params, taps=taps), **kw)
        return ops.distort_ragged_u8(d, t, b.max_hw, C_, kw.pop("params"), kw.pop("taps"), **kw)

    def random(d, t, out=None):
        x = object.__new__(imgproc.RaggedBatch)              # the batch with d and t, unchecked
        x.__dict__.update(b.__dict__, data=d, table=t)
        return imgproc.RandomDistortion(dev, seed=3)(x, out)

    return {
        "resize_ragged_u8": lambda d, t, **kw: ops.resize_ragged_u8(d, t, b.max_hw, C_, 4, 4, **kw),
        "cv_resize_ragged_u8": lambda d, t: ops.cv_resize_ragged_u8(d, t, b.max_hw, C_, 4, 4),
        "eval_ragged_u8": lambda d, t, restored=restored: ops.eval_ragged_u8(d, t, b.max_hw, C_, restored),
        "distort_ragged_u8": distort,
        "RandomDistortion": random,
    }


# what every ragged op answers to a bad buffer or table.  RandomDistortion made
# none of the three type checks before it shared them with the others (it
# launched on whatever a hand-built RaggedBatch held), so its TypeError is new
SHARED = [
    ("a table of the wrong dtype", lambda b: _variant(b, table=b.table.view(torch.int32)), TypeError),
    ("a table of the wrong width", lambda b: _variant(b, table=b.table[:, :15].contiguous()), TypeError),
    ("a non-contiguous data buffer", lambda b: _variant(b, data=torch.cat([b.data, b.data])[::2]), TypeError),
    ("a CPU tensor", lambda b: _variant(b, data=b.data.cpu()), RuntimeError),
]
OPS = ["resize_ragged_u8", "cv_resize_ragged_u8", "eval_ragged_u8", "distort_ragged_u8", "RandomDistortion"]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("what,make,exc", SHARED, ids=[s[0] for s in SHARED])
def test_bad_buffer_or_table(batch, dev, op, what, make, exc):
    _, b = batch
    with pytest.raises(exc):
        _ops(b, dev)[op](*make(b))


def test_bad_arguments_of_one_op(batch, dev):
    from roadrestore import ops
    _, b = batch
    f = _ops(b, dev)
    d, t = b.data, b.table
    with pytest.raises(ValueError):
        f["distort_ragged_u8"](d, t, params=[])                                  # params of the wrong length
    with pytest.raises(ValueError):
        f["distort_ragged_u8"](d, t, taps=torch.zeros(N, K, K - 1))              # taps of the wrong shape
    with pytest.raises(ValueError):
        f["distort_ragged_u8"](d, t, taps=torch.zeros(N + 1, K, K))              # no tap_idx: one per image
    with pytest.raises(TypeError):
        f["distort_ragged_u8"](d, t, tap_idx=torch.zeros(N, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError):
        f["distort_ragged_u8"](d, t, out=d)                                      # out aliasing data
    with pytest.raises(RuntimeError):
        f["RandomDistortion"](d, t, out=d)                                       # ... refused by the library
    with pytest.raises(TypeError):
        f["RandomDistortion"](d, t, out=torch.empty(3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):                                              # image 0 alone has 192 elements
        f["distort_ragged_u8"](d, t, noise=torch.zeros(100, dtype=torch.float64))
    with pytest.raises(ValueError):
        f["distort_ragged_u8"](d, t, mode=2)
    with pytest.raises(ValueError):                                              # restored on 4 channels
        f["eval_ragged_u8"](d, t, restored=torch.zeros((N, 8, 8, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        f["resize_ragged_u8"](d, t, out="f16")
    with pytest.raises(RuntimeError):                                            # n == 0: the workspace query
        ops.resize_ragged_u8(d, t[:0], b.max_hw, C_, 4, 4)
    with pytest.raises(ValueError):                                              # n == 0: a range check
        ops.cv_resize_ragged_u8(d, t[:0], b.max_hw, C_, 4, 4)


def test_good_calls_still_pass(batch, dev):
    """the valid call each refusal above is a variation of"""
    _, b = batch
    for name, f in _ops(b, dev).items():
        f(b.data, b.table)
    torch.cuda.synchronize()


def test_cv_resize_linear_is_cv_resize(batch, dev):
    from roadrestore import imgproc, ops
    imgs, _ = batch
    x = torch.from_numpy(np.stack([imgs[0], imgs[0][::-1].copy()])).to(dev)
    got = ops.cv_resize_linear_u8(x, 5, 11)
    assert torch.equal(got, imgproc.cv_resize(x, (11, 5)))
    assert np.array_equal(got[0].cpu().numpy(), I.cv_resize_linear(imgs[0], 5, 11))
    assert torch.equal(ops.cv_resize_linear_u8(x, 8, 8), x)                      # same size: a copy


def test_distort_random_is_random_distortion(batch, dev):
    """same seed, same step: the ops functions and RandomDistortion draw and write the same"""
    from roadrestore import imgproc, ops
    imgs, b = batch
    x = torch.from_numpy(np.stack([imgs[0], imgs[0][::-1].copy()])).to(dev)
    table = imgproc.motion_blur_table(dev)
    for seed in (3, 11):                                   # two seeds, two steps: eight draws each
        rd, rr = imgproc.RandomDistortion(dev, seed), imgproc.RandomDistortion(dev, seed)
        step_d = torch.zeros((), dtype=torch.int64, device=dev)
        step_r = torch.zeros((), dtype=torch.int64, device=dev)
        for _ in range(2):                                 # the step advances in both
            assert torch.equal(ops.distort_random_u8(x, seed, step_d, table), rd(x))
            got = ops.distort_random_ragged_u8(b.data, b.table, b.max_hw, C_, seed, step_r, table)
            assert torch.equal(got, rr(b).data)
        assert step_d.item() == rd.step.item() == 2 and step_r.item() == rr.step.item() == 2
