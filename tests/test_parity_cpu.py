"""tests/parity.py tested on itself (no GPU): the ideal kernel -- fp32
accumulate, one bf16 store -- stays inside the per-element bound with zero
violations, three deliberately broken kernels are rejected, and two of them
pass the relative-L2 check (< 4e-3) the older conv tests assert -- which is why
the per-element bound exists.  The ideal emulation sums in fp32 in torch's own
order; the bound holds for any order."""
import math

import pytest
import torch
import torch.nn.functional as F

import parity

BF = torch.bfloat16
# (n, h, w, cin, cout)
SHAPES = [(2, 60, 60, 64, 64), (8, 16, 16, 128, 256), (1, 8, 8, 64, 128)]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def rel(a, r):
    a, r = a.double(), r.double()
    return ((a - r).norm() / r.norm()).item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


_CACHE = {}


def _case(shape):
    """bf16-exact operands (the recipe of tests/test_conv3r_gpu.py), the fp32
    accumulator of the ideal kernel, and (ref64, bound64)"""
    if shape not in _CACHE:
        n, h, w, cin, cout = shape
        x = rnd(n, cin, h, w, seed=1).bfloat16().float()
        wt = (rnd(cout, cin, 3, 3, seed=2) / (3 * cin ** 0.5)).bfloat16().float()
        b = rnd(cout, seed=3)
        acc = F.conv2d(x, wt, b, padding=1)                 # fp32 accumulate
        _CACHE[shape] = (x, wt, b, acc, parity.conv_bound(x, wt, b, 1, BF))
    return _CACHE[shape]


def _store(acc):
    return nhwc(acc.to(BF))                                 # one bf16 store, NHWC


def _broken(shape):
    """the three broken kernels, as fp32 accumulators before the store"""
    x, wt, _, acc, _ = _case(shape)
    tap = acc.clone()       # the centre tap dropped at pixel (0, 0) of every image
    tap[:, :, 0, 0] -= x[:, :, 0, 0] @ wt[:, :, 1, 1].t()
    prod = acc.clone()      # one product of K (centre tap, channel 0) dropped on the last column
    prod[:, :, :, -1] -= wt[None, :, 0, 1, 1, None] * x[:, None, 0, :, -1]
    junk = acc.clone()      # one garbage value per image
    for i in range(junk.shape[0]):
        junk[i, (7 * i + 3) % junk.shape[1], junk.shape[2] // 2, junk.shape[3] - 1] = -5.0
    return {"tap": tap, "product": prod, "garbage": junk}


@pytest.mark.parametrize("shape", SHAPES)
def test_ideal_conv_inside_bound(shape):
    _, _, _, acc, (ref, bound) = _case(shape)
    got = _store(acc)
    parity.assert_within(got, ref, bound, f"ideal {shape}")
    used = parity.worst_ratio(got, ref, bound)
    print(f"{shape}: ideal kernel uses {used:.3f} of the bound, L2 {rel(got, ref):.3e}")
    assert used <= 1.0
    # the fp32 accumulator itself against the fp32-output bound
    x, wt, b, _, _ = _case(shape)
    ref32, bound32 = parity.conv_bound(x, wt, b, 1, torch.float32)
    parity.assert_within(nhwc(acc), ref32, bound32, f"ideal fp32 {shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_broken_kernels_rejected(shape):
    _, _, _, _, (ref, bound) = _case(shape)
    for kind, acc in _broken(shape).items():
        got = _store(acc)
        with pytest.raises(AssertionError) as e:
            parity.assert_within(got, ref, bound, kind)
        count = int(str(e.value).split(": ")[1].split(" of ")[0])
        print(f"{shape} {kind}: L2 {rel(got, ref):.2e}, {count} violations")
        if kind == "garbage":
            assert count == shape[0]                        # exactly the one element per image


def test_old_metric_accepts_two_broken_kernels():
    """why the per-element bound exists: at (2, 60, 60, 64 -> 64) the dropped
    tap and the dropped product stay below the 4e-3 relative L2 error of the
    older conv tests"""
    shape = SHAPES[0]
    _, _, _, _, (ref, _) = _case(shape)
    br = _broken(shape)
    for kind in ("tap", "product"):
        assert rel(_store(br[kind]), ref) < 4e-3, kind


def test_nan_and_unwritten_are_violations():
    ref = torch.zeros(1, 2, 2, 4, dtype=torch.float64)
    bound = torch.ones_like(ref)
    got = torch.zeros(1, 2, 2, 4)
    parity.assert_within(got, ref, bound, "zeros")
    got[0, 1, 0, 2] = math.nan
    with pytest.raises(AssertionError, match=r"1 of 16 .*\(1 NaN\).*\(0, 1, 0, 2\)"):
        parity.assert_within(got, ref, bound, "nan")
    with pytest.raises(AssertionError, match="16 of 16"):
        parity.assert_within(torch.full_like(got, math.nan), ref, torch.full_like(ref, math.inf), "all nan")


def test_ideal_wgrad_and_stats_inside_bound():
    n, h, w, cin, cout = SHAPES[0]
    x, _, _, _, _ = _case(SHAPES[0])
    dy = rnd(n, cout, h, w, seed=4).bfloat16().float()
    for k in (3, 1):
        wt = torch.zeros(cout, cin, k, k, requires_grad=True)
        F.conv2d(x, wt, None, padding=k // 2).backward(dy)  # fp32 sums over n h w
        ref, bound = parity.wgrad_bound(x, dy, k)
        parity.assert_within(wt.grad, ref, bound, f"ideal wgrad k{k}")
        # K = 7200 terms: the worst-case bound is wide, one product hides in it;
        # the last image's pixels dropped from one element do not
        bad = wt.grad.clone()
        bad[5, 7, k // 2, k // 2] -= (dy[1, 5] * x[1, 7]).sum()
        with pytest.raises(AssertionError, match="1 of "):
            parity.assert_within(bad, ref, bound, "wgrad, an image dropped")
    # statistics: fp32 sums of the fp32 pre-bias accumulator
    x, wt, _, _, _ = _case(SHAPES[0])
    pre = F.conv2d(x, wt, None, padding=1)
    ref, bound = parity.stats_bound(parity.conv_terms(x, wt, 1), 9 * cin)
    got = torch.stack((pre.sum((0, 2, 3)), (pre * pre).sum((0, 2, 3))), 1)
    parity.assert_within(got, ref, bound, "ideal statistics")
    # the partial band of the last image (rows 48..59 of 60) left out of the sums
    cut = pre.clone()
    cut[-1, :, 48:] = 0
    with pytest.raises(AssertionError):
        parity.assert_within(torch.stack((cut.sum((0, 2, 3)), (cut * cut).sum((0, 2, 3))), 1), ref, bound,
                             "statistics, a band dropped")


def test_activations_and_pool_keep_the_bound():
    shape = SHAPES[2]
    x, wt, b, acc, rb = _case(shape)
    parity.assert_within(_store(F.relu(acc)), *parity.relu(rb), "relu")
    parity.assert_within(_store(torch.where(acc > 0, acc, 0.17 * acc)), *parity.prelu(rb, 0.17), "prelu")
    m = rnd(*acc.shape, seed=9)
    parity.assert_within(_store(torch.where(m > 0, acc, torch.zeros(()))), *parity.masked(rb, m), "mask")
    parity.assert_within(_store(F.max_pool2d(F.relu(acc), 2)), *parity.pooled(parity.relu(rb)), "pool")
    r = rnd(*acc.shape, seed=10).bfloat16().float()
    parity.assert_within(_store(F.relu(acc + r)), *parity.relu(parity.conv_bound(x, wt, b, 1, BF, extra=r)), "res")
    # rounds=2 doubles the store term only
    b1, b2 = rb[1], parity.conv_bound(x, wt, b, 1, BF, rounds=2)[1]
    assert torch.allclose(b2 - b1, parity.HALF_ULP_BF16 * rb[0].abs(), rtol=1e-12, atol=0)


def test_guard_bands_cpu():
    dev = torch.device("cpu")
    buf, v = parity.guarded((2, 5, 7, 64), BF, dev)
    assert v.shape == (2, 5, 7, 64) and bool(torch.isnan(v).all())
    assert buf.band >= 2 * 7 * 64 and (buf.band * 2) % 256 == 0 and parity.intact(buf)
    buf.raw[buf.band - 1] = 0.0                              # one element before the tensor
    assert not parity.intact(buf)
    buf, v = parity.guarded((3,), torch.float32, dev, fill=torch.ones(3), poison=math.nan)
    assert buf.band * 4 == 256 and parity.intact(buf) and bool((v == 1).all())
    buf.raw[buf.band + 3] = 1.0                              # one element past it
    assert not parity.intact(buf)
    buf, v = parity.guarded((4, 4), torch.uint8, dev)
    assert parity.intact(buf) and bool((v == 0xFF).all())
    assert bool(torch.isnan(v.view(torch.float32)).all())   # an unwritten fp32 workspace slab reads as NaN
    v.zero_()
    assert parity.intact(buf)
