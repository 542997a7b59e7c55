"""Per-element parity and guard bands for the two boundary layers:
csrc/conv_in.hip (3 -> 64 straight from the NCHW fp32 image), csrc/conv_out.hip
(64 -> 3 into NCHW fp32), rr_pack_conv_in / rr_unpack_conv_in_grad and
rr_prelu_bwd.  The packed image-grad route (igemm3_halo_kernel<16,W>, one-shot
and persistent) has its cases in tests/test_conv_elementwise_gpu.py.

The conventions of tests/test_conv_elementwise_gpu.py: the C ABI on buffers of
the test's own; every input (image, dy, t, the library's own pack of the size
it reports, weights, bias, alpha) a view inside NaN bands; every output (y_pre,
y_act, dw, db, dalpha, dx, the col matrix, the workspaces sized by the
library's own query) inside sentinel bands with a NaN interior unless the call
accumulates into it; ``intact`` on every output buffer and every element held
by ``assert_within`` to the bounds of tests/parity.py against an fp64 CPU
reference of exactly the operands the kernel multiplies.

These entry points have no kernel-name query: each launches one kernel chosen
by its arguments alone (conv_out_bwd64_kernel iff cin == 64 and cout == 3, the
generic kernel otherwise; the REC instantiation iff the _rec entry point), so
a shape reaches its instance by construction; the cases say which edge of the
kernel's hand-written index arithmetic they are there for."""
import math
import os

import pytest
import torch

import parity
from parity import TAIL_SHAPES, tail_inputs as _tail_inputs

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = math.nan
RR_EINVAL = -1
DT = [pytest.param(F32, id="f32"), pytest.param(BF, id="bf16")]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _q(t, dt):
    return t.to(dt).float()


def _f32(a):
    """the slope as the kernels read it: rounded to fp32"""
    return None if a is None else float(torch.tensor(a, dtype=torch.float32))


def _sid(s):
    return "x".join(map(str, s))


def _in(t, dt, dev):
    """an input tensor inside NaN bands"""
    return parity.guarded(tuple(t.shape), dt, dev, fill=t.to(dt), poison=NAN)[1]


def _ws(need, dev):
    """a workspace of exactly the bytes the library asked for, inside bands"""
    return parity.guarded((max(int(need), 16),), torch.uint8, dev, band=4096)


def _image(n, cin, h, w, seed):
    """a signed fp32 image whose values are NOT bf16-exact"""
    return rnd(n, cin, h, w, seed=seed) * 0.5 + 0.3


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _all_intact(outs, what):
    for key, (buf, _) in outs.items():
        assert parity.intact(buf), f"{what}: a store outside {key}"


def _report(name, got, rb, dt=BF):
    """the share of the bound in use, printed with RR_PARITY_REPORT=1 only (a
    measurement for DESIGN section 4's table, never asserted)"""
    if os.environ.get("RR_PARITY_REPORT"):
        print("RATIO %s %s %.3g" % (name, "bf16" if dt == BF else "f32", parity.worst_ratio(got, *rb)))


def _p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------
# 1. the first conv forward

MFMA_SHAPES = [(1, 5, 7),       # P = 35: one partial wave
               (3, 9, 11),      # P = 297: the 2nd workgroup has one live wave of 41 rows, three return early
               (2, 1, 70),      # every vertical tap is padding
               (2, 70, 1),      # every horizontal tap is padding
               (3, 6, 8),       # a 16-pixel fragment crosses an image boundary
               (2, 16, 16)]     # whole waves
ACTS = [(0, None), (1, None), (2, 0.25), (2, 0.0), (2, -0.1)]
ACT_IDS = ["none", "relu", "prelu0.25", "prelu0", "prelu-0.1"]
_FIRST = {}


def _first(shape):
    """host operands of the first conv at a shape, once"""
    if shape not in _FIRST:
        n, h, w = shape
        _FIRST[shape] = dict(x=_image(n, 3, h, w, 21), wt=rnd(64, 3, 3, 3, seed=22) / 3.0, b=rnd(64, seed=23) * 0.2,
                             g=_q(rnd(n, h, w, 64, seed=24), BF),
                             t=parity.with_zeros(_q(rnd(n, h, w, 64, seed=25), BF), 26))     # exact +-0 in t: the mask is t > 0
    return _FIRST[shape]


def _pack32(L, ops, d, dev):
    """the library's own kpad-32 pack, of the size the ABI states, between NaN bands"""
    wp = ops.pack_conv_in(d["wt"].to(dev), d["b"].to(dev), BF)
    assert wp.numel() == 64 * ops.KPAD_MFMA
    return parity.guarded((64 * 32,), BF, dev, fill=wp, band=8192, poison=NAN)[1]


@pytest.mark.parametrize("act,alpha", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=_sid)
def test_conv_in_mfma(dev, shape, act, alpha):
    """conv_in_mfma_kernel: the branch-free raw-buffer gather (padding taps
    and dead lanes read offset 2^32 - 1 of a buffer that ends with the image),
    partial waves, and y_pre only / y_act only / both."""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    d = _first(shape)
    alpha = _f32(alpha)
    rb = parity.conv_in_mfma_bounds(d["x"], d["wt"], d["b"], act, alpha)
    x = _in(d["x"], F32, dev)
    wp = _pack32(L, ops, d, dev)
    al = _in(torch.tensor([alpha]), F32, dev) if act == 2 else None
    variants = [(False, True), (True, True)] + ([(True, False)] if act == 0 else [])
    for want_pre, want_act in variants:
        outs = {}
        if want_pre:
            outs["pre"] = parity.guarded((n, h, w, 64), BF, dev)
        if want_act:
            outs["act"] = parity.guarded((n, h, w, 64), BF, dev)
        L.check(L.rr_conv_in_mfma(n, h, w, x.data_ptr(), wp.data_ptr(), act, _p(al),
                                  outs["pre"][1].data_ptr() if want_pre else None,
                                  outs["act"][1].data_ptr() if want_act else None, ops.stream()), "rr_conv_in_mfma")
        torch.cuda.synchronize()
        what = f"rr_conv_in_mfma {_sid(shape)} act {act} alpha {alpha} pre {want_pre} act {want_act}"
        _all_intact(outs, what)
        for key, (_, view) in outs.items():
            parity.assert_within(view, *rb[key], f"{what}: {key}")
            _report("conv_in_mfma." + key, view, rb[key])


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 12, 8)], ids=_sid)
@pytest.mark.parametrize("cin,cout", [(3, 64), (1, 4), (4, 128)])
def test_conv_in_fwd_valu(dev, cin, cout, shape, dt):
    """conv_in_fwd_kernel: fp32 image and weights unrounded, K = 9 cin + 1
    from the bias, output in T, every activation; PReLU at 0.25 and at -0.1,
    whose product with the accumulator is rounded (u |alpha v|: inside the
    K u A >= 10 u |v| the factor 2 of 2 K u A leaves over, tests/parity.py)"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    x0, wt0, b0 = _image(n, cin, h, w, 31), rnd(cout, cin, 3, 3, seed=32) / (3 * cin ** 0.5), rnd(cout, seed=33) * 0.2
    base = parity.conv_bound(x0, wt0, b0, 1, dt)
    x, wt, b = _in(x0, F32, dev), _in(wt0, F32, dev), _in(b0, F32, dev)
    for act, alpha in ACTS[:3] + ACTS[4:]:
        alpha = _f32(alpha)
        al = _in(torch.tensor([alpha]), F32, dev) if act == 2 else None
        rb = {0: base, 1: parity.relu(base), 2: parity.prelu(base, alpha) if act == 2 else None}[act]
        buf, y = parity.guarded((n, h, w, cout), dt, dev)
        L.check(L.rr_conv_in_fwd(ops.rr_dtype(dt), n, h, w, cin, cout, x.data_ptr(), wt.data_ptr(), b.data_ptr(), act,
                                 _p(al), y.data_ptr(), ops.stream()), "rr_conv_in_fwd")
        torch.cuda.synchronize()
        assert parity.intact(buf)
        parity.assert_within(y, *rb, f"rr_conv_in_fwd {cin}->{cout} {_sid(shape)} act {act} alpha {alpha}")
        _report("conv_in_fwd", y, rb, dt)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("cin", [3, 1])
@pytest.mark.parametrize("kpad", [32, 64])
def test_im2col3_bit_exact(dev, kpad, cin, dt):
    """rr_im2col3 against a CPU gather: the tap rounded to T, 1 in column
    9 cin, 0 elsewhere and in padding taps -- the same bits"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = 2, 5, 7
    x0 = _image(n, cin, h, w, 41)
    want = parity.patches3(x0, kpad).float().to(dt).reshape(n, h, w, kpad)       # fp32 values: .float() is exact
    x = _in(x0, F32, dev)
    buf, col = parity.guarded((n, h, w, kpad), dt, dev)
    L.check(L.rr_im2col3(ops.rr_dtype(dt), n, h, w, cin, kpad, x.data_ptr(), col.data_ptr(), ops.stream()), "rr_im2col3")
    torch.cuda.synchronize()
    assert parity.intact(buf)
    assert torch.equal(_bits(col.cpu()), _bits(want))


@pytest.mark.parametrize("kpad", [32, 64])
def test_pack_and_unpack_conv_in_bit_exact(dev, kpad):
    """rr_pack_conv_in ([co][kpad]: the weights, the bias in column 27, zero
    pad columns; both dtypes) and rr_unpack_conv_in_grad (the pad columns of
    its input are NaN here: not read) against the layout written out"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    wt0, b0 = rnd(64, 3, 3, 3, seed=42), rnd(64, seed=43)
    wt, b = _in(wt0, F32, dev), _in(b0, F32, dev)
    for dt in (F32, BF):
        buf, out = parity.guarded((64, kpad), dt, dev)
        L.check(L.rr_pack_conv_in(ops.rr_dtype(dt), 64, 3, kpad, wt.data_ptr(), b.data_ptr(), out.data_ptr(),
                                  ops.stream()), "rr_pack_conv_in")
        torch.cuda.synchronize()
        assert parity.intact(buf)
        want = parity.conv_in_pack(wt0, b0, kpad, dt).to(dt)
        assert bool((want[:, 28:] == 0).all())
        assert torch.equal(_bits(out.cpu()), _bits(want))
    g0 = rnd(64, kpad, seed=44)
    g0[:, 28:] = NAN
    g = _in(g0, F32, dev)
    outs = {"dw": parity.guarded((64, 27), F32, dev), "db": parity.guarded((64,), F32, dev)}
    L.check(L.rr_unpack_conv_in_grad(64, 3, kpad, g.data_ptr(), outs["dw"][1].data_ptr(), outs["db"][1].data_ptr(),
                                     ops.stream()), "rr_unpack_conv_in_grad")
    torch.cuda.synchronize()
    _all_intact(outs, "rr_unpack_conv_in_grad")
    assert torch.equal(_bits(outs["dw"][1].cpu()), _bits(g0[:, :27].contiguous()))
    assert torch.equal(_bits(outs["db"][1].cpu()), _bits(g0[:, 27].contiguous()))


# ---------------------------------------------------------------------------
# 2. the first conv's weight grads

WACT_SHAPES = [(1, 5, 7),
               (3, 6, 8),       # P = 144: a last step of 16 pixels and a step across two images
               (2, 16, 24),     # two ranges of 384
               (1, 24, 40),     # ranges of 512 and 448: split in the middle of a row
               (1, 17, 241),    # P = 4097: nine ranges of 512, the last holding one pixel
               (2, 1, 70), (2, 70, 1)]


@pytest.mark.parametrize("act,alpha", ACTS[1:], ids=ACT_IDS[1:])
@pytest.mark.parametrize("shape", WACT_SHAPES, ids=_sid)
def test_conv_in_wgrad_act(dev, shape, act, alpha):
    """conv_in_wgrad_act_kernel<false> with a pre-activation t of the test's
    own, and <true> (REC) held to the same bounds with t = the bytes
    rr_conv_in_mfma stores for the same image and pack (its y_pre first held
    to the forward's bound)."""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    P = n * h * w
    d = _first(shape)
    alpha = _f32(alpha)
    need = int(L.rr_conv_in_wgrad_act_workspace(n, h, w))
    assert need == parity.conv_in_act_workspace(P)              # the split the bounds' n_sum comes from
    x = _in(d["x"], F32, dev)
    g = _in(d["g"], BF, dev)
    wp = _pack32(L, ops, d, dev)
    al = _in(torch.tensor([alpha]), F32, dev) if act == 2 else None
    # the forward's y_pre: bounded, then downloaded as the recompute's t
    pbuf, pre = parity.guarded((n, h, w, 64), BF, dev)
    L.check(L.rr_conv_in_mfma(n, h, w, x.data_ptr(), wp.data_ptr(), 0, None, pre.data_ptr(), None, ops.stream()),
            "rr_conv_in_mfma")
    torch.cuda.synchronize()
    assert parity.intact(pbuf)
    parity.assert_within(pre, *parity.conv_in_mfma_bounds(d["x"], d["wt"], d["b"], 0, None)["pre"], "y_pre")
    pre_c = pre.float().cpu()
    assert float((pre_c > 0).float().mean()) > 0.2 and float((pre_c <= 0).float().mean()) > 0.2
    z = d["t"] == 0
    assert bool((z & ~torch.signbit(d["t"])).any() and (z & torch.signbit(d["t"])).any())
    for rec in (False, True):
        t_c = pre_c if rec else d["t"]                 # rec: the forward's own output, no zero can be forced into it
        rb = parity.conv_in_wgrad_act_bounds(d["x"], d["g"], t_c, act, alpha if act == 2 else 0.0)
        src = wp if rec else _in(t_c, BF, dev)
        outs = {"dw": parity.guarded((64, 27), F32, dev), "db": parity.guarded((64,), F32, dev),
                "dalpha": parity.guarded((1,), F32, dev), "workspace": _ws(need, dev)}
        fn = L.rr_conv_in_wgrad_act_rec if rec else L.rr_conv_in_wgrad_act
        L.check(fn(n, h, w, x.data_ptr(), g.data_ptr(), src.data_ptr(), act, _p(al), outs["dw"][1].data_ptr(),
                   outs["db"][1].data_ptr(), outs["dalpha"][1].data_ptr(), outs["workspace"][1].data_ptr(), need,
                   ops.stream()), "rr_conv_in_wgrad_act rec=%d" % rec)
        torch.cuda.synchronize()
        what = f"rr_conv_in_wgrad_act{'_rec' if rec else ''} {_sid(shape)} act {act} alpha {alpha}"
        _all_intact(outs, what)
        for key in ("dw", "db"):
            parity.assert_within(outs[key][1], *rb[key], f"{what}: {key}")
            _report("conv_in_wgrad_act." + key, outs[key][1], rb[key])
        if act == 2:
            parity.assert_within(outs["dalpha"][1].reshape(()), *rb["dalpha"], f"{what}: dalpha")
            _report("conv_in_wgrad_act.dalpha", outs["dalpha"][1].reshape(()), rb["dalpha"])
        else:
            assert bool(torch.isnan(outs["dalpha"][1]).all())       # ReLU: no slope grad written


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("cout", [64, 12])
@pytest.mark.parametrize("cin", [3, 1])
@pytest.mark.parametrize("shape", [(1, 5, 7), (1, 41, 53)], ids=_sid)
def test_conv_in_wgrad_valu(dev, shape, cin, cout, dt):
    """conv_in_wgrad_kernel; (1, 41, 53): P = 2173 in ranges of 1087 and 1086
    pixels, each with a ragged last stage of 63 / 62 pixels"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    P = n * h * w
    x0, dy0 = _image(n, cin, h, w, 51), _q(rnd(n, h, w, cout, seed=52), dt)
    ref, bound = parity.conv_in_wgrad_bounds(x0, dy0)
    need = int(L.rr_conv_in_wgrad_workspace(n, h, w, cin, cout))
    assert need == parity.conv_in_wgrad_workspace(P, cout)
    x, dy = _in(x0, F32, dev), _in(dy0, dt, dev)
    outs = {"dw": parity.guarded((cout, 9 * cin), F32, dev), "db": parity.guarded((cout,), F32, dev),
            "workspace": _ws(need, dev)}
    L.check(L.rr_conv_in_wgrad(ops.rr_dtype(dt), n, h, w, cin, cout, x.data_ptr(), dy.data_ptr(),
                               outs["dw"][1].data_ptr(), outs["db"][1].data_ptr(), outs["workspace"][1].data_ptr(), need,
                               ops.stream()), "rr_conv_in_wgrad")
    torch.cuda.synchronize()
    what = f"rr_conv_in_wgrad {cin}->{cout} {_sid(shape)}"
    _all_intact(outs, what)
    k = 9 * cin
    parity.assert_within(outs["dw"][1], ref[:, :k].contiguous(), bound[:, :k].contiguous(), what + ": dw")
    parity.assert_within(outs["db"][1], ref[:, k].contiguous(), bound[:, k].contiguous(), what + ": db")
    _report("conv_in_wgrad.dw", outs["dw"][1], (ref[:, :k].contiguous(), bound[:, :k].contiguous()), dt)
    _report("conv_in_wgrad.db", outs["db"][1], (ref[:, k].contiguous(), bound[:, k].contiguous()), dt)


# ---------------------------------------------------------------------------
# 3. the image grad (VALU; the packed route: tests/test_conv_elementwise_gpu.py)

@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("cin", [3, 1])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 12, 8)], ids=_sid)
def test_conv_in_dgrad_valu(dev, shape, cin, acc, dt):
    """conv_in_dgrad_kernel: K = 9 * 64 (+ 1 accumulated into)"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    cout = 64
    dy0 = _q(rnd(n, cout, h, w, seed=61), dt)
    wt0 = rnd(cout, cin, 3, 3, seed=62) / 24.0
    dx0 = rnd(n, cin, h, w, seed=63)
    rb = parity.conv_in_dgrad_bounds(dy0, wt0, dx0 if acc else None)
    dy, wt = _in(_nhwc(dy0), dt, dev), _in(wt0, F32, dev)
    buf, dx = parity.guarded((n, cin, h, w), F32, dev, fill=dx0 if acc else None)
    L.check(L.rr_conv_in_dgrad(ops.rr_dtype(dt), n, h, w, cin, cout, dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), acc,
                               ops.stream()), "rr_conv_in_dgrad")
    torch.cuda.synchronize()
    assert parity.intact(buf)
    parity.assert_within(dx, *rb, f"rr_conv_in_dgrad cin {cin} {_sid(shape)} acc {acc}", nchw=True)
    _report("conv_in_dgrad", _nhwc(dx.cpu()), rb, dt)


# ---------------------------------------------------------------------------
# 4. the last conv

@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("cout", [3, 1])
@pytest.mark.parametrize("cin", [64, 12])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 9, 11)], ids=_sid)
def test_conv_out_fwd_valu(dev, shape, cin, cout, dt):
    """conv_out_fwd_kernel: x in T, fp32 weights, K = cin + 1, NCHW fp32 out;
    (3, 9, 11): P = 297, a second workgroup and pixels of three images"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    x0 = _q(rnd(n, cin, h, w, seed=71), dt)
    wt0, b0 = rnd(cout, cin, 1, 1, seed=72) / cin ** 0.5, rnd(cout, seed=73)
    rb = parity.conv1x1_bound(x0, wt0, b0, F32)
    x, wt, b = _in(_nhwc(x0), dt, dev), _in(wt0.reshape(cout, cin), F32, dev), _in(b0, F32, dev)
    buf, y = parity.guarded((n, cout, h, w), F32, dev)
    L.check(L.rr_conv_out_fwd(ops.rr_dtype(dt), n, h, w, cin, cout, x.data_ptr(), wt.data_ptr(), b.data_ptr(),
                              y.data_ptr(), ops.stream()), "rr_conv_out_fwd")
    torch.cuda.synchronize()
    assert parity.intact(buf)
    parity.assert_within(y, *rb, f"rr_conv_out_fwd {cin}->{cout} {_sid(shape)}", nchw=True)
    _report("conv_out_fwd", _nhwc(y.cpu()), rb, dt)


OUT_BWD = [(64, 3, (1, 5, 7)),
           (64, 3, (1, 3, 11)),     # P = 33: one pair (pixels 0, 32) and 31 lanes in the trailing call
           (64, 3, (2, 33, 31)),    # P = 2046: two ranges of 1023
           (64, 3, (1, 32, 33)),    # P = 1056 in ranges of 528
           (12, 3, (1, 5, 7)), (12, 1, (1, 5, 7)), (4, 3, (1, 5, 7)), (4, 1, (1, 5, 7)),
           (12, 3, (1, 32, 33)), (4, 1, (1, 32, 33))]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("cin,cout,shape", OUT_BWD, ids=["%d-%d-%s" % (a, b, _sid(s)) for a, b, s in OUT_BWD])
def test_conv_out_bwd(dev, cin, cout, shape, dt):
    """conv_out_bwd64_kernel (cin 64, cout 3) and the generic kernel (every
    other pair), mask on / off, with and without dx"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    P = n * h * w
    dy0 = rnd(n, cout, h, w, seed=81)
    x0 = parity.with_zeros(_q(rnd(n, h, w, cin, seed=82), dt), 87)       # a ReLU output in the model: exact +-0
    assert bool((x0 == 0).any())
    wt0 = rnd(cout, cin, seed=83) / 4.0
    need = int(L.rr_conv_out_bwd_workspace(n, h, w, cin, cout))
    assert need == parity.conv_out_workspace(P, cin, cout)
    dy, x, wt = _in(dy0, F32, dev), _in(x0, dt, dev), _in(wt0, F32, dev)
    assert float((x0 > 0).float().mean()) > 0.2 and float((x0 <= 0).float().mean()) > 0.2
    for mask in (0, 1):
        rb = parity.conv_out_bwd_bounds(dy0, x0, wt0, mask, dt)
        for want_dx in (True, False):
            outs = {"dw": parity.guarded((cout, cin), F32, dev), "db": parity.guarded((cout,), F32, dev),
                    "workspace": _ws(need, dev)}
            if want_dx:
                outs["dx"] = parity.guarded((n, h, w, cin), dt, dev)
            L.check(L.rr_conv_out_bwd(ops.rr_dtype(dt), n, h, w, cin, cout, dy.data_ptr(), x.data_ptr(), wt.data_ptr(),
                                      outs["dx"][1].data_ptr() if want_dx else None, mask, outs["dw"][1].data_ptr(),
                                      outs["db"][1].data_ptr(), outs["workspace"][1].data_ptr(), need, ops.stream()),
                    "rr_conv_out_bwd")
            torch.cuda.synchronize()
            what = f"rr_conv_out_bwd {cin}->{cout} {_sid(shape)} mask {mask} dx {want_dx}"
            _all_intact(outs, what)
            for key in ("dx", "dw", "db"):
                if key in outs:
                    parity.assert_within(outs[key][1], *rb[key], f"{what}: {key}")
                    _report("conv_out_bwd%s.%s" % ("64" if cin == 64 else "", key), outs[key][1], rb[key], dt)


@pytest.mark.parametrize("cin,cout", [(2, 3), (1, 2), (3, 4)])
def test_conv_out_bwd_refuses_cin_below_cout(dev, cin, cout):
    """The partial slab [(cout + 1)][cin] gives the db row cin slots; the
    kernel writes cout values into it.  First on the CPU, from the layout: with
    cin < cout the last of them leaves the workgroup's slab -- for the last
    workgroup it leaves the slab area the workspace query sizes.  Then the
    call: RR_EINVAL, and not a byte of the banded outputs and workspace
    written (nothing is launched at such a shape)."""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = 1, 5, 7
    blocks, _ = parity.conv_out_split(n * h * w)
    slab = (cout + 1) * cin
    last_db = ((blocks - 1) * (cout + 1) + cout) * cin + (cout - 1)      # the kernel's own index expression
    assert not parity.conv_out_db_row_holds(cin, cout) and last_db >= blocks * slab
    # the control, cin = cout: the same expression stays inside
    assert parity.conv_out_db_row_holds(cout, cout)
    assert ((blocks - 1) * (cout + 1) + cout) * cout + cout - 1 < blocks * (cout + 1) * cout
    need = int(L.rr_conv_out_bwd_workspace(n, h, w, cin, cout))
    dy, x = _in(rnd(n, cout, h, w, seed=84), F32, dev), _in(rnd(n, h, w, cin, seed=85), F32, dev)
    wt = _in(rnd(cout, cin, seed=86), F32, dev)
    outs = {"dx": parity.guarded((n, h, w, cin), F32, dev), "dw": parity.guarded((cout, cin), F32, dev),
            "db": parity.guarded((cout,), F32, dev), "workspace": _ws(need, dev)}
    before = {k: b.raw.clone() for k, (b, _) in outs.items()}
    rc = L.rr_conv_out_bwd(ops.rr_dtype(F32), n, h, w, cin, cout, dy.data_ptr(), x.data_ptr(), wt.data_ptr(),
                           outs["dx"][1].data_ptr(), 0, outs["dw"][1].data_ptr(), outs["db"][1].data_ptr(),
                           outs["workspace"][1].data_ptr(), need, ops.stream())
    torch.cuda.synchronize()
    assert rc == RR_EINVAL
    for k, (b, _) in outs.items():
        same = b.raw.view(torch.uint8) == before[k].view(torch.uint8)
        assert bool(same.all()), k


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=_sid)
def test_affine_act_conv_out(dev, shape):
    """tail_conv_out_kernel on banded buffers: y to the residual tail's bound,
    out to the fp64 1x1 of y's stored bytes (K = 64 + the bias), with and
    without y stored"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    n, h, w = shape
    d = _tail_inputs(shape)
    wq = d["wt"].view(3, 64).to(BF).float()
    wpack = ops.pack_conv(d["wt"].to(dev), BF, fwd=True, dgrad=False)[0]
    assert wpack.numel() == ops.pack_elems(BF, 3, 64, 1)
    wp = parity.guarded(tuple(wpack.shape), BF, dev, fill=wpack, band=8192, poison=NAN)[1]
    t2, s = _in(d["t2"], BF, dev), _in(d["s"], BF, dev)
    sc, sh = [_in(v, F32, dev) for v in d["sc"]], [_in(v, F32, dev) for v in d["sh"]]
    bias = _in(d["bias"], F32, dev)
    y_rb = parity.affine_res_bound(d["t2"], d["sc"][0], d["sh"][0], BF, res=d["s"], rs=d["sc"][1], rb=d["sh"][1], relu=True)
    y_c = None
    for want_y in (True, False):
        outs = {"out": parity.guarded((n, 3, h, w), F32, dev)}
        if want_y:
            outs["y"] = parity.guarded((n, h, w, 64), BF, dev)
        L.check(L.rr_affine_act_conv_out(ops.rr_dtype(BF), n, h, w, 64, 3, t2.data_ptr(), sc[0].data_ptr(),
                                         sh[0].data_ptr(), s.data_ptr(), sc[1].data_ptr(), sh[1].data_ptr(),
                                         wp.data_ptr(), bias.data_ptr(), outs["y"][1].data_ptr() if want_y else None,
                                         outs["out"][1].data_ptr(), ops.stream()), "rr_affine_act_conv_out")
        torch.cuda.synchronize()
        what = f"rr_affine_act_conv_out {_sid(shape)} want_y {want_y}"
        _all_intact(outs, what)
        if want_y:
            parity.assert_within(outs["y"][1], *y_rb, what + ": y")
            _report("affine_act_conv_out.y", outs["y"][1], y_rb)
            y_c = outs["y"][1].float().cpu()
        o_rb = parity.conv1x1_nchw_bound(y_c, wq, d["bias"])
        parity.assert_within(outs["out"][1], *o_rb, what + ": out", nchw=True)
        _report("affine_act_conv_out.out", _nhwc(outs["out"][1].cpu()), o_rb)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("count", [1, 4093, 4096, 8200])
def test_prelu_bwd(dev, count, dt):
    """prelu_bwd_kernel: 1 and 4093 end in a count % 4 tail (1: nothing but
    the tail), 4096 fills one workgroup's vectors exactly, 8200 takes three
    workgroups' partials"""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    alpha = 0.25
    blocks = max(1, min(1024, (count + 4095) // 4096))
    dy0, t0 = _q(rnd(count, seed=91), dt), parity.with_zeros(_q(rnd(count, seed=92) - 0.3, dt), 93)
    assert count == 1 or bool(((t0 == 0) & ~torch.signbit(t0)).any() and ((t0 == 0) & torch.signbit(t0)).any())
    rb = parity.prelu_bwd_bounds(dy0, t0, alpha, dt, blocks)
    dy, t, al = _in(dy0, dt, dev), _in(t0, dt, dev), _in(torch.tensor([alpha]), F32, dev)
    outs = {"dx": parity.guarded((count,), dt, dev), "partial": parity.guarded((blocks,), F32, dev),
            "dalpha": parity.guarded((1,), F32, dev)}
    L.check(L.rr_prelu_bwd(ops.rr_dtype(dt), count, dy.data_ptr(), t.data_ptr(), al.data_ptr(), outs["dx"][1].data_ptr(),
                           outs["partial"][1].data_ptr(), blocks, outs["dalpha"][1].data_ptr(), ops.stream()),
            "rr_prelu_bwd")
    torch.cuda.synchronize()
    what = f"rr_prelu_bwd count {count}"
    _all_intact(outs, what)
    parity.assert_within(outs["dx"][1], *rb["dx"], what + ": dx")
    assert bool(torch.isfinite(outs["partial"][1]).all())
    parity.assert_within(outs["dalpha"][1].reshape(()), *rb["dalpha"], what + ": dalpha")
    _report("prelu_bwd.dx", outs["dx"][1], rb["dx"], dt)
    _report("prelu_bwd.dalpha", outs["dalpha"][1].reshape(()), rb["dalpha"], dt)
