"""The two 64-channel boundary activations recomputed instead of stored.

dec1's block output (14:114-115 + 14:149):
rr_affine_act_conv_out (the residual tail and the final 1x1 conv in one pass)
and rr_conv_out_bwd_bnred_rec (the final conv's backward without the stored
block output) against the separate entry points they replace -- bitwise -- and
the ResUNet train step with the paths on against the paths off -- bitwise.
The first conv's pre-activation (14:122-123): rr_conv_in_wgrad_act_rec
against rr_conv_in_wgrad_act fed what rr_conv_in_mfma stores -- bitwise.

Every comparison is on the bit patterns (int views): the new kernels run the
same instructions on the same operands in the same order, so nothing but a
difference of zero is accepted.  The one independent bound (the 1x1 against an
fp64 evaluation) is the fp32 accumulation bound of 64 products and a bias."""
import ctypes as C

import pytest
import torch

from parity import TAIL_SHAPES, tail_inputs as _tail_inputs
from rrpath import set_path

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
RR_EINVAL, RR_EUNSUPPORTED = -1, -2


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def bits(t):
    """the tensor's bit patterns (NaN-safe, -0 != +0)"""
    if not t.is_floating_point():
        return t
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# (the streaming 1x1 takes whole 16-pixel blocks only: not P = 105)
TAIL_CASES = [(s, None) for s in TAIL_SHAPES] + [(s, 64) for s in TAIL_SHAPES[1:]]


@pytest.mark.parametrize("shape,minp", TAIL_CASES,
                         ids=["%s-%s" % ("x".join(map(str, s)), "stream1" if m else "tiled") for s, m in TAIL_CASES])
def test_tail_conv_out_matches_the_two_passes(dev, shape, minp, monkeypatch):
    """(3, 5, 7): P = 105, a partial last 16-pixel block and blocks that cross
    an image; (2, 8, 8), (1, 16, 24): whole blocks, which the streaming 1x1
    (stream1_kernel<1,2,..,NCHW>, the benched shape's kernel) takes from 64
    pixels with stream1_minp=64 -- both references are checked."""
    from roadrestore import ops
    if minp is not None:
        set_path(monkeypatch, "stream1_minp", minp)
    n, h, w = shape
    d = _tail_inputs(shape)
    t2, s = d["t2"].to(dev), d["s"].to(dev)
    sc, sh = [v.to(dev) for v in d["sc"]], [v.to(dev) for v in d["sh"]]
    wt, bias = d["wt"].to(dev), d["bias"].to(dev)
    wpack = ops.pack_conv(wt, BF, fwd=True, dgrad=False)[0]
    y_ref = ops.affine_act(t2, sc[0], sh[0], res=s, res_scale=sc[1], res_shift=sh[1], relu=True)
    out_ref = ops.conv_out_fwd(y_ref, wt, bias, wpack=wpack)
    assert ops.affine_act_conv_out_ok(t2, 3)
    y, out = ops.affine_act_conv_out(t2, sc[0], sh[0], s, sc[1], sh[1], wpack, bias, 3, want_y=True)
    torch.cuda.synchronize()
    assert float((y_ref == 0).float().mean()) > 0.2 and float((y_ref > 0).float().mean()) > 0.2
    assert same_bits(y, y_ref)
    assert same_bits(out, out_ref)
    # y null: the same output, and a sentinel-filled y buffer stays as it was
    ybuf = torch.full_like(y_ref, float("nan"))
    sent = bits(ybuf).clone()
    none, out2 = ops.affine_act_conv_out(t2, sc[0], sh[0], s, sc[1], sh[1], wpack, bias, 3, want_y=False)
    torch.cuda.synchronize()
    assert none is None and same_bits(out2, out_ref)
    assert torch.equal(bits(ybuf), sent)
    # independent: fp32 accumulation of 64 products and a bias, on the bf16 operands
    yq = y_ref.double().cpu().view(n, h * w, 64)
    wq = d["wt"].view(3, 64).to(BF).double()
    ref = torch.einsum("npc,oc->nop", yq, wq) + d["bias"].double().view(1, 3, 1)
    mag = torch.einsum("npc,oc->nop", yq.abs(), wq.abs()) + d["bias"].double().abs().view(1, 3, 1)
    err = (out.double().cpu().view(n, 3, h * w) - ref).abs()
    bound = 65 * 2.0 ** -24 * mag
    print("used %.3f of the fp32 accumulation bound" % float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


def _bn_args(dev, shape):
    n, h, w = shape
    return dict(t0=rnd(n, h, w, 64, seed=11).to(BF).to(dev), t1=rnd(n, h, w, 64, seed=12).to(BF).to(dev),
             dy=rnd(n, 3, h, w, seed=13).to(dev), wt=(rnd(3, 64, seed=14) / 8.0).to(dev),
             aff_s=(rnd(2, 64, seed=15) * 0.7).to(dev), aff_b=(rnd(2, 64, seed=16) * 0.3).to(dev),
             mean=[(rnd(64, seed=17 + i) * 0.2).to(dev) for i in range(2)],
             inv=[(rnd(64, seed=19 + i).abs() + 0.5).to(dev) for i in range(2)])


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 8, 8), (2, 33, 31)], ids=["3x5x7", "2x8x8", "2x33x31"])
def test_bnred_without_the_stored_output(dev, shape):
    """(2, 33, 31): P = 2046 in 32 workgroups of 64 pixels, the last with 62
    (the p + 32 < pe pair loop's tail).  The partial slabs, the column-reduce
    workspace behind them, the BN partial rows, dw and db: the same bits as
    rr_conv_out_bwd_bnred given the stored block output."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc
    n, h, w = shape
    P = n * h * w
    L = rr.lib()
    st = ops.stream()
    a = _bn_args(dev, shape)
    x = ops.affine_act(a["t0"], a["aff_s"][0], a["aff_b"][0], res=a["t1"], res_scale=a["aff_s"][1],
                       res_shift=a["aff_b"][1], relu=True)
    desc = BnBwdDesc(ops.rr_dtype(BF), P, 64, 4, 2, 0, 0, None, None, 0, None, None)
    blocks = L.rr_bn_bwd_blocks(C.byref(desc))
    need = int(L.rr_conv_out_bwd_bnred_workspace(P, 64, 3))
    got = []
    for rec in (False, True):
        ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
        part = torch.full((blocks * 64 * 3 + 16,), float("nan"), device=dev)
        dw = torch.full((3, 64), float("nan"), device=dev)
        db = torch.full((3,), float("nan"), device=dev)
        tail = [a["t0"].data_ptr(), a["mean"][0].data_ptr(), a["inv"][0].data_ptr(), a["t1"].data_ptr(),
                a["mean"][1].data_ptr(), a["inv"][1].data_ptr(), dw.data_ptr(), db.data_ptr(), part.data_ptr(),
                ws.data_ptr(), need, st]
        if rec:
            L.check(L.rr_conv_out_bwd_bnred_rec(n, h, w, 3, C.byref(desc), a["dy"].data_ptr(), a["wt"].data_ptr(),
                                                a["aff_s"].data_ptr(), a["aff_b"].data_ptr(), *tail),
                    "rr_conv_out_bwd_bnred_rec")
        else:
            L.check(L.rr_conv_out_bwd_bnred(C.byref(desc), n, h, w, 3, a["dy"].data_ptr(), x.data_ptr(),
                                            a["wt"].data_ptr(), *tail), "rr_conv_out_bwd_bnred")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all()) and bool(torch.isnan(part[blocks * 64 * 3:]).all())
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(part[:blocks * 64 * 3]).all())
        got.append((ws, part, dw, db))
    for u, v, what in zip(got[0], got[1], ("workspace", "bn partials", "dw", "db")):
        assert same_bits(u, v), what


@pytest.mark.parametrize("alpha", [0.25, 0.0, -0.1], ids=["a0.25", "a0", "a-0.1"])
@pytest.mark.parametrize("shape", [(2, 8, 8), (3, 6, 8), (2, 16, 24), (1, 24, 40)],
                         ids=["2x8x8", "3x6x8", "2x16x24", "1x24x40"])
def test_first_conv_wgrad_act_from_the_pack(dev, shape, alpha):
    """rr_conv_in_wgrad_act_rec == rr_conv_in_wgrad_act fed the pre-activation
    rr_conv_in_mfma writes, bitwise: dw, db, dalpha and the whole workspace
    (partial slabs + column reduce).  (3, 6, 8): P = 144, the last 64-pixel
    step holds 16 pixels and a step straddles two images; (2, 16, 24): P = 768
    in two workgroups of 384 pixels (6 whole steps each); (1, 24, 40): P = 960
    in ranges of 512 and 448 pixels, split in the middle of a row of the image,
    so the second range's first patch rows reach back across the split."""
    import roadrestore as rr
    from roadrestore import ops
    n, h, w = shape
    L = rr.lib()
    st = ops.stream()
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(21)).to(dev)
    wt = (rnd(64, 3, 3, 3, seed=22) / 3.0).to(dev)
    b = (rnd(64, seed=23) * 0.2).to(dev)
    al = torch.tensor([alpha], device=dev)
    dy = rnd(n, h, w, 64, seed=24).to(BF).to(dev)
    wpack = ops.pack_conv_in(wt, b, BF)
    assert wpack.numel() == 64 * 32
    y, pre = ops.first_conv_fwd(x, wt, b, BF, wpack, act=2, alpha=al, want_pre=True)
    y2, none = ops.first_conv_fwd(x, wt, b, BF, wpack, act=2, alpha=al, want_pre=False)
    assert none is None and same_bits(y, y2)
    assert float((pre > 0).float().mean()) > 0.2 and float((pre < 0).float().mean()) > 0.2
    need = int(L.rr_conv_in_wgrad_act_workspace(n, h, w))
    got = []
    for rec in (False, True):
        ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
        dw = torch.full((64, 27), float("nan"), device=dev)
        db = torch.full((64,), float("nan"), device=dev)
        da = torch.full((1,), float("nan"), device=dev)
        fn = L.rr_conv_in_wgrad_act_rec if rec else L.rr_conv_in_wgrad_act
        L.check(fn(n, h, w, x.data_ptr(), dy.data_ptr(), (wpack if rec else pre).data_ptr(), 2, al.data_ptr(),
                   dw.data_ptr(), db.data_ptr(), da.data_ptr(), ws.data_ptr(), need, st), "wgrad_act rec=%d" % rec)
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all())
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()) and bool(torch.isfinite(da).all())
        got.append((ws, dw, db, da))
    for u, v, what in zip(got[0], got[1], ("workspace", "dw", "db", "dalpha")):
        assert same_bits(u, v), what
    assert float(got[0][1].abs().max()) > 0


def test_new_entry_points_reject_without_launching(dev):
    """fp32, C != 64 and cout > 4 (cout != 3 for the backward) are
    RR_EUNSUPPORTED, an unknown dtype RR_EINVAL; no output byte is written."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import RR_BF16, RR_F32, BnBwdDesc
    L = rr.lib()
    st = ops.stream()
    n, h, w = 2, 4, 4
    P = n * h * w
    buf = torch.zeros(P * 128 * 4, dtype=torch.uint8, device=dev)      # any input: large enough for every case
    coef = torch.zeros(256, device=dev)
    y = torch.full((P * 128,), float("nan"), device=dev)
    out = torch.full((P * 8,), float("nan"), device=dev)
    db = torch.full((4,), float("nan"), device=dev)

    def fwd(dtype=RR_BF16, Cc=64, cout=3):
        return L.rr_affine_act_conv_out(dtype, n, h, w, Cc, cout, buf.data_ptr(), coef.data_ptr(), coef.data_ptr(),
                                        buf.data_ptr(), coef.data_ptr(), coef.data_ptr(), buf.data_ptr(),
                                        coef.data_ptr(), y.data_ptr(), out.data_ptr(), st)
    assert fwd(dtype=RR_F32) == RR_EUNSUPPORTED
    assert fwd(Cc=32) == RR_EUNSUPPORTED
    assert fwd(Cc=128) == RR_EUNSUPPORTED
    assert fwd(cout=5) == RR_EUNSUPPORTED
    assert fwd(dtype=7) == RR_EINVAL

    need = int(L.rr_conv_out_bwd_bnred_workspace(P, 128, 4))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)

    def bwd(dtype=RR_BF16, Cc=64, cout=3):
        d = BnBwdDesc(dtype, P, Cc, 4, 2, 0, 0, None, None, 0, None, None)
        return L.rr_conv_out_bwd_bnred_rec(n, h, w, cout, C.byref(d), buf.data_ptr(), coef.data_ptr(), coef.data_ptr(),
                                           coef.data_ptr(), buf.data_ptr(), coef.data_ptr(), coef.data_ptr(),
                                           buf.data_ptr(), coef.data_ptr(), coef.data_ptr(), out.data_ptr(),
                                           db.data_ptr(), y.data_ptr(), ws.data_ptr(), need, st)
    assert bwd(dtype=RR_F32) == RR_EUNSUPPORTED
    assert bwd(Cc=128) == RR_EUNSUPPORTED
    assert bwd(cout=4) == RR_EUNSUPPORTED
    assert bwd(dtype=7) == RR_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(db).all())
    assert bool((ws == 0xA5).all())
    assert fwd() == 0 and bwd() == 0                                    # the control: the same calls, taken
    torch.cuda.synchronize()


def _train_step(dev, dt, shape, on, monkeypatch):
    import roadrestore as rr
    from roadrestore import engine
    from roadrestore.optim import flatten_parameters
    monkeypatch.setattr(engine, "_RECOMPUTE_TAIL", on)
    monkeypatch.setattr(engine, "_RECOMPUTE_FIRST", on)
    g = torch.Generator(device=dev).manual_seed(11)
    clean = torch.rand(shape, generator=g, device=dev)
    bad = (clean * 0.6 + 0.3).clamp(0, 1)
    torch.manual_seed(7)
    m = rr.ResUNet().to(dev)
    m.compute_dtype = dt
    m.train()
    flatten_parameters(m)
    seen = {}
    inner = m._rr_forward

    def spy(x, need_bwd):
        out, S = inner(x, need_bwd=need_bwd)
        seen["S"] = S
        return out, S
    m._rr_forward = spy
    out = m(bad)
    loss = rr.L1Loss()(out, clean)
    loss.backward()
    torch.cuda.synchronize()
    r = {"out": out.detach().clone(), "loss": loss.detach().clone()}
    r.update({"grad " + k: p.grad.detach().clone() for k, p in m.named_parameters()})
    r.update({"buf " + k: v.detach().clone() for k, v in m.named_buffers()})
    return r, seen["S"]


@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (3, 3, 24, 40), (2, 3, 64, 64)], ids=["3x16x16", "3x24x40", "2x64x64"])
def test_resunet_train_step_is_bitwise_the_stored_path(dev, shape, monkeypatch):
    """Output, loss, every gradient and the running statistics of a bf16 train
    step with both recomputes on == with both off, and with them on the forward
    state holds neither dec1's block output nor the first conv's pre-activation."""
    on, S_on = _train_step(dev, BF, shape, True, monkeypatch)
    off, S_off = _train_step(dev, BF, shape, False, monkeypatch)
    assert S_on.dec1.tail_rec and S_on.dec1.out is None and S_on.d1 is None
    assert S_on.e1_rec and S_on.e1pre is None and S_on.e1pack is not None
    assert not S_off.dec1.tail_rec and S_off.dec1.out is not None
    assert not S_off.e1_rec and S_off.e1pre is not None
    assert set(on) == set(off) and len(on) > 100
    bad = [k for k in on if not same_bits(on[k], off[k])]
    assert not bad, bad


def test_resunet_fp32_keeps_the_stored_path(dev, monkeypatch):
    """fp32 is not taken by the new kernels: the engine stores the block output
    and runs today's passes with the key on."""
    r, S = _train_step(dev, F32, (2, 3, 16, 16), True, monkeypatch)
    assert not S.dec1.tail_rec and S.dec1.out is not None and S.d1 is not None
    assert not S.e1_rec and S.e1pre is not None
    assert all(bool(torch.isfinite(v).all()) for v in r.values())
