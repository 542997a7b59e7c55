"""Per-element parity for the fused calls of the backward half of a
ResidualBlock step: rr_igemm_bnbwd (+ rr_bn_bwd_finalize_rows), rr_igemm_pre /
rr_wgrad_pre, rr_igemm_dgrad_sc and rr_bn_bwd_reduce / _reduce_gm / _finalize
/ _apply with the 2x2 max-pool backward folded in.

The discipline of tests/test_conv_elementwise_gpu.py: the C ABI called
directly, inputs inside NaN bands, outputs inside sentinel bands with NaN
interiors, every case asserting the kernel it launches, fp64 CPU references of
bf16-exact (fp32 mode: fp32) operands, every element inside a derived bound of
tests/parity.py.  No norms.  The fp64 reference of a shape is computed once
and shared by its checks (rr_igemm_bnbwd and rr_igemm_dgrad_sc share the 3x3
dgrad of 16x64x64 and 64x32x32).  Each test prints the share of each bound it
used ("used ...": run with -s)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import parity
import route_sweep
from rrpath import set_path  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = math.nan
ALPHA = 0.23


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _q(t, dt):
    return t.to(dt).float()


def _to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _apply_path(monkeypatch, path):
    monkeypatch.setenv("RR_PATH", "")
    for item in path.split(","):
        if item:
            k, v = item.split("=")
            set_path(monkeypatch, k, v)


def _in(t, dt, dev):
    return parity.guarded(tuple(t.shape), dt, dev, fill=t.to(dt), poison=NAN)[1]


def _pack(wp):
    return parity.guarded(tuple(wp.shape), wp.dtype, wp.device, fill=wp, band=8192, poison=NAN)[1]


def _check(got, rb, what, used):
    parity.assert_within(got, rb[0], rb[1], what)
    used[what.rsplit(" ", 1)[-1]] = parity.worst_ratio(got, rb[0], rb[1])


def _report(what, used):
    print(f"used {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in used.items()))


# ---------------------------------------------------------------------------
# the dgrad operands of a shape, shared by rr_igemm_bnbwd and rr_igemm_dgrad_sc

_DGRAD = {}


def _dgrad(dt, mode, shape):
    """dy [n, cg, h, w], the conv weight W [cg, cc, k, k] whose dgrad pack the
    call reads, and the (ref, A) terms of g = conv_transpose(dy, W): a K = k k
    cg term sum per element of g [n, h, w, cc]"""
    key = (dt, mode, shape)
    if key not in _DGRAD:
        n, h, w, cg, cc = shape
        k = 3 if mode == 0 else 1
        dy = _q(rnd(n, cg, h, w, seed=1), dt)
        W = _q(rnd(cg, cc, k, k, seed=31) / (k * cc ** 0.5), dt)
        weq = W.transpose(0, 1).flip(2, 3).contiguous()            # the same sum as a plain conv
        _DGRAD[key] = {"dy": dy, "W": W, "K": k * k * cg, "terms": parity.conv_terms(dy, weq, k // 2)}
    return _DGRAD[key]


# ---------------------------------------------------------------------------
# rr_igemm_bnbwd + rr_bn_bwd_finalize_rows

# (RR_PATH, dtype, mode, (n, h, w, c_in1 = dy's channels, c_out), the kernel
# rr_igemm_bnbwd launches, the plain call's kernel): each the smallest shape
# that keeps its instance.  In the last three the plain call takes a kernel
# the fused call has no instance of, with other partial rows (256 / 512 / 64
# against 528 / 4 / 528): the slabs follow rr_igemm_bnbwd_rows.
BNBWD_CASES = [
    ("", BF, 0, (16, 64, 64, 64, 64), "stream3_kernel<64>", "stream3_kernel<64>"),
    ("", BF, 0, (64, 32, 32, 64, 64), "stream3_kernel<32>", "stream3_kernel<32>"),
    ("stream3=0", BF, 0, (2, 32, 32, 128, 128), "conv3r_kernel<32,128>", "conv3r_kernel<32,128>"),
    ("stream3=0", BF, 0, (3, 29, 13, 128, 64), "conv3r_kernel<s1,64>", "conv3r_kernel<s1,64>"),
    ("conv3r=0,stream3=0", BF, 0, (2, 16, 16, 64, 64), "igemm3_halo_kernel<64,16>", "igemm3_halo_kernel<64,16>"),
    ("", F32, 0, (2, 16, 16, 64, 64), "igemm_kernel<f32,64,128,m0>", "igemm_kernel<f32,64,128,m0>"),
    ("", BF, 1, (2, 16, 16, 64, 64), "igemm_kernel<bf16,64,128,m1>", "igemm_kernel<bf16,64,128,m1>"),
    ("", BF, 0, (4, 176, 96, 64, 64), "conv3r_kernel<s2,64>", "stream3_kernel<s32>"),
    ("stream1_minp=256", BF, 1, (2, 16, 16, 64, 64), "igemm_kernel<bf16,64,128,m1>", "stream1_kernel<4,2>"),
    ("stream1_minp=256", BF, 1, (264, 16, 16, 256, 256), "igemm_kernel<bf16,128,128,m1>", "stream1_kernel<2,8>"),
]
_BN = {}


def _bn_data(dt, mode, shape):
    """t (no sign-ambiguous element), the BN constants and the bounds"""
    key = (dt, mode, shape)
    if key not in _BN:
        n, h, w, cg, cc = shape
        d = dict(_dgrad(dt, mode, shape))
        d["mean"] = rnd(cc, seed=32) * 0.1
        d["inv"] = rnd(cc, seed=33).abs() + 0.5
        gamma, beta = rnd(cc, seed=34).abs() + 0.5, rnd(cc, seed=35) * 0.2
        d["gamma"] = gamma
        d["aff_s"] = gamma * d["inv"]
        d["aff_b"] = beta - d["mean"] * d["aff_s"]
        d["t"] = parity.make_sign_unambiguous(_q(rnd(n, h, w, cc, seed=4), dt), d["aff_s"], d["aff_b"], dt)
        d["bounds"] = parity.bnbwd_bounds(d["terms"], d["K"], d["t"], d["mean"], d["inv"], d["aff_s"], d["aff_b"],
                                          ALPHA, dt)
        _BN[key] = d
    return _BN[key]


def _slab_bytes(rows, cc):
    return (rows * cc * 3 + rows * (cc // 64)) * 4


@pytest.mark.parametrize("case", BNBWD_CASES,
                         ids=lambda c: "%s-%s-m%d-%s-%s" % (c[4], c[0] or "default", c[2], "bf16" if c[1] == BF else "f32",
                                                            "x".join(map(str, c[3]))))
def test_igemm_bnbwd_elementwise(dev, case, monkeypatch):
    """gm per element (the dgrad's bound through the PReLU mask of u's sign),
    the partial slab's column sums over exactly rr_igemm_bnbwd_rows rows and
    the alpha partials against their fp64 sums, every slab element written,
    then dgamma / dbeta / dalpha of rr_bn_bwd_finalize_rows.  The partial view
    is sized by rr_igemm_bnbwd_workspace and banded by the larger of the plain
    and the fused route's slabs (both from the host queries), so no build
    stores outside the allocation: an overrun breaks a band."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc, IgemmDesc
    path, dt, mode, shape, name, plain_name = case
    _apply_path(monkeypatch, path)
    n, h, w, cg, cc = shape
    L = rr.lib()
    desc = IgemmDesc(ops.rr_dtype(dt), mode, n, h, w, cg, 0, cc, 0, 0, 0, 0, 0, 0, 0)
    assert ops.igemm_kernel_name(desc, bnbwd=True) == name and ops.igemm_kernel_name(desc) == plain_name
    rows = L.rr_igemm_bnbwd_rows(C.byref(desc))
    need = int(L.rr_igemm_bnbwd_workspace(C.byref(desc)))
    launched, _, fused_name, plain_rows = route_sweep.launched_bnbwd_rows(desc, path)
    assert fused_name == name and rows == launched > 0 and need == _slab_bytes(rows, cc)
    band = -(-max(_slab_bytes(plain_rows, cc), need) // 256) * 64      # floats, a multiple of 256 bytes
    d = _bn_data(dt, mode, shape)
    assert int(parity.sign_ambiguous(d["t"], d["aff_s"], d["aff_b"]).sum()) == 0      # before any launch
    what = f"{name} {'x'.join(map(str, shape))}"

    wdg = _pack(ops.pack_conv(d["W"].to(dev), dt)[1])
    dy = _in(_to_nhwc(d["dy"]), dt, dev)
    t = _in(d["t"], dt, dev)
    vec = [_in(d[k], F32, dev) for k in ("mean", "inv", "aff_s", "aff_b")]
    al = _in(torch.tensor([ALPHA]), F32, dev)
    gbuf, gm = parity.guarded((n, h, w, cc), dt, dev)
    pbuf, part = parity.guarded((need // 4,), F32, dev, band=band)
    L.check(L.rr_igemm_bnbwd(C.byref(desc), dy.data_ptr(), wdg.data_ptr(), t.data_ptr(), vec[0].data_ptr(),
                             vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(),
                             gm.data_ptr(), part.data_ptr(), ops.stream()), "rr_igemm_bnbwd")
    torch.cuda.synchronize()
    assert parity.intact(gbuf), "a store outside gm"
    assert parity.intact(pbuf), "a store outside the partial slabs"
    # every element of all rows: the two sums, the unused third column, every alpha slot
    assert bool(torch.isfinite(part).all()), f"{int((~torch.isfinite(part)).sum())} slab elements unwritten / NaN"
    used = {}
    b = d["bounds"]
    _check(gm, b["gm"], what + " gm", used)
    slab = part[:rows * cc * 3].view(rows, cc, 3).double().cpu()
    aslab = part[rows * cc * 3:].double().cpu()
    assert aslab.numel() == rows * (cc // 64)
    assert bool((slab[..., 2] == 0).all())
    _check(slab.sum(0)[:, :2], b["sums"], what + " sums", used)
    _check(aslab.sum(), b["alpha"], what + " alpha", used)

    # finalize from the slab
    bd = BnBwdDesc(ops.rr_dtype(dt), n * h * w, cc, 0, 1)
    wsn = int(L.rr_bn_bwd_finalize_rows_workspace(cc, rows))
    outs = {k: parity.guarded((m,), F32, dev) for k, m in (("dgamma", cc), ("dbeta", cc), ("dalpha", 1), ("coef", cc * 6))}
    ws = parity.guarded((max(wsn, 16),), torch.uint8, dev, band=4096)
    gam = _in(d["gamma"], F32, dev)
    L.check(L.rr_bn_bwd_finalize_rows(C.byref(bd), rows, part.data_ptr(), rows * (cc // 64),
                                      part.data_ptr() + rows * cc * 3 * 4, gam.data_ptr(), vec[1].data_ptr(),
                                      outs["dgamma"][1].data_ptr(), outs["dbeta"][1].data_ptr(),
                                      outs["dalpha"][1].data_ptr(), outs["coef"][1].data_ptr(), ws[1].data_ptr(), wsn,
                                      ops.stream()), "rr_bn_bwd_finalize_rows")
    torch.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert parity.intact(buf), f"a store outside {k}"
    assert parity.intact(ws[0])
    sums, sums_b = b["sums"]
    _check(outs["dbeta"][1], parity.cast32((sums[:, 0], sums_b[:, 0])), what + " dbeta", used)
    _check(outs["dgamma"][1], parity.cast32((sums[:, 1], sums_b[:, 1])), what + " dgamma", used)
    _check(outs["dalpha"][1].reshape(()), parity.cast32(b["alpha"]), what + " dalpha", used)
    # coef [c][2][3]: one BN, (gamma invstd, mean gm, mean gm xhat); the second BN's slots stay unwritten
    assert bool(torch.isfinite(outs["coef"][1].view(cc, 2, 3)[:, 0]).all())
    _report(what, used)


# ---------------------------------------------------------------------------
# rr_igemm_pre / rr_wgrad_pre

@pytest.mark.parametrize("shape", [(16, 64, 64), (64, 32, 32)], ids=["16x64x64", "64x32x32"])
def test_igemm_pre_and_wgrad_pre_elementwise(dev, shape, monkeypatch):
    """The folded input is "the bytes rr_affine_act would store".  Step 1
    holds rr_affine_act's a1 to the fp64 PReLU(t1 s + b) (half a bf16 ulp plus
    the fp32 evaluation error).  Step 2 holds rr_igemm_pre's y and statistics
    and rr_wgrad_pre's dw to the fp64 conv / weight grad of exactly those
    bytes.  tests/test_bn1_fold_gpu.py asserts fused == unfused bitwise, i.e.
    that the kernels do read those bytes: that is what makes the bytes of
    step 1 the legitimate operand of step 2's reference."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import IgemmDesc, WgradDesc
    monkeypatch.setenv("RR_PATH", "")
    n, h, w = shape
    L = rr.lib()
    desc = IgemmDesc(ops.rr_dtype(BF), 0, n, h, w, 64, 0, 64, 0, 0, 0, 1, 0, 1, 0)
    assert L.rr_igemm_pre_ok(C.byref(desc)) and ops.igemm_kernel_name(desc) == "stream3_kernel<%d>" % w
    what = "pre %dx%dx%d" % shape
    used = {}
    t1c = _q(rnd(n, h, w, 64, seed=1), BF)
    wt = _q(rnd(64, 64, 3, 3, seed=2) / 24.0, BF)
    bias = rnd(64, seed=3)
    dyc = _q(rnd(n, 64, h, w, seed=4), BF)
    scc, shc = rnd(64, seed=21).abs() + 0.5, rnd(64, seed=22) * 0.2
    t1 = _in(t1c, BF, dev)
    sc, sh, al = _in(scc, F32, dev), _in(shc, F32, dev), _in(torch.tensor([ALPHA]), F32, dev)
    s = ops.stream()

    # step 1: the bytes
    abuf, a1 = parity.guarded((n, h, w, 64), BF, dev)
    L.check(L.rr_affine_act(ops.rr_dtype(BF), n * h * w, 64, t1.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                            al.data_ptr(), None, None, None, 0, a1.data_ptr(), s), "rr_affine_act")
    torch.cuda.synchronize()
    assert parity.intact(abuf)
    _check(a1, parity.affine_prelu_bound(t1c, scc, shc, ALPHA, BF), what + " a1", used)
    a1c = _to_nchw(a1.float().cpu())

    # step 2: the conv and the weight grad of those bytes
    terms = parity.conv_terms(a1c, wt, 1)
    wp = _pack(ops.pack_conv(wt.to(dev), BF)[0])
    bd = _in(bias, F32, dev)
    blocks = L.rr_igemm_stat_blocks(C.byref(desc))
    outs = {"y": parity.guarded((n, h, w, 64), BF, dev), "stats": parity.guarded((blocks, 64, 2), F32, dev)}
    L.check(L.rr_igemm_pre(C.byref(desc), t1.data_ptr(), wp.data_ptr(), bd.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                           al.data_ptr(), outs["y"][1].data_ptr(), outs["stats"][1].data_ptr(), s), "rr_igemm_pre")
    torch.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert parity.intact(buf), f"rr_igemm_pre: a store outside {k}"
    _check(outs["y"][1], parity.epilogue_bound(terms, 576, bias, BF), what + " y", used)
    _check(outs["stats"][1].double().sum(0).cpu(), parity.stats_bound(terms, 576), what + " stats", used)

    wd = WgradDesc(ops.rr_dtype(BF), 0, n, h, w, 64, 0, 64, 0)
    assert L.rr_wgrad_pre_ok(C.byref(wd))
    need = int(L.rr_wgrad_workspace(C.byref(wd)))
    gd = _in(_to_nhwc(dyc), BF, dev)
    wbuf, dw = parity.guarded((64, 64, 3, 3), F32, dev)
    sbuf, ws = parity.guarded((max(need, 16),), torch.uint8, dev, band=4096)
    L.check(L.rr_wgrad_pre(C.byref(wd), gd.data_ptr(), t1.data_ptr(), sc.data_ptr(), sh.data_ptr(), al.data_ptr(),
                           dw.data_ptr(), ws.data_ptr(), need, s), "rr_wgrad_pre")
    torch.cuda.synchronize()
    assert parity.intact(wbuf) and parity.intact(sbuf)
    _check(dw, parity.wgrad_bound(a1c, dyc, 3), what + " dw", used)
    _report(what, used)


# ---------------------------------------------------------------------------
# rr_igemm_dgrad_sc

@pytest.mark.parametrize("shape", [(16, 64, 64), (65, 16, 64), (64, 32, 32)], ids=["16x64x64", "65x16x64", "64x32x32"])
def test_igemm_dgrad_sc_elementwise(dev, shape, monkeypatch):
    """The 3x3 dgrad plus the 1x1 dgrad of the second gradient as ONE sum of K
    = 576 + 64 products, rounded once: the kernel adds the 1x1 products into
    the same fp32 accumulators after the nine taps (csrc/stream3.hip, the SC
    branch of the step loop) and stores once."""
    import roadrestore as rr
    from roadrestore import ops
    monkeypatch.setenv("RR_PATH", "")
    n, h, w = shape
    L = rr.lib()
    d = _dgrad(BF, 0, (n, h, w, 64, 64))
    dsc_c = _q(rnd(n, 64, h, w, seed=5), BF)
    w1 = _q(rnd(64, 64, 1, 1, seed=41) / 8.0, BF)                   # the shortcut conv [c_sc, c_out, 1, 1]
    t1 = parity.conv_terms(dsc_c, w1.transpose(0, 1).contiguous(), 0)
    terms = (d["terms"][0] + t1[0], d["terms"][1] + t1[1])
    dy = _in(_to_nhwc(d["dy"]), BF, dev)
    dsc = _in(_to_nhwc(dsc_c), BF, dev)
    desc = ops.dgrad_sc_desc(dy, n, h, w, 64)
    assert ops.igemm_dgrad_sc_kernel_name(desc, 64) == "stream3_kernel<%d,sc>" % w
    wdg = _pack(ops.pack_conv(d["W"].to(dev), BF)[1])
    wsc = _pack(ops.pack_conv(w1.to(dev), BF)[1])
    ybuf, y = parity.guarded((n, h, w, 64), BF, dev)
    L.check(L.rr_igemm_dgrad_sc(C.byref(desc), dy.data_ptr(), wdg.data_ptr(), dsc.data_ptr(), wsc.data_ptr(), 64,
                                y.data_ptr(), ops.stream()), "rr_igemm_dgrad_sc")
    torch.cuda.synchronize()
    assert parity.intact(ybuf)
    used = {}
    what = "dgrad_sc %dx%dx%d" % shape
    _check(y, parity.epilogue_bound(terms, 576 + 64, None, BF), what + " y", used)
    _report(what, used)


# ---------------------------------------------------------------------------
# the BN backward behind ReLU + MaxPool2d(2, 2): mask kind 3

def _first_max_index(x):
    """window index 2 dy + dx of the first maximum of each 2x2 window of x [n, h, w, c]"""
    n, h, w, c = x.shape
    win = x.view(n, h // 2, 2, w // 2, 2, c)
    best, idx = win[:, :, 0, :, 0, :].clone(), torch.zeros(n, h // 2, w // 2, c, dtype=torch.uint8)
    for k in (1, 2, 3):
        v = win[:, :, k // 2, :, k % 2, :]
        idx = torch.where(v > best, torch.full_like(idx, k), idx)
        best = torch.maximum(best, v)
    return idx


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (3, 12, 20, 128), (1, 6, 10, 256)],
                         ids=["2x16x16x64", "3x12x20x128", "1x6x10x256"])
def test_bn_bwd_pool_elementwise(dev, shape, dt):
    """fp64 reference: the 2x2 max-pool backward through the recorded index,
    the ReLU mask, the BN backward.  rr_bn_bwd_reduce (sums of the unrounded
    gm) -> rr_bn_bwd_finalize -> rr_bn_bwd_apply (mask kind 3: gm, dt0), and
    rr_bn_bwd_reduce_gm (gm stored, the stored values summed) -> finalize ->
    apply on the stored gm (mask kind 0), as ops.bn_backward runs them."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc
    n, h, w, cc = shape
    L = rr.lib()
    aux_c = _q(F.relu(rnd(n, h, w, cc, seed=51)), dt)
    idx_c = _first_max_index(aux_c)
    g_c, t_c = _q(rnd(n, h, w, cc, seed=52), dt), _q(rnd(n, h, w, cc, seed=53) * 2 + 0.3, dt)
    pdy_c = _q(rnd(n, h // 2, w // 2, cc, seed=54), dt)
    mean_c, inv_c = rnd(cc, seed=55) * 0.1 + 0.3, rnd(cc, seed=56).abs() + 0.5
    gamma_c = rnd(cc, seed=57).abs() + 0.5
    g, aux, t0, pdy = (_in(x, dt, dev) for x in (g_c, aux_c, t_c, pdy_c))
    idx = parity.guarded((n, h // 2, w // 2, cc), torch.uint8, dev, fill=idx_c)[1]
    mean, inv, gamma = (_in(x, F32, dev) for x in (mean_c, inv_c, gamma_c))
    d = BnBwdDesc(ops.rr_dtype(dt), n * h * w, cc, 3, 1, h, w, pdy.data_ptr(), idx.data_ptr(), 0, None, None)
    d0 = BnBwdDesc(ops.rr_dtype(dt), n * h * w, cc, 0, 1, 0, 0, None, None, 0, None, None)
    blocks = L.rr_bn_bwd_blocks(C.byref(d))
    assert blocks > 0
    s = ops.stream()
    for with_gm in (False, True):
        b = parity.pool_bwd_bounds(g_c, pdy_c, idx_c, aux_c, t_c, mean_c, inv_c, gamma_c, dt, sum_stored=with_gm)
        what = "bn_bwd pool %s %s %s" % ("x".join(map(str, shape)), "bf16" if dt == BF else "f32",
                                         "reduce_gm" if with_gm else "reduce")
        used = {}
        pbuf, part = parity.guarded((blocks * cc * 3 + blocks,), F32, dev, band=1024)
        outs = {}
        if with_gm:
            outs["gm"] = parity.guarded(shape, dt, dev)
            L.check(L.rr_bn_bwd_reduce_gm(C.byref(d), g.data_ptr(), aux.data_ptr(), t0.data_ptr(), mean.data_ptr(),
                                          inv.data_ptr(), part.data_ptr(), outs["gm"][1].data_ptr(), s),
                    "rr_bn_bwd_reduce_gm")
        else:
            L.check(L.rr_bn_bwd_reduce(C.byref(d), g.data_ptr(), aux.data_ptr(), None, None, None, t0.data_ptr(),
                                       mean.data_ptr(), inv.data_ptr(), None, None, None, part.data_ptr(), s),
                    "rr_bn_bwd_reduce")
        torch.cuda.synchronize()
        assert parity.intact(pbuf), "a store outside the partials"
        slab = part[:blocks * cc * 3].view(blocks, cc, 3).double().cpu()
        assert bool(torch.isfinite(slab[..., :2]).all())
        _check(slab.sum(0)[:, :2], b["sums"], what + " sums", used)
        if with_gm:
            assert parity.intact(outs["gm"][0])
            _check(outs["gm"][1], b["gm"], what + " gm", used)
        coef = parity.guarded((cc * 6,), F32, dev)
        small = {k: parity.guarded((cc,), F32, dev) for k in ("dgamma", "dbeta")}
        L.check(L.rr_bn_bwd_finalize(C.byref(d), part.data_ptr(), gamma.data_ptr(), inv.data_ptr(), None, None,
                                     small["dgamma"][1].data_ptr(), small["dbeta"][1].data_ptr(), None, None, None,
                                     coef[1].data_ptr(), s), "rr_bn_bwd_finalize")
        dbuf, dt0 = parity.guarded(shape, dt, dev)
        if with_gm:
            L.check(L.rr_bn_bwd_apply(C.byref(d0), outs["gm"][1].data_ptr(), None, None, None, None, t0.data_ptr(),
                                      mean.data_ptr(), inv.data_ptr(), None, None, None, coef[1].data_ptr(),
                                      dt0.data_ptr(), None, None, s), "rr_bn_bwd_apply")
        else:
            outs["gm"] = parity.guarded(shape, dt, dev)
            L.check(L.rr_bn_bwd_apply(C.byref(d), g.data_ptr(), aux.data_ptr(), None, None, None, t0.data_ptr(),
                                      mean.data_ptr(), inv.data_ptr(), None, None, None, coef[1].data_ptr(),
                                      dt0.data_ptr(), None, outs["gm"][1].data_ptr(), s), "rr_bn_bwd_apply")
        torch.cuda.synchronize()
        assert parity.intact(dbuf) and parity.intact(outs["gm"][0]) and parity.intact(coef[0])
        assert all(parity.intact(v[0]) for v in small.values())
        sums, sums_b = b["sums"]
        _check(small["dbeta"][1], parity.cast32((sums[:, 0], sums_b[:, 0])), what + " dbeta", used)
        _check(small["dgamma"][1], parity.cast32((sums[:, 1], sums_b[:, 1])), what + " dgamma", used)
        if not with_gm:
            _check(outs["gm"][1], b["gm"], what + " gm", used)
        _check(dt0, b["dt"], what + " dt0", used)
        _report(what, used)
