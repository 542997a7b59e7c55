"""Per-element parity and guard bands for every convolution family: tap-reuse
conv3r (whole-row and row-segment tiles, 4- and 8-wave workgroups), the
row-streaming stream3 (whole rows and column strips), stream1 (1x1, convT),
the LDS-halo and tiled implicit GEMM (with the image grad, c_out = 3 into NCHW
fp32: the narrow 16-column halo tile one-shot and persistent, and the tiled
kernel where it is not eligible), and the weight grads.

Every case forces its family with RR_PATH, asserts the kernel instance the
library will launch, and calls the C ABI directly on buffers of its own:
  * inputs (x1, x2, the packed weights, bias, mask, residual, alpha, dy) are
    views into NaN-banded buffers: a read past a tensor that reaches a result
    makes it NaN.  A pack is written by the library's own rr_pack_conv /
    rr_pack_convT into exactly rr_pack_conv_elems (convT: 4 co ci) elements
    and then copied between the bands, so a K tail, a c_out that is no tile
    multiple or the tap-reuse tiles behind the plain layout cannot be read
    past the pack's end unnoticed;
  * outputs (y1, y2, the pooled tensor, the statistics slab sized by
    rr_igemm_stat_blocks, the weight-grad workspace sized by
    rr_wgrad_workspace, dw) are views into sentinel-banded buffers whose
    interior starts as NaN unless the call accumulates into it: a store
    outside the tensor breaks a band, an element never written stays NaN;
  * every output element is held to the derived bound of tests/parity.py
    against an fp64 CPU reference of bf16-exact (fp32 mode: fp32) operands.
Shapes are the smallest that keep each kernel instance (found with the
host-only name query, which needs no GPU); the fp64 reference of a shape is
computed once and shared by its epilogues.  The fused calls (rr_igemm_pre,
rr_wgrad_pre, rr_igemm_bnbwd, rr_igemm_dgrad_sc, the BN backward with the pool
backward folded in) get the bands and the unwritten-element check here; every
element of theirs is held to a derived bound in
tests/test_fused_elementwise_gpu.py."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

import parity
from rrpath import set_path  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = math.nan
ALPHA = 0.17

# epilogue -> (act, accumulate, has_bias, has_mask, want_stats, out_nchw); "split" sets out_split
EPI = {
    "plain": (0, 0, 0, 0, 0, 0),
    "bias": (0, 0, 1, 0, 0, 0),
    "bias_relu": (1, 0, 1, 0, 0, 0),
    "bias_stats": (0, 0, 1, 0, 1, 0),
    "acc": (0, 1, 0, 0, 0, 0),
    "mask": (0, 0, 0, 1, 0, 0),
    "acc_mask": (0, 1, 0, 1, 0, 0),
    "split": (0, 0, 0, 0, 0, 0),
    "prelu": (2, 0, 1, 0, 0, 0),
    "res_relu": (1 | 4, 0, 1, 0, 0, 0),
    "pool": (1 | 8, 0, 1, 0, 0, 0),
    "pool_only": (1 | 8 | 16, 0, 1, 0, 0, 0),
    "nchw": (0, 0, 1, 0, 0, 1),
    "nchw_plain": (0, 0, 0, 0, 0, 1),
    "nchw_acc": (0, 1, 0, 0, 0, 1),
}
LOAD = ["plain", "bias_relu", "bias_stats", "acc", "mask", "acc_mask"]
EX = ["prelu", "res_relu", "pool", "pool_only"]
ALL = LOAD + ["split"] + EX
ALL64 = LOAD + EX     # c_out = 64: no column split (out_split is a multiple of 64 inside (0, c_out))

W4, W8 = "stream3=0,conv3r_wg=4", "stream3=0,conv3r_wg=8"
SEG, SEG4, SEG8 = "stream3=0", "stream3=0,conv3r_segwg=4", "stream3=0,conv3r_segwg=8"
S1 = "stream1_minp=1024"
TILED = "conv3r=0,stream3=0"
IMG = ["nchw_plain", "nchw_acc"]      # the image grad: 64 -> 3 into NCHW fp32, K = 576 (+ 1 accumulated into)

# (RR_PATH, dtype, mode, (n, h, w, c_in1, c_in2, c_out), kernel instance, epilogues)
# modes: 0 3x3, 1 1x1, 2 convT up (c_out = 4 * channels), 3 convT down
CASES = [
    # ---- conv3r, whole-row tiles, 4-wave workgroups
    (W4, BF, 0, (2, 64, 64, 64, 64, 64), "conv3r_kernel<64,64>", ALL64),           # two rows per wave, concat
    (W4, BF, 0, (1, 64, 64, 64, 0, 128), "conv3r_kernel<64,128>", ALL),
    (W4, BF, 0, (1, 32, 32, 128, 0, 128), "conv3r_kernel<32,128>", ALL),         # 16-row tiles inside an image
    (W4, BF, 0, (2, 32, 32, 128, 0, 256), "conv3r_kernel<32,128>", ALL),         # two column blocks
    (W4, BF, 0, (2, 32, 32, 128, 64, 64), "conv3r_kernel<32,64>", ALL64),          # concat
    (W4, BF, 0, (3, 16, 16, 128, 0, 256), "conv3r_kernel<16,128>", ALL),         # whole images, odd count
    (W4, BF, 0, (6, 8, 8, 128, 0, 128), "conv3r_kernel<8,128,32>", ALL),         # image pairs
    (W4, BF, 0, (512, 8, 8, 64, 0, 512), "conv3r_kernel<8,128>", ["plain", "bias_stats", "acc_mask", "pool"]),
    # ---- the 8-wave, one-per-CU variant
    (W8, BF, 0, (2, 64, 64, 64, 64, 64), "conv3r_kernel<64,64,32,w8>", ALL64),
    (W8, BF, 0, (1, 64, 64, 64, 0, 128), "conv3r_kernel<64,128,w8>", ALL),
    (W8, BF, 0, (1, 32, 32, 128, 0, 128), "conv3r_kernel<32,128,w8>", ALL),
    (W8, BF, 0, (2, 32, 32, 128, 64, 64), "conv3r_kernel<32,64,32,w8>", ALL64),
    (W8, BF, 0, (2, 16, 16, 128, 0, 256), "conv3r_kernel<16,128,w8>", ALL),
    (W8, BF, 0, (3, 16, 16, 128, 0, 256), "conv3r_kernel<16,128,32,w8>", ALL),
    (W8, BF, 0, (8, 8, 8, 128, 0, 128), "conv3r_kernel<8,128,w8>", ALL),
    (W8, BF, 0, (12, 8, 8, 128, 0, 128), "conv3r_kernel<8,128,32,w8>", ALL),
    # ---- conv3r row segments (any H x W)
    (SEG, BF, 0, (2, 60, 60, 64, 0, 64), "conv3r_kernel<s2,64>", ALL64),           # partial band of 16 rows
    (SEG, BF, 0, (3, 36, 52, 64, 64, 128), "conv3r_kernel<s2,128>", ALL),        # odd size, concat
    (SEG, BF, 0, (2, 15, 17, 64, 0, 128), "conv3r_kernel<s2,128,w8>", ALL),      # odd sizes, floor pool
    (SEG, BF, 0, (3, 29, 13, 128, 0, 64), "conv3r_kernel<s1,64>", ALL64),
    (SEG, BF, 0, (2, 14, 14, 64, 0, 64), "conv3r_kernel<s1,64>", ALL64),
    (SEG, BF, 0, (1, 8, 8, 64, 0, 128), "conv3r_kernel<s1,128,w8>", ALL),
    (SEG8, BF, 0, (2, 60, 60, 64, 0, 64), "conv3r_kernel<s2,64,w8>", ALL64),
    (SEG8, BF, 0, (3, 29, 13, 128, 0, 64), "conv3r_kernel<s1,64,w8>", ALL64),
    (SEG4, BF, 0, (2, 15, 17, 64, 0, 128), "conv3r_kernel<s2,128>", ALL),
    (SEG4, BF, 0, (1, 8, 8, 64, 0, 128), "conv3r_kernel<s1,128>", ALL),
    # ---- stream3: whole rows (one 256-pixel step per workgroup at the least: P >= 65536)
    ("", BF, 0, (16, 64, 64, 64, 0, 64), "stream3_kernel<64>", LOAD + EX),
    ("", BF, 0, (65, 16, 64, 64, 0, 64), "stream3_kernel<64>", ["bias_stats", "acc_mask", "res_relu"]),
    ("", BF, 0, (64, 32, 32, 64, 0, 64), "stream3_kernel<32>", LOAD + EX),
    # ---- stream3 column strips (the router takes widths that are multiples of
    # 32 only: 96 = 3 and 160 = 5 strips, neither a multiple of 64)
    ("", BF, 0, (8, 96, 96, 64, 0, 64), "stream3_kernel<s32>", ["plain", "bias_relu"] + EX),
    ("", BF, 0, (4, 104, 160, 64, 0, 64), "stream3_kernel<s32>", ["bias_relu", "res_relu", "pool"]),
    # ---- stream1: 1x1, convT up; convT down stays on the tiled kernel
    (S1, BF, 1, (4, 32, 32, 64, 0, 128), "stream1_kernel<8,2>", ["plain", "bias_relu", "acc", "split"]),
    (S1, BF, 1, (4, 32, 32, 64, 0, 128), "stream1_kernel<4,2>", ["bias_stats"]),
    (S1, BF, 1, (11, 16, 16, 64, 64, 64), "stream1_kernel<4,4>", ["plain", "bias_relu", "bias_stats", "acc", "mask"]),
    (S1, BF, 1, (8, 14, 14, 128, 0, 64), "stream1_kernel<4,4>", ["plain", "bias_relu", "bias_stats", "acc", "mask"]),
    # the 2-column-block wave tiles: K = 192 / 256 / 384
    (S1, BF, 1, (11, 16, 16, 256, 0, 128), "stream1_kernel<2,8>", ["plain", "bias_relu", "bias_stats", "acc", "split"]),
    (S1, BF, 1, (8, 14, 14, 128, 0, 96), "stream1_kernel<2,4>", ["plain", "bias_relu", "bias_stats"]),   # c_out % 64 != 0
    (S1, BF, 1, (8, 14, 14, 64, 0, 96), "stream1_kernel<2,2>", ["bias_stats"]),
    (S1, BF, 1, (8, 14, 14, 128, 64, 64), "stream1_kernel<2,6>", ["plain", "bias_relu"]),
    (S1, BF, 1, (8, 14, 14, 128, 256, 128), "stream1_kernel<2,12>", ["plain", "bias_relu", "bias_stats", "split"]),
    (S1, BF, 2, (8, 14, 14, 256, 0, 256), "stream1_kernel<2,8>", ["plain", "bias"]),
    (S1, BF, 1, (11, 16, 16, 64, 0, 3), "stream1_kernel<1,2>", ["nchw"]),
    (S1, BF, 1, (8, 14, 14, 64, 0, 3), "stream1_kernel<1,2>", ["nchw"]),
    (S1, BF, 2, (4, 32, 32, 64, 0, 256), "stream1_kernel<8,2>", ["plain", "bias", "bias_relu"]),
    (S1, BF, 2, (11, 16, 16, 128, 0, 256), "stream1_kernel<4,4>", ["plain", "bias"]),
    (S1, BF, 2, (8, 14, 14, 128, 0, 256), "stream1_kernel<4,4>", ["plain", "bias"]),
    (S1, BF, 3, (8, 14, 14, 64, 0, 128), "igemm_kernel<bf16,64,128,m3>", ["plain", "mask"]),
    (S1, BF, 3, (4, 32, 32, 64, 0, 64), "igemm_kernel<bf16,64,128,m3>", ["plain", "mask"]),
    # ---- LDS-halo and tiled implicit GEMM
    (TILED, F32, 0, (1, 5, 7, 128, 0, 64), "igemm_kernel<f32,64,128,m0>", LOAD + ["nchw"]),
    (TILED, F32, 0, (2, 8, 8, 64, 0, 64), "igemm_kernel<f32,64,128,m0>", LOAD + ["nchw"]),
    (TILED, F32, 0, (2, 16, 16, 64, 0, 256), "igemm_kernel<f32,64,128,m0>", LOAD + ["split", "nchw"]),
    (TILED, BF, 0, (1, 5, 7, 128, 0, 64), "igemm_kernel<bf16,64,128,m0>", LOAD + ["nchw"]),
    (TILED, BF, 0, (2, 8, 8, 64, 0, 64), "igemm_kernel<bf16,64,128,m0>", LOAD + ["nchw"]),
    (TILED, BF, 0, (2, 16, 16, 64, 0, 256), "igemm3_halo_kernel<64,16>", LOAD + ["split"]),
    (TILED + ",igemm_halo=0", BF, 0, (2, 16, 16, 64, 0, 256), "igemm_kernel<bf16,64,128,m0>", ["bias_stats", "acc_mask"]),
    # ---- the image grad (c_out = 3, NCHW fp32): the narrow 16-column halo tile, one launch of one 256-pixel
    # tile per workgroup at the smallest eligible shape of each width ...
    ("", BF, 0, (4, 8, 8, 64, 0, 3), "igemm3_halo_kernel<16,8>", IMG),
    ("", BF, 0, (1, 16, 16, 64, 0, 3), "igemm3_halo_kernel<16,16>", IMG),
    ("", BF, 0, (1, 8, 32, 64, 0, 3), "igemm3_halo_kernel<16,32>", IMG),
    ("", BF, 0, (1, 8, 64, 64, 0, 3), "igemm3_halo_kernel<16,64>", IMG),
    # ... and persistent: past 512 tiles the launcher starts 512 workgroups that walk tiles b, b + 512, ... with
    # the next tile's halo held in registers (513, 516, 528, 528 tiles: workgroups with 2 tiles and with 1);
    # 65 x 64 x 64 = 1040 tiles: workgroups get 3 or 2.  The NaN interior catches a tile never written, the
    # accumulate form's fill one accumulated twice.
    ("", BF, 0, (2052, 8, 8, 64, 0, 3), "igemm3_halo_kernel<16,8>", IMG),
    ("", BF, 0, (516, 16, 16, 64, 0, 3), "igemm3_halo_kernel<16,16>", IMG),
    ("", BF, 0, (132, 32, 32, 64, 0, 3), "igemm3_halo_kernel<16,32>", IMG),
    ("", BF, 0, (33, 64, 64, 64, 0, 3), "igemm3_halo_kernel<16,64>", IMG),
    ("", BF, 0, (65, 64, 64, 64, 0, 3), "igemm3_halo_kernel<16,64>", IMG),
    # the tiled kernel where the halo route is not eligible (odd sizes, a height no multiple of 8, a width of 112)
    ("", BF, 0, (1, 5, 7, 64, 0, 3), "igemm_kernel<bf16,64,128,m0>", IMG),
    ("", BF, 0, (3, 40, 16, 64, 0, 3), "igemm_kernel<bf16,64,128,m0>", IMG),
    ("", BF, 0, (1, 20, 112, 64, 0, 3), "igemm_kernel<bf16,64,128,m0>", IMG),
]


def _id(case, epi=None):
    path, dt, mode, shape, name, _ = case
    s = "%dx%dx%d_%d+%d-%d" % shape
    tag = f"{name}-m{mode}-{'bf16' if dt == BF else 'f32'}-{s}"
    return tag if epi is None else f"{tag}-{epi}"


PARAMS = [pytest.param(c, e, id=_id(c, e)) for c in CASES for e in c[5]]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _q(t, dt):
    """operands exact in the compute dtype, as fp32 on the CPU"""
    return t.to(dt).float()


def _to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _apply_path(monkeypatch, path):
    monkeypatch.setenv("RR_PATH", "")
    for item in path.split(","):
        if item:
            k, v = item.split("=")
            set_path(monkeypatch, k, v)


_DATA = {}


def _data(dt, mode, shape):
    """CPU operands of a shape and the (ref, A) terms of its plain sum, once"""
    key = (dt, mode, shape)
    if key in _DATA:
        return _DATA[key]
    n, h, w, c1, c2, co = shape
    cin = c1 + c2
    d = {}
    if mode in (0, 1):
        k = 3 if mode == 0 else 1
        d["x"] = _q(rnd(n, cin, h, w, seed=1), dt)
        d["wt"] = _q(rnd(co, cin, k, k, seed=2) / (k * cin ** 0.5), dt)
        d["K"] = k * k * cin
        d["terms"] = parity.conv_terms(d["x"], d["wt"], k // 2)
        d["oshape"] = (n, h, w, co)
    elif mode == 2:                          # convT up: co = 4 * channels
        ct = co // 4
        d["x"] = _q(rnd(n, cin, h, w, seed=1), dt)
        d["wt"] = _q(rnd(cin, ct, 2, 2, seed=2) / cin ** 0.5, dt)
        d["oshape"] = (n, 2 * h, 2 * w, ct)
    else:                                    # convT down: x1 = the fine-grid gradient, c1 channels
        d["x"] = _q(rnd(n, c1, 2 * h, 2 * w, seed=1), dt)
        d["wt"] = _q(rnd(co, c1, 2, 2, seed=2) / (2 * c1 ** 0.5), dt)
        d["oshape"] = (n, h, w, co)
    oc = d["oshape"][3]
    d["b"] = rnd(oc, seed=3)
    d["y0"] = _q(rnd(d["oshape"][0], oc, d["oshape"][1], d["oshape"][2], seed=4), dt)
    d["m"] = _q(rnd(d["oshape"][0], oc, d["oshape"][1], d["oshape"][2], seed=5), dt)
    _DATA[key] = d
    return d


def _bound(d, dt, mode, epi):
    """(ref64, bound64) NHWC of the full-size output of epilogue ``epi``"""
    act, acc, bias, msk, _, nchw = EPI[epi]
    b = d["b"] if bias else None
    odt = F32 if nchw else dt
    if mode == 2:
        rb = parity.convt_up_bound(d["x"], d["wt"], b, odt)
    elif mode == 3:
        rb = parity.convt_down_bound(d["x"], d["wt"], odt)
    else:
        extra = d["y0"] if (acc or act & 4) else None        # accumulated into / residual
        rb = parity.epilogue_bound(d["terms"], d["K"], b, odt, extra=extra)
    if act & 3 == 1:
        rb = parity.relu(rb)
    elif act & 3 == 2:
        rb = parity.prelu(rb, ALPHA)
    if msk:
        rb = parity.masked(rb, d["m"])
    return rb


def _in(t, dt, dev):
    """an input tensor inside NaN bands"""
    return parity.guarded(tuple(t.shape), dt, dev, fill=t.to(dt), poison=NAN)[1]


def _pack(wp):
    """a weight pack (the library's own, of the size it reports) copied between NaN bands"""
    return parity.guarded(tuple(wp.shape), wp.dtype, wp.device, fill=wp, band=8192, poison=NAN)[1]


@pytest.mark.parametrize("case,epi", PARAMS)
def test_conv_elementwise(dev, case, epi, monkeypatch):
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import IgemmDesc
    path, dt, mode, shape, name, _ = case
    _apply_path(monkeypatch, path)
    n, h, w, c1, c2, co = shape
    act, acc, bias, msk, stats, nchw = EPI[epi]
    split = co // 2 if epi == "split" else 0
    L = rr.lib()
    desc = IgemmDesc(ops.rr_dtype(dt), mode, n, h, w, c1, c2, co, split, act, acc, bias, msk, stats, nchw)
    assert ops.igemm_kernel_name(desc) == name
    d = _data(dt, mode, shape)
    oshape = d["oshape"]
    on, oh, ow, oc = oshape

    # packed weights and inputs
    if mode in (0, 1):
        wp, _ = ops.pack_conv(d["wt"].to(dev), dt)
    elif mode == 2:
        wp, _ = ops.pack_convT(d["wt"].to(dev), dt)
    else:
        _, wp = ops.pack_convT(d["wt"].to(dev), dt)
    if mode in (0, 1):
        assert wp.numel() == ops.pack_elems(dt, co, c1 + c2, 3 if mode == 0 else 1)
    else:
        assert wp.numel() == 4 * d["wt"].shape[0] * d["wt"].shape[1]
    wp = _pack(wp)
    xh = _to_nhwc(d["x"])
    x1 = _in(xh[..., :c1], dt, dev)
    x2 = _in(xh[..., c1:], dt, dev) if c2 else None
    bd = None
    if bias:
        bd = _in(ops.bias_tile4(d["b"].to(dev)).cpu() if mode == 2 else d["b"], F32, dev)
    md = _in(_to_nhwc(d["m"]), dt, dev) if msk else None
    rd = _in(_to_nhwc(d["y0"]), dt, dev) if act & 4 else None
    ad = _in(torch.tensor([ALPHA]), F32, dev) if act & 3 == 2 else None

    # outputs
    outs = {}
    y0h = _to_nhwc(d["y0"])
    if split:
        outs["y1"] = parity.guarded((on, oh, ow, split), dt, dev)
        outs["y2"] = parity.guarded((on, oh, ow, oc - split), dt, dev)
    elif nchw:
        outs["y1"] = parity.guarded((on, oc, oh, ow), F32, dev, fill=d["y0"] if acc else None)
    elif not act & 16:
        outs["y1"] = parity.guarded(oshape, dt, dev, fill=y0h if acc else None)
    if act & 8:
        outs["pool"] = parity.guarded((on, oh // 2, ow // 2, oc), dt, dev)
    if stats:
        blocks = L.rr_igemm_stat_blocks(C.byref(desc))
        assert blocks > 0
        outs["stats"] = parity.guarded((blocks, co, 2), F32, dev)

    def p(key):
        return outs[key][1].data_ptr() if key in outs else None

    def q(t):
        return None if t is None else t.data_ptr()

    if act > 1:
        L.check(L.rr_igemm_ex(C.byref(desc), q(x1), q(x2), q(wp), q(bd), q(ad), q(rd), p("y1"), p("pool"),
                              q(md), p("stats"), ops.stream()), "rr_igemm_ex")
    else:
        L.check(L.rr_igemm(C.byref(desc), q(x1), q(x2), q(wp), q(bd), p("y1"), p("y2"), q(md), p("stats"),
                           ops.stream()), "rr_igemm")
    torch.cuda.synchronize()

    for key, (buf, _) in outs.items():
        assert parity.intact(buf), f"{key}: a store outside the tensor"
    what = _id(case, epi)
    ref, bound = _bound(d, dt, mode, epi)
    if split:
        parity.assert_within(outs["y1"][1], ref[..., :split].contiguous(), bound[..., :split].contiguous(), what + " y1")
        parity.assert_within(outs["y2"][1], ref[..., split:].contiguous(), bound[..., split:].contiguous(), what + " y2")
    elif "y1" in outs:
        parity.assert_within(outs["y1"][1], ref, bound, what, nchw=bool(nchw))
        if epi in IMG and os.environ.get("RR_PARITY_REPORT"):     # a measurement for DESIGN section 4's table, never asserted
            print("RATIO %s %s %.3g" % (name, epi, parity.worst_ratio(outs["y1"][1].permute(0, 2, 3, 1), ref, bound)))
    if act & 8:
        yp = outs["pool"][1]
        parity.assert_within(yp, *parity.pooled((ref, bound)), what + " pooled")
        if "y1" in outs:            # the stronger statement where the full output exists
            full = outs["y1"][1].float().permute(0, 3, 1, 2)
            assert torch.equal(yp.float().permute(0, 3, 1, 2), F.max_pool2d(full, 2))
    if stats:
        got = outs["stats"][1].double().sum(0).cpu()
        parity.assert_within(got, *parity.stats_bound(d["terms"], d["K"]), what + " statistics [c, (sum, sumsq)]")


# ---------------------------------------------------------------------------
# conv + ReLU + pool in one pass (rr_igemm_pool): the pooled tensor and the
# window index guarded

POOL_CASES = [
    ("", (16, 64, 64, 64, 0, 64), 1, 1, "stream3_kernel<64,pool>"),
    ("", (16, 64, 64, 64, 0, 64), 0, 1, "stream3_kernel<64,pool>"),
    ("", (64, 32, 32, 64, 0, 64), 1, 0, "stream3_kernel<32,pool>"),
    ("", (8, 96, 96, 64, 0, 64), 1, 0, "stream3_kernel<s32,pool>"),
    ("", (2, 15, 17, 64, 0, 128), 1, 0, "conv3r_kernel<s2,128,w8>"),
    ("stream3=0", (1, 32, 32, 128, 0, 128), 1, 1, "conv3r_kernel<32,128>"),
]


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "%s-%dx%dx%d-b%d-i%d" % ((c[4],) + c[1][:3] + c[2:4]))
def test_igemm_pool_elementwise(dev, case, monkeypatch):
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import IgemmDesc
    path, shape, bias, with_idx, name = case
    _apply_path(monkeypatch, path)
    n, h, w, c1, c2, co = shape
    L = rr.lib()
    desc = IgemmDesc(ops.rr_dtype(BF), 0, n, h, w, c1, c2, co, 0, 1, 0, bias, 0, 0, 0)
    assert L.rr_igemm_pool_kernel_name(C.byref(desc), with_idx).decode() == name
    d = _data(BF, 0, shape)
    wp = _pack(ops.pack_conv(d["wt"].to(dev), BF)[0])
    x1 = _in(_to_nhwc(d["x"]), BF, dev)
    bd = _in(d["b"], F32, dev) if bias else None
    pbuf, yp = parity.guarded((n, h // 2, w // 2, co), BF, dev)
    ibuf, idx = parity.guarded((n, h // 2, w // 2, co), torch.uint8, dev) if with_idx else (None, None)
    L.check(L.rr_igemm_pool(C.byref(desc), x1.data_ptr(), None, wp.data_ptr(), bd.data_ptr() if bias else None,
                            yp.data_ptr(), idx.data_ptr() if with_idx else None, ops.stream()), "rr_igemm_pool")
    torch.cuda.synchronize()
    assert parity.intact(pbuf) and (ibuf is None or parity.intact(ibuf))
    rb = parity.relu(parity.epilogue_bound(d["terms"], d["K"], d["b"] if bias else None, BF))
    parity.assert_within(yp, *parity.pooled(rb), name + " pooled")
    if with_idx:
        assert int(idx.max()) <= 3                      # every index written (the interior starts as 0xFF)


# ---------------------------------------------------------------------------
# weight grads: rr_wgrad, and rr_wgrad_partial + rr_wgrad_reduce, workspace guarded

# The bound 2 K u A grows with K = n h w.  At the swgrad shapes K = 32768, so it
# allows about 3.9e-3 A: a whole image missing from one element of dW would still
# pass (tests/test_parity_cpu.py shows the effect at K = 7200).  Those cases
# contribute mainly the guard bands and the unwritten-element check; the norm
# tests of tests/test_swgrad_gpu.py remain the sharper numeric check there.
# (RR_PATH, dtype, k, (n, h, w, c_in, c_out), kernel instance)
WGRAD_CASES = [
    ("", BF, 3, (3, 12, 10, 128, 64), "wgrad_kernel<bf16,64,128,m0>"),
    ("", BF, 3, (1, 16, 16, 64, 128), "wgrad3_halo_kernel<16>"),
    ("", BF, 3, (1, 64, 64, 64, 64), "wgrad3_halo_kernel<64>"),
    ("", BF, 3, (8, 64, 64, 64, 64), "swgrad_kernel<64>"),
    ("", BF, 3, (32, 32, 32, 64, 64), "swgrad_kernel<32>"),
    ("", F32, 3, (3, 12, 10, 128, 64), "wgrad_kernel<f32,64,128,m0>"),
    ("", F32, 3, (1, 16, 16, 64, 128), "wgrad_kernel<f32,128,64,m0>"),
    ("", BF, 1, (3, 12, 10, 128, 64), "wgrad_kernel<bf16,64,128,m1>"),
    ("", BF, 1, (1, 64, 64, 64, 64), "wgrad_kernel<bf16,64,64,m1>"),
    ("", F32, 1, (1, 16, 16, 64, 128), "wgrad_kernel<f32,128,64,m1>"),
    ("swgrad=0", BF, 3, (8, 64, 64, 64, 64), "wgrad3_halo_kernel<64>"),
    ("swgrad=0,wgrad_halo=0", BF, 3, (1, 16, 16, 64, 128), "wgrad_kernel<bf16,128,64,m0>"),
    ("swgrad=0,wgrad_halo=0", BF, 3, (1, 64, 64, 64, 64), "wgrad_kernel<bf16,64,64,m0>"),
]
_WDATA = {}


def _wdata(dt, k, shape):
    key = (dt, k, shape)
    if key not in _WDATA:
        n, h, w, ci, co = shape
        x = _q(rnd(n, ci, h, w, seed=11), dt)
        dy = _q(rnd(n, co, h, w, seed=12), dt)
        dw0 = rnd(co, ci, k, k, seed=13)
        _WDATA[key] = (x, dy, dw0, parity.wgrad_bound(x, dy, k), parity.wgrad_bound(x, dy, k, dw0=dw0))
    return _WDATA[key]


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("case", WGRAD_CASES,
                         ids=lambda c: "%s-%s-k%d-%s" % (c[4], c[0] or "default", c[2], "x".join(map(str, c[3]))))
def test_wgrad_elementwise(dev, case, acc, monkeypatch):
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import WgradDesc
    path, dt, k, shape, name = case
    _apply_path(monkeypatch, path)
    n, h, w, ci, co = shape
    L = rr.lib()
    desc = WgradDesc(ops.rr_dtype(dt), 0 if k == 3 else 1, n, h, w, ci, 0, co, acc)
    assert ops.wgrad_kernel_name(desc) == name
    x, dy, dw0, rb_write, rb_acc = _wdata(dt, k, shape)
    ref, bound = rb_acc if acc else rb_write
    xd = _in(_to_nhwc(x), dt, dev)
    gd = _in(_to_nhwc(dy), dt, dev)
    need = int(L.rr_wgrad_workspace(C.byref(desc)))
    for two_calls in (False, True):
        wbuf, dw = parity.guarded((co, ci, k, k), F32, dev, fill=dw0 if acc else None)
        # the band starts exactly where the library said the workspace ends
        sbuf, ws = parity.guarded((max(need, 16),), torch.uint8, dev, band=4096)
        if two_calls:
            L.check(L.rr_wgrad_partial(C.byref(desc), gd.data_ptr(), xd.data_ptr(), None, ws.data_ptr(), need,
                                       ops.stream()), "rr_wgrad_partial")
            L.check(L.rr_wgrad_reduce(C.byref(desc), ws.data_ptr(), need, dw.data_ptr(), ops.stream()),
                    "rr_wgrad_reduce")
        else:
            L.check(L.rr_wgrad(C.byref(desc), gd.data_ptr(), xd.data_ptr(), None, dw.data_ptr(), ws.data_ptr(),
                               need, ops.stream()), "rr_wgrad")
        torch.cuda.synchronize()
        assert parity.intact(wbuf), "a store outside dw"
        assert parity.intact(sbuf), "a store outside the workspace"
        parity.assert_within(dw, ref, bound, f"{name} {'partial + reduce' if two_calls else 'rr_wgrad'} acc={acc}")


# ---------------------------------------------------------------------------
# the fused calls: bands and the unwritten-element check (their per-element
# bounds: tests/test_fused_elementwise_gpu.py)

def _finite_and_intact(bufs, what):
    for key, (buf, view) in bufs.items():
        assert parity.intact(buf), f"{what}: a store outside {key}"
        assert bool(torch.isfinite(view.float()).all()), f"{what}: NaN / unwritten element in {key}"


@pytest.mark.parametrize("shape", [(16, 64, 64), (64, 32, 32)], ids=["16x64x64", "64x32x32"])
def test_igemm_pre_and_wgrad_pre_canary(dev, shape, monkeypatch):
    """rr_igemm_pre / rr_wgrad_pre: BN1 + PReLU folded into conv2's input"""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import IgemmDesc, WgradDesc
    monkeypatch.setenv("RR_PATH", "")
    n, h, w = shape
    L = rr.lib()
    desc = IgemmDesc(ops.rr_dtype(BF), 0, n, h, w, 64, 0, 64, 0, 0, 0, 1, 0, 1, 0)
    assert L.rr_igemm_pre_ok(C.byref(desc)) and ops.igemm_kernel_name(desc) == "stream3_kernel<%d>" % w
    d = _data(BF, 0, (n, h, w, 64, 0, 64))
    wp = _pack(ops.pack_conv(d["wt"].to(dev), BF)[0])
    t1 = _in(_to_nhwc(d["x"]), BF, dev)
    bd = _in(d["b"], F32, dev)
    sc = _in(rnd(64, seed=21).abs() + 0.5, F32, dev)
    sh = _in(rnd(64, seed=22) * 0.2, F32, dev)
    al = _in(torch.tensor([0.23]), F32, dev)
    outs = {"y": parity.guarded((n, h, w, 64), BF, dev),
            "stats": parity.guarded((L.rr_igemm_stat_blocks(C.byref(desc)), 64, 2), F32, dev)}
    L.check(L.rr_igemm_pre(C.byref(desc), t1.data_ptr(), wp.data_ptr(), bd.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                           al.data_ptr(), outs["y"][1].data_ptr(), outs["stats"][1].data_ptr(), ops.stream()),
            "rr_igemm_pre")
    torch.cuda.synchronize()
    _finite_and_intact(outs, "rr_igemm_pre")
    wd = WgradDesc(ops.rr_dtype(BF), 0, n, h, w, 64, 0, 64, 0)
    assert L.rr_wgrad_pre_ok(C.byref(wd))
    need = int(L.rr_wgrad_workspace(C.byref(wd)))
    gd = _in(_to_nhwc(d["y0"]), BF, dev)
    outs = {"dw": parity.guarded((64, 64, 3, 3), F32, dev),
            "workspace": parity.guarded((max(need, 16),), torch.uint8, dev, band=4096)}
    L.check(L.rr_wgrad_pre(C.byref(wd), gd.data_ptr(), t1.data_ptr(), sc.data_ptr(), sh.data_ptr(), al.data_ptr(),
                           outs["dw"][1].data_ptr(), outs["workspace"][1].data_ptr(), need, ops.stream()),
            "rr_wgrad_pre")
    torch.cuda.synchronize()
    assert parity.intact(outs["dw"][0]) and parity.intact(outs["workspace"][0])
    assert bool(torch.isfinite(outs["dw"][1]).all())


@pytest.mark.parametrize("path,shape,prefix", [
    ("", (16, 64, 64, 64, 64), "stream3_kernel"),
    ("stream3=0", (2, 32, 32, 128, 128), "conv3r_kernel<32"),
    ("stream3=0", (3, 29, 13, 128, 64), "conv3r_kernel<s"),
    ("conv3r=0,stream3=0", (2, 16, 16, 64, 64), "igemm"),
], ids=["stream3", "conv3r-rows", "conv3r-seg", "halo"])
def test_igemm_bnbwd_canary(dev, path, shape, prefix, monkeypatch):
    """rr_igemm_bnbwd: the dgrad with the BN / PReLU backward reduce in its
    epilogue; gm and the partial rows (rr_igemm_bnbwd_rows of them, sized by
    rr_igemm_bnbwd_workspace)"""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import IgemmDesc
    _apply_path(monkeypatch, path)
    n, h, w, cg, cc = shape
    L = rr.lib()
    desc = IgemmDesc(ops.rr_dtype(BF), 0, n, h, w, cg, 0, cc, 0, 0, 0, 0, 0, 0, 0)
    assert ops.igemm_kernel_name(desc, bnbwd=True).startswith(prefix)
    need = int(L.rr_igemm_bnbwd_workspace(C.byref(desc)))
    assert need > 0 and need % 4 == 0
    d = _data(BF, 0, (n, h, w, cg, 0, cc))
    wdg = _pack(ops.pack_conv(rnd(cg, cc, 3, 3, seed=31).div(3 * cc ** 0.5).to(dev), BF)[1])
    g2 = _in(_to_nhwc(d["x"]), BF, dev)
    t = _in(_to_nhwc(d["y0"]), BF, dev)
    vec = [_in(v, F32, dev) for v in (rnd(cc, seed=32) * 0.1, rnd(cc, seed=33).abs() + 0.5,
                                      rnd(cc, seed=34).abs() + 0.5, rnd(cc, seed=35) * 0.2)]
    al = _in(torch.tensor([0.23]), F32, dev)
    outs = {"gm": parity.guarded((n, h, w, cc), BF, dev), "partial": parity.guarded((need // 4,), F32, dev, band=1024)}
    L.check(L.rr_igemm_bnbwd(C.byref(desc), g2.data_ptr(), wdg.data_ptr(), t.data_ptr(), vec[0].data_ptr(),
                             vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(),
                             outs["gm"][1].data_ptr(), outs["partial"][1].data_ptr(), ops.stream()), "rr_igemm_bnbwd")
    torch.cuda.synchronize()
    for key, (buf, _) in outs.items():
        assert parity.intact(buf), f"a store outside {key}"
    assert bool(torch.isfinite(outs["gm"][1].float()).all())
    # partial rows [rows][c][3] (the third column unused) + alpha rows: no NaN written
    rows = L.rr_igemm_bnbwd_rows(C.byref(desc))
    assert need == (rows * cc * 3 + rows * (cc // 64)) * 4
    part = outs["partial"][1][:rows * cc * 3].view(rows, cc, 3)
    assert bool(torch.isfinite(part[..., :2]).all())


@pytest.mark.parametrize("shape", [(2, 16, 16, 64), (3, 12, 20, 128), (1, 6, 10, 256)],
                         ids=["2x16x16x64", "3x12x20x128", "1x6x10x256"])
def test_bn_bwd_pool_canary(dev, shape):
    """rr_bn_bwd_reduce / rr_bn_bwd_reduce_gm / rr_bn_bwd_apply with the 2x2
    max-pool backward folded in (mask kind 3): the pooled grad and its window
    index are read at half size beside the full-size tensors"""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc
    n, h, w, cc = shape
    L = rr.lib()
    aux_c = F.relu(rnd(n, h, w, cc, seed=51)).to(BF)
    _, idx_d = ops.maxpool2_fwd(aux_c.to(dev))
    g = _in(rnd(n, h, w, cc, seed=52), BF, dev)
    aux = _in(aux_c, BF, dev)
    t0 = _in(rnd(n, h, w, cc, seed=53) * 2 + 0.3, BF, dev)
    pdy = _in(rnd(n, h // 2, w // 2, cc, seed=54), BF, dev)
    idx = parity.guarded((n, h // 2, w // 2, cc), torch.uint8, dev, fill=idx_d)[1]
    mean = _in(rnd(cc, seed=55) * 0.1 + 0.3, F32, dev)
    inv = _in(rnd(cc, seed=56).abs() + 0.5, F32, dev)
    gamma = _in(rnd(cc, seed=57).abs() + 0.5, F32, dev)
    d = BnBwdDesc(ops.rr_dtype(BF), n * h * w, cc, 3, 1, h, w, pdy.data_ptr(), idx.data_ptr(), 0, None, None)
    blocks = L.rr_bn_bwd_blocks(C.byref(d))
    assert blocks > 0
    s = ops.stream()
    for with_gm in (True, False):
        outs = {"partial": parity.guarded((blocks * cc * 3 + blocks,), F32, dev, band=1024)}
        if with_gm:
            outs["gm"] = parity.guarded(shape, BF, dev)
            L.check(L.rr_bn_bwd_reduce_gm(C.byref(d), g.data_ptr(), aux.data_ptr(), t0.data_ptr(), mean.data_ptr(),
                                          inv.data_ptr(), outs["partial"][1].data_ptr(), outs["gm"][1].data_ptr(), s),
                    "rr_bn_bwd_reduce_gm")
        else:
            L.check(L.rr_bn_bwd_reduce(C.byref(d), g.data_ptr(), aux.data_ptr(), None, None, None, t0.data_ptr(),
                                       mean.data_ptr(), inv.data_ptr(), None, None, None,
                                       outs["partial"][1].data_ptr(), s), "rr_bn_bwd_reduce")
        torch.cuda.synchronize()
        for key, (buf, _) in outs.items():
            assert parity.intact(buf), f"a store outside {key} (gm {with_gm})"
        part = outs["partial"][1][:blocks * cc * 3].view(blocks, cc, 3)
        assert bool(torch.isfinite(part[..., :2]).all())
        if with_gm:
            assert bool(torch.isfinite(outs["gm"][1].float()).all())
    # finalize from the last partials, then the apply with the pool backward in it
    coef = parity.guarded((cc * 6,), F32, dev)
    small = {k: parity.guarded((cc,), F32, dev) for k in ("dgamma", "dbeta")}
    L.check(L.rr_bn_bwd_finalize(C.byref(d), outs["partial"][1].data_ptr(), gamma.data_ptr(), inv.data_ptr(), None,
                                 None, small["dgamma"][1].data_ptr(), small["dbeta"][1].data_ptr(), None, None, None,
                                 coef[1].data_ptr(), s), "rr_bn_bwd_finalize")
    outs = {"dt0": parity.guarded(shape, BF, dev), "gm": parity.guarded(shape, BF, dev)}
    L.check(L.rr_bn_bwd_apply(C.byref(d), g.data_ptr(), aux.data_ptr(), None, None, None, t0.data_ptr(),
                              mean.data_ptr(), inv.data_ptr(), None, None, None, coef[1].data_ptr(),
                              outs["dt0"][1].data_ptr(), None, outs["gm"][1].data_ptr(), s), "rr_bn_bwd_apply")
    torch.cuda.synchronize()
    outs.update(small)
    _finite_and_intact(outs, "rr_bn_bwd_apply (pool)")
    # coef [C][2][3]: one BN here, the second BN's slots stay unwritten
    assert parity.intact(coef[0]) and bool(torch.isfinite(coef[1].view(cc, 2, 3)[:, 0]).all())


@pytest.mark.parametrize("shape", [(16, 64, 64), (65, 16, 64), (64, 32, 32)], ids=["16x64x64", "65x16x64", "64x32x32"])
def test_igemm_dgrad_sc_canary(dev, shape, monkeypatch):
    """rr_igemm_dgrad_sc: the 3x3 dgrad + the 1x1 shortcut dgrad in one pass"""
    import roadrestore as rr
    from roadrestore import ops
    monkeypatch.setenv("RR_PATH", "")
    n, h, w = shape
    L = rr.lib()
    d = _data(BF, 0, (n, h, w, 64, 0, 64))
    dy = _in(_to_nhwc(d["x"]), BF, dev)
    dsc = _in(_to_nhwc(d["y0"]), BF, dev)
    desc = ops.dgrad_sc_desc(dy, n, h, w, 64)
    assert ops.igemm_dgrad_sc_kernel_name(desc, 64) == "stream3_kernel<%d,sc>" % w
    wdg = _pack(ops.pack_conv(d["wt"].to(dev), BF)[1])
    wsc = _pack(ops.pack_conv(_q(rnd(64, 64, 1, 1, seed=41) / 8.0, BF).to(dev), BF)[1])
    outs = {"y": parity.guarded((n, h, w, 64), BF, dev)}
    L.check(L.rr_igemm_dgrad_sc(C.byref(desc), dy.data_ptr(), wdg.data_ptr(), dsc.data_ptr(), wsc.data_ptr(), 64,
                                outs["y"][1].data_ptr(), ops.stream()), "rr_igemm_dgrad_sc")
    torch.cuda.synchronize()
    _finite_and_intact(outs, "rr_igemm_dgrad_sc")
