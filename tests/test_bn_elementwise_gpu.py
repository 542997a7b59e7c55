"""Per-element parity for the rest of csrc/bn.hip and the fused final-conv
tail of csrc/conv_out.hip: rr_bn_bwd_reduce / _reduce_gm / _finalize / _apply
in every mask kind, with one and two BatchNorms, in train and eval mode, on
the 8-channel and the 4-channel kernels and at the edges of the shared reduce
skeleton; rr_conv_out_bwd_bnred -> rr_bn_bwd_finalize ->
rr_bn_bwd_apply_convout; rr_affine_act, rr_affine_act_pool, rr_channel_sum and
rr_bn_stats.

The discipline of tests/test_fused_elementwise_gpu.py: the C ABI called
directly, inputs inside NaN bands, every output and workspace inside sentinel
bands with a NaN interior, fp64 CPU references of dtype-exact operands computed
once per shape, every element inside a derived bound of tests/parity.py
(bn_bwd_bounds, affine_res_bound, affine_pool_bounds, colsum_bound,
colstats_bound, convout_tail_bounds).  No norms.  tests/test_parity_cpu.py
holds the self-tests of those bounds.  Each test prints the share of each
bound it used ("used ...": run with -s)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import parity
from test_fused_elementwise_gpu import _check, _in, _report

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
ALPHA = float(torch.tensor(0.23))          # the slope as the kernels read it: exact in fp32
RR_EINVAL, RR_EUNSUPPORTED, RR_EWORKSPACE = -1, -2, -4
EW_GRID_ROWS = 2048 * 256 * 8              # elements of one grid-stride trip of the 8-channel elementwise kernels


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _q(t, dt):
    return t.to(dt).float()


def _dn(dt):
    return "bf16" if dt == BF else "f32"


def _skeleton(P):
    """(blocks, rows per block) of the reduce skeleton: min(1024, ceil(P / 64)) workgroups"""
    blocks = max(1, min(1024, -(-P // 64)))
    return blocks, -(-P // blocks)


def _out(shape, dt, dev):
    return parity.guarded(tuple(shape), dt, dev)


def _ptr(v):
    return None if v is None else v.data_ptr()


def _slab(part, blocks, cols, P, what):
    """the partial rows [blocks, cols] on the host: every element written,
    every workgroup past the last row (r0 >= P) left an exactly zero row"""
    slab = part[:blocks * cols].view(blocks, cols).double().cpu()
    assert bool(torch.isfinite(slab).all()), f"{what}: {int((~torch.isfinite(slab)).sum())} partial elements unwritten / NaN"
    rpb = _skeleton(P)[1]
    first_empty = -(-P // rpb)
    assert bool((slab[first_empty:] == 0).all()), f"{what}: an empty workgroup's partial row is not zero"
    return slab, blocks - first_empty


# ---------------------------------------------------------------------------
# the BN backward: reduce -> finalize -> apply

_BN = {}


def _bn_data(dt, shape):
    """operands exact in ``dt`` for every mask kind of one [n, h, w, c]; the
    kind-2 PReLU input and the kinds-4/5 t0 hold no sign-ambiguous element
    (at most 1 % moved by the fix-up: asserted)"""
    key = (dt, shape)
    if key not in _BN:
        n, h, w, c = shape
        d = {"g": _q(rnd(n, h, w, c, seed=61), dt), "aux": _q(F.relu(rnd(n, h, w, c, seed=62)), dt),
             "t1": _q(rnd(n, h, w, c, seed=64) - 0.2, dt),
             "mean": [rnd(c, seed=65) * 0.1 + 0.3, rnd(c, seed=66) * 0.1 - 0.2],
             "inv": [rnd(c, seed=67).abs() + 0.5, rnd(c, seed=68).abs() + 0.5],
             "gamma": [rnd(c, seed=69).abs() + 0.5, rnd(c, seed=70).abs() + 0.5]}
        beta = [rnd(c, seed=71) * 0.2, rnd(c, seed=72) * 0.2]
        d["s"] = [d["gamma"][i] * d["inv"][i] for i in range(2)]
        d["b"] = [beta[i] - d["mean"][i] * d["s"][i] for i in range(2)]
        t0 = _q(rnd(n, h, w, c, seed=63) * 2 + 0.3, dt)
        d["t0"] = t0
        tp = _q(rnd(n, h, w, c, seed=73), dt)
        d["taux"] = parity.make_sign_unambiguous(tp, d["s"][0], d["b"][0], dt)
        d["t0u"], moved = parity.make_sign_unambiguous2(t0, d["s"][0], d["b"][0], d["t1"], d["s"][1], d["b"][1], dt)
        assert int(parity.sign_ambiguous(d["taux"], d["s"][0], d["b"][0]).sum()) == 0
        assert int(parity.sign_ambiguous2(d["t0u"], d["s"][0], d["b"][0], d["t1"], d["s"][1], d["b"][1]).sum()) == 0
        assert float((d["taux"] != tp).double().mean()) <= 0.01 and float(moved.double().mean()) <= 0.01
        if h % 2 == 0 and w % 2 == 0:
            d["pdy"] = _q(rnd(n, h // 2, w // 2, c, seed=74), dt)
            d["pidx"] = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=torch.Generator().manual_seed(75),
                                      dtype=torch.uint8)
        _BN[key] = d
    return _BN[key]


_BOUNDS = {}


def _bn_bounds(dt, shape, kind, nbn, eval_mode=False, sum_stored=False):
    key = (dt, shape, kind, nbn, eval_mode, sum_stored)
    if key not in _BOUNDS:
        d = _bn_data(dt, shape)
        n, h, w, c = shape
        g, e_g = d["g"].double(), None
        t0 = d["t0u"] if kind >= 4 else d["t0"]
        slope = u = du = None
        if kind in (3, 5):
            g = g + parity.unpooled(d["pdy"], d["pidx"], h, w)
            e_g = parity.U * g.abs()                         # one fp32 add
        if kind == 0:
            keep = torch.ones(shape, dtype=torch.bool)
        elif kind in (1, 3):
            keep = d["aux"] > 0
        elif kind == 2:
            ts = d["taux"].double() * d["s"][0].double()
            u = ts + d["b"][0].double()
            du = 2.0 * parity.U * (ts.abs() + d["b"][0].double().abs())
            keep, slope = u > 0, ALPHA
        else:
            keep = ((t0.double() * d["s"][0].double() + d["b"][0].double())
                    + (d["t1"].double() * d["s"][1].double() + d["b"][1].double())) > 0
        _BOUNDS[key] = parity.bn_bwd_bounds(g, keep, [t0, d["t1"]][:nbn], d["mean"][:nbn], d["inv"][:nbn], d["gamma"][:nbn],
                                            dt, eval_mode=eval_mode, slope=slope, u=u, du=du, e_g=e_g,
                                            n_sum=_skeleton(n * h * w)[1], sum_stored=sum_stored)
    return _BOUNDS[key]


def _run_bn_bwd(dev, dt, shape, kind, nbn, gm_out=False, reduce_gm=False, eval_mode=False, dbias=False):
    """one reduce -> finalize -> apply of a mask kind; every output asserted"""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc
    n, h, w, c = shape
    P = n * h * w
    L = rr.lib()
    s = ops.stream()
    d = _bn_data(dt, shape)
    b = _bn_bounds(dt, shape, kind, nbn, eval_mode, sum_stored=reduce_gm)
    what = "bn_bwd k%d nbn%d %s %s%s%s%s" % (kind, nbn, "x".join(map(str, shape)), _dn(dt), " gm_out" if gm_out else "",
                                            " reduce_gm" if reduce_gm else "", " eval" if eval_mode else "")
    used = {}
    g = _in(d["g"], dt, dev)
    aux = _in(d["taux"] if kind == 2 else d["aux"], dt, dev) if kind in (1, 2, 3) else None
    t0 = _in(d["t0u"] if kind >= 4 else d["t0"], dt, dev)
    t1 = _in(d["t1"], dt, dev) if nbn == 2 else None
    mean = [_in(x, F32, dev) for x in d["mean"][:nbn]] + [None]
    inv = [_in(x, F32, dev) for x in d["inv"][:nbn]] + [None]
    gamma = [_in(x, F32, dev) for x in d["gamma"][:nbn]] + [None]
    aff_s = aff_b = alpha = None
    if kind == 2:
        aff_s, aff_b, alpha = _in(d["s"][0], F32, dev), _in(d["b"][0], F32, dev), _in(torch.tensor([ALPHA]), F32, dev)
    elif kind >= 4:
        aff_s, aff_b = _in(torch.cat(d["s"]), F32, dev), _in(torch.cat(d["b"]), F32, dev)
    pdy = pidx = None
    if kind in (3, 5):
        pdy = _in(d["pdy"], dt, dev)
        pidx = parity.guarded(tuple(d["pidx"].shape), torch.uint8, dev, fill=d["pidx"])[1]
    dbs = [_out((c,), F32, dev) for _ in range(nbn)] if dbias else []
    desc = BnBwdDesc(ops.rr_dtype(dt), P, c, kind, nbn, h if pdy is not None else 0, w if pdy is not None else 0,
                     _ptr(pdy), _ptr(pidx), int(eval_mode), dbs[0][1].data_ptr() if dbias else None,
                     dbs[1][1].data_ptr() if dbias and nbn == 2 else None)
    blocks, rpb = _skeleton(P)
    assert L.rr_bn_bwd_blocks(C.byref(desc)) == blocks

    # reduce
    pbuf, part = parity.guarded((blocks * c * 3 + blocks,), F32, dev, band=1024)
    gbuf = gm = None
    if reduce_gm:
        gbuf, gm = _out(shape, dt, dev)
        L.check(L.rr_bn_bwd_reduce_gm(C.byref(desc), g.data_ptr(), aux.data_ptr(), t0.data_ptr(), mean[0].data_ptr(),
                                      inv[0].data_ptr(), part.data_ptr(), gm.data_ptr(), s), "rr_bn_bwd_reduce_gm")
    else:
        L.check(L.rr_bn_bwd_reduce(C.byref(desc), g.data_ptr(), _ptr(aux), _ptr(aff_s), _ptr(aff_b), _ptr(alpha),
                                   t0.data_ptr(), mean[0].data_ptr(), inv[0].data_ptr(), _ptr(t1), _ptr(mean[1]),
                                   _ptr(inv[1]), part.data_ptr(), s), "rr_bn_bwd_reduce")
    torch.cuda.synchronize()
    assert parity.intact(pbuf), "a store outside the partials"
    slab, empty = _slab(part, blocks, c * 3, P, what)
    slab = slab.view(blocks, c, 3)
    if nbn == 1:
        assert bool((slab[..., 2] == 0).all())
    _check(slab.sum(0), b["sums"], what + " sums", used)
    if kind == 2:
        aslab = part[blocks * c * 3:].double().cpu()
        assert bool(torch.isfinite(aslab).all()) and bool((aslab[blocks - empty:] == 0).all())
        _check(aslab.sum(), b["alpha"], what + " alpha", used)
    if reduce_gm:
        assert parity.intact(gbuf), "a store outside gm"
        _check(gm, b["gm"], what + " gm", used)

    # finalize
    names = [k + str(i) for i in range(nbn) for k in ("dgamma", "dbeta")] + (["dalpha"] if kind == 2 else [])
    small = {k: _out((1,) if k == "dalpha" else (c,), F32, dev) for k in names}
    cbuf, coef = _out((c * 6,), F32, dev)

    def sp(k):
        return small[k][1].data_ptr() if k in small else None
    L.check(L.rr_bn_bwd_finalize(C.byref(desc), part.data_ptr(), gamma[0].data_ptr(), inv[0].data_ptr(), _ptr(gamma[1]),
                                 _ptr(inv[1]), sp("dgamma0"), sp("dbeta0"), sp("dgamma1"), sp("dbeta1"), sp("dalpha"),
                                 coef.data_ptr(), s), "rr_bn_bwd_finalize")
    torch.cuda.synchronize()
    assert parity.intact(cbuf) and all(parity.intact(v[0]) for v in small.values()) and all(parity.intact(v[0]) for v in dbs)
    for k in names:
        _check(small[k][1].reshape(b[k][0].shape), b[k], what + " " + k, used)
    cf = coef.view(c, 2, 3)[:, :nbn]
    _check(cf, (b["coef"][0][:, :nbn], b["coef"][1][:, :nbn]), what + " coef", used)
    if eval_mode:
        assert bool((cf[..., 1:] == 0).all())                # count = +inf: the batch terms are exactly zero
    for i, (buf, v) in enumerate(dbs):
        _check(v, b["dbias%d" % i], what + " dbias%d" % i, used)

    # apply
    dts = [_out(shape, dt, dev) for _ in range(nbn)]
    if reduce_gm:       # the apply reads the stored gm alone: mask kind 0
        d0 = BnBwdDesc(ops.rr_dtype(dt), P, c, 0, 1, 0, 0, None, None, int(eval_mode), None, None)
        L.check(L.rr_bn_bwd_apply(C.byref(d0), gm.data_ptr(), None, None, None, None, t0.data_ptr(), mean[0].data_ptr(),
                                  inv[0].data_ptr(), None, None, None, coef.data_ptr(), dts[0][1].data_ptr(), None, None,
                                  s), "rr_bn_bwd_apply")
    else:
        if gm_out:
            gbuf, gm = _out(shape, dt, dev)
        L.check(L.rr_bn_bwd_apply(C.byref(desc), g.data_ptr(), _ptr(aux), _ptr(aff_s), _ptr(aff_b), _ptr(alpha),
                                  t0.data_ptr(), mean[0].data_ptr(), inv[0].data_ptr(), _ptr(t1), _ptr(mean[1]),
                                  _ptr(inv[1]), coef.data_ptr(), dts[0][1].data_ptr(),
                                  dts[1][1].data_ptr() if nbn == 2 else None, _ptr(gm) if gm_out else None, s),
                "rr_bn_bwd_apply")
    torch.cuda.synchronize()
    assert all(parity.intact(v[0]) for v in dts) and parity.intact(cbuf) and (gbuf is None or parity.intact(gbuf))
    if gm_out:
        _check(gm, b["gm"], what + " gm", used)
    for i in range(nbn):
        _check(dts[i][1], b["dt%d" % i], what + " dt%d" % i, used)
    _report(what, used)


@DTYPES
@pytest.mark.parametrize("c", [8, 64, 1024])
def test_bn_bwd_8ch_elementwise(dev, c, dt):
    """The 8-channel kernels at P = 2 * 8 * 12 = 192 rows (3 workgroups): C = 8
    is one thread per row (R = 256 thread rows, more than the 64 rows of a
    workgroup), C = 1024 two thread rows and the rcs[4 * 1024] LDS limit of
    the recomputed mask.  Kinds 0, 1, 2 with one and two BNs, gm_out on and
    off; kind 4; kind 5 (the pool backward); rr_bn_bwd_reduce_gm for kind 1."""
    shape = (2, 8, 12, c)
    for kind in (0, 1, 2):
        for nbn in (1, 2):
            for gm_out in (False, True):
                _run_bn_bwd(dev, dt, shape, kind, nbn, gm_out=gm_out)
    _run_bn_bwd(dev, dt, shape, 4, 2)
    _run_bn_bwd(dev, dt, shape, 5, 2)
    _run_bn_bwd(dev, dt, shape, 1, 1, reduce_gm=True)


@DTYPES
@pytest.mark.parametrize("P", [5, 85 * 3 + 1])
@pytest.mark.parametrize("c", [12, 192])
def test_bn_bwd_4ch_elementwise(dev, c, P, dt):
    """The 4-channel fallback kernels (C not 8 * 2^k): C = 12 has R = 85 thread
    rows and one idle thread, C = 192 has R = 5 and 16 idle threads (the tr < R
    guard).  P = 5 is fewer rows than either R; P = 85 * 3 + 1 = 256 is four
    workgroups of 64 rows: 13 passes of the 5 thread rows at C = 192, with one
    row left for the last pass."""
    shape = (1, 1, P, c)
    for kind in (0, 1, 2):
        for nbn in (1, 2):
            _run_bn_bwd(dev, dt, shape, kind, nbn, gm_out=(nbn == 1))


@pytest.mark.parametrize("c,kind,want", [(12, 3, RR_EUNSUPPORTED), (12, 4, RR_EUNSUPPORTED), (12, 5, RR_EUNSUPPORTED),
                                         (192, 3, RR_EUNSUPPORTED), (192, 4, RR_EUNSUPPORTED), (192, 5, RR_EUNSUPPORTED),
                                         (6, 0, RR_EINVAL), (6, 1, RR_EINVAL)])
def test_bn_bwd_4ch_rejections(dev, c, kind, want):
    """the pool-backward and recomputed-mask kinds exist as 8-channel kernels
    only; C % 4 != 0 is invalid.  Every pointer is valid, so the channel count
    is the only reason; nothing is launched or written."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc
    L = rr.lib()
    n, h, w = 1, 2, 4
    P = n * h * w
    x = torch.zeros(P * 192 * 2, device=dev)
    idx = torch.zeros(P * 192, dtype=torch.uint8, device=dev)
    obuf, out = _out((P * 192 * 3,), F32, dev)
    p = x.data_ptr()
    desc = BnBwdDesc(ops.rr_dtype(F32), P, c, kind, 2, h, w, p, idx.data_ptr(), 0, None, None)
    s = ops.stream()
    o = out.data_ptr()
    assert L.rr_bn_bwd_reduce(C.byref(desc), p, p, p, p, p, p, p, p, p, p, p, o, s) == want
    assert L.rr_bn_bwd_finalize(C.byref(desc), p, p, p, p, p, o, o, o, o, None, o, s) == want
    assert L.rr_bn_bwd_apply(C.byref(desc), p, p, p, p, p, p, p, p, p, p, p, p, o, o, None, s) == want
    torch.cuda.synchronize()
    assert parity.intact(obuf) and bool(torch.isnan(out).all())


@DTYPES
@pytest.mark.parametrize("P", [1, 63, 65, 4481, 65600])
def test_bn_bwd_block_edges(dev, P, dt):
    """The edges of the reduce skeleton, C = 64 kind 1 with two BNs and C = 8
    kind 2: one row; one row short of and one past a 64-row workgroup; 4481 =
    71 workgroups of 64 rows, the last with 1; and 65600 > 65536, where the
    1024-workgroup cap gives 65 rows each, workgroup 1009 gets 15 rows and
    workgroups 1010..1023 none: their partial rows must be written as zeros
    (asserted in _slab).  65600 rows x 64 channels is also more than the 2048
    * 256 * 8 elements of one grid-stride trip of bn_bwd_apply8_kernel, so its
    last 64 rows are written by the second trip."""
    if P == 65600:
        assert P * 64 > EW_GRID_ROWS > (P - 65) * 64 and _skeleton(P) == (1024, 65) and P - 1009 * 65 == 15
    _run_bn_bwd(dev, dt, (1, 1, P, 64), 1, 2)
    _run_bn_bwd(dev, dt, (1, 1, P, 8), 2, 1, gm_out=True)


@DTYPES
@pytest.mark.parametrize("c", [64, 12])
def test_bn_bwd_eval_mode(dev, c, dt):
    """eval-mode BatchNorm (d->eval: count = +inf): dt = gamma invstd gm,
    dgamma = sum gm xhat, dbeta = sum gm, and dbias = gamma invstd sum gm
    written by the finalize -- with dbias0 / dbias1 both given and both NULL;
    the 8-channel path (C = 64) and the 4-channel one (C = 12)"""
    shape = (2, 8, 12, c)
    for nbn in (1, 2):
        for dbias in (True, False):
            _run_bn_bwd(dev, dt, shape, 1, nbn, eval_mode=True, dbias=dbias)


# ---------------------------------------------------------------------------
# rr_conv_out_bwd_bnred -> rr_bn_bwd_finalize -> rr_bn_bwd_apply_convout

def _convout_args(dev, dt, shape):
    n, h, w = shape
    d = _bn_data(dt, (n, h, w, 64))
    a = {"dy": _in(rnd(n, 3, h, w, seed=95), F32, dev), "wt": _in(rnd(3, 64, seed=96) / 8.0, F32, dev),
         "t0": _in(d["t0u"], dt, dev), "t1": _in(d["t1"], dt, dev),
         "mean": [_in(x, F32, dev) for x in d["mean"]], "inv": [_in(x, F32, dev) for x in d["inv"]],
         "gamma": [_in(x, F32, dev) for x in d["gamma"]],
         "s": [_in(x, F32, dev) for x in d["s"]], "b": [_in(x, F32, dev) for x in d["b"]],
         "aff_s": _in(torch.cat(d["s"]), F32, dev), "aff_b": _in(torch.cat(d["b"]), F32, dev)}
    return d, a


@DTYPES
@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 5, 7), (2, 33, 31), (1, 258, 256)],
                         ids=["1x2x2", "3x5x7", "2x33x31", "1x258x256"])
def test_convout_tail_elementwise(dev, shape, dt):
    """The final conv's backward fused with the BN-backward reduce of dec1's
    tail, and the apply that recomputes the conv's input grad.  (1, 2, 2): one
    partial workgroup with fewer pixels than its 32 pixel lanes; (3, 5, 7):
    several images in one workgroup, the nn * 3 + co plane indexing of the NCHW
    dy; (2, 33, 31): the p + 32 < pe pair loop and its tail in 32 workgroups;
    (1, 258, 256): P = 66048 > 65536, the last 7 workgroups without a pixel.
    The block output x is what rr_affine_act stores for the sign-unambiguous
    t0, t1, so the reduce's stored mask (x > 0) and the apply's recomputed one
    are the same tensor: asserted on the host before anything is compared."""
    import roadrestore as rr
    from roadrestore import ops
    from roadrestore._lib import BnBwdDesc
    n, h, w = shape
    P, c = n * h * w, 64
    L = rr.lib()
    s = ops.stream()
    d, a = _convout_args(dev, dt, shape)
    what = "convout tail %s %s" % ("x".join(map(str, shape)), _dn(dt))
    used = {}
    xbuf, x = _out((n, h, w, c), dt, dev)
    L.check(L.rr_affine_act(ops.rr_dtype(dt), P, c, a["t0"].data_ptr(), a["s"][0].data_ptr(), a["b"][0].data_ptr(), None,
                            a["t1"].data_ptr(), a["s"][1].data_ptr(), a["b"][1].data_ptr(), 1, x.data_ptr(), s),
            "rr_affine_act")
    torch.cuda.synchronize()
    assert parity.intact(xbuf)
    x_c = x.float().cpu()
    v = ((d["t0u"].double() * d["s"][0].double() + d["b"][0].double())
         + (d["t1"].double() * d["s"][1].double() + d["b"][1].double()))
    keep = v > 0
    assert torch.equal(x_c > 0, keep), "the stored mask differs from the recomputed one"
    _check(x, parity.affine_res_bound(d["t0u"], d["s"][0], d["b"][0], dt, res=d["t1"], rs=d["s"][1], rb=d["b"][1],
                                      relu=True), what + " x", used)
    blocks, rpb = _skeleton(P)
    b = parity.convout_tail_bounds(a["dy"].cpu(), a["wt"].cpu(), keep, [d["t0u"], d["t1"]], d["mean"], d["inv"], d["gamma"],
                                   dt, x_c, n_sum=rpb)

    desc = BnBwdDesc(ops.rr_dtype(dt), P, c, 4, 2, 0, 0, None, None, 0, None, None)
    assert L.rr_bn_bwd_blocks(C.byref(desc)) == blocks
    need = int(L.rr_conv_out_bwd_bnred_workspace(P, c, 3))
    wbuf, ws = parity.guarded((need,), torch.uint8, dev, band=4096)
    pbuf, part = parity.guarded((blocks * c * 3,), F32, dev, band=1024)
    outs = {"dw": _out((3, c), F32, dev), "db": _out((3,), F32, dev)}

    def bnred(desc_, cout=3, n_=n, nbytes=need):
        return L.rr_conv_out_bwd_bnred(C.byref(desc_), n_, h, w, cout, a["dy"].data_ptr(), x.data_ptr(), a["wt"].data_ptr(),
                                       a["t0"].data_ptr(), a["mean"][0].data_ptr(), a["inv"][0].data_ptr(),
                                       a["t1"].data_ptr(), a["mean"][1].data_ptr(), a["inv"][1].data_ptr(),
                                       outs["dw"][1].data_ptr(), outs["db"][1].data_ptr(), part.data_ptr(), ws.data_ptr(),
                                       nbytes, s)

    # the rejections first: nothing may be launched or written
    def variant(**kw):
        f = dict(dtype=ops.rr_dtype(dt), P=P, C=c, mask_kind=4, nbn=2, eval=0)
        f.update(kw)
        return BnBwdDesc(f["dtype"], f["P"], f["C"], f["mask_kind"], f["nbn"], 0, 0, None, None, f["eval"], None, None)
    assert bnred(variant(C=128)) == RR_EUNSUPPORTED
    assert bnred(desc, cout=2) == RR_EUNSUPPORTED
    assert bnred(variant(eval=1)) == RR_EINVAL
    assert bnred(variant(mask_kind=1)) == RR_EINVAL
    assert bnred(variant(P=P + 1)) == RR_EINVAL
    assert bnred(desc, nbytes=need - 1) == RR_EWORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(outs["dw"][1]).all()) and bool((ws == 0xFF).all())

    L.check(bnred(desc), "rr_conv_out_bwd_bnred")
    torch.cuda.synchronize()
    assert parity.intact(pbuf) and parity.intact(wbuf) and all(parity.intact(v[0]) for v in outs.values())
    slab, _ = _slab(part, blocks, c * 3, P, what)
    _check(slab.view(blocks, c, 3).sum(0), b["sums"], what + " sums", used)
    _check(outs["dw"][1], b["dw"], what + " dw", used)
    _check(outs["db"][1], b["db"], what + " db", used)

    names = ["dgamma0", "dbeta0", "dgamma1", "dbeta1"]
    small = {k: _out((c,), F32, dev) for k in names}
    cbuf, coef = _out((c * 6,), F32, dev)
    L.check(L.rr_bn_bwd_finalize(C.byref(desc), part.data_ptr(), a["gamma"][0].data_ptr(), a["inv"][0].data_ptr(),
                                 a["gamma"][1].data_ptr(), a["inv"][1].data_ptr(), small["dgamma0"][1].data_ptr(),
                                 small["dbeta0"][1].data_ptr(), small["dgamma1"][1].data_ptr(),
                                 small["dbeta1"][1].data_ptr(), None, coef.data_ptr(), s), "rr_bn_bwd_finalize")
    dts = [_out((n, h, w, c), dt, dev) for _ in range(2)]
    L.check(L.rr_bn_bwd_apply_convout(C.byref(desc), h, w, a["dy"].data_ptr(), a["wt"].data_ptr(), 3, a["aff_s"].data_ptr(),
                                      a["aff_b"].data_ptr(), a["t0"].data_ptr(), a["mean"][0].data_ptr(),
                                      a["inv"][0].data_ptr(), a["t1"].data_ptr(), a["mean"][1].data_ptr(),
                                      a["inv"][1].data_ptr(), coef.data_ptr(), dts[0][1].data_ptr(), dts[1][1].data_ptr(),
                                      s), "rr_bn_bwd_apply_convout")
    torch.cuda.synchronize()
    assert parity.intact(cbuf) and all(parity.intact(v[0]) for v in small.values()) and all(parity.intact(v[0]) for v in dts)
    for k in names:
        _check(small[k][1], b[k], what + " " + k, used)
    _check(coef.view(c, 2, 3), b["coef"], what + " coef", used)
    for i in range(2):
        _check(dts[i][1], b["dt%d" % i], what + " dt%d" % i, used)
    _report(what, used)


# ---------------------------------------------------------------------------
# rr_affine_act

def _affine_data(dt, shape, seed=0):
    """x and res on several scales (randn 2^(1.5 randn)), shifts near +1 (see
    tests/test_parity_cpu.py::_affine_case: the tie rule of the pooled index);
    x fixed up so that the PReLU decision (``xp``) and the sign before the
    ReLU with a plain (``xr``) and an affine (``xa``) residual are unambiguous"""
    c = shape[-1]
    d = {"s": rnd(c, seed=81).abs() + 0.5, "b": rnd(c, seed=82) * 0.2 + 1.0,
         "rs": rnd(c, seed=83).abs() + 0.5, "rb": rnd(c, seed=84) * 0.2 + 1.0}
    x = _q(rnd(*shape, seed=85 + seed) * torch.exp2(rnd(*shape, seed=87 + seed) * 1.5), dt)
    d["res"] = _q(rnd(*shape, seed=86 + seed) * torch.exp2(rnd(*shape, seed=88 + seed) * 1.5), dt)
    one, zero = torch.ones(c), torch.zeros(c)
    d["xp"] = parity.make_sign_unambiguous(x, d["s"], d["b"], dt)
    d["xr"], m1 = parity.make_sign_unambiguous2(x, d["s"], d["b"], d["res"], one, zero, dt)
    d["xa"], m2 = parity.make_sign_unambiguous2(x, d["s"], d["b"], d["res"], d["rs"], d["rb"], dt)
    assert int(parity.sign_ambiguous(d["xp"], d["s"], d["b"]).sum()) == 0
    assert int(parity.sign_ambiguous2(d["xr"], d["s"], d["b"], d["res"], one, zero).sum()) == 0
    assert int(parity.sign_ambiguous2(d["xa"], d["s"], d["b"], d["res"], d["rs"], d["rb"]).sum()) == 0
    for moved in ((d["xp"] != x), m1, m2):
        assert float(moved.double().mean()) <= 0.01
    return d


# name: (x, PReLU, res, res affine, ReLU)
AFFINE_VARIANTS = {"plain": ("xp", False, False, False, 0), "prelu": ("xp", True, False, False, 0),
                   "res-relu": ("xr", False, True, False, 1), "res-affine-relu": ("xa", False, True, True, 1),
                   "prelu-res": ("xp", True, True, False, 0)}


def _affine_bound(d, dt, variant):
    xk, pre, res, aff, relu = AFFINE_VARIANTS[variant]
    return parity.affine_res_bound(d[xk], d["s"], d["b"], dt, alpha=ALPHA if pre else None, res=d["res"] if res else None,
                                   rs=d["rs"] if aff else None, rb=d["rb"] if aff else None, relu=bool(relu))


@DTYPES
@pytest.mark.parametrize("c,P", [(64, 1), (64, 97), (64, 65600), (12, 1), (12, 97), (1024, 1), (1024, 97)])
def test_affine_act_elementwise(dev, c, P, dt):
    """y = act(x s + b [+ res | + res rs + rb]) in its five forms on the
    8-channel kernel (C = 64; C = 1024: 128 threads per row) and the 4-channel
    one (C = 12).  P = 65600 at C = 64 is past the 2048-workgroup grid cap of
    affine_act8_kernel: the last 64 rows are a second grid-stride trip."""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    s = ops.stream()
    if P == 65600:
        assert P * c > EW_GRID_ROWS
    d = _affine_data(dt, (P, c))
    dev_t = {k: _in(d[k], dt, dev) for k in ("xp", "xr", "xa", "res")}
    vec = {k: _in(d[k], F32, dev) for k in ("s", "b", "rs", "rb")}
    al = _in(torch.tensor([ALPHA]), F32, dev)
    what = "affine_act %dx%d %s" % (P, c, _dn(dt))
    used = {}
    for name, (xk, pre, res, aff, relu) in AFFINE_VARIANTS.items():
        ybuf, y = _out((P, c), dt, dev)
        L.check(L.rr_affine_act(ops.rr_dtype(dt), P, c, dev_t[xk].data_ptr(), vec["s"].data_ptr(), vec["b"].data_ptr(),
                                al.data_ptr() if pre else None, dev_t["res"].data_ptr() if res else None,
                                vec["rs"].data_ptr() if aff else None, vec["rb"].data_ptr() if aff else None, relu,
                                y.data_ptr(), s), "rr_affine_act")
        torch.cuda.synchronize()
        assert parity.intact(ybuf), name
        _check(y, _affine_bound(d, dt, name), what + " " + name, used)
    _report(what, used)


def test_affine_act_rejections(dev):
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    x = torch.zeros(64 * 8, device=dev)
    ybuf, y = _out((64 * 8,), F32, dev)
    p, s = x.data_ptr(), ops.stream()
    f = ops.rr_dtype(F32)
    assert L.rr_affine_act(f, 8, 64, p, p, p, None, p, p, None, 1, y.data_ptr(), s) == RR_EINVAL     # rs without rb
    assert L.rr_affine_act(f, 8, 64, p, p, p, None, p, None, p, 1, y.data_ptr(), s) == RR_EINVAL     # rb without rs
    assert L.rr_affine_act(f, 8, 6, p, p, p, None, None, None, None, 0, y.data_ptr(), s) == RR_EINVAL   # C % 4
    torch.cuda.synchronize()
    assert parity.intact(ybuf) and bool(torch.isnan(y).all())


# ---------------------------------------------------------------------------
# rr_affine_act_pool

@DTYPES
@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 6, 10), (3, 8, 12)], ids=["1x2x2", "2x6x10", "3x8x12-ties"])
@pytest.mark.parametrize("c", [8, 64])
def test_affine_act_pool_elementwise(dev, c, shape, dt):
    """y, the pooled tensor and the first-max window index of the residual
    tail + MaxPool2d(2, 2), with an affine residual + ReLU and in the plain
    form.  The index is held to the first maximum of the fp64 reference
    wherever it is decided (parity.affine_pool_bounds); the undecided share is
    asserted <= 2 %.  (3, 8, 12) forces ties: in every fourth window column
    the window's second element is a bit copy of its third, which stores the
    same value -- the first of the two must win."""
    import roadrestore as rr
    from roadrestore import ops
    n, h, w = shape
    L = rr.lib()
    s = ops.stream()
    d = dict(_affine_data(dt, (n, h, w, c), seed=10))      # seeds chosen on the CPU: every case within the 2 % below
    if shape == (3, 8, 12):
        for k in ("xp", "xa", "res"):
            v = d[k].clone()
            v[:, 0::2, 1::8] = v[:, 1::2, 0::8]
            d[k] = v
        assert int(parity.sign_ambiguous2(d["xa"], d["s"], d["b"], d["res"], d["rs"], d["rb"]).sum()) == 0
    vec = {k: _in(d[k], F32, dev) for k in ("s", "b", "rs", "rb")}
    res = _in(d["res"], dt, dev)
    used = {}
    what = "affine_act_pool %s %s" % ("x".join(map(str, shape + (c,))), _dn(dt))
    for name in ("res-affine-relu", "plain"):
        xk, _, has_res, _, relu = AFFINE_VARIANTS[name]
        x = _in(d[xk], dt, dev)
        rb = _affine_bound(d, dt, name)
        prb, idx_ref, sure = parity.affine_pool_bounds(rb, (d[xk], d["res"]) if has_res else (d[xk],))
        share = 1.0 - float(sure.double().mean())
        assert share <= 0.02, f"{share:.3f} of the windows have a tie inside the bound"
        ybuf, y = _out((n, h, w, c), dt, dev)
        pbuf, yp = _out((n, h // 2, w // 2, c), dt, dev)
        ibuf, idx = parity.guarded((n, h // 2, w // 2, c), torch.uint8, dev)
        L.check(L.rr_affine_act_pool(ops.rr_dtype(dt), n, h, w, c, x.data_ptr(), vec["s"].data_ptr(), vec["b"].data_ptr(),
                                     res.data_ptr() if has_res else None, vec["rs"].data_ptr() if has_res else None,
                                     vec["rb"].data_ptr() if has_res else None, relu, y.data_ptr(), yp.data_ptr(),
                                     idx.data_ptr(), s), "rr_affine_act_pool")
        torch.cuda.synchronize()
        assert parity.intact(ybuf) and parity.intact(pbuf) and parity.intact(ibuf), name
        _check(y, rb, what + " " + name + ":y", used)
        _check(yp, prb, what + " " + name + ":pooled", used)
        idx_c = idx.cpu()
        assert bool((idx_c < 4).all()), "an index never written"
        wrong = (idx_c != idx_ref) & sure
        assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} window indices differ, first {wrong.nonzero()[:4].tolist()}"
        # the pooled value is the stored y at the index the kernel reports, whatever the tie
        win = y.float().cpu().view(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
        assert torch.equal(win.gather(-1, idx_c.long()[..., None])[..., 0], yp.float().cpu())
        assert torch.equal(win.max(-1).values, yp.float().cpu())
        if shape == (3, 8, 12):
            assert int(((idx_ref == 1) & sure)[:, :, 0::4].sum()) > 0        # forced ties that the first element wins
        used[name + ":undecided"] = share
    _report(what, used)


def test_affine_act_pool_rejections(dev):
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    x = torch.zeros(4 * 4 * 16, device=dev)
    obuf, o = _out((4 * 4 * 16,), F32, dev)
    p, q, s, f = x.data_ptr(), o.data_ptr(), ops.stream(), ops.rr_dtype(F32)
    assert L.rr_affine_act_pool(f, 1, 3, 4, 8, p, p, p, None, None, None, 1, q, q, q, s) == RR_EINVAL    # odd h
    assert L.rr_affine_act_pool(f, 1, 4, 3, 8, p, p, p, None, None, None, 1, q, q, q, s) == RR_EINVAL    # odd w
    assert L.rr_affine_act_pool(f, 1, 4, 4, 12, p, p, p, None, None, None, 1, q, q, q, s) == RR_EINVAL   # C % 8
    torch.cuda.synchronize()
    assert parity.intact(obuf) and bool(torch.isnan(o).all())


# ---------------------------------------------------------------------------
# rr_channel_sum / rr_bn_stats

@DTYPES
@pytest.mark.parametrize("P", [1, 63, 65, 4481, 65600])
@pytest.mark.parametrize("c", [12, 64, 1024])
def test_channel_sum_and_bn_stats_elementwise(dev, c, P, dt):
    """The column sums behind every conv bias grad, plain and accumulating
    into ``out``, and the (sum, sum of squares) partials of a standalone
    BatchNorm2d: C = 12 (85 thread rows, one idle thread), 64, 1024 (one thread
    row), over the block edges of the reduce skeleton; empty workgroups' partial
    rows are zero; a workspace one float short is refused."""
    import roadrestore as rr
    from roadrestore import ops
    L = rr.lib()
    s = ops.stream()
    x_c = _q(rnd(P, c, seed=91), dt)
    out0 = rnd(c, seed=92) * 5
    blocks, rpb = _skeleton(P)
    what = "colsum %dx%d %s" % (P, c, _dn(dt))
    used = {}
    x = _in(x_c, dt, dev)
    need = int(L.rr_channel_sum_workspace(P, c))
    assert need == blocks * c * 4 and L.rr_bn_stats_blocks(P) == blocks
    wbuf, ws = parity.guarded((need // 4,), F32, dev, band=1024)
    obuf, out = _out((c,), F32, dev)
    f = ops.rr_dtype(dt)
    assert L.rr_channel_sum(f, P, c, x.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), need - 4, s) == RR_EWORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(out).all())
    L.check(L.rr_channel_sum(f, P, c, x.data_ptr(), out.data_ptr(), 0, ws.data_ptr(), need, s), "rr_channel_sum")
    torch.cuda.synchronize()
    assert parity.intact(wbuf) and parity.intact(obuf)
    slab, _ = _slab(ws, blocks, c, P, what)
    cb = parity.colsum_bound(x_c, rpb)
    _check(slab.sum(0), cb, what + " partials", used)
    _check(out, cb, what + " sum", used)
    abuf, acc = parity.guarded((c,), F32, dev, fill=out0)
    ws.fill_(math.nan)
    L.check(L.rr_channel_sum(f, P, c, x.data_ptr(), acc.data_ptr(), 1, ws.data_ptr(), need, s), "rr_channel_sum")
    torch.cuda.synchronize()
    assert parity.intact(wbuf) and parity.intact(abuf)
    _check(acc, parity.colsum_bound(x_c, rpb, out0), what + " accumulated", used)
    sbuf, st = parity.guarded((blocks * c * 2,), F32, dev, band=1024)
    L.check(L.rr_bn_stats(f, P, c, x.data_ptr(), st.data_ptr(), s), "rr_bn_stats")
    torch.cuda.synchronize()
    assert parity.intact(sbuf)
    slab, _ = _slab(st, blocks, c * 2, P, what)
    _check(slab.view(blocks, c, 2).sum(0), parity.colstats_bound(x_c, rpb), what + " stats", used)
    _report(what, used)
