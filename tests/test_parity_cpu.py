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


# ---------------------------------------------------------------------------
# the bounds of the fused BN / PReLU backward calls (parity.bnbwd_bounds,
# cast32, affine_prelu_bound, pool_bwd_bounds): a CPU emulation of the ideal
# kernel -- bf16 operands, fp32 accumulation in a shuffled order, the
# documented rounding points -- passes; seven broken kernels are rejected, and
# the relative L2 error the older tests assert (< 2e-2) is printed beside each

ALPHA = 0.23
BN_SHAPE = (2, 16, 16, 64, 128)      # n, h, w, dy's channels, c_out: two 64-channel groups, 4 partial rows
BN_ROWS = 4


def _bn_case():
    if "bn" not in _CACHE:
        n, h, w, cg, cc = BN_SHAPE
        d = {"dy": rnd(n, cg, h, w, seed=1).bfloat16().float(),
             "weq": (rnd(cc, cg, 3, 3, seed=31) / (3 * cg ** 0.5)).bfloat16().float(),
             "mean": rnd(cc, seed=32) * 0.1, "inv": rnd(cc, seed=33).abs() + 0.5}
        gamma, beta = rnd(cc, seed=34).abs() + 0.5, rnd(cc, seed=35) * 0.2
        d["aff_s"] = gamma * d["inv"]
        d["aff_b"] = beta - d["mean"] * d["aff_s"]
        d["t"] = parity.make_sign_unambiguous(rnd(n, h, w, cc, seed=4).bfloat16().float(), d["aff_s"], d["aff_b"])
        assert int(parity.sign_ambiguous(d["t"], d["aff_s"], d["aff_b"]).sum()) == 0
        d["bounds"] = parity.bnbwd_bounds(parity.conv_terms(d["dy"], d["weq"], 1), 9 * cg, d["t"], d["mean"], d["inv"],
                                          d["aff_s"], d["aff_b"], ALPHA, BF)
        _CACHE["bn"] = d
    return _CACHE["bn"]


def _emulate_bnbwd(d, mutation=None):
    """(gm bf16 [n, h, w, c], slab fp32 [rows, c, 3], alpha slab fp32 [rows, c / 64])
    as the ideal rr_igemm_bnbwd writes them, or with one ``mutation``"""
    n, h, w, cg, cc = BN_SHAPE
    gen = torch.Generator().manual_seed(7)
    pc = torch.randperm(cg, generator=gen)                       # the K loop in another order
    g = nhwc(F.conv2d(d["dy"][:, pc], d["weq"][:, pc], None, padding=1))      # fp32 accumulate
    t, mean = d["t"], d["mean"]
    u = t * d["aff_s"] + d["aff_b"]                              # fp32
    pos = u > 0
    if mutation == "mask from t on one tile":                    # 8 rows x 16 columns x 64 channels
        pos = pos.clone()
        pos[0, :8, :16, :64] = t[0, :8, :16, :64] > 0
    al = torch.tensor(ALPHA)
    gm = torch.where(pos, g, al * g)
    if mutation == "alpha on the wrong branch of one element":
        gm[1, 9, 5, 70] = (g if not pos[1, 9, 5, 70] else al * g)[1, 9, 5, 70]
    if mutation == "xhat from the neighbouring channel's mean":
        mean = mean.roll(1)
    tx = gm * ((t - mean) * d["inv"])
    gu = torch.where(pos, torch.zeros(()), g * u)                # fp32 products
    pp = torch.randperm(n * h * w, generator=gen)                # the pixels in another order, 4 row blocks
    slab = torch.zeros(BN_ROWS, cc, 3)
    aslab = torch.zeros(BN_ROWS, cc // 64)
    for r, rows in enumerate(pp.chunk(BN_ROWS)):
        slab[r, :, 0] = gm.reshape(-1, cc)[rows].sum(0)          # fp32 sums
        slab[r, :, 1] = tx.reshape(-1, cc)[rows].sum(0)
        aslab[r] = gu.reshape(-1, cc // 64, 64)[rows].double().sum((0, 2)).float()   # fp64 sum, one fp32 store
    if mutation == "one partial row dropped":
        slab, aslab = slab[1:], aslab[1:]
    if mutation == "one partial row duplicated":
        slab, aslab = torch.cat((slab, slab[:1])), torch.cat((aslab, aslab[:1]))
    if mutation == "the second group's alpha partial in the first group's slot":
        aslab = torch.stack((aslab[:, 1], torch.zeros(aslab.shape[0])), 1)
    return gm.to(BF), slab, aslab


BN_MUTATIONS = ["mask from t on one tile", "alpha on the wrong branch of one element", "one partial row dropped",
                "one partial row duplicated", "the second group's alpha partial in the first group's slot",
                "xhat from the neighbouring channel's mean"]


def _bn_quantities(out):
    """what the GPU test holds to a bound, from the emulation's output"""
    gm, slab, aslab = out
    sums = slab.double().sum(0)[:, :2]
    al = aslab.double().sum()
    return {"gm": gm, "sums": sums, "alpha": al, "dbeta": sums[:, 0].float(), "dgamma": sums[:, 1].float(),
            "dalpha": al.float()}


def _bn_bounds(d):
    b = d["bounds"]
    s, sb = b["sums"]
    return {"gm": b["gm"], "sums": b["sums"], "alpha": b["alpha"], "dbeta": parity.cast32((s[:, 0], sb[:, 0])),
            "dgamma": parity.cast32((s[:, 1], sb[:, 1])), "dalpha": parity.cast32(b["alpha"])}


def test_ideal_bnbwd_inside_bounds():
    d = _bn_case()
    got, bounds = _bn_quantities(_emulate_bnbwd(d)), _bn_bounds(d)
    for k, rb in bounds.items():
        parity.assert_within(got[k], rb[0], rb[1], f"ideal bnbwd {k}")
        print(f"ideal bnbwd {k}: uses {parity.worst_ratio(got[k], rb[0], rb[1]):.3g} of the bound")


@pytest.mark.parametrize("mutation", BN_MUTATIONS)
def test_broken_bnbwd_rejected(mutation):
    d = _bn_case()
    got, bounds = _bn_quantities(_emulate_bnbwd(d, mutation)), _bn_bounds(d)
    rejected = []
    for k, rb in bounds.items():
        try:
            parity.assert_within(got[k], rb[0], rb[1], k)
        except AssertionError:
            rejected.append(k)
    l2 = {k: rel(got[k], bounds[k][0]) for k in ("gm", "dgamma", "dbeta", "dalpha")}
    print(f"{mutation}: rejected by {rejected}; relative L2 " + ", ".join(f"{k} {v:.2e}" for k, v in l2.items()))
    assert rejected, mutation


def test_ideal_affine_prelu_inside_bound():
    t = rnd(2, 16, 16, 64, seed=1).bfloat16().float()
    s, b = rnd(64, seed=21).abs() + 0.5, rnd(64, seed=22) * 0.2
    u = t * s + b
    got = torch.where(u > 0, u, torch.tensor(ALPHA) * u).to(BF)
    ref, bound = parity.affine_prelu_bound(t, s, b, ALPHA, BF)
    parity.assert_within(got, ref, bound, "ideal affine + PReLU")
    print(f"ideal affine + PReLU: uses {parity.worst_ratio(got, ref, bound):.3g} of the bound")
    bad = got.clone()                     # the slope forgotten on one element (the most negative u)
    i = int(u.reshape(-1).argmin())
    bad.view(-1)[i] = u.reshape(-1)[i]
    with pytest.raises(AssertionError, match="1 of "):
        parity.assert_within(bad, ref, bound, "PReLU slope forgotten")


def _pool_case(dt):
    n, h, w, cc = 2, 16, 16, 64
    q = (lambda x: x.to(dt).float())
    aux = q(F.relu(rnd(n, h, w, cc, seed=51)))
    win = aux.view(n, h // 2, 2, w // 2, 2, cc)
    best, idx = win[:, :, 0, :, 0, :].clone(), torch.zeros(n, h // 2, w // 2, cc, dtype=torch.uint8)
    for k in (1, 2, 3):
        v = win[:, :, k // 2, :, k % 2, :]
        idx = torch.where(v > best, torch.full_like(idx, k), idx)
        best = torch.maximum(best, v)
    return {"aux": aux, "idx": idx, "g": q(rnd(n, h, w, cc, seed=52)), "t": q(rnd(n, h, w, cc, seed=53) * 2 + 0.3),
            "pdy": q(rnd(n, h // 2, w // 2, cc, seed=54)), "mean": rnd(cc, seed=55) * 0.1 + 0.3,
            "inv": rnd(cc, seed=56).abs() + 0.5, "gamma": rnd(cc, seed=57).abs() + 0.5}


def _emulate_pool_bwd(d, dt, sum_stored, wrong_window=False):
    """gm, the column sums of 4 shuffled row blocks and dt0 as the ideal
    reduce / finalize / apply compute them (fp32, the apply's folded form)"""
    n, h, w, cc = d["g"].shape
    idx = d["idx"].clone()
    if wrong_window:
        idx[1, 3, 2, 17] = (idx[1, 3, 2, 17] + 1) % 4
    up = torch.zeros_like(d["g"])
    win = up.view(n, h // 2, 2, w // 2, 2, cc)
    for k in range(4):
        win[:, :, k // 2, :, k % 2, :] = torch.where(idx == k, d["pdy"], torch.zeros(()))
    gm = torch.where(d["aux"] > 0, d["g"] + up, torch.zeros(()))          # fp32
    gms = gm.to(dt)
    src = gms.float() if sum_stored else gm
    xhat = (d["t"] - d["mean"]) * d["inv"]
    pp = torch.randperm(n * h * w, generator=torch.Generator().manual_seed(9))
    s0 = torch.stack([src.reshape(-1, cc)[r].sum(0) for r in pp.chunk(4)]).double().sum(0)
    s1 = torch.stack([(src * xhat).reshape(-1, cc)[r].sum(0) for r in pp.chunk(4)]).double().sum(0)
    P = n * h * w
    c0, c1, c2 = d["gamma"] * d["inv"], (s0 / P).float(), (s1 / P).float()
    qq = c0 * c2 * d["inv"]
    dt0 = (-qq) * d["t"] + (c0 * src + (qq * d["mean"] - c0 * c1))
    return {"gm": gms, "sums": torch.stack((s0, s1), 1), "dt": dt0.to(dt)}


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("sum_stored", [False, True], ids=["reduce", "reduce_gm"])
def test_ideal_pool_bwd_inside_bounds_and_wrong_window_rejected(dt, sum_stored):
    d = _pool_case(dt)
    bounds = parity.pool_bwd_bounds(d["g"], d["pdy"], d["idx"], d["aux"], d["t"], d["mean"], d["inv"], d["gamma"], dt,
                                    sum_stored)
    got = _emulate_pool_bwd(d, dt, sum_stored)
    for k, rb in bounds.items():
        parity.assert_within(got[k], rb[0], rb[1], f"ideal pool backward {k}")
        print(f"ideal pool backward {k}: uses {parity.worst_ratio(got[k], rb[0], rb[1]):.3g} of the bound")
    # the pooled gradient of one window routed to the next window position
    bad = _emulate_pool_bwd(d, dt, sum_stored, wrong_window=True)
    with pytest.raises(AssertionError):
        parity.assert_within(bad["gm"], *bounds["gm"], "gm, a window misrouted")
    print("a pool-backward gradient at the wrong window position: relative L2 gm %.2e, dt0 %.2e, sums %.2e"
          % (rel(bad["gm"], bounds["gm"][0]), rel(bad["dt"], bounds["dt"][0]), rel(bad["sums"], bounds["sums"][0])))


# ---------------------------------------------------------------------------
# the bounds of the BN backward family, the residual affine forward, the column
# sums and the fused final-conv tail (parity.bn_bwd_bounds, sign_ambiguous2,
# affine_res_bound / affine_pool_bounds, colsum_bound / colstats_bound,
# convout_tail_bounds): fp32 emulations of the kernels' arithmetic -- the
# per-workgroup row ranges of the reduce skeleton, the per-thread partials, the
# fp64 finalize, the apply's folded coefficients -- sit inside the bounds in
# bf16 and fp32; ten broken kernels are rejected; one of them passes the norms
# the older tests assert.

F32 = torch.float32
ZERO = torch.zeros(())
ALPHA32 = float(torch.tensor(ALPHA))       # the slope as the kernels read it: exact in fp32


def _q(t, dt):
    return t.to(dt).float()


def _skeleton(P):
    """(blocks, rows per block) of csrc/bn.hip's reduce_blocks"""
    blocks = max(1, min(1024, -(-P // 64)))
    return blocks, -(-P // blocks)


def _block_rows(term, R, drop_last=False):
    """the partial rows [blocks, c] of term [P, c] (fp32) as a workgroup of R
    thread rows sums them: thread row tr takes rows r0 + tr, r0 + tr + R, ...
    in order, then the R partials are added in order"""
    P, c = term.shape
    blocks, rpb = _skeleton(P)
    out = torch.zeros(blocks, c)
    for bk in range(blocks):
        r0, r1 = bk * rpb, min(P, (bk + 1) * rpb)
        if drop_last:
            r1 -= 1
        acc = torch.zeros(R, c)
        for k in range(r0, max(r0, r1), R):
            m = min(R, r1 - k)
            acc[:m] += term[k:k + m]
        v = torch.zeros(c)
        for rr in range(R):
            v = v + acc[rr]
        out[bk] = v
    return out


_BNB = {}


def _bnb_case(dt, shape=(2, 8, 12, 64)):
    """operands exact in ``dt`` of every mask kind of one shape"""
    key = (dt, shape)
    if key not in _BNB:
        n, h, w, c = shape
        d = {"shape": shape, "g": _q(rnd(n, h, w, c, seed=61), dt), "aux": _q(F.relu(rnd(n, h, w, c, seed=62)), dt),
             "t": [_q(rnd(n, h, w, c, seed=63) * 2 + 0.3, dt), _q(rnd(n, h, w, c, seed=64) - 0.2, dt)],
             "mean": [rnd(c, seed=65) * 0.1 + 0.3, rnd(c, seed=66) * 0.1 - 0.2],
             "inv": [rnd(c, seed=67).abs() + 0.5, rnd(c, seed=68).abs() + 0.5],
             "gamma": [rnd(c, seed=69).abs() + 0.5, rnd(c, seed=70).abs() + 0.5],
             "beta": [rnd(c, seed=71) * 0.2, rnd(c, seed=72) * 0.2]}
        d["s"] = [d["gamma"][i] * d["inv"][i] for i in range(2)]
        d["b"] = [d["beta"][i] - d["mean"][i] * d["s"][i] for i in range(2)]
        # kind 2: aux = the PReLU input, no sign-ambiguous u
        tp = _q(rnd(n, h, w, c, seed=73), dt)
        d["taux"] = parity.make_sign_unambiguous(tp, d["s"][0], d["b"][0], dt)
        d["moved2"] = float((d["taux"] != tp).double().mean())
        # kinds 4 / 5: the mask recomputed from t0, t1
        d["t0u"], moved = parity.make_sign_unambiguous2(d["t"][0], d["s"][0], d["b"][0], d["t"][1], d["s"][1], d["b"][1], dt)
        d["moved4"] = float(moved.double().mean())
        _BNB[key] = d
    return _BNB[key]


def _bnb_operands(d, kind, nbn):
    """(g, keep, t list, slope, u, du) of a mask kind, fp64 / fp32 as the bounds take them"""
    t = [d["t0u"] if kind >= 4 else d["t"][0], d["t"][1]][:nbn]
    slope = u = du = None
    if kind == 0:
        keep = torch.ones_like(d["g"], dtype=torch.bool)
    elif kind == 1:
        keep = d["aux"] > 0
    elif kind == 2:
        ts = d["taux"].double() * d["s"][0].double()
        u = ts + d["b"][0].double()
        du = 2.0 * parity.U * (ts.abs() + d["b"][0].double().abs())
        keep, slope = u > 0, ALPHA32
    else:
        v = (t[0].double() * d["s"][0].double() + d["b"][0].double()) + (t[1].double() * d["s"][1].double() + d["b"][1].double())
        keep = v > 0
    return d["g"], keep, t, slope, u, du


def _bnb_bounds(d, dt, kind, nbn, eval_mode=False):
    g, keep, t, slope, u, du = _bnb_operands(d, kind, nbn)
    P = g.numel() // g.shape[-1]
    return parity.bn_bwd_bounds(g, keep, t, d["mean"][:nbn], d["inv"][:nbn], d["gamma"][:nbn], dt, eval_mode=eval_mode,
                                slope=slope, u=u, du=du, n_sum=_skeleton(P)[1])


BNB_MUTATIONS = {
    "the last row of each block's range dropped": (1, 2, False),
    "the BN1 sum uses mean0": (1, 2, False),
    "the mask is aux >= 0": (1, 1, False),
    "the alpha sum also takes u > 0 terms": (2, 1, False),
    "the sign of D flipped for one 8-channel group": (0, 2, False),
    "eval mode keeps the batch terms": (1, 2, True),
    "dbias without gamma invstd": (1, 2, True),
    "rows past the first grid-stride trip unwritten": (4, 2, False),
}


def _emulate_bn_bwd(d, dt, kind, nbn, eval_mode=False, mutation=None):
    """reduce -> finalize -> apply in fp32 as csrc/bn.hip's 8-channel kernels
    run them (products and sums rounded one by one: no contraction)"""
    n, h, w, c = d["shape"]
    P = n * h * w
    R = 256 // (c // 8)
    g = d["g"]
    t = [d["t0u"] if kind >= 4 else d["t"][0], d["t"][1]]
    ag = torch.zeros_like(g)
    if kind == 0:
        gm = g.clone()
    elif kind == 1:
        gm = torch.where((d["aux"] >= 0) if mutation == "the mask is aux >= 0" else (d["aux"] > 0), g, ZERO)
    elif kind == 2:
        u = d["taux"] * d["s"][0] + d["b"][0]
        gm = torch.where(u > 0, g, torch.tensor(ALPHA32) * g)
        ag = g * u if mutation == "the alpha sum also takes u > 0 terms" else torch.where(u > 0, ZERO, g * u)
    else:
        v = (t[0] * d["s"][0] + d["b"][0]) + (t[1] * d["s"][1] + d["b"][1])
        gm = torch.where(F.relu(v) > 0, g, ZERO)
    drop = mutation == "the last row of each block's range dropped"
    cols = [_block_rows(gm.reshape(P, c), R, drop)]
    for i in range(2):
        if i < nbn:
            mean = d["mean"][0] if (i == 1 and mutation == "the BN1 sum uses mean0") else d["mean"][i]
            cols.append(_block_rows((gm * ((t[i] - mean) * d["inv"][i])).reshape(P, c), R, drop))
        else:
            cols.append(torch.zeros_like(cols[0]))
    slab = torch.stack(cols, 2)                                     # [blocks, c, 3]
    arow = _block_rows(ag.reshape(P, c), R, drop).sum(1)            # one alpha partial per block, fp32
    s = slab.double().sum(0)
    count = math.inf if (eval_mode and mutation != "eval mode keeps the batch terms") else float(P)
    out = {"gm": gm.to(dt), "sums": s, "coef": torch.zeros(c, 2, 3)}
    if kind == 2:
        out["alpha"] = arow.double().sum()
        out["dalpha"] = out["alpha"].float()
    for i in range(nbn):
        out["dbeta%d" % i], out["dgamma%d" % i] = s[:, 0].float(), s[:, 1 + i].float()
        c0, c1, c2 = d["gamma"][i] * d["inv"][i], (s[:, 0] / count).float(), (s[:, 1 + i] / count).float()
        out["coef"][:, i] = torch.stack((c0, c1, c2), 1)
        if eval_mode:
            out["dbias%d" % i] = s[:, 0].float() if mutation == "dbias without gamma invstd" else c0 * s[:, 0].float()
        q = c0 * c2 * d["inv"][i]
        fD = q * d["mean"][i] - c0 * c1
        if mutation == "the sign of D flipped for one 8-channel group" and i == 0:
            fD = fD.clone()
            fD[8:16] = -fD[8:16]
        o = (-q) * t[i] + (c0 * gm + fD)
        if mutation == "rows past the first grid-stride trip unwritten":
            o.view(P, c)[128:] = math.nan                           # a grid of 4 workgroups: 4 * 256 / (c / 8) rows
        out["dt%d" % i] = o.to(dt)
    return out


def _rejected(got, bounds):
    bad = []
    for k, rb in bounds.items():
        try:
            parity.assert_within(got[k], rb[0], rb[1], k)
        except AssertionError:
            bad.append(k)
    return bad


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_sign_fixups_within_their_caps(dt):
    """zero ambiguous elements after the fix-up, at most 1 % of them moved"""
    d = _bnb_case(dt)
    assert int(parity.sign_ambiguous(d["taux"], d["s"][0], d["b"][0]).sum()) == 0
    assert int(parity.sign_ambiguous2(d["t0u"], d["s"][0], d["b"][0], d["t"][1], d["s"][1], d["b"][1]).sum()) == 0
    assert d["moved2"] <= 0.01 and d["moved4"] <= 0.01
    assert bool((d["t0u"].to(dt).float() == d["t0u"]).all())
    # an element on the threshold is ambiguous, and the fix-up moves it off
    s0, b0, s1, b1 = torch.tensor([1.5]), torch.tensor([-1.5]), torch.tensor([0.25]), torch.tensor([0.0])
    t0, t1 = torch.tensor([[1.0]]), torch.tensor([[0.0]])
    assert bool(parity.sign_ambiguous2(t0, s0, b0, t1, s1, b1).all())
    fixed, moved = parity.make_sign_unambiguous2(t0, s0, b0, t1, s1, b1, dt)
    assert bool(moved.all()) and not bool(parity.sign_ambiguous2(fixed, s0, b0, t1, s1, b1).any())


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind,nbn,eval_mode", [(0, 1, False), (0, 2, False), (1, 1, False), (1, 2, False), (2, 1, False),
                                                (2, 2, False), (4, 2, False), (1, 1, True), (1, 2, True)])
def test_ideal_bn_bwd_inside_bounds(dt, kind, nbn, eval_mode):
    d = _bnb_case(dt)
    bounds = _bnb_bounds(d, dt, kind, nbn, eval_mode)
    got = _emulate_bn_bwd(d, dt, kind, nbn, eval_mode)
    assert set(got) == set(bounds)
    for k, rb in bounds.items():
        parity.assert_within(got[k], rb[0], rb[1], f"ideal bn_bwd kind {kind} nbn {nbn} {k}")
    print(f"ideal bn_bwd kind {kind} nbn {nbn} eval {eval_mode}: used " +
          ", ".join(f"{k} {parity.worst_ratio(got[k], *rb):.3g}" for k, rb in bounds.items()))
    if eval_mode:
        assert bool((bounds["coef"][0][:, :nbn, 1:] == 0).all())


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mutation", list(BNB_MUTATIONS))
def test_broken_bn_bwd_rejected(dt, mutation):
    kind, nbn, eval_mode = BNB_MUTATIONS[mutation]
    d = _bnb_case(dt)
    bounds = _bnb_bounds(d, dt, kind, nbn, eval_mode)
    bad = _rejected(_emulate_bn_bwd(d, dt, kind, nbn, eval_mode, mutation), bounds)
    print(f"{mutation}: rejected by {bad}")
    assert bad, mutation


def test_old_metrics_accept_a_flipped_coefficient():
    """At 16 x 64 x 64 x 64 (the shape of the fused-tail model test) the apply with the sign of D flipped for channels
    8..15 of BN0 passes the 5e-2 relative L2 of close() in bf16 and the 1e-2 of
    the fused-tail test on every output, and fails the per-element bound of dt0
    on all of those channels."""
    d = _bnb_case(BF, (16, 64, 64, 64))
    bounds = _bnb_bounds(d, BF, 1, 2)
    got = _emulate_bn_bwd(d, BF, 1, 2, mutation="the sign of D flipped for one 8-channel group")
    worst = max(rel(got[k], bounds[k][0]) for k in ("gm", "dt0", "dt1", "dgamma0", "dbeta0", "dgamma1", "dbeta1"))
    print(f"D flipped on one channel group: worst relative L2 {worst:.2e}")
    assert worst < 1e-2 < 5e-2
    with pytest.raises(AssertionError):
        parity.assert_within(got["dt0"], *bounds["dt0"], "dt0")
    viol = ((got["dt0"].double() - bounds["dt0"][0]).abs() > bounds["dt0"][1])
    assert bool(viol[..., 8:16].any()) and not bool(viol[..., :8].any()) and not bool(viol[..., 16:].any())


# ---- the residual / PReLU affine forward and its pooled form

def _affine_case(dt, shape=(2, 6, 10, 64)):
    """x and res on several scales (randn 2^(1.5 randn)): the gap between the
    two largest values of a window is then rarely inside half a bf16 ulp of
    them; shifts near +1 keep windows with no positive value rare"""
    n, h, w, c = shape
    s, b = rnd(c, seed=81).abs() + 0.5, rnd(c, seed=82) * 0.2 + 1.0
    rs, rb = rnd(c, seed=83).abs() + 0.5, rnd(c, seed=84) * 0.2 + 1.0
    x = rnd(n, h, w, c, seed=85) * torch.exp2(rnd(n, h, w, c, seed=87) * 1.5)
    res = rnd(n, h, w, c, seed=86) * torch.exp2(rnd(n, h, w, c, seed=88) * 1.5)
    return {"x": _q(x, dt), "res": _q(res, dt), "s": s, "b": b, "rs": rs, "rb": rb}


AFFINE_VARIANTS = {
    "plain": dict(),
    "prelu": dict(alpha=ALPHA32),
    "res-relu": dict(res=True, relu=True),
    "res-affine-relu": dict(res=True, rs=True, relu=True),
    "prelu-res": dict(alpha=ALPHA32, res=True),
}


def _emulate_affine(d, dt, alpha=None, res=False, rs=False, relu=False, affine_on_x=False):
    v = d["x"] * d["s"] + d["b"]
    if alpha is not None:
        v = torch.where(v > 0, v, torch.tensor(alpha) * v)
    if res:
        r = d["x"] if affine_on_x else d["res"]
        if rs:
            r = r * d["rs"] + d["rb"]
        v = v + r
    if relu:
        v = F.relu(v)
    return v.to(dt)


def _affine_bound(d, dt, alpha=None, res=False, rs=False, relu=False):
    return parity.affine_res_bound(d["x"], d["s"], d["b"], dt, alpha=alpha, res=d["res"] if res else None,
                                   rs=d["rs"] if rs else None, rb=d["rb"] if rs else None, relu=relu)


def _pool_first_max(y):
    n, h, w, c = y.shape
    win = y.float().reshape(n, h // 2, 2, w // 2, 2, c)
    best, idx = win[:, :, 0, :, 0, :].clone(), torch.zeros(n, h // 2, w // 2, c, dtype=torch.uint8)
    for k in (1, 2, 3):
        v = win[:, :, k // 2, :, k % 2, :]
        idx = torch.where(v > best, torch.full_like(idx, k), idx)
        best = torch.maximum(best, v)
    return best.to(y.dtype), idx


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_ideal_affine_res_inside_bounds_and_wrong_residual_rejected(dt):
    d = _affine_case(dt)
    for name, kw in AFFINE_VARIANTS.items():
        ref, bound = _affine_bound(d, dt, **kw)
        got = _emulate_affine(d, dt, **kw)
        parity.assert_within(got, ref, bound, f"ideal affine {name}")
        print(f"ideal affine {name}: uses {parity.worst_ratio(got, ref, bound):.3g} of the bound")
        if kw.get("res"):
            with pytest.raises(AssertionError):
                parity.assert_within(_emulate_affine(d, dt, affine_on_x=True, **kw), ref, bound, name)
    # the plain PReLU form agrees with the older helper's reference
    assert torch.equal(_affine_bound(d, dt, alpha=ALPHA32)[0], parity.affine_prelu_bound(d["x"], d["s"], d["b"], ALPHA32, dt)[0])


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("ties", [False, True], ids=["plain", "ties"])
def test_ideal_affine_pool_inside_bounds(dt, ties):
    d = dict(_affine_case(dt, (3, 8, 12, 64)))
    if ties:                                                      # window positions 1 and 2 bit-identical in every 4th window column
        for k in ("x", "res"):
            v = d[k].clone()
            v[:, 0::2, 1::8] = v[:, 1::2, 0::8]
            d[k] = v
    kw = AFFINE_VARIANTS["res-affine-relu"]
    rb = _affine_bound(d, dt, **kw)
    (pref, pbound), idx, sure = parity.affine_pool_bounds(rb, (d["x"], d["res"]))
    y = _emulate_affine(d, dt, **kw)
    yp, yi = _pool_first_max(y)
    parity.assert_within(yp, pref, pbound, "ideal pooled")
    share = 1.0 - float(sure.double().mean())
    print(f"affine pool {'ties' if ties else 'plain'}: {share:.4f} of the windows undecided")
    assert share <= 0.02
    assert bool((yi == idx)[sure].all())
    if ties:
        # the forced ties are decided (bit-identical operands: the first of the pair), and
        # a kernel that takes the LAST maximum there is caught
        tied = ((idx == 1) & sure)[:, :, 0::4]
        assert int(tied.sum()) > 0
        bad = yi.clone()
        bad[:, :, 0::4] = torch.where(tied, torch.full_like(idx[:, :, 0::4], 2), yi[:, :, 0::4])
        assert not bool((bad == idx)[sure].all())


# ---- column sums and statistics

@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("P,c", [(63, 12), (4481, 64)])
def test_ideal_colsum_and_colstats_inside_bounds(dt, P, c):
    x = _q(rnd(P, c, seed=91), dt)
    out0 = rnd(c, seed=92) * 5
    R = 256 // (c // 4)
    n_sum = _skeleton(P)[1]
    rows = _block_rows(x, R)
    s = rows.double().sum(0).float()
    parity.assert_within(s, *parity.colsum_bound(x, n_sum), "ideal colsum")
    parity.assert_within(out0 + s, *parity.colsum_bound(x, n_sum, out0), "ideal colsum, accumulate")
    st = torch.stack((rows.double().sum(0), _block_rows(x * x, R).double().sum(0)), 1)
    parity.assert_within(st, *parity.colstats_bound(x, n_sum), "ideal colstats")
    print(f"colsum {P}x{c}: uses {parity.worst_ratio(s, *parity.colsum_bound(x, n_sum)):.3g},"
          f" colstats {parity.worst_ratio(st, *parity.colstats_bound(x, n_sum)):.3g}")
    dropped = _block_rows(x, R, drop_last=True)
    with pytest.raises(AssertionError):
        parity.assert_within(dropped.double().sum(0).float(), *parity.colsum_bound(x, n_sum), "colsum, rows dropped")
    with pytest.raises(AssertionError):                           # accumulate ignored
        parity.assert_within(s, *parity.colsum_bound(x, n_sum, out0), "colsum, out not accumulated")


# ---- the fused final-conv tail

def _convout_case(dt, shape=(3, 5, 7)):
    n, h, w = shape
    d = dict(_bnb_case(dt, (n, h, w, 64)))
    d["dy"] = rnd(n, 3, h, w, seed=95)
    d["wt"] = rnd(3, 64, seed=96) / 8.0
    # the block output, as rr_affine_act stores it
    v = (d["t0u"] * d["s"][0] + d["b"][0]) + (d["t"][1] * d["s"][1] + d["b"][1])
    d["x"] = F.relu(v).to(dt).float()
    return d


def _emulate_convout(d, dt, mutation=None):
    n, h, w, c = d["shape"]
    P = n * h * w
    dy = d["dy"]
    if mutation == "the convout dy of image 1 read from image 0":
        dy = dy.clone()
        dy[1] = dy[0]
    dyn = dy.permute(0, 2, 3, 1).reshape(P, 3)
    g = torch.zeros(P, c)
    for co in range(3):
        g = g + dyn[:, co:co + 1] * d["wt"][co]
    g = g.to(dt).float()
    x = d["x"].reshape(P, c)
    gm = torch.where(x > 0, g, ZERO)
    t = [d["t0u"].reshape(P, c), d["t"][1].reshape(P, c)]
    cols = [_block_rows(gm, 32)] + [_block_rows(gm * ((t[i] - d["mean"][i]) * d["inv"][i]), 32) for i in range(2)]
    s = torch.stack(cols, 2).double().sum(0)
    out = {"sums": s, "dw": torch.stack([_block_rows(dyn[:, co:co + 1] * x, 32).double().sum(0) for co in range(3)]).float(),
           "db": _block_rows(dyn, 32).double().sum(0).float()}
    for i in range(2):
        out["dbeta%d" % i], out["dgamma%d" % i] = s[:, 0].float(), s[:, 1 + i].float()
        c0, c1, c2 = d["gamma"][i] * d["inv"][i], (s[:, 0] / P).float(), (s[:, 1 + i] / P).float()
        q = c0 * c2 * d["inv"][i]
        out["dt%d" % i] = ((-q) * t[i] + (c0 * gm + (q * d["mean"][i] - c0 * c1))).reshape(n, h, w, c).to(dt)
    return out


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_ideal_convout_tail_inside_bounds_and_wrong_image_rejected(dt):
    d = _convout_case(dt)
    n, h, w, c = d["shape"]
    v = (d["t0u"].double() * d["s"][0].double() + d["b"][0].double()) + (d["t"][1].double() * d["s"][1].double() + d["b"][1].double())
    assert torch.equal(d["x"] > 0, v > 0)                         # the stored mask is the recomputed one
    bounds = parity.convout_tail_bounds(d["dy"], d["wt"], v > 0, [d["t0u"], d["t"][1]], d["mean"], d["inv"], d["gamma"], dt,
                                        d["x"], n_sum=_skeleton(n * h * w)[1])
    keys = ["sums", "dw", "db", "dgamma0", "dbeta0", "dgamma1", "dbeta1", "dt0", "dt1"]
    got = _emulate_convout(d, dt)
    for k in keys:
        parity.assert_within(got[k], *bounds[k], f"ideal convout tail {k}")
    print("ideal convout tail: used " + ", ".join(f"{k} {parity.worst_ratio(got[k], *bounds[k]):.3g}" for k in keys))
    bad = _rejected(_emulate_convout(d, dt, "the convout dy of image 1 read from image 0"), {k: bounds[k] for k in keys})
    print(f"dy of image 1 read from image 0: rejected by {bad}")
    assert "dt0" in bad and "dw" in bad


# ---------------------------------------------------------------------------
# The boundary layers (csrc/conv_in.hip, csrc/conv_out.hip, rr_prelu_bwd):
# each helper's ideal kernel -- the stated operand rounding, the launcher's
# ranges, a SHUFFLED summation order inside a range in fp32, fp64 across
# ranges, the stated stores -- inside its bound in both dtypes, and the broken
# kernels of the hand-written border / image-crossing / partial-step
# arithmetic rejected, with the score each gets under the older checks.

def _shuffle(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _patch_rows(xq, img, y, xx, lo=None):
    """[len, 28] fp32 patch rows (27 taps + the ones column) of pixels (img, y,
    xx) of xq [n, 3, h, w]; ``lo``: (flat pixel index of each row, first pixel
    of the range) -- taps whose source pixel lies before the range read 0"""
    n, _, h, w = xq.shape
    xp = F.pad(xq, (1, 1, 1, 1))
    j = torch.arange(27)
    ci, ky, kx = j // 9, (j % 9) // 3, j % 3
    v = xp[img[:, None], ci[None, :], y[:, None] + ky[None, :], xx[:, None] + kx[None, :]]
    if lo is not None:
        p, p0 = lo
        src = p[:, None] + (ky[None, :] - 1) * w + (kx[None, :] - 1)
        v = torch.where(src < p0, torch.zeros(()), v)
    return torch.cat((v, torch.ones(len(img), 1)), 1)


def _pix(P, h, w):
    p = torch.arange(P)
    return p, p // (h * w), (p % (h * w)) // w, p % w


def _emu_conv_in_mfma(x, wt, b, act, alpha, mutation=None):
    """rr_conv_in_mfma as the ideal kernel (mutation None): bf16(x) patches,
    the bf16 pack, the K = 32 sum in fp32 in a shuffled order, y_pre and
    y_act each one bf16 store of the accumulator -> (pre, act) NHWC"""
    n, _, h, w = x.shape
    P = n * h * w
    xq = x.to(BF).float()
    p, img, y, xx = _pix(P, h, w)
    pt = torch.zeros(P, 32)
    pt[:, :28] = _patch_rows(xq, img, y, xx)
    if mutation == "left border reads the previous row":
        # no x check on the left: tap (ky, 0) of column 0 reads flat offset rem + (ky - 1) w - 1 of the plane
        flat = xq.reshape(n, 3, h * w)
        rem = p % (h * w)
        for ci in range(3):
            for ky in range(3):
                src = rem + (ky - 1) * w - 1
                ok = (xx == 0) & (src >= 0) & (src < h * w) & (y + ky - 1 >= 0) & (y + ky - 1 < h)
                pt[ok, ci * 9 + ky * 3] = flat[img[ok], ci, src[ok]]
    if mutation == "no bias on the last partial wave" and P % 64:
        pt[P - P % 64:, 27] = 0.0
    pack = parity.conv_in_pack(wt, b, 32, BF)
    perm = _shuffle(32, 5)
    acc = pt[:, perm] @ pack[:, perm].t()
    a32 = torch.tensor(0.0 if alpha is None else alpha)
    ya = {0: acc, 1: acc.clamp_min(0), 2: torch.where(acc > 0, acc, a32 * acc)}[act]
    return acc.to(BF).reshape(n, h, w, 64), ya.to(BF).reshape(n, h, w, 64)


def _first_case(shape, zeros=False):
    n, h, w = shape
    x = rnd(n, 3, h, w, seed=21) * 0.5 + 0.3
    wt, b = rnd(64, 3, 3, 3, seed=22) / 3.0, rnd(64, seed=23) * 0.2
    g, t = rnd(n, h, w, 64, seed=24).to(BF).float(), rnd(n, h, w, 64, seed=25).to(BF).float()
    if zeros:
        t = torch.where(torch.rand(t.shape, generator=torch.Generator().manual_seed(26)) < 0.02, torch.zeros(()), t)
    return x, wt, b, g, t


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 9, 11), (2, 1, 70), (2, 70, 1)])
def test_ideal_conv_in_mfma_inside_bound_and_broken_rejected(shape):
    x, wt, b, _, _ = _first_case(shape)
    for act, alpha in ((0, None), (1, None), (2, 0.25), (2, 0.0), (2, float(torch.tensor(-0.1)))):
        rb = parity.conv_in_mfma_bounds(x, wt, b, act, alpha)
        pre, ya = _emu_conv_in_mfma(x, wt, b, act, alpha)
        parity.assert_within(pre, *rb["pre"], "ideal y_pre")
        parity.assert_within(ya, *rb["act"], "ideal y_act")
        print(f"conv_in_mfma {shape} act {act}: ideal uses {parity.worst_ratio(pre, *rb['pre']):.3f} (pre)"
              f" {parity.worst_ratio(ya, *rb['act']):.3f} (act) of the bound")
    rb = parity.conv_in_mfma_bounds(x, wt, b, 2, 0.25)
    muts = ["left border reads the previous row"] if shape[1] > 1 and shape[2] > 1 else []   # (a previous row to read)
    muts += ["no bias on the last partial wave"] if (shape[0] * shape[1] * shape[2]) % 64 else []
    for m in muts:
        pre, ya = _emu_conv_in_mfma(x, wt, b, 2, 0.25, mutation=m)
        for got, key in ((pre, "pre"), (ya, "act")):
            with pytest.raises(AssertionError):
                parity.assert_within(got, *rb[key], m)
        print(f"conv_in_mfma {shape} '{m}': relative L2 {rel(pre, rb['pre'][0]):.2e} (pre) {rel(ya, rb['act'][0]):.2e} (act);"
              " the older check asserts < 4e-3")


def _emu_wgrad_act(x, g, t, act, alpha, mutation=None):
    """rr_conv_in_wgrad_act as the ideal kernel: gp bit for bit, bf16 patches,
    one fp32 accumulator per range of ``conv_in_act_split`` over its pixels in
    a shuffled order, fp64 across, one fp32 store -> (dw, db, dalpha)"""
    n, _, h, w = x.shape
    P = n * h * w
    blocks, ppb = parity.conv_in_act_split(P)
    xq = x.to(BF).float()
    a32 = torch.tensor(alpha if act == 2 else 0.0)
    g2, t2 = g.reshape(P, 64), t.reshape(P, 64)
    keep = (t2 >= 0) if mutation == "mask t >= 0" else (t2 > 0)
    gp = torch.where(keep, g2, a32 * g2).to(BF).float()
    term = torch.where(keep, torch.zeros(()), g2 * t2)
    p, img, y, xx = _pix(P, h, w)
    slab = torch.zeros(blocks, 64, 28, dtype=torch.float64)
    arow = torch.zeros(blocks, dtype=torch.float64)
    for bk in range(blocks):
        p0, p1 = bk * ppb, min(P, (bk + 1) * ppb)
        if p0 >= p1:
            continue
        i = img[p0:p1].clone()
        if mutation == "first image's index for a whole step":
            for q0 in range(p0, p1, 64):
                i[q0 - p0:q0 - p0 + 64] = img[q0]
        lo = (p[p0:p1], p0) if mutation == "no reach back across the split" else None
        pt = _patch_rows(xq, i, y[p0:p1], xx[p0:p1], lo).to(BF).float()
        perm = _shuffle(p1 - p0, 7 + bk)
        acc = gp[p0:p1][perm].t() @ pt[perm]
        if mutation == "dead pixels count in the ones row":
            # the clamped load's g (pixel p0) not zeroed and a 1 in the ones row for the dead pixels of the last step
            acc[:, 27] += (-(p1 - p0) % 64) * gp[p0]
        slab[bk] = acc.double()
        arow[bk] = term[p0:p1].reshape(-1)[_shuffle((p1 - p0) * 64, 9 + bk)].sum().double()
    tot = slab.sum(0).float()
    return tot[:, :27].contiguous(), tot[:, 27].contiguous(), arow.sum().float()


WACT_MUTATIONS = {
    "first image's index for a whole step": (3, 6, 8),       # P = 144: the steps 0..63 and 64..127 each span two images
    "dead pixels count in the ones row": (3, 6, 8),          # the last step, 128..191, has 48 dead pixels
    "mask t >= 0": (1, 5, 7),
    "no reach back across the split": (1, 24, 40),           # ranges of 512 and 448, split inside row 12
}


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 6, 8), (2, 16, 24), (1, 24, 40), (1, 17, 241), (2, 1, 70), (2, 70, 1)])
def test_ideal_conv_in_wgrad_act_inside_bounds(shape):
    x, wt, b, g, t = _first_case(shape, zeros=True)
    for act, alpha in ((1, 0.0), (2, 0.25), (2, float(torch.tensor(-0.1)))):
        rb = parity.conv_in_wgrad_act_bounds(x, g, t, act, alpha)
        dw, db, da = _emu_wgrad_act(x, g, t, act, alpha)
        parity.assert_within(dw, *rb["dw"], "ideal dw")
        parity.assert_within(db, *rb["db"], "ideal db")
        parity.assert_within(da, *rb["dalpha"], "ideal dalpha")
        print(f"conv_in_wgrad_act {shape} act {act}: ideal uses {parity.worst_ratio(dw, *rb['dw']):.3f} (dw)"
              f" {parity.worst_ratio(db, *rb['db']):.3f} (db) {parity.worst_ratio(da, *rb['dalpha']):.3f} (dalpha)")


@pytest.mark.parametrize("mutation", list(WACT_MUTATIONS))
def test_broken_conv_in_wgrad_act_rejected(mutation):
    """dead pixels: their g is zeroed by the kernel, so a 1 in the ones row
    alone would add 0; the broken kernel here also keeps the g the clamped
    load brought (pixel p0's), which is what the zeroing and the live-only 1
    together rule out"""
    shape = WACT_MUTATIONS[mutation]
    x, wt, b, g, t = _first_case(shape, zeros=True)
    rb = parity.conv_in_wgrad_act_bounds(x, g, t, 2, 0.25)
    dw, db, da = _emu_wgrad_act(x, g, t, 2, 0.25, mutation=mutation)
    bad = 0
    for got, key in ((dw, "dw"), (db, "db"), (da, "dalpha")):
        try:
            parity.assert_within(got, *rb[key], mutation)
        except AssertionError:
            bad += 1
    assert bad >= 1, mutation
    old = float((dw.double() - rb["dw"][0]).abs().max() / rb["dw"][0].abs().max())
    print(f"'{mutation}' {shape}: relative L2 {rel(dw, rb['dw'][0]):.2e} (dw) {rel(db, rb['db'][0]):.2e} (db);"
          f" max error / max|dw| {old:.2e} (the older check asserts <= 2e-4)")


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_ideal_conv_in_valu_kernels_inside_bounds(dt):
    """rr_conv_in_fwd, rr_conv_in_wgrad (64-pixel fp32 stages in a shuffled
    order, folded in fp64, one fp32 store per range of 2048, fp64 across),
    rr_conv_in_dgrad and rr_conv_out_fwd"""
    n, cin, h, w, cout = 1, 3, 41, 53, 12
    P = n * h * w
    x = rnd(n, cin, h, w, seed=51) * 0.5 + 0.3
    wt, b = rnd(cout, cin, 3, 3, seed=32) / 5.0, rnd(cout, seed=33) * 0.2
    acc = F.conv2d(x, wt, b, padding=1)
    for act, f in ((0, lambda v: v), (1, F.relu), (2, lambda v: torch.where(v > 0, v, 0.25 * v))):
        rb = parity.conv_bound(x, wt, b, 1, dt)
        rb = {0: rb, 1: parity.relu(rb), 2: parity.prelu(rb, 0.25)}[act]
        parity.assert_within(nhwc(f(acc).to(dt)), *rb, "ideal rr_conv_in_fwd")
    dy = rnd(n, h, w, cout, seed=52).to(dt).float()
    ref, bound = parity.conv_in_wgrad_bounds(x, dy)
    blocks, ppb = parity.conv_in_wgrad_split(P)
    assert (blocks, ppb) == (2, 1087)
    pt = parity.patches3(x).float()
    d2 = dy.reshape(P, cout)
    tot = torch.zeros(cout, 28, dtype=torch.float64)
    for bk in range(blocks):
        a64 = torch.zeros(cout, 28, dtype=torch.float64)
        for p0 in range(bk * ppb, min(P, (bk + 1) * ppb), 64):
            p1 = min(P, (bk + 1) * ppb, p0 + 64)
            perm = _shuffle(p1 - p0, p0)
            a64 += (d2[p0:p1][perm].t() @ pt[p0:p1][perm]).double()
        tot += a64.float().double()
    parity.assert_within(tot.float(), ref, bound, "ideal rr_conv_in_wgrad")
    print(f"conv_in_wgrad {dt}: ideal uses {parity.worst_ratio(tot.float(), ref, bound):.3f} of the bound")
    # the image grad and the last conv's forward: one fp32 sum, one store
    g = rnd(2, 64, 12, 8, seed=61).to(dt).float()
    wg = rnd(64, 3, 3, 3, seed=62) / 24.0
    dx0 = rnd(2, 3, 12, 8, seed=63)
    parity.assert_within(F.conv_transpose2d(g, wg, padding=1), *parity.conv_in_dgrad_bounds(g, wg), "ideal dgrad", nchw=True)
    parity.assert_within(F.conv_transpose2d(g, wg, padding=1) + dx0, *parity.conv_in_dgrad_bounds(g, wg, dx0),
                         "ideal dgrad, accumulate", nchw=True)
    xo = rnd(3, 12, 9, 11, seed=71).to(dt).float()
    wo, bo = rnd(3, 12, 1, 1, seed=72) / 12 ** 0.5, rnd(3, seed=73)
    parity.assert_within(F.conv2d(xo, wo, bo), *parity.conv1x1_bound(xo, wo, bo, F32), "ideal rr_conv_out_fwd", nchw=True)
    y = rnd(2, 8, 8, 64, seed=74).to(BF).float()
    wq = (rnd(3, 64, seed=75) / 8.0).to(BF).float()
    parity.assert_within((y.reshape(-1, 64) @ wq.t() + bo).reshape(2, 8, 8, 3).permute(0, 3, 1, 2),
                         *parity.conv1x1_nchw_bound(y, wq, bo), "ideal tail 1x1", nchw=True)


def _emu_image_grad(g, wt, base, G, mutation=None):
    """the persistent image-grad walk: 256-pixel tiles, G workgroups, workgroup
    b takes tiles b, b + G, ...; the ideal tile is the fp32 transposed conv
    (+ base when accumulating); NaN where nothing is written"""
    n, _, h, w = g.shape
    full = F.conv_transpose2d(g, wt, padding=1).permute(0, 2, 3, 1).reshape(-1, 3)     # [P, 3]
    tiles = full.shape[0] // 256
    out = torch.full_like(full, math.nan) if base is None else base.permute(0, 2, 3, 1).reshape(-1, 3).clone()
    for bk in range(G):
        walk = list(range(bk, tiles, G))
        for k, t in enumerate(walk):
            if mutation == "last ragged tile skipped" and t == tiles - 1:
                continue
            src = t
            if mutation == "next halo from tile t + 1" and k > 0:
                src = min(walk[k - 1] + 1, tiles - 1)        # the halo held in registers belongs to the wrong tile
            v = full[src * 256:(src + 1) * 256]
            out[t * 256:(t + 1) * 256] = v if base is None else out[t * 256:(t + 1) * 256] + v
    return out.reshape(n, h, w, 3).permute(0, 3, 1, 2)


@pytest.mark.parametrize("acc", [False, True], ids=["write", "accumulate"])
def test_ideal_image_grad_walk_inside_bound_and_broken_rejected(acc):
    """11 tiles over 4 workgroups: workgroups with 3 and with 2 tiles (the
    ragged walk of 65 x 64 x 64 over 512 workgroups, scaled down)"""
    g = rnd(11, 64, 16, 16, seed=74).to(BF).float()
    wt = (rnd(64, 3, 3, 3, seed=75) * 0.1).to(BF).float()
    base = rnd(11, 3, 16, 16, seed=76) if acc else None
    rb = parity.conv_in_dgrad_bounds(g, wt, base)
    parity.assert_within(_emu_image_grad(g, wt, base, 4), *rb, "ideal walk", nchw=True)
    for m in ("next halo from tile t + 1", "last ragged tile skipped"):
        got = _emu_image_grad(g, wt, base, 4, mutation=m)
        with pytest.raises(AssertionError):
            parity.assert_within(got, *rb, m, nchw=True)
        score = rel(torch.nan_to_num(nhwc(got)), rb[0])
        print(f"image grad '{m}' acc {acc}: relative L2 {score:.2e} (unwritten elements counted as 0);"
              " the older check asserts < 1e-5 over the tensor and per image")


def _emu_conv_out_bwd(dy, x, wt, mask, dt, mutation=None):
    """rr_conv_out_bwd as the ideal kernel: dx = K = cout fp32 products, one
    store; dw / db one fp32 sum per range of ``conv_out_split`` in a shuffled
    order, the slabs [(cout + 1)][cin] summed in fp64, one fp32 store"""
    cout, cin = wt.shape
    n, _, h, w = dy.shape
    P = n * h * w
    blocks, ppb = parity.conv_out_split(P)
    d2, x2 = dy.permute(0, 2, 3, 1).reshape(P, cout), x.reshape(P, cin)
    keep = (x2 >= 0) if mutation == "mask x >= 0" else (x2 > 0)
    gx = d2 @ wt
    dx = (torch.where(keep, gx, torch.zeros(())) if mask else gx).to(dt).float()
    ws = torch.zeros(blocks * (cout + 1) * cin + 4096)                    # the slabs, then what lies behind them
    for bk in range(blocks):
        pb, pe = bk * ppb, min(P, (bk + 1) * ppb)
        live = torch.arange(pb, pe)
        if mutation == "trailing pixels of the pair loop dropped":
            off = live - pb
            tail = (off % 64 < 32) & (live + 32 >= pe)
            dx[live[tail]] = math.nan
            live = live[~tail]
        live = live[_shuffle(len(live), 11 + bk)]
        o = bk * (cout + 1) * cin
        ws[o:o + cout * cin] = (d2[live].t() @ x2[live]).reshape(-1)
        ws[o + cout * cin:o + cout * cin + cout] = d2[live].sum(0)
    slab = ws[:blocks * (cout + 1) * cin].reshape(blocks, cout + 1, cin).double()
    dw = slab[:, :cout].sum(0).float()
    if mutation == "db summed with the slab stride of cin rows":
        idx = torch.arange(blocks)[:, None] * (cin + 1) * cin + cout * cin + torch.arange(cout)[None, :]
        db = ws[idx.clamp_max(ws.numel() - 1)].double().sum(0).float()
    else:
        db = slab[:, cout, :cout].sum(0).float()
    return dx.reshape(n, h, w, cin), dw, db


OUTBWD_MUTATIONS = {
    "trailing pixels of the pair loop dropped": (64, 3, (1, 3, 11)),      # P = 33: lane 0 takes the pair (0, 32), lanes 1..31 the trailing call
    "mask x >= 0": (64, 3, (1, 5, 7)),
    "db summed with the slab stride of cin rows": (12, 3, (2, 33, 31)),   # two ranges: the second slab is misplaced
}


def _outbwd_case(cin, cout, shape, dt):
    n, h, w = shape
    dy = rnd(n, cout, h, w, seed=81)
    x = rnd(n, h, w, cin, seed=82).to(dt).float()
    x = torch.where(torch.rand(x.shape, generator=torch.Generator().manual_seed(87)) < 0.02, torch.zeros(()), x)
    return dy, x, rnd(cout, cin, seed=83) / 4.0


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("cin,cout,shape", [(64, 3, (1, 3, 11)), (64, 3, (2, 33, 31)), (12, 3, (1, 32, 33)), (4, 1, (1, 5, 7))])
def test_ideal_conv_out_bwd_inside_bounds(cin, cout, shape, dt):
    dy, x, wt = _outbwd_case(cin, cout, shape, dt)
    for mask in (0, 1):
        rb = parity.conv_out_bwd_bounds(dy, x, wt, mask, dt)
        got = dict(zip(("dx", "dw", "db"), _emu_conv_out_bwd(dy, x, wt, mask, dt)))
        for key in got:
            parity.assert_within(got[key], *rb[key], f"ideal {key}")
        print(f"conv_out_bwd {cin}->{cout} {shape} {dt} mask {mask}: ideal uses "
              + " ".join(f"{parity.worst_ratio(got[k], *rb[k]):.3f} ({k})" for k in got))


@pytest.mark.parametrize("mutation", list(OUTBWD_MUTATIONS))
def test_broken_conv_out_bwd_rejected(mutation):
    cin, cout, shape = OUTBWD_MUTATIONS[mutation]
    dy, x, wt = _outbwd_case(cin, cout, shape, BF)
    rb = parity.conv_out_bwd_bounds(dy, x, wt, 1, BF)
    got = dict(zip(("dx", "dw", "db"), _emu_conv_out_bwd(dy, x, wt, 1, BF, mutation=mutation)))
    bad = []
    for key in got:
        try:
            parity.assert_within(got[key], *rb[key], mutation)
        except AssertionError:
            bad.append(key)
    assert bad, mutation
    print(f"'{mutation}' {cin}->{cout} {shape}: outside the bound: {bad}; relative L2 "
          + " ".join(f"{rel(torch.nan_to_num(got[k]), rb[k][0]):.2e} ({k})" for k in got)
          + "; the older check is close() at 5e-2 on one shape, 2 x 12 x 8")


def test_conv_out_db_row_layout():
    """the finding behind the cin >= cout rule of rr_conv_out_bwd, from the
    layout alone: the kernel's db index of the last workgroup against the end
    of the slab area the workspace query sizes"""
    for cin, cout in ((2, 3), (1, 2), (3, 4), (1, 4)):
        for blocks in (1, 2, 7):
            last = ((blocks - 1) * (cout + 1) + cout) * cin + (cout - 1)
            assert last >= blocks * (cout + 1) * cin and not parity.conv_out_db_row_holds(cin, cout)
    for cin, cout in ((3, 3), (4, 3), (12, 1), (64, 3), (64, 4)):
        for blocks in (1, 2, 7):
            last = ((blocks - 1) * (cout + 1) + cout) * cin + (cout - 1)
            assert last < blocks * (cout + 1) * cin and parity.conv_out_db_row_holds(cin, cout)


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("count", [1, 4093, 4096, 8200])
def test_ideal_prelu_bwd_inside_bounds(count, dt):
    """the grid-stride split of prelu_bwd_kernel: thread (b, l) takes vectors
    b 256 + l, + blocks 256, ...; per-thread fp32 chains, a tree per
    workgroup (torch's fp32 sum here), fp64 across, one store"""
    blocks = max(1, min(1024, (count + 4095) // 4096))
    dy, t = rnd(count, seed=91).to(dt).float(), (rnd(count, seed=92) - 0.3).to(dt).float()
    rb = parity.prelu_bwd_bounds(dy, t, 0.25, dt, blocks)
    dx = torch.where(t > 0, dy, 0.25 * dy).to(dt)
    term = torch.where(t > 0, torch.zeros(()), dy * t)
    n4 = count // 4
    vec = torch.arange(n4)
    owner = (vec // 256) % blocks
    tot = 0.0
    for b in range(blocks):
        part = term[:n4 * 4].reshape(n4, 4)[owner == b].reshape(-1)
        if b == 0:
            part = torch.cat((part, term[n4 * 4:]))
        tot += float(part[_shuffle(len(part), b)].sum()) if len(part) else 0.0
    parity.assert_within(dx, *rb["dx"], "ideal dx")
    parity.assert_within(torch.tensor(tot).float(), *rb["dalpha"], "ideal dalpha")
    # broken: the tail dropped (what a count % 4 != 0 call would have lost)
    if count % 4 and float(term[n4 * 4:].abs().sum()) > 0:
        with pytest.raises(AssertionError):
            parity.assert_within(torch.tensor(float(term[:n4 * 4].double().sum())).float(), *rb["dalpha"], "tail dropped")
