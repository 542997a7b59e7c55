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
