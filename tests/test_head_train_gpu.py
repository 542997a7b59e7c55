"""Training the VGG16 classifier head on the GPU (05:59-82): Linear weight /
bias / input grads, training-mode Dropout, CrossEntropyLoss, the softmax
confidence, SGD, the head end to end over frozen features, and a HIP-graph
replay of one head step.

Bounds: a GEMM element against the fp64 product of the same operands is held
to the fp32 summation bound 2 K 2^-24 sum|a||b| (K the reduction length); the
end-to-end gradients to the project's fp32 bound (rel-L2 1e-3 per tensor,
test_fullsize_gpu.py) and, in bf16, to 1.25 x an ideal-bf16 head + 1e-3."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 64            # sentinel elements on both sides of an output (keeps 16-byte alignment)


def _guarded(shape, dtype, dev, fill=None):
    """a tensor of ``shape`` inside a larger sentinel-filled buffer"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), -777.0, dtype=dtype, device=dev)
    view = buf[PAD:PAD + numel].view(shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _sentinels_intact(buf):
    return bool((buf[:PAD] == -777.0).all() and (buf[-PAD:] == -777.0).all())


def _operands(n, fin, fout, dt, seed):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(n, fout, generator=g)
    x = torch.randn(n, fin, generator=g)
    w = torch.randn(fout, fin, generator=g)
    if dt == torch.bfloat16:
        dy, x, w = (t.bfloat16().float() for t in (dy, x, w))
    return dy, x, w


SHAPES = [(1, 64, 1), (5, 192, 43), (33, 256, 128), (64, 1024, 200), (64, 4096, 43)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,fin,fout", SHAPES)
def test_linear_wgrad(dev, dt, n, fin, fout):
    import roadrestore as rr
    dy, x, _ = _operands(n, fin, fout, dt, seed=n + fin + fout)
    dy64, x64 = dy.double(), x.double()
    ref_w, abs_w = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
    ref_b, abs_b = dy64.sum(0), dy64.abs().sum(0)
    dyd, xd = dy.to(dev).to(dt), x.to(dev).to(dt)
    bw, dw = _guarded((fout, fin), torch.float32, dev)
    bb, db = _guarded((fout,), torch.float32, dev)
    rr.ops.linear_wgrad(dyd, xd, dw=dw, db=db)
    got_w, got_b = dw.cpu().double(), db.cpu().double()
    ew, eb = (got_w - ref_w).abs(), (got_b - ref_b).abs()
    print("wgrad max err / bound", (ew / (2 * n * U * abs_w)).max().item(),
          (eb / (2 * n * U * abs_b)).max().item())
    assert (ew <= 2 * n * U * abs_w).all()
    assert (eb <= 2 * n * U * abs_b).all()
    assert _sentinels_intact(bw) and _sentinels_intact(bb)
    # bitwise repeatable
    dw2, db2 = rr.ops.linear_wgrad(dyd, xd)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    # accumulate: dw += ..., one more fp32 addition per element
    g = torch.Generator().manual_seed(7)
    pw, pb = torch.randn(fout, fin, generator=g), torch.randn(fout, generator=g)
    bw, dw = _guarded((fout, fin), torch.float32, dev, fill=pw.to(dev))
    bb, db = _guarded((fout,), torch.float32, dev, fill=pb.to(dev))
    rr.ops.linear_wgrad(dyd, xd, dw=dw, db=db, accumulate=True)
    ew = (dw.cpu().double() - (pw.double() + ref_w)).abs()
    eb = (db.cpu().double() - (pb.double() + ref_b)).abs()
    assert (ew <= 2 * (n + 1) * U * (abs_w + pw.double().abs())).all()
    assert (eb <= 2 * (n + 1) * U * (abs_b + pb.double().abs())).all()
    assert _sentinels_intact(bw) and _sentinels_intact(bb)
    # without a bias grad
    dw3, db3 = rr.ops.linear_wgrad(dyd, xd, want_db=False)
    assert db3 is None and torch.equal(dw3, dw2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,fin,fout", SHAPES)
def test_linear_dgrad(dev, dt, n, fin, fout):
    import roadrestore as rr
    dy, _, w = _operands(n, fin, fout, dt, seed=3 * n + fin + fout)
    dy64, w64 = dy.double(), w.double()
    ref, aref = dy64 @ w64, dy64.abs() @ w64.abs()
    bound = 2 * fout * U * aref
    dyd, wd = dy.to(dev).to(dt), w.to(dev).to(dt)       # the forward pack: [fout][fin] in dt
    bx, dx = _guarded((n, fin), torch.float32, dev)
    rr.ops.linear_dgrad(dyd, wd, fin, dx=dx)
    err = (dx.cpu().double() - ref).abs()
    print("dgrad max err / bound", (err / bound).max().item())
    assert (err <= bound).all()
    assert _sentinels_intact(bx)
    assert torch.equal(rr.ops.linear_dgrad(dyd, wd, fin), dx)
    # the ReLU in front of the layer folded in: dx *= (mask > 0)
    g = torch.Generator().manual_seed(11)
    mask = torch.randn(n, fin, generator=g).clamp_(min=0)
    bx, dxm = _guarded((n, fin), torch.float32, dev)
    rr.ops.linear_dgrad(dyd, wd, fin, mask=mask.to(dev), dx=dxm)
    keep = mask > 0
    assert 0 < keep.sum() < keep.numel()
    got = dxm.cpu()
    assert (got[~keep] == 0).all()
    assert torch.equal(got[keep], dx.cpu()[keep])
    assert _sentinels_intact(bx)


# ---------------------------------------------------------------------------
# Dropout

@pytest.mark.parametrize("p", [0.5, 0.25])
def test_dropout(dev, p):
    import roadrestore as rr
    R, C = 64, 4096
    keep_p = 1.0 - p
    scale = np.float32(1.0 / (1.0 - p))
    d = rr.nn.Dropout(p).to(dev).train()
    d.seed = 1234
    d.reset_step(5)
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(1)).to(dev).requires_grad_()
    y = d(x)
    assert d.step_count() == 6                     # the device counter advanced by one
    m5 = rr.ops.dropout_mask((R, C), p, 1234, 5, dev)
    m6 = rr.ops.dropout_mask((R, C), p, 1234, 6, dev)
    xs = x.detach().cpu().numpy()
    want = np.where(m5.cpu().numpy() != 0, xs * scale, np.float32(0))
    assert np.array_equal(y.detach().cpu().numpy(), want)      # exactly 0 or x * fp32(1/(1-p))
    # backward = g * mask * scale
    g = torch.randn(R, C, generator=torch.Generator().manual_seed(2)).to(dev)
    y.backward(g)
    wantg = np.where(m5.cpu().numpy() != 0, g.cpu().numpy() * scale, np.float32(0))
    assert np.array_equal(x.grad.cpu().numpy(), wantg)
    # the same (seed, step) gives the same mask; the next call the next one
    d.reset_step(5)
    with torch.no_grad():
        assert torch.equal(d(x), y.detach())
        y6 = d(x)
    assert d.step_count() == 7
    assert torch.equal(y6 != 0, (m6 != 0) & (x.detach() != 0))
    # statistics of the keep mask
    k = (m5 != 0).double().cpu()
    sd = math.sqrt(p * keep_p)
    assert abs(k.mean().item() - keep_p) <= 5 * sd / math.sqrt(R * C)
    assert ((k.mean(1) - keep_p).abs() <= 6 * sd / math.sqrt(C)).all()
    assert ((k.mean(0) - keep_p).abs() <= 6 * sd / math.sqrt(R)).all()
    agree = ((m5 != 0) == (m6 != 0)).double().mean().item()
    q = p * p + keep_p * keep_p
    assert abs(agree - q) <= 5 * math.sqrt(q * (1 - q) / (R * C))
    # another seed, another mask
    assert not torch.equal(rr.ops.dropout_mask((R, C), p, 1235, 5, dev), m5)
    # eval: the very same object
    d.eval()
    assert d(x) is x


# ---------------------------------------------------------------------------
# CrossEntropyLoss and the softmax confidence

def _ce_case(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(n, k, generator=g) * 3
    lg[0, 0] = 80.0                                   # a row with logits of +-80
    lg[0, k - 1] = -80.0
    if n > 2:
        lg[2] = torch.linspace(-80, 80, k)
    tg = torch.randint(0, k, (n,), generator=g)
    tg[0] = k - 1                                     # the -80 logit as the target
    return lg, tg


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("n,k", [(1, 43), (7, 43), (64, 43), (5, 1000), (3, 2)])
def test_cross_entropy(dev, n, k):
    import roadrestore as rr
    lg, tg = _ce_case(n, k, seed=n * 1000 + k)
    refs = {}
    for dt in (torch.float64, torch.float32):
        l = lg.clone().to(dt).requires_grad_()
        loss = F.cross_entropy(l, tg)
        loss.backward()
        refs[dt] = (loss.detach(), l.grad)
    l64, g64 = refs[torch.float64]
    l32, g32 = refs[torch.float32]
    ld = lg.to(dev).requires_grad_()
    crit = rr.CrossEntropyLoss()
    loss = crit(ld, tg.to(dev))
    loss.backward()
    assert torch.isfinite(loss).all() and torch.isfinite(ld.grad).all()
    floor = 8 * U
    e_loss = abs(loss.item() - l64.item()) / abs(l64.item())
    c_loss = abs(l32.item() - l64.item()) / abs(l64.item())
    e_grad, c_grad = _rel_l2(ld.grad.cpu(), g64), _rel_l2(g32, g64)
    print("CE loss err", e_loss, "cpu fp32", c_loss, "grad err", e_grad, "cpu fp32", c_grad)
    assert e_loss <= max(4 * c_loss, floor)
    assert e_grad <= max(4 * c_grad, floor)
    # autograd's incoming grad scales the gradient on the device
    ld2 = lg.to(dev).requires_grad_()
    (crit(ld2, tg.to(dev)) * 3.0).backward()
    assert _rel_l2(ld2.grad.cpu(), 3 * g64) <= max(4 * c_grad, floor)
    # bitwise repeatable
    ld3 = lg.to(dev).requires_grad_()
    loss3 = crit(ld3, tg.to(dev))
    loss3.backward()
    assert torch.equal(loss3, loss) and torch.equal(ld3.grad, ld.grad)
    # a target outside [0, k): NaN loss, that row's gradient zero, the others as before
    for bad in (k, -1, 2 ** 40):
        tb = tg.clone()
        tb[n - 1] = bad
        lb = lg.to(dev).requires_grad_()
        lossb = crit(lb, tb.to(dev))
        lossb.backward()
        assert torch.isnan(lossb)
        assert (lb.grad[n - 1] == 0).all()
        assert torch.equal(lb.grad[:n - 1], ld.grad[:n - 1])


@pytest.mark.parametrize("n,k", [(1, 43), (7, 43), (64, 43), (5, 1000), (3, 2)])
def test_softmax_max(dev, n, k):
    import roadrestore as rr
    lg, _ = _ce_case(n, k, seed=n * 77 + k)
    if n > 1:
        lg[1, :] = 0.5                               # every entry tied: index 0
        lg[n - 1, k - 1] = lg[n - 1, 0] = 90.0       # two maxima: the first
    ld = lg.to(dev)
    conf, pred = rr.ops.softmax_max(ld)
    assert torch.equal(pred, rr.ops.argmax_rows(ld))
    c64, _ = torch.softmax(lg.double(), 1).max(1)
    c32, _ = torch.softmax(lg, 1).max(1)
    err = ((conf.cpu().double() - c64).abs() / c64).max().item()
    cpu = ((c32.double() - c64).abs() / c64).max().item()
    print("softmax_max err", err, "cpu fp32", cpu)
    assert err <= max(4 * cpu, 8 * U)
    c2, p2 = torch.ops.rr.softmax_max(ld)
    assert torch.equal(c2, conf) and torch.equal(p2, pred)


# ---------------------------------------------------------------------------
# SGD

SGD_CFGS = {"momentum": dict(momentum=0.9), "plain": dict(momentum=0.0),
            "wd": dict(momentum=0.9, weight_decay=1e-4),
            "nesterov": dict(momentum=0.9, nesterov=True),
            "dampening": dict(momentum=0.9, dampening=0.1)}


def _f32(v):
    return float(np.float32(v))


def _sgd_step_ref(p, buf, g, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """one torch.optim.SGD step restated in fp64 from the fp32 inputs (the
    parameter, buffer and gradient as fp32 tensors, the hyper-parameters as
    the fp32 values the kernel receives) -> (p after, |lr * update|, |lr * buf|)"""
    lr, mu, damp, wd = _f32(lr), _f32(momentum), _f32(dampening), _f32(weight_decay)
    p, g = p.double(), g.double()
    g = g + wd * p
    d = g
    if mu != 0:
        b = g.clone() if buf is None else mu * buf.double() + (1 - damp) * g
        d = g + mu * b if nesterov else b
    else:
        b = g
    return p - lr * d, (lr * b).abs()


@pytest.mark.parametrize("cfg", list(SGD_CFGS), ids=list(SGD_CFGS))
@pytest.mark.parametrize("mode", ["flat", "per_param", "capturable"])
def test_sgd(dev, cfg, mode):
    """every step is held to 2^-23 (|p| + |lr buf|) per element against the
    fp64 restatement of that step from the state the GPU held before it
    (buf: the momentum buffer after the step; the gradient where momentum is 0)"""
    import roadrestore as rr
    kw = SGD_CFGS[cfg]
    lr = 0.05
    sizes = [1, 43, 4099, 2 ** 20]
    gen = torch.Generator().manual_seed(len(cfg) + len(mode))
    p0 = [torch.randn(s, generator=gen) for s in sizes]
    grads = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(3)]
    if mode == "flat":
        flat = torch.cat(p0).to(dev)
        ps, off = [], 0
        for s in sizes:
            ps.append(torch.nn.Parameter(flat[off:off + s]))
            off += s
    else:
        ps = [torch.nn.Parameter(t.to(dev)) for t in p0]
    opt = rr.SGD(ps, lr=lr, capturable=(mode == "capturable"), **kw)
    worst = 0.0
    for s in range(3):
        if mode == "flat":
            gflat = torch.cat(grads[s]).to(dev)
            off = 0
            for p, n in zip(ps, sizes):
                p.grad = gflat[off:off + n]
                off += n
        else:
            for p, g in zip(ps, grads[s]):
                p.grad = g.to(dev)
        before = [(p.detach().cpu(), opt.state[p]["momentum_buffer"].cpu()
                   if "momentum_buffer" in opt.state.get(p, {}) else None) for p in ps]
        assert all((b is None) == (s == 0 or not kw["momentum"]) for _, b in before)
        generation = rr.optim.GENERATION[0]
        opt.step()
        assert rr.optim.GENERATION[0] > generation                 # packed-weight caches see it
        for i, p in enumerate(ps):
            want, lrbuf = _sgd_step_ref(before[i][0], before[i][1], grads[s][i], lr, **kw)
            err = (p.detach().cpu().double() - want).abs()
            bound = 2.0 ** -23 * (want.abs() + lrbuf)
            worst = max(worst, (err / bound).max().item())
            assert (err <= bound).all(), (cfg, mode, s, sizes[i], (err / bound).max().item())
            if kw["momentum"] and s == 0:      # the first step's buffer is the gradient, undamped
                wd = _f32(kw.get("weight_decay", 0.0))
                b0 = grads[s][i].double() + wd * before[i][0].double()
                assert torch.equal(opt.state[p]["momentum_buffer"].cpu(), b0.float())
    print("sgd worst err / bound", worst)
    if kw["momentum"]:
        assert all("momentum_buffer" in opt.state[p] for p in ps)
        assert opt.state[ps[1]]["momentum_buffer"].shape == ps[1].shape
    else:
        assert all("momentum_buffer" not in opt.state[p] for p in ps)
    if mode == "flat":
        assert opt._gstate[0]["key"] is not None                  # one launch over the span
    else:
        assert opt._gstate[0]["key"] is None
    if mode == "capturable":
        assert opt._gstate[0]["step_dev"].item() == 3
        assert isinstance(opt.param_groups[0]["lr"], torch.Tensor)


# ---------------------------------------------------------------------------
# the head, end to end

class _Ref:
    """CPU references of the seeded VGG16 of test_vgg16_top1_golden on
    S.classifier_batch(8, 64), labels arange(8) % 43 -- computed once."""

    def __init__(self):
        from oracle import reference_cpu as R
        from oracle import seeded as S
        self.sd = S.seeded_state_dict(S.load_manifest("vgg16"), seed=3)
        self.x = S.classifier_batch(8, 64)
        self.y = torch.arange(8) % 43
        with torch.no_grad():
            self.logits = R.vgg16_forward(self.sd, self.x)
            f = R.vgg16_features_forward(self.sd, self.x)
            self.feat = torch.flatten(F.adaptive_avg_pool2d(f, (7, 7)), 1)
        self.keys = [f"classifier.{i}.{t}" for i in (0, 3, 6) for t in ("weight", "bias")]

    def head(self, feat, params, masks=None, scale=1.0, rnd=None):
        """logits of the classifier on pooled features; ``masks``: the two
        dropout keep masks; ``rnd``: rounds the GEMM operands (bf16 emulation)"""
        rnd = rnd or (lambda t: t)
        h = feat
        for j, i in enumerate((0, 3, 6)):
            h = F.linear(rnd(h), rnd(params[f"classifier.{i}.weight"]), params[f"classifier.{i}.bias"])
            if i != 6:
                h = F.relu(h)
                if masks is not None:
                    h = h * masks[j].to(h.dtype) * scale
        return h

    def grads(self, feat, dtype, masks=None, scale=1.0, rnd=None):
        """(logits, loss, {key: grad}) by CPU autograd in ``dtype``"""
        P = {k: self.sd[k].to(dtype).clone().requires_grad_() for k in self.keys}
        lg = self.head(feat.to(dtype), P, masks, scale, rnd)
        loss = F.cross_entropy(lg, self.y)
        loss.backward()
        return lg.detach(), loss.detach(), {k: P[k].grad for k in self.keys}


_REF = []


@pytest.fixture(scope="module")
def ref():
    if not _REF:
        _REF.append(_Ref())
    return _REF[0]


def _model(ref, dev, dtype=torch.float32, freeze=True):
    import roadrestore as rr
    v = rr.vgg16(num_classes=43)
    v.load_state_dict(ref.sd)
    v = v.to(dev)
    if freeze:
        for p in v.features.parameters():
            p.requires_grad = False
    if dtype != torch.float32:
        v.compute_dtype = dtype
        for m in v.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = dtype
    return v


def _check_fp32(v, lg, ref_lg, ref_g):
    err = (lg.detach().cpu() - ref_lg).abs().max().item()
    print("logit max err", err)
    assert err <= 1e-3 * max(1.0, ref_lg.abs().max().item())
    for k, g in ref_g.items():
        got = v.get_parameter(k).grad
        assert got is not None, k
        r = _rel_l2(got.cpu(), g)
        print(k, "grad rel-L2", r)
        assert r <= 1e-3, (k, r)
    assert all(p.grad is None for p in v.features.parameters())


def test_head_eval_mode_grads(dev, ref):
    import roadrestore as rr
    v = _model(ref, dev).eval()
    lg = v(ref.x.to(dev))
    loss = rr.CrossEntropyLoss()(lg, ref.y.to(dev))
    loss.backward()
    # CPU autograd of the oracle's own forward
    from oracle import reference_cpu as R
    P = {k: t.clone() for k, t in ref.sd.items()}
    for k in ref.keys:
        P[k].requires_grad_()
    rl = R.vgg16_forward(P, ref.x)
    rloss = F.cross_entropy(rl, ref.y)
    rloss.backward()
    assert abs(loss.item() - rloss.item()) <= 1e-3 * max(1.0, abs(rloss.item()))
    _check_fp32(v, lg, rl.detach(), {k: P[k].grad for k in ref.keys})
    # the no-grad call keeps returning the fused schedule's eval-mode logits
    with torch.no_grad():
        lg0 = v(ref.x.to(dev))
        v.train()
        assert torch.equal(v(ref.x.to(dev)), lg0)


def test_head_training_mode_grads(dev, ref):
    import roadrestore as rr
    v = _model(ref, dev).train()
    drops = [m for m in v.classifier if isinstance(m, rr.nn.Dropout)]
    for i, d in enumerate(drops):
        d.seed = 100 + i
        d.reset_step(0)
    lg = v(ref.x.to(dev))
    rr.CrossEntropyLoss()(lg, ref.y.to(dev)).backward()
    masks = [rr.ops.dropout_mask((8, 4096), 0.5, 100 + i, 0, dev).cpu() for i in range(2)]
    rl, _, rg = ref.grads(ref.feat, torch.float32, masks, 2.0)
    _check_fp32(v, lg, rl, rg)
    assert [d.step_count() for d in drops] == [1, 1]


def _ideal_bf16_head(feat, sd, y, round_logits=False):
    """the head with every GEMM operand (forward and backward) rounded to
    bf16 and fp64 accumulation, by hand: {key: grad}"""
    r = lambda t: t.bfloat16().double()
    W = {i: sd[f"classifier.{i}.weight"].double() for i in (0, 3, 6)}
    B = {i: sd[f"classifier.{i}.bias"].double() for i in (0, 3, 6)}
    a0 = feat.double()
    z1 = r(a0) @ r(W[0]).t() + B[0]
    a1 = z1.clamp_min(0)
    z2 = r(a1) @ r(W[3]).t() + B[3]
    a2 = z2.clamp_min(0)
    z3 = r(a2) @ r(W[6]).t() + B[6]
    if round_logits:
        z3 = r(z3)
    n = z3.shape[0]
    d3 = (torch.softmax(z3, 1) - F.one_hot(y, z3.shape[1]).double()) / n
    d2 = (r(d3) @ r(W[6])) * (z2 > 0)
    d1 = (r(d2) @ r(W[3])) * (z1 > 0)
    out = {}
    for i, d, a in ((0, d1, a0), (3, d2, a1), (6, d3, a2)):
        out[f"classifier.{i}.weight"] = r(d).t() @ r(a)
        out[f"classifier.{i}.bias"] = r(d).sum(0)
    return out


def test_head_bf16_as_accurate_as_ideal(dev, ref):
    """bf16 head: gradient error against fp64 <= 1.25 x that of an ideal bf16
    head (GEMM operands rounded to bf16, fp64 accumulation) + 1e-3, all three
    on the pooled features the bf16 model itself computes."""
    import roadrestore as rr
    from roadrestore import engine
    v = _model(ref, dev, torch.bfloat16).eval()
    with torch.no_grad():
        feat = engine.vgg_pooled_features(v, ref.x.to(dev), v._wc, torch.bfloat16).float().cpu()
    lg = v(ref.x.to(dev))
    rr.CrossEntropyLoss()(lg, ref.y.to(dev)).backward()
    _, _, g64 = ref.grads(feat, torch.float64)
    gid = _ideal_bf16_head(feat, ref.sd, ref.y)
    gid_r = _ideal_bf16_head(feat, ref.sd, ref.y, round_logits=True)
    res = {}
    for k in ref.keys:
        got = _rel_l2(v.get_parameter(k).grad.cpu(), g64[k])
        ideal = _rel_l2(gid[k], g64[k])
        print(k, "bf16 grad rel-L2", got, "ideal", ideal, "(ideal with bf16 logits",
              _rel_l2(gid_r[k], g64[k]), ")")
        res[k] = (got, ideal)
    for k, (got, ideal) in res.items():
        assert got <= 1.25 * ideal + 1e-3, (k, got, ideal)


def test_head_sgd_three_steps(dev, ref):
    import roadrestore as rr
    v = _model(ref, dev).eval()
    head = [v.get_parameter(k) for k in ref.keys]
    opt = rr.SGD(head, lr=1e-3, momentum=0.9)
    crit = rr.CrossEntropyLoss()
    P = {k: ref.sd[k].clone().requires_grad_() for k in ref.keys}
    ropt = torch.optim.SGD([P[k] for k in ref.keys], lr=1e-3, momentum=0.9)
    xd, yd = ref.x.to(dev), ref.y.to(dev)
    prev = None
    for s in range(3):
        opt.zero_grad()
        lg = v(xd)
        crit(lg, yd).backward()
        opt.step()
        ropt.zero_grad()
        rl = ref.head(ref.feat, P)
        F.cross_entropy(rl, ref.y).backward()
        ropt.step()
        err = (lg.detach().cpu() - rl.detach()).abs().max().item()
        print("step", s, "logit err", err)
        assert err <= 1e-3 * max(1.0, rl.abs().max().item())
        if prev is not None:       # this forward used the updated weights (version bump)
            assert err < (lg.detach().cpu() - prev).abs().max().item()
        prev = rl.detach()
    for k in ref.keys:
        d_got = v.get_parameter(k).detach().cpu() - ref.sd[k]
        d_ref = P[k].detach() - ref.sd[k]
        r = _rel_l2(d_got, d_ref)
        print(k, "update rel-L2", r)
        # three gradients of rel-L2 <= 1e-3 each, nearly parallel at lr 1e-3: their
        # weighted sum keeps that bound up to the change of the later gradients
        assert r <= 2e-3, (k, r)


def test_classifier_alone_matches_model_route(dev, ref):
    import roadrestore as rr
    from roadrestore import engine
    v = _model(ref, dev).eval()
    crit = rr.CrossEntropyLoss()
    xd, yd = ref.x.to(dev), ref.y.to(dev)
    loss_model = crit(v(xd), yd)
    with torch.no_grad():
        feat = engine.vgg_pooled_features(v, xd, v._wc, torch.float32).float()
    assert feat.shape == (8, 25088)
    lg = v.classifier(feat)
    loss_alone = crit(lg, yd)
    loss_alone.backward()
    assert v.classifier[0].weight.grad is not None
    # the same kernels in the same order; fp32 reorder bound over the three GEMMs
    assert abs(loss_alone.item() - loss_model.item()) <= 2 * 25088 * U * max(1.0, abs(loss_model.item()))


def test_head_guards(dev, ref):
    v = _model(ref, dev, freeze=False).eval()
    x = ref.x[:1].to(dev)
    with pytest.raises(NotImplementedError, match="freeze"):
        v(x)
    for p in v.features.parameters():
        p.requires_grad = False
    with pytest.raises(NotImplementedError, match="freeze"):
        v(x.clone().requires_grad_())
    feat = torch.zeros(1, 512, 7, 7, device=dev, requires_grad=True)
    with pytest.raises(NotImplementedError):
        v.avgpool(feat)


# ---------------------------------------------------------------------------
# HIP-graph replay of one head step

def test_head_step_graph_replay(dev):
    """one head step (forward, CE, backward, capturable SGD; training-mode
    Dropout) captured on one stream: three replays equal three eager steps
    from the same weights, seed and step"""
    import roadrestore as rr
    torch.manual_seed(5)
    n, fin, hid, k = 8, 256, 128, 43

    def build():
        torch.manual_seed(5)
        net = torch.nn.Sequential(rr.nn.Linear(fin, hid), rr.nn.ReLU(True), rr.nn.Dropout(),
                                  rr.nn.Linear(hid, k)).to(dev).train()
        net[2].seed = 99
        return net

    g = torch.Generator().manual_seed(6)
    feat = torch.randn(n, fin, generator=g).to(dev)
    y = (torch.arange(n) % k).to(dev)
    crit = rr.CrossEntropyLoss()

    def one_step(net, opt):
        loss = crit(net(feat), y)
        loss.backward()
        opt.step()
        return loss

    def reset(net, opt, w0):
        with torch.no_grad():
            for p, w in zip(net.parameters(), w0):
                p.copy_(w)
        opt._gstate[0]["step_dev"].zero_()       # the next step is a first step again
        opt._gstate[0]["step"] = 0
        net[2].reset_step(0)
        opt.zero_grad(set_to_none=True)

    # eager
    net = build()
    w0 = [p.detach().clone() for p in net.parameters()]
    opt = rr.SGD(net.parameters(), lr=1e-3, momentum=0.9, capturable=True)
    one_step(net, opt)                            # makes the device counters
    reset(net, opt, w0)
    eager_losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        eager_losses.append(one_step(net, opt).clone())
    eager_w = [p.detach().clone() for p in net.parameters()]
    assert net[2].step_count() == 3

    # captured
    net2 = build()
    opt2 = rr.SGD(net2.parameters(), lr=1e-3, momentum=0.9, capturable=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_step(net2, opt2)                      # warm-up
    torch.cuda.current_stream().wait_stream(side)
    reset(net2, opt2, w0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = one_step(net2, opt2)
    reset(net2, opt2, w0)                         # the capture ran nothing
    for i in range(3):
        graph.replay()
        assert torch.equal(static_loss, eager_losses[i]), i
    torch.cuda.synchronize()
    assert net2[2].step_count() == 3
    assert opt2._gstate[0]["step_dev"].item() == 3
    for a, b in zip(net2.parameters(), eager_w):
        assert torch.equal(a.detach(), b)
