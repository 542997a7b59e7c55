"""Per-element error bounds and guard bands for the kernel parity tests.

A relative L2 norm over a whole tensor hides an error confined to a tile
corner, the last column of a strip, a partial band or one image of a pair
(tests/test_parity_cpu.py shows two such broken kernels passing 4e-3).  The
helpers here bound every output element on its own, and wrap every operand in
poisoned bands so that a store or a used load outside a tensor, or an element
never written, shows up.  New kernel tests use these, not a norm.

The bound (derived, not measured).  Let

  u = 2^-24      unit roundoff of fp32 (24-bit significand, round to nearest);
  K              the number of terms summed into one output: 9 cin (3x3),
                 cin (1x1, convT up), 4 cin (convT down), n h w (a weight
                 grad), plus 1 per added operand (bias, the accumulated y0, a
                 residual);
  A              the same operation on |x| and |w| (plus |bias|, |y0|, |res|):
                 the sum of the magnitudes of the K terms.

Operands are bf16-exact (their products are then exact in fp32) or fp32 (one
rounding, u, per product).  A sum of K fp32 terms in ANY order, by FMA chain
or by tree, has error at most (K - 1) u A + O(u^2) (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2); with fp32 products at most
K u A + O(u^2).  Hence, with a factor that absorbs the O(u^2) terms, the one
extra fp32 product of a PReLU slope and the second-order term of the store
below,

  fp32 output:  bound = 2 K u A
  bf16 output:  bound = 2^-8 |ref| + 2 K u A

bf16 keeps 8 significand bits, so a store rounded once to nearest moves a
value v by at most 2^-8 |v| (half an ulp); v is within K u A of ref, and
2^-8 K u A is far inside the K u A the factor 2 leaves over.  An output that
was rounded to bf16 TWICE (an intermediate stored and read back) gets
``rounds=2``: 2 * 2^-8 |ref|; the call site must say why.

ReLU, PReLU with |alpha| <= 1, and a mask taken from a separate tensor are
1-Lipschitz: |f(a) - f(b)| <= |a - b|, so they map ref and keep the bound.
The 2x2 max is 1-Lipschitz in the maximum norm: the pooled bound is the
maximum of the bound over the window.

BN statistics partials (summed over their rows; of the pre-bias sum): with
e_p = 2 K u A_p the bound of pixel p and P pixels per channel summed in fp32
in any order (error at most P u sum|t|, doubled as above),

  sum:             sum_p e_p + 2 P u sum_p |ref_p|
  sum of squares:  sum_p (2 |ref_p| e_p + e_p^2) + 2 P u sum_p ref_p^2

((r + d)^2 - r^2 = 2 r d + d^2 with |d| <= e_p).

References are fp64 on the CPU.  Activations are taken NCHW (torch's layout)
and everything returned is NHWC, the kernels' layout.

Plain helper module, imported like rrpath: no fixtures, no pytest settings.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 unit roundoff
HALF_ULP_BF16 = 2.0 ** -8   # bf16 unit roundoff (8 significand bits)
SENTINEL = -768.0       # finite, exact in bf16 and fp32


# ---------------------------------------------------------------------------
# the check

def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def assert_within(got, ref64, bound64, what, nchw=False):
    """|got - ref64| <= bound64 for every element; a NaN in ``got`` is a
    violation.  ``got`` in the layout of ``ref64`` (NHWC), or NCHW with
    ``nchw`` (the fp32 model-boundary outputs).  The failure message gives the
    number of violations, the worst ratio and the NHWC index of the worst
    element with its position in the 8 / 16-row and 16 / 32-column grids the
    kernels tile by."""
    got = got.detach().double().cpu()
    if nchw:
        got = _nhwc(got)
    assert got.shape == ref64.shape == bound64.shape, (what, got.shape, ref64.shape, bound64.shape)
    assert bool((bound64 >= 0).all()) and bool(torch.isfinite(ref64).all()), what
    err = (got - ref64).abs()
    bad = ~(err <= bound64)                       # NaN compares false: a violation
    count = int(bad.sum())
    if count == 0:
        return
    ratio = err / bound64.clamp_min(1e-300)
    ratio = torch.where(torch.isnan(got), torch.full_like(ratio, math.inf), ratio)
    flat = int(torch.where(bad, ratio, torch.full_like(ratio, -1.0)).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), got.shape))
    where = ""
    if got.dim() == 4:
        _, h, w, _ = idx
        where = (f" [n, h, w, c] of {tuple(got.shape)}: row {h} = {h // 16}*16+{h % 16} = {h // 8}*8+{h % 8},"
                 f" column {w} = {w // 32}*32+{w % 32} = {w // 16}*16+{w % 16}, channel {idx[3]}"
                 f" = {idx[3] // 32}*32+{idx[3] % 32};")
    first = [tuple(int(i) for i in r) for r in bad.nonzero()[:6]]
    raise AssertionError(
        f"{what}: {count} of {got.numel()} elements outside the bound ({int(torch.isnan(got).sum())} NaN);"
        f" worst ratio {float(ratio.reshape(-1)[flat]):.3g} at {idx}{where}"
        f" got {float(got.reshape(-1)[flat])!r}, ref {float(ref64.reshape(-1)[flat])!r},"
        f" bound {float(bound64.reshape(-1)[flat]):.3g}; first violations {first}")


def worst_ratio(got, ref64, bound64):
    """max |got - ref| / bound (for printing how much of a bound is used)"""
    got = got.detach().double().cpu()
    return float(((got - ref64).abs() / bound64.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------
# bounds

def _round_term(ref, out_dtype, rounds):
    if out_dtype == torch.float32:
        assert rounds == 1
        return torch.zeros_like(ref)
    assert out_dtype == torch.bfloat16 and rounds in (1, 2)
    return rounds * HALF_ULP_BF16 * ref.abs()


def _finish(ref, A, K, out_dtype, rounds):
    return ref, _round_term(ref, out_dtype, rounds) + 2.0 * K * U * A


def conv_terms(x, w, padding):
    """(ref, A) of the plain convolution, fp64 NHWC: the sum and the sum of
    the magnitudes of its terms (shared by the epilogue variants of a shape)."""
    x, w = x.double(), w.double()
    return _nhwc(F.conv2d(x, w, None, padding=padding)), _nhwc(F.conv2d(x.abs(), w.abs(), None, padding=padding))


def epilogue_bound(terms, K, bias, out_dtype, extra=None, rounds=1):
    """(ref64, bound64) from (ref, A) ``terms`` of a K-term sum, with
    ``bias`` [c] and ``extra`` (NCHW: the accumulated y0 or the residual)
    added: one more term each."""
    ref, A = terms
    if bias is not None:
        ref, A, K = ref + bias.double(), A + bias.double().abs(), K + 1
    if extra is not None:
        e = _nhwc(extra.double())
        ref, A, K = ref + e, A + e.abs(), K + 1
    return _finish(ref, A, K, out_dtype, rounds)


def conv_bound(x, w, bias, padding, out_dtype, extra=None, rounds=1):
    """3x3 (padding 1) or 1x1 (padding 0) convolution of x [n, cin, h, w]
    with w [cout, cin, k, k]: K = k k cin (+ 1 per bias / extra)."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return epilogue_bound(conv_terms(x, w, padding), K, bias, out_dtype, extra, rounds)


def conv1x1_bound(x, w, bias, out_dtype, extra=None):
    """K = cin"""
    return conv_bound(x, w, bias, 0, out_dtype, extra)


def convt_up_bound(x, w, bias, out_dtype):
    """ConvTranspose2d(k 2, stride 2) forward of x [n, cin, h, w] with
    w [cin, cout, 2, 2]: every output pixel has one tap, K = cin (+ 1)."""
    x, w = x.double(), w.double()
    ref = _nhwc(F.conv_transpose2d(x, w, None, stride=2))
    A = _nhwc(F.conv_transpose2d(x.abs(), w.abs(), None, stride=2))
    return epilogue_bound((ref, A), w.shape[0], bias, out_dtype)


def convt_down_bound(g, w, out_dtype):
    """its input grad: g [n, cout, 2h, 2w] gathered 2x2 with w [cin, cout, 2,
    2], K = 4 cout terms (the channels of the gathered operand)."""
    g, w = g.double(), w.double()
    ref = _nhwc(F.conv2d(g, w, None, stride=2))
    A = _nhwc(F.conv2d(g.abs(), w.abs(), None, stride=2))
    return _finish(ref, A, 4 * w.shape[1], out_dtype, 1)


def _wgrad64(x, dy, k):
    n, ci, h, w = x.shape
    co = dy.shape[1]
    p = k // 2
    xp = F.pad(x, (p, p, p, p))
    g = dy.permute(1, 0, 2, 3).reshape(co, -1)
    out = torch.empty(co, ci, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + h, kx:kx + w].permute(1, 0, 2, 3).reshape(ci, -1)
            out[:, :, ky, kx] = g @ xs.t()
    return out


def wgrad_bound(x, dy, k, dw0=None):
    """conv weight grad dW[co][ci][ky][kx] = sum_p dy[p, co] x[p + tap, ci]
    (fp32 output, torch's layout) of x [n, cin, h, w], dy [n, cout, h, w]:
    K = n h w (+ 1 with ``dw0`` accumulated into)."""
    x, dy = x.double(), dy.double()
    ref, A = _wgrad64(x, dy, k), _wgrad64(x.abs(), dy.abs(), k)
    K = x.shape[0] * x.shape[2] * x.shape[3]
    if dw0 is not None:
        ref, A, K = ref + dw0.double(), A + dw0.double().abs(), K + 1
    return _finish(ref, A, K, torch.float32, 1)


def relu(rb):
    return rb[0].clamp_min(0), rb[1]


def prelu(rb, alpha):
    assert abs(alpha) <= 1
    return torch.where(rb[0] > 0, rb[0], alpha * rb[0]), rb[1]


def masked(rb, mask):
    """result * (mask > 0), mask NCHW, a tensor of its own"""
    return torch.where(_nhwc(mask) > 0, rb[0], torch.zeros((), dtype=torch.float64)), rb[1]


def pooled(rb):
    """MaxPool2d(2), floor sizes: the max of ref, and of the bound, per window"""
    def mp(t):
        return F.max_pool2d(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    return mp(rb[0]), mp(rb[1])


def stats_bound(terms, K):
    """BN statistics of the pre-bias sum, (ref64, bound64) [c, 2] =
    (sum, sum of squares) per channel, from (ref, A) NHWC ``terms``."""
    ref, A = terms
    c = ref.shape[-1]
    r, e = ref.reshape(-1, c), (2.0 * K * U * A).reshape(-1, c)
    P = r.shape[0]
    s_ref, q_ref = r.sum(0), (r * r).sum(0)
    s_b = e.sum(0) + 2.0 * P * U * r.abs().sum(0)
    q_b = (2.0 * r.abs() * e + e * e).sum(0) + 2.0 * P * U * q_ref
    return torch.stack((s_ref, q_ref), 1), torch.stack((s_b, q_b), 1)


# ---------------------------------------------------------------------------
# the fused BN / PReLU backward epilogues
#
# rr_igemm_bnbwd works on the fp32 accumulator g of a dgrad (pixel p, channel
# c; e_p = 2 K u A_p its bound as above):
#   u_p  = t_p s + b                  fp32, contracted to an fma or not
#   gm_p = u_p > 0 ? g_p : alpha g_p  stored in the compute dtype
#   column sums over the pixels of sum gm and sum gm xhat, xhat_p = (t_p -
#   mean) invstd, of the unrounded gm, in fp32; and sum over u_p <= 0 of
#   g_p u_p over pixels AND channels, the products in fp32, the sum in fp64.
#
# The sign of u.  Everything is a function of sign(u_p).  t is bf16-exact (8
# significand bits) and s is fp32 (24), so t s is exact in fp64; rounded to
# fp32 once after adding b it is the fma's u, rounded twice the unfused one.
# ``sign_ambiguous`` marks the elements where the two disagree or either is
# zero; the tests fix their inputs so that there are none, and then the mask
# is a tensor of its own (|m| <= 1, 1-Lipschitz) and gm keeps the bound of g.
#
# Column sums (the model is stats_bound).  |gm_p - ref_p| <= e_p; the factor 2
# in e_p leaves K u A_p >= K u |g_p|, K >= 64, which covers the rounding of
# alpha g, the two roundings of xhat_p and the one of gm_p xhat_p (3 u
# |gm_p xhat_p|).  P fp32 terms summed in any order add (P - 1) u sum|term|:
#   sum gm:       sum_p e_p          + P u sum_p |gm_p|
#   sum gm xhat:  sum_p e_p |xhat_p| + P u sum_p |gm_p xhat_p|
# (The row-streaming kernel sums gm t and forms invstd (sum gm t - mean sum gm)
# per workgroup: its worst case has |t_p| + |mean| where this has |t_p - mean|.
# It is held to the same, tighter, bound.)
#
# The alpha partial, N = P c terms: sum_{u <= 0} e_p |u_p| for the accumulator,
# and N 2^-53 sum|g_p u_p| for the fp64 summation:
#   sum_{u <= 0} e_p |u_p| + N 2^-53 sum |g_p u_p|
# Three fp32 roundings have no term of their own: the fp32 u_p is within d_p =
# 2 u (|t_p s| + |b|) of the exact one either way (|g_p| d_p), the product
# g_p u_p is rounded once and each row's fp64 sum once to fp32 (2 u |g_p u_p|).
# They are inside the K u A_p |u_p| the factor 2 of e_p leaves over, summed
# over the elements -- not element by element where u_p cancels -- and
# bnbwd_bounds asserts that for its inputs.
# (The row-streaming kernel sums these in fp32; it is held to the same bound.)

def sign_ambiguous(t, s, b):
    """elements of t [..., c] (bf16-exact, fp32) whose fp32 u = t s + b has
    another sign as an fma than as a product and a sum, or is zero either way"""
    t, s, b = t.float(), s.float(), b.float()
    two = t * s + b                                             # two roundings
    one = (t.double() * s.double() + b.double()).float()        # one (the product is exact in fp64)
    return ((two > 0) != (one > 0)) | (two == 0) | (one == 0)


def make_sign_unambiguous(t, s, b, dtype=torch.bfloat16):
    """t with every ambiguous element moved to the neighbouring value of
    ``dtype`` away from zero (repeated until none is left); exact in ``dtype``
    in and out"""
    ity = torch.int16 if dtype == torch.bfloat16 else torch.int32
    t = t.float().clone()
    for _ in range(4):
        bad = sign_ambiguous(t, s, b)
        if not bool(bad.any()):
            break
        nxt = (t.to(dtype).view(ity) + 1).view(dtype).float()       # sign-magnitude: one ulp away from zero
        t = torch.where(bad, nxt, t)
    return t


def bnbwd_bounds(terms, K, t, mean, invstd, aff_s, aff_b, alpha, out_dtype):
    """(ref64, bound64) of gm [n, h, w, c], of the column sums [c, 2] = (sum
    gm, sum gm xhat) and of the alpha sum (0-d), from (ref, A) NHWC ``terms``
    of the K-term dgrad and t NHWC; no element of t may be sign-ambiguous."""
    assert abs(alpha) <= 1
    g, A = terms
    e = 2.0 * K * U * A
    t, s, b = t.double(), aff_s.double(), aff_b.double()
    u = t * s + b
    neg = ~(u > 0)
    gm = torch.where(neg, alpha * g, g)
    xhat = (t - mean.double()) * invstd.double()
    c = g.shape[-1]
    P = g.numel() // c

    def col(x):
        return x.reshape(-1, c).sum(0)
    tx = gm * xhat
    sums = torch.stack((col(gm), col(tx)), 1)
    sums_b = torch.stack((col(e) + P * U * col(gm.abs()), col(e * xhat.abs()) + P * U * col(tx.abs())), 1)
    gu = torch.where(neg, g * u, torch.zeros((), dtype=torch.float64))
    zero = torch.zeros((), dtype=torch.float64)
    a_b = torch.where(neg, e * u.abs(), zero).sum() + g.numel() * 2.0 ** -53 * gu.abs().sum()
    # the roundings of u, of g u and of each row's store, inside what the factor 2 of e leaves over
    du = 2.0 * U * ((t * s).abs() + b.abs())
    assert float(torch.where(neg, g.abs() * du + 2.0 * U * gu.abs(), zero).sum()) <= 0.5 * float(
        torch.where(neg, e * u.abs(), zero).sum())
    return {"gm": (gm, _round_term(gm, out_dtype, 1) + e), "sums": (sums, sums_b), "alpha": (gu.sum(), a_b)}


def cast32(rb):
    """a value inside (ref, bound) in fp64, rounded once to fp32 (the
    finalize's dgamma / dbeta / dalpha from its fp64 sums of the partial rows;
    the fp64 sum of R fp32 rows adds R 2^-53 of the magnitudes, inside the u)"""
    ref, bound = rb
    return ref, bound + 2.0 * U * (ref.abs() + bound)


def _stored(ref, ev, out_dtype):
    """the bound of a value within ev of ref after one store in ``out_dtype``"""
    if out_dtype == torch.float32:
        return ev
    assert out_dtype == torch.bfloat16
    return ev + HALF_ULP_BF16 * (ref.abs() + ev)


def affine_prelu_bound(t, s, b, alpha, out_dtype):
    """rr_affine_act: y = PReLU(t s + b) of t NHWC, stored in ``out_dtype``.
    The fp32 u is within 2 u (|t s| + |b|) of the exact one (fma or not), the
    slope is one more fp32 product, PReLU with |alpha| <= 1 is 1-Lipschitz;
    then one store: half an ulp of a value within ev of ref."""
    assert abs(alpha) <= 1
    t, s, b = t.double(), s.double(), b.double()
    u = t * s + b
    ref = torch.where(u > 0, u, alpha * u)
    ev = 2.0 * U * ((t * s).abs() + b.abs()) + U * ref.abs()
    return ref, _stored(ref, ev, out_dtype)


def pool_bwd_bounds(g, pdy, idx, aux, t, mean, invstd, gamma, out_dtype, sum_stored):
    """The BN backward behind a ReLU and a 2x2 max-pool (mask kind 3), all
    NHWC: gt = g + unpool(pdy, idx) (the window position idx = 2 dy + dx gets
    the pooled grad; one fp32 add, u |gt|), gm = gt (aux > 0), the column sums
    [c, 2] = (sum gm, sum gm xhat) of the unrounded gm -- of the stored gm with
    ``sum_stored`` (rr_bn_bwd_reduce_gm) -- and the apply
      dt = a (gm - m0 - xhat m1),  a = gamma invstd, m0 = sum gm / P, m1 = sum gm xhat / P.
    Bounds: e_p = u |gm_p|, or the stored gm's bound where the stored value
    is what is summed and what the apply reads; the sums as bnbwd_bounds; dt =
    a gm + (-a invstd m1) t + a (mean invstd m1 - m0) evaluated in fp32 from
    fp32 coefficients: a e_p, the sums' bounds over P, 8 u of the magnitudes
    of its terms (6 coefficient and 2 fma roundings), one store."""
    g, pdy, t = g.double(), pdy.double(), t.double()
    n, h, w, c = g.shape
    up = torch.zeros_like(g)
    win = up.view(n, h // 2, 2, w // 2, 2, c)
    for k in range(4):
        win[:, :, k // 2, :, k % 2, :] = torch.where(idx == k, pdy, torch.zeros((), dtype=torch.float64))
    gt = g + up
    gm = torch.where(aux > 0, gt, torch.zeros((), dtype=torch.float64))
    gm_b = _stored(gm, U * gm.abs(), out_dtype)
    e = gm_b if sum_stored else U * gm.abs()
    P = n * h * w
    xhat = (t - mean.double()) * invstd.double()

    def col(x):
        return x.reshape(-1, c).sum(0)
    tx = gm * xhat
    sums = torch.stack((col(gm), col(tx)), 1)
    sums_b = torch.stack((col(e) + P * U * col(gm.abs()), col(e * xhat.abs()) + P * U * col(tx.abs())), 1)
    a = gamma.double() * invstd.double()
    m0, m1 = sums[:, 0] / P, sums[:, 1] / P
    dt = a * (gm - m0 - xhat * m1)
    mag = a.abs() * (gm.abs() + m0.abs() + m1.abs() * invstd.double() * (t.abs() + mean.double().abs()))
    ev = a.abs() * (e + sums_b[:, 0] / P + xhat.abs() * sums_b[:, 1] / P) + 8.0 * U * mag
    return {"gm": (gm, gm_b), "sums": (sums, sums_b), "dt": (dt, _stored(dt, ev, out_dtype))}


# ---------------------------------------------------------------------------
# guard bands

class Guarded:
    """the whole buffer of a guarded tensor: ``raw`` = band | tensor | band"""

    def __init__(self, raw, band, poison):
        self.raw, self.band, self.poison = raw, band, poison


def default_band(shape, dtype):
    """two full image rows of an NHWC tensor (2 w c elements; the last two
    extents of any other shape), at least 256 bytes, rounded up to a multiple
    of 256 bytes: a walk one halo row too far stays inside the buffer, and the
    view keeps the alignment of a fresh allocation"""
    item = torch.empty((), dtype=dtype).element_size()
    rows = 2 * int(shape[-1]) * (int(shape[-2]) if len(shape) > 1 else 1)
    nbytes = -(-max(rows * item, 256) // 256) * 256
    return nbytes // item


def guarded(shape, dtype, dev, fill=None, band=None, poison=SENTINEL):
    """(buf, view): ``view`` of ``shape`` inside a larger buffer whose bands
    before and after it hold ``poison`` -- the finite SENTINEL for an output
    (check it with ``intact``), NaN for an input (a read past the tensor that
    reaches a result makes it NaN).  The interior is ``fill``, or NaN where
    none is given: an element a non-accumulating kernel never writes then fails
    ``assert_within``.  (Integer dtypes: bands 0xA5; default interior 0xFF,
    which no window index equals and which reads as NaN in an fp32 workspace.)"""
    numel = 1
    for s in shape:
        numel *= int(s)
    band = default_band(shape, dtype) if band is None else int(band)
    fp = dtype.is_floating_point
    if not fp:
        poison = 0xA5
    raw = torch.full((numel + 2 * band,), poison, dtype=dtype, device=dev)
    view = raw[band:band + numel].view(shape)
    if fill is not None:
        view.copy_(fill)
    else:
        view.fill_(math.nan if fp else 0xFF)
    assert not raw.is_cuda or view.data_ptr() % 256 == 0
    return Guarded(raw, band, poison), view


def intact(buf):
    """both bands of a ``guarded`` buffer still hold their poison"""
    lo, hi = buf.raw[:buf.band], buf.raw[buf.raw.numel() - buf.band:]
    if isinstance(buf.poison, float) and math.isnan(buf.poison):
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    want = torch.full((), buf.poison, dtype=buf.raw.dtype, device=buf.raw.device)
    return bool((lo == want).all() and (hi == want).all())


# ---------------------------------------------------------------------------
# the BN backward family (csrc/bn.hip: rr_bn_bwd_reduce / _reduce_gm /
# _finalize / _apply, all mask kinds, one or two BNs, train and eval mode),
# the residual / PReLU affine forward, the column sums, and the fused
# final-conv tail (rr_conv_out_bwd_bnred + rr_bn_bwd_apply_convout)
#
# The reduce skeleton.  A workgroup sums its own rows in fp32 (per-thread
# chains, an LDS pass over the thread rows) into ONE partial row; the partial
# rows are summed in fp64 (the finalize; the tests sum the slab in fp64
# themselves).  So no fp32 sum has more than ``n_sum`` = rows_per_block =
# ceil(P / blocks) terms per channel, and the any-order bound (n - 1) u
# sum|term| holds block by block: in all, n_sum u sum_p |term_p|.  ``n_sum``
# defaults to P (one fp32 sum of everything, the model of stats_bound).  The
# fp64 sum of <= 1024 rows adds 1024 2^-53, inside the u the count leaves over
# ((n - 1) needed, n charged).
#
# gm and its error e_p as the sums see it.  g carries e_g (0 for a plain
# tensor; u |g + unpool| for the one fp32 add of kinds 3 and 5; the stored
# bound of the recomputed final-conv grad).  A keep-mask is a tensor of its
# own once its sign is unambiguous (``sign_ambiguous`` for kind 2,
# ``sign_ambiguous2`` for the recomputed mask of kinds 4 and 5; an ``aux > 0``
# mask of a stored tensor is exact): kept elements keep e_g, dropped ones are
# exactly 0, and the PReLU slope of kind 2 is one fp32 product,
# |alpha| e_g + u |alpha g|.  rr_bn_bwd_reduce_gm sums the STORED gm: e_p is
# then the stored bound.
#
# Column sums [c, 3] = (sum gm, sum gm xhat0, sum gm xhat1), xhat_i = (t_i -
# mean_i) invstd_i in fp32: two roundings, both relative to the result (the
# subtraction is rounded once, the product once), and the product gm xhat one
# more: 3 u |gm xhat| per term.
#   sum gm:        sum_p e_p            + n_sum u sum_p |gm_p|
#   sum gm xhat_i: sum_p e_p |xhat_i,p| + (n_sum + 4) u sum_p |gm_p xhat_i,p|
# (3 for the term, 1 for the second order).
#
# The alpha sum of kind 2, sum over u_p <= 0 of g_p u_p over pixels AND
# channels: bn.hip sums it in fp32 per workgroup (n_sum C terms) and in fp64
# across.  The fp32 u_p is within d_p = 2 u (|t_p s| + |b|) of the exact one,
# the product is rounded once:
#   sum_{u <= 0} (e_g |u_p| + |g_p| d_p + 2 u |g_p u_p|) + n_sum C u sum |g_p u_p|
#
# The finalize is fp64 and stores fp32 (``cast32``): dbeta_i = sum gm,
# dgamma_i = sum gm xhat_i, dalpha; coef [c][2][3] = (a_i = gamma_i invstd_i
# as an fp32 product, m0 = sum gm / P, m_i = sum gm xhat_i / P); eval mode
# divides by +inf: m0 = m_i = 0 exactly, and dbias_i = a_i * (float) sum gm
# (three fp32 roundings: 4 u with the second order).
#
# The apply.  Train: dt_i = a_i (gm - m0 - xhat_i m_i); eval: dt_i = a_i gm.
# The 8-channel kernel folds it to A gm + B t + D with q = a m inv, B = -q, D
# = fma(q, mean, -a m0) and two fmas; the 4-channel kernel evaluates it as
# written.  Either way at most 7 fp32 roundings touch any one of the four terms
# a gm, a m0, q t, q mean, each relative to a value no larger than their
# magnitudes' sum: 8 u (|a| (|gm| + |m0| + |m_i| inv (|t| + |mean|))), as
# pool_bwd_bounds.  Added to a e_p (the apply's own gm: unrounded except where
# it reads the stored one) and a (sums' bounds / P) through m0 and m_i; one
# store.

def _col(x):
    return x.reshape(-1, x.shape[-1]).sum(0)


_Z = torch.zeros((), dtype=torch.float64)


def sign_ambiguous2(t0, s0, b0, t1, s1, b1):
    """elements whose fp32 v = (t0 s0 + b0) + (t1 s1 + b1) (the recomputed
    ReLU mask of kinds 4 and 5, the residual tail's forward) can differ in
    sign from the exact one under any contraction choice: each affine is within
    2 u (|t s| + |b|) of exact, the add rounds once more (relative to v: it
    cannot change a sign): |v| <= 4 u (|t0 s0| + |b0| + |t1 s1| + |b1|), or
    v = 0.  t s is exact in fp64 (8 or 24 bits times 24); the three fp64 adds
    are 2^-29 of the threshold."""
    p0, p1 = t0.double() * s0.double(), t1.double() * s1.double()
    b0, b1 = b0.double(), b1.double()
    v = (p0 + b0) + (p1 + b1)
    return (v.abs() <= 4.0 * U * (p0.abs() + b0.abs() + p1.abs() + b1.abs())) | (v == 0)


def _away(t, dtype):
    ity = torch.int16 if dtype == torch.bfloat16 else torch.int32
    return (t.to(dtype).view(ity) + 1).view(dtype).float()          # sign-magnitude: one ulp away from zero


def make_sign_unambiguous2(t0, s0, b0, t1, s1, b1, dtype=torch.bfloat16):
    """(t0', moved): t0 with every ambiguous element moved to the neighbouring
    value of ``dtype`` away from zero, repeated until none is left; ``moved``
    marks the elements that changed"""
    t = t0.float().clone()
    for _ in range(8):
        bad = sign_ambiguous2(t, s0, b0, t1, s1, b1)
        if not bool(bad.any()):
            break
        t = torch.where(bad, _away(t, dtype), t)
    return t, t != t0.float()


def unpooled(pdy, idx, h, w):
    """the MaxPool2d(2) backward of pdy [n, h/2, w/2, c] through the window
    index idx = 2 dy + dx, fp64 [n, h, w, c]"""
    pdy = pdy.double()
    n, _, _, c = pdy.shape
    up = torch.zeros(n, h, w, c, dtype=torch.float64)
    win = up.view(n, h // 2, 2, w // 2, 2, c)
    for k in range(4):
        win[:, :, k // 2, :, k % 2, :] = torch.where(idx == k, pdy, _Z)
    return up


def bn_bwd_bounds(g, keep, t, mean, invstd, gamma, out_dtype, eval_mode=False, slope=None, u=None, du=None,
                  e_g=None, n_sum=None, sum_stored=False):
    """The general BN backward of nbn = len(t) BatchNorms fed by one gm.
    g [..., c] the upstream grad (fp64, with the bound ``e_g`` or exact), keep
    the boolean mask computed by the caller (kinds 0: all true; 1, 3: aux > 0;
    4, 5: the recomputed v > 0; 2: u > 0), ``slope`` the PReLU slope of kind 2
    with u = t s + b (fp64) and ``du`` the bound of its fp32 value; t, mean,
    invstd, gamma lists of nbn tensors.  ``sum_stored``: the sums are taken of
    the stored gm, which the apply then reads (rr_bn_bwd_reduce_gm).  Returns {name: (ref64, bound64)} of gm, sums [c, 3], coef [c,
    2, 3], dgamma0/1, dbeta0/1, dt0/1, with a slope alpha (the fp64 sum) and
    dalpha, in eval mode dbias0/1.  The derivation is above."""
    nbn = len(t)
    assert nbn in (1, 2) and len(mean) == len(invstd) == len(gamma) == nbn
    g = g.double()
    c = g.shape[-1]
    P = g.numel() // c
    n_sum = P if n_sum is None else int(n_sum)
    e_g = torch.zeros_like(g) if e_g is None else e_g.double()
    if slope is None:
        gm = torch.where(keep, g, _Z)
        e_raw = torch.where(keep, e_g, _Z)
    else:
        assert abs(slope) <= 1 and u is not None and du is not None
        gm = torch.where(keep, g, slope * g)
        e_raw = torch.where(keep, e_g, abs(slope) * e_g + U * gm.abs())
    gm_b = _stored(gm, e_raw, out_dtype)
    e = gm_b if sum_stored else e_raw
    t = [x.double() for x in t]
    mean, invstd = [x.double() for x in mean], [x.double() for x in invstd]
    a = [(torch.ones(c, dtype=torch.float64) if gm_ is None else gm_.double()) * iv for gm_, iv in zip(gamma, invstd)]
    xhat = [(t[i] - mean[i]) * invstd[i] for i in range(nbn)]
    zc = torch.zeros(c, dtype=torch.float64)
    cols, cols_b = [_col(gm)], [_col(e) + n_sum * U * _col(gm.abs())]
    for i in range(2):
        if i < nbn:
            tx = gm * xhat[i]
            cols.append(_col(tx))
            cols_b.append(_col(e * xhat[i].abs()) + (n_sum + 4) * U * _col(tx.abs()))
        else:
            cols.append(zc)
            cols_b.append(zc)                       # one BN: the third column is exactly zero
    sums, sums_b = torch.stack(cols, 1), torch.stack(cols_b, 1)
    out = {"gm": (gm, gm_b), "sums": (sums, sums_b)}
    if slope is not None:
        neg = ~keep
        gu = torch.where(neg, g * u, _Z)
        a_b = torch.where(neg, e_g * u.abs() + g.abs() * du + 2.0 * U * gu.abs(), _Z).sum() \
            + n_sum * c * U * gu.abs().sum()
        out["alpha"] = (gu.sum(), a_b)
        out["dalpha"] = cast32(out["alpha"])
    coef = torch.zeros(c, 2, 3, dtype=torch.float64)
    coef_b = torch.zeros_like(coef)
    for i in range(nbn):
        s0, s0b, si, sib = sums[:, 0], sums_b[:, 0], sums[:, 1 + i], sums_b[:, 1 + i]
        out["dbeta%d" % i] = cast32((s0, s0b))
        out["dgamma%d" % i] = cast32((si, sib))
        if eval_mode:
            m0, mi, m0b, mib = zc, zc, zc, zc
            ref = a[i] * s0
            out["dbias%d" % i] = (ref, a[i].abs() * s0b + 4.0 * U * (ref.abs() + a[i].abs() * s0b))
        else:
            (m0, m0b), (mi, mib) = cast32((s0 / P, s0b / P)), cast32((si / P, sib / P))
        coef[:, i, 0], coef_b[:, i, 0] = a[i], U * a[i].abs()
        coef[:, i, 1], coef_b[:, i, 1] = m0, m0b
        coef[:, i, 2], coef_b[:, i, 2] = mi, mib
        dt = a[i] * (gm - m0 - xhat[i] * mi)
        mag = a[i].abs() * (gm.abs() + e + (m0.abs() + m0b) + (mi.abs() + mib) * invstd[i] * (t[i].abs() + mean[i].abs()))
        ev = a[i].abs() * (e + m0b + xhat[i].abs() * mib) + 8.0 * U * mag
        out["dt%d" % i] = (dt, _stored(dt, ev, out_dtype))
    out["coef"] = (coef, coef_b)
    return out


# ---------------------------------------------------------------------------
# rr_affine_act / rr_affine_act_pool
#
#   u = x s + b            fp32, fma or not: within 2 u (|x s| + |b|)
#   a = PReLU(u)           (when a slope is given) one more fp32 product, u |a|;
#                          PReLU with |alpha| <= 1 is 1-Lipschitz and continuous,
#                          so the error of u passes through whatever its sign
#   r = res rs + rb        within 2 u (|res rs| + |rb|); a plain res is exact
#   v = a + r              one fp32 add: u |v| (+ second order: u times the errors)
#   y = ReLU(v)            1-Lipschitz
# then one store.  Without res the add and r drop out.

def affine_res_bound(x, s, b, out_dtype, alpha=None, res=None, rs=None, rb=None, relu=False):
    """(ref64, bound64) of y = act(x s + b [+ res | + res rs + rb]) of x
    [..., c], act in {none, PReLU before the residual (``alpha``), ReLU after
    (``relu``)}, stored once in ``out_dtype``"""
    x, s, b = x.double(), s.double(), b.double()
    v = x * s + b
    ev = 2.0 * U * ((x * s).abs() + b.abs())
    if alpha is not None:
        assert abs(alpha) <= 1
        v = torch.where(v > 0, v, alpha * v)
        ev = ev + U * v.abs()
    if res is not None:
        r = res.double()
        if rs is not None:
            er = 2.0 * U * ((r * rs.double()).abs() + rb.double().abs())
            r = r * rs.double() + rb.double()
            ev = ev + er
        else:
            assert rb is None
        v = v + r
        ev = ev + U * (v.abs() + ev)
    if relu:
        v = v.clamp_min(0)
    return v, _stored(v, ev, out_dtype)


def affine_pool_bounds(rb, operands):
    """The pooled companion of ``affine_res_bound``'s (ref, bound) NHWC ``rb``:
    (pooled ref, pooled bound) by ``pooled`` (the window max of the STORED
    values: each within its bound of ref, and the max is 1-Lipschitz), the
    first-max window index 2 dy + dx of ref, and ``sure`` -- the windows whose
    index is decided: every other element of the window either lies below the
    maximum by more than the two bounds (ref_k + bound_k < ref_a - bound_a:
    then the stored values are ordered the same way), or has bit-identical
    ``operands`` (x, res, ...: same channel, same arithmetic, the same stored
    value, and the first of them wins in ref as in the kernel).  Windows with a
    tie inside the bound are not sure and left out of the index check."""
    ref, bound = rb
    n, h, w, c = ref.shape

    def win(t):
        return t.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    wr, wb = win(ref), win(bound)
    best = wr.max(-1, keepdim=True).values
    idx = (wr == best).to(torch.uint8).argmax(-1)                      # the first maximum
    ra, ba = wr.gather(-1, idx[..., None]), wb.gather(-1, idx[..., None])
    same = torch.ones_like(wr, dtype=torch.bool)
    for o in operands:
        wo = win(o.double())
        same &= wo == wo.gather(-1, idx[..., None])
    ok = (wr + wb < ra - ba) | same
    return pooled(rb), idx.to(torch.uint8), ok.all(-1)


# ---------------------------------------------------------------------------
# rr_channel_sum / rr_bn_stats: plain tensors, e_p = 0 in stats_bound's model,
# the reduce skeleton above (n_sum terms per fp32 sum, fp64 across).

def colsum_bound(x, n_sum=None, out0=None):
    """(ref64, bound64) [c] of the column sums of x [P, c], stored fp32 once
    (``cast32``); with ``out0`` the accumulate form out0 + (float) s: one more
    fp32 add"""
    x = x.double()
    n_sum = x.shape[0] if n_sum is None else int(n_sum)
    ref, bound = cast32((x.sum(0), n_sum * U * x.abs().sum(0)))
    if out0 is not None:
        ref = ref + out0.double()
        bound = bound + U * (ref.abs() + bound)
    return ref, bound


def colstats_bound(x, n_sum=None):
    """(ref64, bound64) [c, 2] = (sum, sum of squares) of x [P, c] summed over
    the partial rows: the squares are fp32 products or the exact product of an
    fma, one rounding more per term at the most"""
    x = x.double()
    n_sum = x.shape[0] if n_sum is None else int(n_sum)
    q = (x * x).sum(0)
    return torch.stack((x.sum(0), q), 1), torch.stack((n_sum * U * x.abs().sum(0), (n_sum + 1) * U * q), 1)


# ---------------------------------------------------------------------------
# rr_conv_out_bwd_bnred -> rr_bn_bwd_finalize -> rr_bn_bwd_apply_convout

def convout_tail_bounds(dy, wt, keep, t, mean, invstd, gamma, out_dtype, x, n_sum=None):
    """The final 1x1 conv's backward fused with the BN backward of the block
    before it.  dy [n, 3, h, w] fp32 (NCHW), wt [3, c]: g = round_T(sum_co dy
    w), K = 3 fp32 products of fp32 operands (2 K u A), continuous through the
    store (``_stored``): the reduce sums that stored g and the apply reads it
    (both recompute and round it); then ``bn_bwd_bounds`` with nbn = 2 and
    that bound as e_g.  dw [3, c] = sum_p dy x and db [3] = sum_p dy are K = P
    sums of fp32 products (``wgrad_bound``'s model), x [n, h, w, c] the block
    output."""
    dyn = dy.double().permute(0, 2, 3, 1)                               # [n, h, w, 3]
    w64 = wt.double()
    g = dyn @ w64
    e_acc = 2.0 * 3 * U * (dyn.abs() @ w64.abs())
    e_g = _stored(g, e_acc, out_dtype)
    out = bn_bwd_bounds(g, keep, t, mean, invstd, gamma, out_dtype, e_g=e_g, n_sum=n_sum)
    P = g.numel() // g.shape[-1]
    d2, x2 = dyn.reshape(P, 3), x.double().reshape(P, -1)
    out["dw"] = _finish(d2.t() @ x2, d2.abs().t() @ x2.abs(), P, torch.float32, 1)
    out["db"] = _finish(d2.sum(0), d2.abs().sum(0), P, torch.float32, 1)
    return out


# ---------------------------------------------------------------------------
# the boundary layers: csrc/conv_in.hip (3 -> 64 from the NCHW fp32 image),
# csrc/conv_out.hip (64 -> 3 into NCHW fp32) and rr_prelu_bwd
#
# Operands.  rr_conv_in_mfma and rr_conv_in_wgrad_act[_rec] multiply the image
# rounded to bf16 (RNE) with the weights and the bias as the kpad-32 pack
# holds them (bf16, the bias in column 27 against a patch column of ones): all
# products are exact in fp32, the forward sums K = 28 of them from a zero
# accumulator.  The VALU entry points (rr_conv_in_fwd / _wgrad / _dgrad,
# rr_conv_out_fwd / _bwd) multiply the fp32 image and weights unrounded with
# activations or grads in T: one rounding per product, inside the 2 K u A.
#
# No mask is sign-ambiguous: t and x are given tensors compared with 0
# exactly; the forward's activations are continuous (1-Lipschitz).
#
# The reduce skeleton (as the BN family above): a workgroup sums the terms of
# its pixel range in fp32 into one partial row, the rows are summed in fp64
# (rr_colreduce + a finalize) and stored once as fp32 (``cast32``):
#   n_sum u sum|term|, then cast32,
# n_sum the number of terms of the longest fp32 sum -- the any-order bound
# (n - 1) u sum|term| of n terms, plus one u where the products are rounded.
# The splits below restate each launcher's; the tests assert them against the
# library's workspace queries (partial rows of ``blocks`` workgroups in fp32 +
# min(blocks, 64) column-reduce rows in fp64).

def _ceil_div(a, b):
    return -(-int(a) // int(b))


def colreduce_chunks(rows):
    """rr_colreduce's fp64 rows behind the partial slabs"""
    return max(1, rows) if rows < 64 else 64


def _split_bytes(blocks, cols):
    return blocks * cols * 4 + colreduce_chunks(blocks) * cols * 8


def conv_in_act_split(P):
    """(workgroups, pixels per workgroup) of rr_conv_in_wgrad_act[_rec]:
    ceil(P / 512) ranges (2048 at the most) of whole 64-pixel steps"""
    blocks = max(1, min(2048, _ceil_div(P, 512)))
    return blocks, _ceil_div(_ceil_div(P, blocks), 64) * 64


def conv_in_act_workspace(P):
    """rr_conv_in_wgrad_act_workspace: slabs of [64][32] + a dalpha row of 32"""
    return _split_bytes(conv_in_act_split(P)[0], 64 * 32 + 32)


def conv_in_wgrad_split(P):
    """rr_conv_in_wgrad: ceil(P / 2048) ranges, 1024 at the most"""
    blocks = max(1, min(1024, _ceil_div(P, 2048)))
    return blocks, _ceil_div(P, blocks)


def conv_in_wgrad_workspace(P, cout):
    return _split_bytes(conv_in_wgrad_split(P)[0], cout * 32)


def conv_out_split(P):
    """rr_conv_out_bwd: ceil(P / 1024) ranges, 2048 at the most"""
    blocks = max(1, min(2048, _ceil_div(P, 1024)))
    return blocks, _ceil_div(P, blocks)


def conv_out_workspace(P, cin, cout):
    """slabs of cout dw rows + one db row, cin slots each"""
    return _split_bytes(conv_out_split(P)[0], (cout + 1) * cin)


def conv_out_db_row_holds(cin, cout):
    """the db row of a slab [(cout + 1)][cin] has cin slots for cout values:
    with cin < cout, value co >= cin of workgroup b lands at slab offset
    (cout + 1) cin + (co - cin) -- the next workgroup's slab, or, for the last
    workgroup, the column-reduce rows behind the slabs"""
    return cout <= cin


def prelu_bwd_chain(count, blocks):
    """terms of the longest per-thread fp32 chain of rr_prelu_bwd: 4 per
    grid-stride trip over the count / 4 vectors, 1 more for the count % 4 tail"""
    return 4 * _ceil_div(max(count // 4, 1), blocks * 256) + 1


def bf16r(t):
    """t rounded to bf16 (RNE), fp64"""
    return t.float().to(torch.bfloat16).double()


def patches3(x, kpad=None):
    """the 3x3 patch rows [P, 9 cin + 1] (or kpad columns) of x [n, cin, h, w],
    fp64: column j = ci 9 + ky 3 + kx holds x[n, ci, y + ky - 1, x + kx - 1] (0
    outside the image), column 9 cin holds 1, the rest 0 -- rr_im2col3's layout"""
    x = x.double()
    n, cin, h, w = x.shape
    col = F.unfold(x, 3, padding=1).permute(0, 2, 1).reshape(n * h * w, 9 * cin)
    out = torch.zeros(n * h * w, 9 * cin + 1 if kpad is None else kpad, dtype=torch.float64)
    out[:, :9 * cin] = col
    out[:, 9 * cin] = 1.0
    return out


def conv_in_pack(wt, b, kpad, dtype):
    """rr_pack_conv_in's [cout][kpad] in ``dtype`` (as fp32): the weights
    [cout][cin 9], the bias in column 9 cin, zeros up to kpad"""
    cout, kk = wt.shape[0], wt.shape[1] * 9
    out = torch.zeros(cout, kpad)
    out[:, :kk] = wt.reshape(cout, kk)
    if b is not None:
        out[:, kk] = b
    return out.to(dtype).float()


def conv_in_mfma_bounds(x, wt, b, act, alpha):
    """rr_conv_in_mfma of x [n, 3, h, w] fp32, wt [64, 3, 3, 3], b [64]: {pre,
    act: (ref64, bound64)} NHWC.  Operands: bf16(x), the bf16 kpad-32 pack; K =
    28 exact products from a zero accumulator (2 K u A); y_pre and y_act are
    each ONE bf16 store of the fp32 accumulator v (y_act = PReLU(v), not of
    the rounded y_pre: the slope's fp32 product adds u |alpha v|; act 0 and
    ReLU add nothing)."""
    n, _, h, w = x.shape
    pt = patches3(bf16r(x), 32)
    pack = conv_in_pack(wt, b, 32, torch.bfloat16).double()
    ref = (pt @ pack.t()).reshape(n, h, w, -1)
    e = 2.0 * 28 * U * (pt.abs() @ pack.abs().t()).reshape(n, h, w, -1)
    out = {"pre": (ref, _stored(ref, e, torch.bfloat16))}
    if act == 0:
        ra, ea = ref, e
    elif act == 1:
        ra, ea = ref.clamp_min(0), e
    else:
        assert abs(alpha) <= 1
        ra = torch.where(ref > 0, ref, alpha * ref)
        ea = e + U * ra.abs()
    out["act"] = (ra, _stored(ra, ea, torch.bfloat16))
    return out


def conv_in_gp(g, t, act, alpha):
    """gp = bf16(t > 0 ? g : fp32(alpha g)) (ReLU: alpha = 0) of g, t NHWC
    bf16-exact: the operand of the fused weight grad, reproduced bit for bit"""
    g32, t32 = g.float(), t.float()
    al = torch.tensor(float(alpha) if act == 2 else 0.0, dtype=torch.float32)
    return torch.where(t32 > 0, g32, al * g32).to(torch.bfloat16).double()


def conv_in_wgrad_act_bounds(x, g, t, act, alpha):
    """rr_conv_in_wgrad_act[_rec]: {dw [64, 27], db [64], dalpha 0-d}.
    dW[co][j] = sum_p gp[p, co] patch[p, j] of gp (``conv_in_gp``) and the bf16
    patch rows with their ones column (db): exact products, one MFMA
    accumulator per workgroup over its <= ppb pixels (n_sum = ppb), fp64
    across, one fp32 store.  dalpha = sum_{t <= 0} g t: g t exact in fp32 (8 x
    8 bits); a thread adds its 2 pixels x 8 channels of each 64-pixel step in
    one chain (16 ppb / 64 terms), a 256-wide LDS tree adds 8 levels: no term
    is touched by more than ppb / 4 + 8 fp32 adds; fp64 across, one store."""
    P = g.numel() // 64
    _, ppb = conv_in_act_split(P)
    gp = conv_in_gp(g, t, act, alpha).reshape(P, 64)
    pt = patches3(bf16r(x), 28)
    ref, S = gp.t() @ pt, gp.abs().t() @ pt.abs()
    r, bd = cast32((ref, ppb * U * S))
    out = {"dw": (r[:, :27].contiguous(), bd[:, :27].contiguous()), "db": (r[:, 27].contiguous(), bd[:, 27].contiguous())}
    term = torch.where(t.double() > 0, _Z, g.double() * t.double())
    out["dalpha"] = cast32((term.sum(), (ppb // 4 + 8) * U * term.abs().sum()))
    return out


def conv_in_wgrad_bounds(x, dy):
    """rr_conv_in_wgrad (VALU) of x [n, cin, h, w] fp32 unrounded and dy [n, h,
    w, cout] in T: (ref64, bound64) [cout, 9 cin + 1], the bias grad in the
    last column.  64-term fp32 stage sums (64 rounded products in one chain:
    64 u), folded into fp64, ONE fp32 store per workgroup (u of its partial),
    one more u for the second order and the fp64 folds: 66 u sum|term|; fp64
    across workgroups, one store (``cast32``)."""
    cout = dy.shape[-1]
    pt = patches3(x)
    d = dy.double().reshape(-1, cout)
    return cast32((d.t() @ pt, 66 * U * (d.abs().t() @ pt.abs())))


def conv_in_dgrad_bounds(dy, wt, dx0=None):
    """rr_conv_in_dgrad (and the packed image-grad route): dy [n, cout, h, w]
    (NCHW here), wt [cout, cin, 3, 3] -> the image grad, NHWC for
    ``assert_within(nchw=True)``; K = 9 cout (+ 1 accumulated into dx0, NCHW)"""
    dy, wt = dy.double(), wt.double()
    ref = _nhwc(F.conv_transpose2d(dy, wt, padding=1))
    A = _nhwc(F.conv_transpose2d(dy.abs(), wt.abs(), padding=1))
    return epilogue_bound((ref, A), 9 * wt.shape[0], None, torch.float32, extra=dx0)


def conv_out_bwd_bounds(dy, x, wt, mask_relu, dtype):
    """rr_conv_out_bwd of dy [n, cout, h, w] fp32, x [n, h, w, cin] in T, wt
    [cout, cin] fp32: dx = sum_co dy w (K = cout fp32 products), masked by x >
    0 (a tensor of its own), one store; dw [cout, cin] = sum_p dy x and db =
    sum_p dy: one fp32 sum of <= ppb rounded products per workgroup (n_sum =
    ppb, ``conv_out_split``), fp64 across, one store."""
    cout, cin = wt.shape
    d = dy.double().permute(0, 2, 3, 1).contiguous()
    w64, x64 = wt.double(), x.double()
    dx = _finish(d @ w64, d.abs() @ w64.abs(), cout, dtype, 1)
    if mask_relu:
        dx = (torch.where(x64 > 0, dx[0], _Z), dx[1])
    P = x64.numel() // cin
    _, ppb = conv_out_split(P)
    d2, x2 = d.reshape(P, cout), x64.reshape(P, cin)
    return {"dx": dx, "dw": cast32((d2.t() @ x2, ppb * U * (d2.abs().t() @ x2.abs()))),
            "db": cast32((d2.sum(0), ppb * U * d2.abs().sum(0)))}


def conv1x1_nchw_bound(y, wq, bias):
    """out [n, h, w, cout] (for ``assert_within(nchw=True)``) = bias + y w of
    y [n, h, w, c] and wq [cout, c] as stored: K = c + 1"""
    y, wq, bias = y.double(), wq.double(), bias.double()
    return _finish(y @ wq.t() + bias, y.abs() @ wq.abs().t() + bias.abs(), wq.shape[1] + 1, torch.float32, 1)


def prelu_bwd_bounds(dy, t, alpha, dtype, blocks):
    """rr_prelu_bwd of flat dy, t in T: dx = t > 0 ? dy : alpha dy, one fp32
    product (u |alpha dy|), one store; dalpha = sum_{t <= 0} dy t: a product
    (exact in bf16, one rounding in fp32), a per-thread chain of
    ``prelu_bwd_chain`` terms and a 256-wide tree (8 levels) per workgroup,
    fp64 across the ``blocks`` partials, one store."""
    assert abs(alpha) <= 1
    d, t = dy.double(), t.double()
    ref = torch.where(t > 0, d, alpha * d)
    dx = (ref, _stored(ref, torch.where(t > 0, _Z, U * ref.abs()), dtype))
    term = torch.where(t > 0, _Z, d * t)
    n_sum = prelu_bwd_chain(d.numel(), blocks) + 8 + (0 if dtype == torch.bfloat16 else 1)
    return {"dx": dx, "dalpha": cast32((term.sum(), n_sum * U * term.abs().sum()))}


# ---------------------------------------------------------------------------
# shared inputs of the boundary tests

def with_zeros(t, seed, share=0.02):
    """t with about ``share`` of its elements set to an exact 0, half of them
    to -0.0: what a mask written as ``>= 0`` instead of ``> 0`` gets wrong (a
    ReLU output, the x of the last conv's backward, is full of them)"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(t.shape, generator=g)
    t = torch.where(r < share, torch.zeros(()), t)
    return torch.where(r < share / 2, torch.full((), -0.0), t)


TAIL_SHAPES = [(3, 5, 7), (2, 8, 8), (1, 16, 24)]
_TAIL = {}


def tail_inputs(shape):
    """one set of host inputs of the residual tail + final 1x1 conv per shape,
    shared by the tests and left unchanged"""
    if shape not in _TAIL:
        def rnd(*sh, seed):
            return torch.randn(*sh, generator=torch.Generator().manual_seed(seed))
        n, h, w = shape
        sc = [rnd(64, seed=3) * 0.7, rnd(64, seed=4) * 0.7]          # about half the scales negative
        _TAIL[shape] = dict(t2=rnd(n, h, w, 64, seed=1).to(torch.bfloat16), s=rnd(n, h, w, 64, seed=2).to(torch.bfloat16),
                            sc=sc, sh=[rnd(64, seed=5) * 0.3, rnd(64, seed=6) * 0.3],
                            wt=rnd(3, 64, 1, 1, seed=7) / 8.0, bias=rnd(3, seed=8))
        assert all(int((v < 0).sum()) >= 8 for v in sc)
    return _TAIL[shape]
