"""Every launching entry point refuses a dtype that is neither RR_F32 nor
RR_BF16 (include/roadrestore.h, next to rr_dtype): RR_EINVAL, and not a byte
of any buffer it was handed is written.

One table of (entry point, argument builder).  Each builder gives otherwise
valid arguments at the smallest shape the call accepts; every pointer is a
live 1-MiB device allocation (far more than the fp32 reading of the shape
needs, so that a library that took the unknown dtype for fp32 -- as most of
these calls once did -- would stay inside it), inputs zero, outputs and
workspaces filled with a sentinel byte.  The call runs with dtype 7, then, as
the control that the other arguments are indeed valid, with RR_BF16 (the dtype
every route takes), which must return RR_OK -- or, for the three calls whose
only kernels start at batches of 32768 and 65536 pixels, get as far as the
routing (CONTROL).
"""
import ctypes as C
import os
import re

import pytest
import torch

import roadrestore
from roadrestore import _lib as L

pytestmark = pytest.mark.gpu

BAD = 7
RR_EINVAL = -1
NB = 1 << 20          # bytes of every buffer
SENTINEL = 0xA5
N, H, W = 1, 4, 4     # the small map of the plain calls
P = N * H * W
C8 = 8
H64 = 8               # the 64-channel map of the descriptor calls and the 64-channel conv_out forms
P64 = N * H64 * H64

RR_EUNSUPPORTED = -2
# the control's status where it is not RR_OK: streaming-kernel-only calls, no
# route at this size (past the argument checks, which is what the control is for)
CONTROL = {"rr_igemm_dgrad_sc": RR_EUNSUPPORTED, "rr_igemm_pre": RR_EUNSUPPORTED,
           "rr_wgrad_pre": RR_EUNSUPPORTED}

# return a count or a yes/no for a descriptor and launch nothing
QUERIES = {"rr_igemm_stat_blocks", "rr_igemm_bnbwd_rows", "rr_igemm_pre_ok", "rr_wgrad_pre_ok",
           "rr_bn_bwd_blocks"}


class Bufs:
    """The device buffers of one call."""

    def __init__(self):
        self.outs, self.keep = [], []

    def zeros(self):
        t = torch.zeros(NB, dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()

    def out(self):
        t = torch.full((NB,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.outs.append(t)
        return t.data_ptr()

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in self.outs)


def igemm_desc(dt, **kw):
    f = dict(dtype=dt, mode=L.RR_CONV3X3, n=N, h=H64, w=H64, c_in1=64, c_in2=0, c_out=64, out_split=0,
             act=0, accumulate=0, has_bias=0, has_mask=0, want_stats=0, out_nchw=0)
    f.update(kw)
    return L.IgemmDesc(**f)


def wgrad_desc(dt, **kw):
    f = dict(dtype=dt, mode=L.RR_CONV3X3, n=N, h=H64, w=H64, c_in1=64, c_in2=0, c_out=64, accumulate=0)
    f.update(kw)
    return L.WgradDesc(**f)


def bnbwd_desc(dt, **kw):
    f = dict(dtype=dt, P=P64, C=64, mask_kind=0, nbn=1, h=H64, w=H64, pool_dy=None, pool_idx=None,
             eval=0, dbias0=None, dbias1=None)
    f.update(kw)
    return L.BnBwdDesc(**f)


def ws_of(size):
    assert 0 < size <= NB, size
    return size


# builder(lib, dtype, b) -> argument tuple (without the trailing stream)
def _plain(name, *rest):
    """dtype first, then fixed arguments; 'i' = zero input, 'o' = sentinel output"""
    def build(lib, dt, b):
        return (dt,) + tuple(b.zeros() if a == "i" else b.out() if a == "o" else a for a in rest)
    return name, build


def _loss(name, *rest):
    def build(lib, dt, b):
        return (0, dt) + tuple(b.zeros() if a == "i" else b.out() if a == "o" else a for a in rest)
    return name, build


def _pack_batch(lib, dt, b):
    job = L.PackJob(w=b.zeros(), w_fwd=b.out(), w_dgrad=b.out(), c_out=8, c_in=8, k=3, pad_=0, begin=0)
    jobs = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).cuda()
    b.keep.append(jobs)
    return (dt, 1, jobs.data_ptr(), 8 * 8 * 9)


def _igemm(lib, dt, b):
    return (C.byref(igemm_desc(dt)), b.zeros(), None, b.zeros(), None, b.out(), None, None, None)


def _igemm_ex(lib, dt, b):
    d = igemm_desc(dt, act=L.RR_ACT_PRELU, has_bias=1)
    return (C.byref(d), b.zeros(), None, b.zeros(), b.zeros(), b.zeros(), None, b.out(), None, None, None)


def _igemm_pool(lib, dt, b):
    d = igemm_desc(dt, act=L.RR_ACT_RELU, has_bias=1)
    return (C.byref(d), b.zeros(), None, b.zeros(), b.zeros(), b.out(), b.out())


def _igemm_dgrad_sc(lib, dt, b):
    return (C.byref(igemm_desc(dt)), b.zeros(), b.zeros(), b.zeros(), b.zeros(), 64, b.out())


def _igemm_pre(lib, dt, b):
    d = igemm_desc(dt, has_bias=1, want_stats=1)
    return (C.byref(d), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.out(), b.out())


def _igemm_bnbwd(lib, dt, b):
    return (C.byref(igemm_desc(dt)),) + tuple(b.zeros() for _ in range(8)) + (b.out(), b.out())


def _wgrad(lib, dt, b):
    d = wgrad_desc(dt)
    ws = ws_of(lib.rr_wgrad_workspace(C.byref(wgrad_desc(L.RR_BF16))))
    return (C.byref(d), b.zeros(), b.zeros(), None, b.out(), b.out(), ws)


def _wgrad_partial(lib, dt, b):
    ws = ws_of(lib.rr_wgrad_workspace(C.byref(wgrad_desc(L.RR_BF16))))
    return (C.byref(wgrad_desc(dt)), b.zeros(), b.zeros(), None, b.out(), ws)


def _wgrad_reduce(lib, dt, b):
    ws = ws_of(lib.rr_wgrad_workspace(C.byref(wgrad_desc(L.RR_BF16))))
    return (C.byref(wgrad_desc(dt)), b.zeros(), ws, b.out())


def _wgrad_pre(lib, dt, b):
    ws = ws_of(lib.rr_wgrad_workspace(C.byref(wgrad_desc(L.RR_BF16))))
    return (C.byref(wgrad_desc(dt)), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.out(), b.out(), ws)


def _bn_reduce(lib, dt, b):
    return (C.byref(bnbwd_desc(dt)), b.zeros(), None, None, None, None, b.zeros(), b.zeros(), b.zeros(),
            None, None, None, b.out())


def _bn_reduce_gm(lib, dt, b):
    d = bnbwd_desc(dt, mask_kind=1)
    return (C.byref(d), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.zeros(), b.out(), b.out())


def _bn_finalize(lib, dt, b):
    return (C.byref(bnbwd_desc(dt)), b.zeros(), b.zeros(), b.zeros(), None, None, b.out(), b.out(), None,
            None, None, b.out())


def _bn_finalize_rows(lib, dt, b):
    ws = ws_of(lib.rr_bn_bwd_finalize_rows_workspace(64, 4))
    return (C.byref(bnbwd_desc(dt)), 4, b.zeros(), 0, None, b.zeros(), b.zeros(), b.out(), b.out(), None,
            b.out(), b.out(), ws)


def _bn_apply(lib, dt, b):
    return (C.byref(bnbwd_desc(dt)), b.zeros(), None, None, None, None, b.zeros(), b.zeros(), b.zeros(),
            None, None, None, b.zeros(), b.out(), None, None)


def _bn_apply_convout(lib, dt, b):
    d = bnbwd_desc(dt, mask_kind=4, nbn=2)
    return (C.byref(d), H64, H64, b.zeros(), b.zeros(), 3) + tuple(b.zeros() for _ in range(9)) + \
        (b.out(), b.out())


def _conv_out_bwd_bnred(lib, dt, b):
    d = bnbwd_desc(dt, mask_kind=4, nbn=2)
    ws = ws_of(lib.rr_conv_out_bwd_bnred_workspace(P64, 64, 3))
    return (C.byref(d), N, H64, H64, 3) + tuple(b.zeros() for _ in range(9)) + \
        (b.out(), b.out(), b.out(), b.out(), ws)


def _conv_in_wgrad(lib, dt, b):
    ws = ws_of(lib.rr_conv_in_wgrad_workspace(N, H, W, 3, 64))
    return (dt, N, H, W, 3, 64, b.zeros(), b.zeros(), b.out(), b.out(), b.out(), ws)


def _conv_out_bwd(cin, cout, hw):
    def build(lib, dt, b):
        ws = ws_of(lib.rr_conv_out_bwd_workspace(N, hw, hw, cin, cout))
        return (dt, N, hw, hw, cin, cout, b.zeros(), b.zeros(), b.zeros(), b.out(), 0, b.out(), b.out(),
                b.out(), ws)
    return build


def _channel_sum(lib, dt, b):
    ws = ws_of(lib.rr_channel_sum_workspace(P, C8))
    return (dt, P, C8, b.zeros(), b.out(), 0, b.out(), ws)


def _loss_fwd(lib, dt, b):
    ws = ws_of(lib.rr_loss_workspace(64))
    return (0, dt, 64, b.zeros(), b.zeros(), b.out(), 1.0, 0, b.out(), ws)


TABLE = [
    ("rr_igemm", _igemm), ("rr_igemm_ex", _igemm_ex), ("rr_igemm_pool", _igemm_pool),
    ("rr_igemm_dgrad_sc", _igemm_dgrad_sc), ("rr_igemm_pre", _igemm_pre), ("rr_igemm_bnbwd", _igemm_bnbwd),
    ("rr_wgrad", _wgrad), ("rr_wgrad_partial", _wgrad_partial), ("rr_wgrad_reduce", _wgrad_reduce),
    ("rr_wgrad_pre", _wgrad_pre),
    ("rr_bn_bwd_reduce", _bn_reduce), ("rr_bn_bwd_reduce_gm", _bn_reduce_gm),
    ("rr_bn_bwd_finalize", _bn_finalize), ("rr_bn_bwd_finalize_rows", _bn_finalize_rows),
    ("rr_bn_bwd_apply", _bn_apply), ("rr_bn_bwd_apply_convout", _bn_apply_convout),
    ("rr_conv_out_bwd_bnred", _conv_out_bwd_bnred),
    _plain("rr_pack_conv", 8, 8, 3, "i", "o", "o"),
    ("rr_pack_conv_batch", _pack_batch),
    _plain("rr_pack_convT", 8, 8, "i", "o", "o"),
    _plain("rr_pack_conv_in", 64, 3, 32, "i", "i", "o"),
    _plain("rr_im2col3", N, H, W, 3, 32, "i", "o"),
    _plain("rr_conv_in_fwd", N, H, W, 3, 64, "i", "i", "i", 0, "i", "o"),
    ("rr_conv_in_wgrad", _conv_in_wgrad),
    _plain("rr_conv_in_dgrad", N, H, W, 3, 64, "i", "i", "o", 0),
    _plain("rr_conv_out_fwd", N, H, W, C8, 3, "i", "i", "i", "o"),
    ("rr_conv_out_bwd", _conv_out_bwd(C8, 3, H)),
    ("rr_conv_out_bwd", _conv_out_bwd(64, 3, H64)),          # the 64 -> 3 kernel
    _plain("rr_affine_act", P, C8, "i", "i", "i", None, None, None, None, 1, "o"),      # 8-wide
    _plain("rr_affine_act", P, 12, "i", "i", "i", None, None, None, None, 1, "o"),      # 4-wide
    _plain("rr_affine_act_pool", N, H, W, C8, "i", "i", "i", None, None, None, 1, "o", "o", "o"),
    ("rr_channel_sum", _channel_sum),
    _plain("rr_bn_stats", P, C8, "i", "o"),
    _plain("rr_maxpool2_fwd", N, H, W, C8, "i", "o", "o"),
    _plain("rr_maxpool2_fwd", N, H, W, 4, "i", "o", "o"),
    _plain("rr_maxpool2_bwd", N, H // 2, W // 2, C8, "i", "i", "o", 0, None),
    _plain("rr_maxpool2_bwd", N, H // 2, W // 2, 4, "i", "i", "o", 0, None),
    _plain("rr_maxpool2_bwd_pooled", N, H, W, C8, "i", "i", "i", "o"),
    _plain("rr_nearest_resize", N, H, W, 5, 5, C8, "i", "o"),
    _plain("rr_nearest_resize_bwd", N, H, W, 5, 5, C8, "i", "o"),
    _plain("rr_adaptive_avgpool_flatten", N, H, W, C8, 2, 2, "i", "o"),
    _plain("rr_prelu_bwd", P * C8, "i", "i", "i", "o", "o", 1, "o"),
    _plain("rr_nchw_to_nhwc", N, C8, H, W, "i", "o"),
    _plain("rr_nhwc_to_nchw", N, C8, H, W, "i", "o"),
    ("rr_loss_fwd", _loss_fwd),
    _loss("rr_loss_bwd", 64, "i", "i", "i", 1.0, "o", "o", 0, 0),      # 8-wide
    _loss("rr_loss_bwd", 63, "i", "i", "i", 1.0, "o", "o", 0, 0),      # scalar
    _plain("rr_linear_wgrad", 1, 64, 8, "i", "i", "o", "o", 0),
    _plain("rr_linear_dgrad", 1, 64, 8, "i", "i", None, "o"),
]


def expected_names():
    """Status-returning entry points of _SIGS with a dtype argument
    (include/roadrestore.h names the parameters) or one of the three
    descriptors that carry a dtype."""
    descs = tuple(C.POINTER(t) for t in (L.IgemmDesc, L.WgradDesc, L.BnBwdDesc))
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "roadrestore.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    with_dtype = {m.group(1) for m in re.finditer(r"\b(rr_\w+)\s*\(([^)]*)\)\s*;", hdr)
                  if re.search(r"\bint\s+dtype\b", m.group(2))}
    names = set()
    for name, (res, args) in L._SIGS.items():
        if res is C.c_int and (name in with_dtype or (args and args[0] in descs)):
            names.add(name)
    assert with_dtype - {"rr_pack_conv_elems"} <= names, with_dtype - names     # (a count, not a status)
    return names - QUERIES


def test_table_covers_every_entry_point():
    assert {name for name, _ in TABLE} == expected_names()


@pytest.mark.parametrize("idx", range(len(TABLE)), ids=[f"{n}-{i}" for i, (n, _) in enumerate(TABLE)])
def test_unknown_dtype_is_refused(idx):
    name, build = TABLE[idx]
    lib = roadrestore.lib()
    fn = getattr(lib, name)
    b = Bufs()
    rc = fn(*build(lib, BAD, b), None)
    torch.cuda.synchronize()
    assert rc == RR_EINVAL, (name, rc)
    assert b.untouched(), name
    # the control: the same arguments with a dtype the library knows
    c = Bufs()
    rc = fn(*build(lib, L.RR_BF16, c), None)
    torch.cuda.synchronize()
    assert rc == CONTROL.get(name, 0), (name, rc)
