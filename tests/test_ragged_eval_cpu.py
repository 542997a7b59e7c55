"""Host-side contract of the ragged cv2.resize and the fused evaluation
(rr_cv_resize_ragged_u8, rr_eval_ragged_workspace, rr_eval_ragged_u8,
imgproc.restoration_quality): every bad argument is refused before any launch,
so these run without a GPU.  The pointers handed in are never dereferenced."""
import pytest
import torch

RR_EINVAL, RR_EWORKSPACE = -1, -4
# stand-ins for device pointers (8-byte aligned, never read: every call below
# must return before it launches)
IN, TAB, OUT, RST, PSNR, SSIM, WS = (0x1000 * k for k in range(1, 8))


def _lib():
    import roadrestore
    return roadrestore.lib()


def test_eval_workspace_query():
    L = _lib()
    assert L.rr_eval_ragged_workspace(2, 3, 7, 7) > 0
    assert L.rr_eval_ragged_workspace(64, 3, 224, 224) > 0
    # more images or more blocks never need less
    assert L.rr_eval_ragged_workspace(64, 3, 224, 224) >= 32 * L.rr_eval_ragged_workspace(2, 3, 7, 7)
    for n, c, oh, ow in [(2, 3, 6, 7), (2, 3, 7, 6), (2, 0, 7, 7), (2, 5, 7, 7), (0, 3, 7, 7), (-1, 3, 7, 7)]:
        assert L.rr_eval_ragged_workspace(n, c, oh, ow) == 0, (n, c, oh, ow)


def _cv(L, n=2, c=3, max_h=50, max_w=50, oh=16, ow=16, inp=IN, in_bytes=10000, tab=TAB, out=OUT, lanes=0):
    return L.rr_cv_resize_ragged_u8(n, c, max_h, max_w, oh, ow, inp, in_bytes, tab, out, lanes, None)


def _ev(L, n=2, c=3, max_h=50, max_w=50, oh=16, ow=16, clean=IN, clean_bytes=10000, tab=TAB, rst=RST,
        psnr=PSNR, ssim=SSIM, lanes=0, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(L.rr_eval_ragged_workspace(n, c, oh, ow), 64)
    return L.rr_eval_ragged_u8(n, c, max_h, max_w, oh, ow, clean, clean_bytes, tab, rst, psnr, ssim, lanes,
                               ws, ws_bytes, None)


BAD_COMMON = [dict(c=5), dict(c=0), dict(n=0), dict(n=-3), dict(max_h=0), dict(max_w=-1), dict(oh=0),
              dict(ow=-7), dict(lanes=7), dict(lanes=15), dict(tab=None)]


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(inp=None), dict(out=None), dict(in_bytes=0),
                                              dict(in_bytes=2 ** 63)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_cv_resize_ragged_rejects_before_launch(bad):
    assert _cv(_lib(), **bad) == RR_EINVAL


@pytest.mark.parametrize("bad", BAD_COMMON + [dict(clean=None), dict(rst=None), dict(psnr=None),
                                              dict(ssim=None), dict(ws=None), dict(clean_bytes=0),
                                              dict(clean_bytes=2 ** 63), dict(oh=6), dict(ow=6)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_eval_ragged_rejects_before_launch(bad):
    assert _ev(_lib(), **bad) == RR_EINVAL


def test_eval_ragged_short_workspace():
    L = _lib()
    for n, c, oh, ow in [(2, 3, 7, 7), (3, 1, 40, 70)]:
        need = L.rr_eval_ragged_workspace(n, c, oh, ow)
        assert _ev(L, n=n, c=c, oh=oh, ow=ow, ws_bytes=need - 1) == RR_EWORKSPACE
        assert _ev(L, n=n, c=c, oh=oh, ow=ow, ws_bytes=0) == RR_EWORKSPACE


def test_restoration_quality_checks_arguments_on_the_host(monkeypatch):
    """CPU tensors, a wrong dtype or rank, or mismatched batches raise before
    the library is reached"""
    from roadrestore import imgproc, ops

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "lib", no_library)
    monkeypatch.setattr(imgproc, "lib", no_library)
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(TypeError):
        imgproc.restoration_quality(u8, u8)                          # host tensors
    with pytest.raises(TypeError):
        imgproc.restoration_quality(u8.float(), u8.float())          # dtype
    with pytest.raises(TypeError):
        imgproc.restoration_quality(u8, u8[0])                       # rank
    with pytest.raises(TypeError):
        imgproc.restoration_quality([u8], "restored")
    for fn in (ops.cv_resize_ragged_u8, ops.eval_ragged_u8):
        tail = (16, 16) if fn is ops.cv_resize_ragged_u8 else (u8,)
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            fn(torch.zeros(64, dtype=torch.uint8), torch.zeros(2, 16, dtype=torch.uint8), (8, 8), 3, *tail)
        with pytest.raises(TypeError):
            fn(None, None, (8, 8), 3, *tail)


def test_restoration_quality_is_public():
    from roadrestore import imgproc, ops
    assert "restoration_quality" in imgproc.__all__ and "restoration_quality" in imgproc.__doc__
    assert {"cv_resize_ragged_u8", "eval_ragged_u8"} <= set(ops.__all__)
    assert callable(imgproc.RaggedBatch.cv_resize)
