"""The library routes each conv / weight-grad call once (csrc/route.h
conv_route, wgrad.hip wgrad_route): every host-only routing query over the
sweep of tests/route_sweep.py answers what the build before that change
answered (tests/golden/routing_*.json, recorded from it; the BN-backward slab
columns re-recorded when they began to follow the kernel rr_igemm_bnbwd
launches), under every RR_PATH setting the parity tests force.  No launch, no
GPU."""
import ctypes as C
import json
import os

import pytest

import route_sweep as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.mark.parametrize("path", RS.PATHS)
def test_routing_sweep_matches_recorded_digest(path, monkeypatch):
    """names (plain, bnbwd, dgrad_sc), statistics rows, bnbwd workspace and
    rows, pre_ok of every conv row; name, workspace and pre_ok of every
    weight-grad row: SHA-256 and row count per RR_PATH setting"""
    monkeypatch.setenv("RR_PATH", path)
    want = golden("routing_sweep_digest.json")[path]
    assert RS.digest(RS.conv_table()) == want["conv"]
    assert RS.digest(RS.wgrad_table()) == want["wgrad"]


def test_routing_of_the_model_shapes_row_by_row(monkeypatch):
    """the readable part of the table: what ResUNet, SimpleUNet and VGG16 run
    at 64x64 and 224x224 (a mismatch names its descriptor)"""
    want = golden("routing_model_rows.json")
    assert sorted(want) == sorted(RS.MODEL_PATHS)
    for path, tables in want.items():
        monkeypatch.setenv("RR_PATH", path)
        got = {"conv": RS.conv_table(True, RS.MODEL_GEOMS, RS.MODEL_CHANS, (0, 1)),
               "wgrad": RS.wgrad_table(True, RS.MODEL_GEOMS, RS.MODEL_CHANS, (0, 1))}
        for kind in ("conv", "wgrad"):
            assert len(got[kind]) == len(tables[kind]) > 0
            for g, w in zip(got[kind], tables[kind]):
                assert g == w, (path, kind)


@pytest.mark.parametrize("path", RS.PATHS)
def test_pool_kernel_name_is_the_launched_kernel(path, monkeypatch):
    """rr_igemm_pool_kernel_name(d, with_index) names what rr_igemm_pool
    launches.  The recorded answers predate with_index and named the streaming
    kernel wherever it takes the plain layer; the launch takes it with the
    index only on whole-row maps (w <= 64) and without it only on biased
    layers, else the tap-reuse conv of the ReLU | POOL | NOFULL descriptor."""
    import roadrestore
    from roadrestore._lib import RR_ACT_NOFULL, RR_ACT_POOL, RR_ACT_RELU, IgemmDesc
    L = roadrestore.lib()
    rec = golden("routing_pool_names.json")
    descs = list(RS.pool_descs())
    old = [rec["names"][i] for i in rec["index"][path]]
    assert len(old) == len(descs)

    def conv3r_name(d):   # the ex name with the streaming kernel off: conv3r's, or "unsupported"
        d2 = IgemmDesc.from_buffer_copy(d)
        d2.act = RR_ACT_RELU | RR_ACT_POOL | RR_ACT_NOFULL
        return L.rr_igemm_kernel_name(C.byref(d2), 0).decode()

    monkeypatch.setenv("RR_PATH", path)
    got = [(L.rr_igemm_pool_kernel_name(C.byref(d), 1).decode(),
            L.rr_igemm_pool_kernel_name(C.byref(d), 0).decode()) for d in descs]
    monkeypatch.setenv("RR_PATH", (path + "," if path else "") + "stream3=0")
    c3 = [conv3r_name(d) for d in descs]
    nstrip = nbias = 0
    for d, o, (g1, g0), c in zip(descs, old, got, c3):
        s3 = o.startswith("stream3")
        strip, nobias = s3 and d.w > 64, s3 and not d.has_bias
        nstrip += strip
        nbias += nobias
        assert g1 == (c if strip else o), (path, d.n, d.h, d.w, d.c_in1, d.c_in2, d.c_out, d.has_bias)
        assert g0 == (c if nobias else o), (path, d.n, d.h, d.w, d.c_in1, d.c_in2, d.c_out, d.has_bias)
    if "stream3=0" not in path:
        assert nbias > 0 and (nstrip > 0) == ("stream3_strips=0" not in path)


# geometries at which the plain call and rr_igemm_bnbwd take different kernels
# (kept out of route_sweep.GEOMS: the recorded digests keep their meaning):
# 3x3 column strips (plain: stream3_kernel<s32>) and, with stream1_minp=256,
# 1x1 maps whose stream1 row count is above (2x16x16) and below (264x16x16)
# the tiled kernel's
BNBWD_GEOMS = [(4, 176, 96), (2, 224, 224), (2, 16, 16), (264, 16, 16)]
BNBWD_PATHS = RS.PATHS + ["stream1_minp=256"]


def bnbwd_descs():
    """the descriptors of the sweep rr_igemm_bnbwd accepts: 3x3 / 1x1, the
    all-zero flag set, one source, whole 64-channel column tiles"""
    from roadrestore._lib import IgemmDesc
    for dt in (0, 1):
        for mode in (0, 1):
            for (n, h, w) in RS.GEOMS + [g for g in BNBWD_GEOMS if g not in RS.GEOMS]:
                for (c1, c2, co) in RS.CHANS:
                    if c2 == 0 and co % 64 == 0:
                        yield IgemmDesc(dt, mode, n, h, w, c1, 0, co, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("path", BNBWD_PATHS)
def test_bnbwd_slabs_follow_the_launched_kernel(path, monkeypatch):
    """rr_igemm_bnbwd_rows / rr_igemm_bnbwd_workspace size the partial slabs
    for the kernel rr_igemm_bnbwd launches (the CK_BNBWD route), which is not
    the plain call's where that takes stream1 or a stream3 strip instance:
    sized from rr_igemm_stat_blocks the launch stored past the workspace and
    over its own alpha partials (3x3 64 -> 64 at 2x224x224: 784 rows into 256),
    or the finalize summed rows nobody wrote (1x1 at 2x16x16 with
    stream1_minp=256: 4 of 512).  On the build before rr_igemm_bnbwd_rows the
    workspace equation below fails for exactly those rows: bf16 only, per
    setting "" 53, stream3=0 47, conv3r=0 53, "stream3=0,conv3r=0" 47,
    swgrad=0 53, "swgrad=0,wgrad_halo=0" 53, stream1=0 6, conv3r_wg=8 53,
    stream3_strips=0 47, stream1_minp=256 193 of the 1188 descriptors (6 of
    them 3x3 column strips wherever the strips are on, the rest 1x1 stream1
    maps)."""
    import roadrestore
    L = roadrestore.lib()
    kinds = {"strip": 0, "stream1_more": 0, "stream1_fewer": 0}
    count = 0
    for d in bnbwd_descs():
        rows, plain, fused, plain_rows = RS.launched_bnbwd_rows(d, path)
        monkeypatch.setenv("RR_PATH", path)
        key = (path, d.dtype, d.mode, d.n, d.h, d.w, d.c_in1, d.c_out, plain, fused)
        assert rows > 0, key
        assert L.rr_igemm_bnbwd_rows(C.byref(d)) == rows, key
        assert L.rr_igemm_bnbwd_workspace(C.byref(d)) == (rows * d.c_out * 3 + rows * (d.c_out // 64)) * 4, key
        count += 1
        if plain != fused and plain_rows != rows:
            assert plain.startswith("stream1_kernel") or plain == "stream3_kernel<s32>", key
            if plain.startswith("stream3"):
                kinds["strip"] += 1
            else:
                kinds["stream1_more" if plain_rows > rows else "stream1_fewer"] += 1
    assert count == 2 * 2 * (len(RS.GEOMS) + 3) * 11 == 1188
    # every mismatch kind is in the sweep
    if path == "":
        assert kinds["strip"] > 0, kinds
    if path == "stream1_minp=256":
        assert min(kinds.values()) > 0, kinds


def _name64(L):
    from roadrestore._lib import RR_BF16, RR_CONV3X3, IgemmDesc
    d = IgemmDesc(RR_BF16, RR_CONV3X3, 16, 64, 64, 64, 0, 64, 0, 0, 0, 1, 0, 1, 0)
    return L.rr_igemm_kernel_name(C.byref(d), 0).decode()


@pytest.mark.parametrize("path,stream3,conv3r", [
    (" stream3 = 0 ", 0, 1),            # spaces around key and value are ignored
    ("stream3=x", 1, 1),                # not a whole integer: the item is ignored, the default holds
    ("stream3=0 ,conv3r=0", 0, 0),
    ("stream3=,stream3=0x0, stream3=0", 0, 1),   # the first valid item of a key wins
    ("stream3=1,stream3=0", 1, 1),
    ("stream3=0000000000", 1, 1),       # more than 9 digits: ignored
    ("stream3= -0,conv3r = +0", 0, 0),
])
def test_rr_path_grammar_is_the_same_in_c_and_python(path, stream3, conv3r, monkeypatch):
    """one grammar on both sides (csrc/common.h rr_path_read, _lib.path_flag):
    the library seen through the kernel it names for a 64 -> 64 64x64 conv"""
    import roadrestore
    from roadrestore._lib import path_flag
    monkeypatch.setenv("RR_PATH", path)
    assert path_flag("stream3", 1) == stream3
    assert path_flag("conv3r", 1) == conv3r
    want = "stream3_kernel<64>" if stream3 else "conv3r_kernel<64,64>" if conv3r else "igemm3_halo_kernel<64,64>"
    assert _name64(roadrestore.lib()) == want
