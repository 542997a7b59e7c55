"""The library routes each conv / weight-grad call once (csrc/route.h
conv_route, wgrad.hip wgrad_route): every host-only routing query over the
sweep of tests/route_sweep.py answers what the build before that change
answered (tests/golden/routing_*.json, recorded from it), under every RR_PATH
setting the parity tests force.  No launch, no GPU."""
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
    pre_ok of every conv row; name, workspace and pre_ok of every weight-grad
    row: SHA-256 and row count per RR_PATH setting"""
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
