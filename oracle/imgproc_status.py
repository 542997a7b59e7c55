"""What the image-side C entry points answer before they launch anything: the
workspace sizes, the draw offsets and the status of every kind of bad call.

``collect(L)`` makes the calls on a loaded library (``roadrestore.lib()``) and
returns them as one dict; tests/test_imgproc_status_cpu.py compares that with
tests/golden/imgproc_status.json.  ``python -m oracle.imgproc_status --record``
writes the fixture from the library in the tree -- run it on the commit whose
behaviour is to be kept, before the change that must not move it.

Every status call here fails validation, so none launches and none touches
the host dummies it passes for device pointers; ``collect`` refuses to return
an RR_ELAUNCH, or an RR_OK outside the calls known to return early.
"""
import ctypes as C
import itertools
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                       "imgproc_status.json")
ELAUNCH = -3
BIG = 1 << 63                      # a size_t above INT64_MAX
NS = (-1, 0, 1, 3, 64)
CS = (0, 1, 2, 3, 4, 5)
IN_HW = ((-1, 5), (0, 5), (5, 0), (1, 1), (33, 250), (250, 33), (4097, 40), (40, 4097))   # 4097 / 32: past RS_MAXK
OUT_HW = ((0, 32), (32, -1), (1, 1), (6, 7), (7, 6), (7, 7), (32, 32), (24, 40), (224, 224))

# the tables of tests/test_ragged_cpu.py: (records, keyword arguments of its _check)
_OK, _NB = (0, 10, 10), 10 * 10 * 3
RAGGED_TABLES = (
    (((7, 1, 1), (10, 250, 15), (11260, 2, 250)), dict(in_bytes=12760)),
    (((0, 250, 250),), dict(in_bytes=250 * 250 * 3)),
    (((0, 250, 250),), dict(c=1, in_bytes=250 * 250)),
    ((_OK,), dict(in_bytes=_NB)),
    ((_OK, (0, 0, 10)), dict(in_bytes=_NB)),
    ((_OK, (0, 10, 0)), dict(in_bytes=_NB)),
    (((0, 1, 251),), dict(in_bytes=10 ** 6)),
    (((0, 251, 1),), dict(in_bytes=10 ** 6)),
    ((_OK, (1, 10, 10)), dict(in_bytes=_NB)),
    ((_OK, (-1, 10, 10)), dict(in_bytes=_NB)),
    ((_OK, (-2 ** 63, 10, 10)), dict(in_bytes=_NB)),
    ((_OK, (2 ** 62, 10, 10)), dict(in_bytes=_NB)),
    ((_OK,), dict(c=5, in_bytes=10 ** 6)),
    ((_OK,), dict(c=0, in_bytes=10 ** 6)),
    ((_OK,), dict(n=0, in_bytes=_NB)),
    ((_OK,), dict(null=True, in_bytes=_NB)),
    ((_OK,), dict(in_bytes=_NB, max_w=128 * 32 + 1)),
    ((_OK,), dict(in_bytes=_NB, max_h=128 * 32 + 1)),
    ((_OK,), dict(in_bytes=_NB, max_w=127 * 32)),
    ((_OK,), dict(in_bytes=BIG)),
    ((_OK,), dict(in_bytes=_NB, oh=0)),
)


def _workspaces(L):
    q = {}

    def sweep(name, *axes):
        fn = getattr(L, name)
        q[name] = {",".join(map(str, a)): int(fn(*a)) for a in axes}

    dense = [(n, h, w, c, oh, ow) for n in NS for (h, w) in IN_HW for c in CS for (oh, ow) in OUT_HW]
    sweep("rr_resize_workspace", *dense)
    sweep("rr_resize_ragged_workspace", *[(n, c, h, w, oh, ow) for (n, h, w, c, oh, ow) in dense])
    sweep("rr_eval_ragged_workspace", *[(n, c, oh, ow) for n in NS + (1 << 29,) for c in CS for (oh, ow) in OUT_HW])
    sweep("rr_ssim_workspace", *[(n, c) for n in NS for c in CS])
    nhwc = [(n, h, w, c) for n in NS for (h, w) in IN_HW for c in CS]
    sweep("rr_distort_workspace", *nhwc)
    sweep("rr_distort_random_workspace", *nhwc)
    sweep("rr_distort_ragged_workspace", *[(n, c, h, w) for (n, h, w, c) in nhwc])
    return q


def _draws(L, ws):
    out = {}
    for name, shapes in (("rr_distort_random_draws", ((8, 8, 3), (33, 47, 1))),          # h, w, c
                         ("rr_distort_random_ragged_draws", ((3, 9, 8), (1, 33, 47)))):  # c, max_h, max_w
        for n in (1, 3, 64):
            for s in shapes:
                po, io, so = C.c_size_t(), C.c_size_t(), C.c_size_t()
                rc = getattr(L, name)(n, *s, ws, C.byref(po), C.byref(io), C.byref(so))
                out[f"{name}:{n},{','.join(map(str, s))}"] = [int(rc), po.value, io.value, so.value]
    return out


def _entry_points(L, buf):
    """name -> (argument names in the C order, valid values, {label: changed arguments}, labels that
    return RR_OK without a launch)"""
    base = C.addressof(buf)
    IN, OUT, TAB, WS, A, B, D = (base + 64 * i for i in range(1, 8))       # distinct, 64-byte aligned
    mean = C.cast((C.c_float * 4)(0.5, 0.5, 0.5, 0.5), C.c_void_p)
    buf._keep = mean
    null = lambda *names: {f"null {k}": {k: None} for k in names}
    dims = lambda **kw: {f"{k} {v}": {k: v} for k, vs in kw.items() for v in (vs if isinstance(vs, tuple) else (vs,))}
    norm = {"out_kind 2": dict(out_kind=2), "mean without std": dict(mean=mean), "std without mean": dict(mean=None, std=mean),
            "mean with out_kind 0": dict(mean=mean, std=mean, out_kind=0)}
    size = {"in_bytes 0": dict(in_bytes=0), "in_bytes above INT64_MAX": dict(in_bytes=BIG)}
    short = lambda need: {"ws_bytes one short": dict(ws_bytes=need - 1)}
    e = {}

    need = L.rr_resize_workspace(2, 8, 8, 3, 4, 4)
    e["rr_resize_bilinear_u8"] = (
        "n h w c oh ow in out_kind mean std out ws ws_bytes stream",
        (2, 8, 8, 3, 4, 4, IN, 1, None, None, OUT, WS, need, None),
        {**null("in", "out", "ws"), **norm, **short(need),
         **dims(n=0, c=(0, 5), h=0, oh=0, w=4097)}, ())

    need = L.rr_resize_ragged_workspace(2, 3, 9, 8, 4, 4)
    e["rr_resize_ragged_u8"] = (
        "n c max_h max_w oh ow in in_bytes images_dev out_kind mean std out ws ws_bytes stream",
        (2, 3, 9, 8, 4, 4, IN, 1000, TAB, 1, None, None, OUT, WS, need, None),
        {**null("in", "images_dev", "out", "ws"), **norm, **size, **short(need),
         **dims(n=0, c=(0, 5), max_h=0, oh=0, max_w=513)}, ())

    e["rr_cv_resize_linear_u8"] = (
        "n h w c oh ow in out simd_lanes stream", (2, 8, 8, 3, 4, 4, IN, OUT, 0, None),
        {**null("in", "out"), **dims(simd_lanes=3, n=(-1, 0), h=0, oh=0, c=(0, 5))}, ("n 0",))

    cvg = dict(dims(simd_lanes=3, n=0, c=(0, 5), max_h=0, oh=0),
               **{"oh * ow * c above INT32_MAX": dict(oh=32768, ow=32768), "2^31 workgroups": dict(n=1 << 29, oh=64, ow=64)})
    e["rr_cv_resize_ragged_u8"] = (
        "n c max_h max_w oh ow in in_bytes images_dev out simd_lanes stream",
        (2, 3, 9, 8, 4, 4, IN, 1000, TAB, OUT, 0, None),
        {**null("in", "images_dev", "out"), **size, **cvg}, ())

    need = L.rr_eval_ragged_workspace(2, 3, 8, 8)
    e["rr_eval_ragged_u8"] = (
        "n c max_h max_w oh ow in in_bytes images_dev restored psnr ssim simd_lanes ws ws_bytes stream",
        (2, 3, 9, 8, 8, 8, IN, 1000, TAB, OUT, A, B, 0, WS, need, None),
        {**null("in", "images_dev", "restored", "psnr", "ssim", "ws"), **size, **cvg, **short(need),
         **dims(oh=6, ow=6), "misaligned ws": dict(ws=WS + 4)}, ())

    need = L.rr_ssim_workspace(2, 3)
    e["rr_ssim_u8"] = (
        "n h w c a b out ws ws_bytes stream", (2, 8, 8, 3, IN, OUT, A, WS, need, None),
        {**null("a", "b", "out", "ws"), **short(need), **dims(n=0, c=0, h=6, w=6)}, ())

    need = L.rr_distort_workspace(2, 8, 8, 3)
    e["rr_distort_u8"] = (
        "n h w c mode in out params taps noise seed ws ws_bytes stream",
        (2, 8, 8, 3, 0, IN, OUT, A, B, None, 1, WS, need, None),
        {**null("in", "out", "params", "taps", "ws"), **short(need), **dims(n=0, h=0, w=0, c=(0, 5), mode=2)}, ())

    need = L.rr_distort_random_workspace(2, 8, 8, 3)
    e["rr_distort_random_u8"] = (
        "n h w c in out seed step table ws ws_bytes stream", (2, 8, 8, 3, IN, OUT, 1, A, B, WS, need, None),
        {**null("in", "out", "step", "table", "ws"), **short(need), **dims(n=0, h=0, w=0, c=(0, 5))}, ())

    need = L.rr_distort_ragged_workspace(2, 3, 9, 8)
    rag = {**size, **short(need), **dims(n=0, c=(0, 5), max_h=0, max_w=0), "in == out": dict(out=IN)}
    e["rr_distort_ragged_u8"] = (
        "n c mode max_h max_w in in_bytes images_dev out params taps tap_idx noise seed ws ws_bytes stream",
        (2, 3, 0, 9, 8, IN, 1000, TAB, OUT, A, B, None, None, 1, WS, need, None),
        {**null("in", "images_dev", "out", "params", "taps", "ws"), **rag, **dims(mode=2)}, ())
    e["rr_distort_random_ragged_u8"] = (
        "n c max_h max_w in in_bytes images_dev out seed step table ws ws_bytes stream",
        (2, 3, 9, 8, IN, 1000, TAB, OUT, 1, A, B, WS, need, None),
        {**null("in", "images_dev", "out", "step", "table", "ws"), **rag}, ())

    e["rr_motion_blur_kernel"] = ("k angle taps", (5, 45, A), {**null("taps"), **dims(k=(0, 16))}, ())
    e["rr_motion_blur_table"] = ("table", (A,), null("table"), ())
    return e


def _statuses(L, buf):
    out = {}
    for name, (names, valid, bad, returns_ok) in _entry_points(L, buf).items():
        names, fn = names.split(), getattr(L, name)
        assert len(names) == len(valid), name

        def call(*changes):
            args = dict(zip(names, valid))
            for ch in changes:
                assert set(ch) <= set(names), (name, ch)
                args.update(ch)
            return int(fn(*args.values()))

        for label, ch in bad.items():
            out[f"{name}: {label}"] = call(ch)
        # two bad arguments at once: which check comes first
        for (la, a), (lb, b) in itertools.combinations(bad.items(), 2):
            if not set(a) & set(b):
                out[f"{name}: {la} + {lb}"] = call(a, b)
        for key, rc in out.items():
            if key.startswith(name + ": "):
                early = any(lab in key.split(": ", 1)[1].split(" + ") for lab in returns_ok)
                if rc == ELAUNCH or (rc == 0 and not early):
                    raise AssertionError(f"{key} passed validation (status {rc}): it must not be called here")
    return out


def _ragged_check(L):
    from roadrestore._lib import RaggedImage
    out = []
    for recs, kw in RAGGED_TABLES:
        kw = dict(dict(c=3, max_h=250, max_w=250, oh=32, ow=32, n=len(recs), null=False), **kw)
        tab = (RaggedImage * len(recs))(*[RaggedImage(*r) for r in recs])
        out.append(int(L.rr_ragged_check(kw["n"], kw["c"], kw["in_bytes"], None if kw["null"] else C.cast(tab, C.c_void_p),
                                         kw["max_h"], kw["max_w"], kw["oh"], kw["ow"])))
    return out


def collect(L):
    buf = C.create_string_buffer(1024)
    return {"workspace": _workspaces(L), "draws": _draws(L, C.addressof(buf)), "status": _statuses(L, buf),
            "ragged_check": _ragged_check(L)}


def compact(full):
    """collect()'s dict as the fixture holds it: the sweeps and the pairs as bare lists in the order
    collect makes the calls (their keys are the code above), the rest keyed"""
    pairs = {}
    for key, rc in full["status"].items():
        if " + " in key:
            pairs.setdefault(key.split(": ", 1)[0], []).append(rc)
    return {"workspace": {fn: list(d.values()) for fn, d in full["workspace"].items()},
            "draws": full["draws"],
            "status": {k: rc for k, rc in full["status"].items() if " + " not in k},
            "status_pairs": pairs,
            "ragged_check": full["ragged_check"]}


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m oracle.imgproc_status --record")
    import roadrestore
    fix = compact(collect(roadrestore.lib()))
    with open(FIXTURE, "w") as f:                    # one line per query, per draw and per bad call
        f.write("{\n" + ",\n".join(
            f'"{part}": ' + (json.dumps(v) if isinstance(v, list) else
                             "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(x)}" for k, x in v.items()) + "\n}")
            for part, v in fix.items()) + "\n}\n")
    print("wrote", FIXTURE)
