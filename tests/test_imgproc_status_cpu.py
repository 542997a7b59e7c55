"""CPU: what the image-side entry points (csrc/resize.hip, quality.hip,
distort.hip) answer before any launch -- every workspace size, the draw
offsets, the status of each kind of bad call and of two bad arguments at once
(which check comes first), rr_ragged_check on test_ragged_cpu's tables --
against tests/golden/imgproc_status.json, recorded by
``python -m oracle.imgproc_status --record`` before the three files were split
out of one.  No call here passes validation, so nothing is launched."""
import json

import pytest

from oracle import imgproc_status as S


@pytest.fixture(scope="module")
def pair():
    import roadrestore
    with open(S.FIXTURE) as f:
        want = json.load(f)
    full = S.collect(roadrestore.lib())
    return want, S.compact(full), full


def test_fixture_holds_no_launch(pair):
    want, _, _ = pair
    rcs = list(want["status"].values()) + [rc for v in want["status_pairs"].values() for rc in v]
    assert S.ELAUNCH not in rcs and len(rcs) > 900 and len(want["workspace"]) == 7


@pytest.mark.parametrize("part", ["workspace", "draws", "status", "status_pairs", "ragged_check"])
def test_same_answers_as_recorded(pair, part):
    want, got, full = pair
    want, got = want[part], got[part]
    if part == "ragged_check":
        assert got == want
        return
    assert list(got) == list(want)
    # the calls behind a bare list, in its order (oracle.imgproc_status.compact)
    names = {"workspace": {fn: list(d) for fn, d in full["workspace"].items()},
             "status_pairs": {fn: [k for k in full["status"] if k.startswith(fn + ": ") and " + " in k]
                              for fn in got}}.get(part)
    for key in got:
        if names is None:
            assert got[key] == want[key], key
            continue
        assert len(got[key]) == len(want[key]) == len(names[key]), key
        diff = [(n, w, g) for n, w, g in zip(names[key], want[key], got[key]) if w != g]
        assert not diff, f"{key}: {len(diff)} differ (call, recorded, now): {diff[:10]}"
