"""The pool walk's step after its registers and waits were rearranged: the same results.

Two facts, on the shapes where that change can go wrong (tests/walk_step_cases.py says why these): dragon, car_boxed and
sportscar, 60 x 44 and 8 x 8, 4 bounces, the reference camera and one camera of the benchmark's path, `shdefer` and
`shpool`, the job list and the forced cursor, spp 1 and 4, one frame after another in one process.
  * Every frame's rgb (f32 bits), hit, t and bounce_hit equal the same build's `persist4` frame, and so do the ray
    counters.
  * On a counting renderer the wave steps, their histogram and the per-ray node / leaf / triangle counts equal the
    figures of the commit before the change (tests/golden/walk_step_counts.json).
"""
import json
import os

import numpy as np
import pytest

from tests import walk_step_cases as wc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_step_counts.json")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", wc.SCENES)
def test_frames_equal_persist4(name):
    from prt import device
    lst, cur = wc.Session(name), wc.Session(name, flags=device.FLAG_POOL_CURSOR)
    try:
        for W, H, ci, spp in wc.shapes():
            ref = lst.render(W, H, ci, spp, "persist4")
            assert "pool_all" not in ref["launch"]["build_bits"] and "pool_level" not in ref["launch"]["build_bits"]
            for v in wc.VARIANTS:
                for how, s in (("list", lst), ("cursor", cur)):
                    got = s.render(W, H, ci, spp, v)
                    what = (name, wc.key(W, H, ci, spp, v), how)
                    if how == "cursor":
                        assert "pool_list" not in got["launch"]["build_bits"], (what, got["launch"])
                    np.testing.assert_array_equal(got["hit"], ref["hit"], err_msg=f"{what}: hit")
                    np.testing.assert_array_equal(got["bounce_hit"], ref["bounce_hit"], err_msg=f"{what}: bounce_hit")
                    assert np.array_equal(bits(got["t"]), bits(ref["t"])), (what, "t")
                    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"])), (what, np.abs(got["rgb"] - ref["rgb"]).max())
                    for k in ("primary", "reflection", "shadow", "hits", "pixels"):
                        assert got["stats"][k] == ref["stats"][k], (what, k, got["stats"][k], ref["stats"][k])
                    assert got["stats"]["stack_overflows"] == 0, what
    finally:
        lst.close()
        cur.close()


@pytest.mark.parametrize("name", wc.SCENES)
def test_counts_equal_parent(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = wc.counts(name)  # (asserts that the list and the cursor agree)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        for k in wc.COUNT_KEYS + wc.RAY_KEYS:
            assert got[case][k] == want[case][k], (name, case, k, got[case][k], want[case][k])
    pools = [c for c in want if want[c]["shadow_wave_steps"] > 0]
    assert pools, "no case walked a shadow ray"
