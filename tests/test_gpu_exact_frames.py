"""Frames through the short division / root / normalize forms (rt_exact.hpp) equal the strict kernel's.

dragon, car_boxed and sportscar at 60 x 44 and 8 x 8, the reference camera and camera 7 of the benchmark's path, spp 1
and 4, 4 bounces, with `persist4`, `shpool` and `shdefer`: rgb (f32 bits), hit, t, bounce_hit and the ray counters equal
the strict kernel's frame of the same renderer. The even width gives the centre column zero direction components --
the guards' fallback -- in real frames; 60 x 44 has partial tiles, 8 x 8 is one tile. (The strict kernel itself is held to
the oracle by tests/test_gpu_parity.py.)
"""
import numpy as np
import pytest

from tests import walk_step_cases as wc

pytestmark = pytest.mark.gpu
VARIANTS = ("persist4", "shpool", "shdefer")
RAY_KEYS = ("primary", "reflection", "shadow", "hits", "pixels")


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def render(r, W, H, ci, spp, kernel, variant=None):
    import torch
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    bh = torch.zeros((H, W, wc.BOUNCES), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kw = {"variant": variant} if variant else {}
    r.render(wc.camera(W, H, ci), W, H, bounces=wc.BOUNCES, spp=spp, kernel=kernel, rgb=rgb, hit=hit, t=t, bounce_hit=bh,
             **kw)
    r.sync()
    return {"rgb": rgb.cpu().numpy(), "hit": hit.cpu().numpy(), "t": t.cpu().numpy(), "bounce_hit": bh.cpu().numpy(),
            "stats": r.stats()}


@pytest.mark.parametrize("name", wc.SCENES)
def test_frames_equal_strict(name):
    from prt import device
    r = device.Renderer(0)
    r.upload(wc.scene(name))
    try:
        for W, H, ci, spp in wc.shapes():
            ref = render(r, W, H, ci, spp, "strict")
            assert (ref["hit"] >= 0).any(), (name, W, H, ci, "the frame misses the scene")
            for v in VARIANTS:
                got = render(r, W, H, ci, spp, "fast", v)
                what = (name, wc.key(W, H, ci, spp, v))
                np.testing.assert_array_equal(got["hit"], ref["hit"], err_msg=f"{what}: hit")
                np.testing.assert_array_equal(got["bounce_hit"], ref["bounce_hit"], err_msg=f"{what}: bounce_hit")
                assert np.array_equal(bits(got["t"]), bits(ref["t"])), (what, "t")
                assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"])), (what, np.abs(got["rgb"] - ref["rgb"]).max())
                for k in RAY_KEYS:
                    assert got["stats"][k] == ref["stats"][k], (what, k, got["stats"][k], ref["stats"][k])
                assert got["stats"]["stack_overflows"] == 0, what
    finally:
        r.close()
