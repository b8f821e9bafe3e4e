"""The pool kernels' job-list hand-out on the GPU (rt_shpool.hpp shadow_pool<.., LIST>, rt_pool_list.hpp).

`shdefer` (one pool for all levels) and `shpool` (one per level) against the strict kernel: rgb, hit, t and the BGRA8
quantisation bit for bit and the primary / reflection / shadow ray counts, on frames small enough for a few seconds
each: 64x40 (40 whole tiles) and 36x20 (partial tiles: lanes without a pixel that still work in the pool), dragon and
car_boxed (2 lights) and sportscar (4 lights) at 4 bounces, regroup 1 / 16 / 63 / 64, bounces 1, bounce_hit, spp = 4,
single frames and a 4-frame batch.

The list hands the same ray to the same lane in the same round as the cursor it replaces, so with the cursor forced
(rt_opts.flags RT_FLAG_POOL_CURSOR, as RT_FLAG_UNPACKED_* force the unpacked builds) the frames AND the counting
builds' wave steps, their histogram and the shadow walks' node / leaf / triangle counts are equal, not merely close.
rt_launch_info.build says which hand-out ran. LISTED names the launches that must take the list: dragon under both
pool kernels, car_boxed and two_cars under the per-level pool. Under the all-levels pool car_boxed's lists (2 KB per
workgroup) miss the 40 KB of a workgroup at 4 per CU by 128 B and two_cars' (4 KB) by 3.2 KB -- their stacks are
deeper -- so those run the cursor, as sportscar's per-level pool does (4 lights, depth 15); sportscar's all-levels
pool never fitted and runs PERSIST4 as before.
"""
import numpy as np
import pytest

from prt import host

pytestmark = pytest.mark.gpu
_SCENES = {}
_STRICT = {}
SIZES = [(64, 40), (36, 20)]
STEP_KEYS = ("wave_steps", "shadow_wave_steps", "steps_hist", "sh_inner", "sh_leaf", "sh_tri", "ch_inner", "ch_leaf",
             "ch_tri", "steps_lanes_16", "steps_lanes_32", "steps_lanes_48", "steps_lanes_64")
RAY_KEYS = ("primary", "reflection", "shadow", "shadow_skipped", "hits", "pixels")


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = host.Scene.named(name).build_bvh(3)
    return _SCENES[name]


def cams(W, H, n):
    out = []
    for i in range(n):
        c = host.camera(W, H)
        c.pos.x += i * 0.02
        c.ul.x += i * 0.02
        out.append(c)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def render(name, W, H, kernel, variant=None, bounces=4, spp=1, regroup=0, n=1, flags=0, counters=False,
           want_bounce_hit=False):
    """n = 1: rt_render; n > 1: one rt_render_frames batch on the camera path. Every output as numpy, with the stats
    and the launch info."""
    import torch
    from prt import device
    r = device.Renderer(0, counters=counters, flags=flags)
    r.upload(scene(name))
    rgb = torch.zeros((n, H, W, 3), dtype=torch.float32, device="cuda")
    hit = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    t = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
    px = torch.zeros((n, H, W), dtype=torch.int32, device="cuda")
    bh = torch.zeros((n, H, W, bounces), dtype=torch.int32, device="cuda") if want_bounce_hit else None
    torch.cuda.synchronize()
    kw = dict(bounces=bounces, spp=spp, kernel=kernel, variant=variant, regroup=regroup, rgb=rgb, hit=hit, t=t, bgra=px,
              bounce_hit=bh)
    if n == 1:
        r.render(cams(W, H, 1)[0], W, H, **kw)
    else:
        r.render_frames(cams(W, H, n), W, H, **kw)
    r.sync()
    out = {"rgb": rgb.cpu().numpy(), "hit": hit.cpu().numpy(), "t": t.cpu().numpy(), "bgra": px.cpu().numpy(),
           "stats": r.stats(), "launch": r.launch_info()}
    if bh is not None:
        out["bounce_hit"] = bh.cpu().numpy()
    r.close()
    return out


def strict(name, W, H, bounces=4, spp=1, n=1, want_bounce_hit=False):
    """the strict kernel's frames of a case, computed once and shared"""
    key = (name, W, H, bounces, spp, n, want_bounce_hit)
    if key not in _STRICT:
        _STRICT[key] = render(name, W, H, "strict", bounces=bounces, spp=spp, n=n, want_bounce_hit=want_bounce_hit)
    return _STRICT[key]


def same_frames(got, ref, what):
    np.testing.assert_array_equal(got["hit"], ref["hit"], err_msg=f"{what}: hit")
    assert np.array_equal(bits(got["t"]), bits(ref["t"])), f"{what}: t"
    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"])), (what, np.abs(got["rgb"] - ref["rgb"]).max())
    np.testing.assert_array_equal(got["bgra"], ref["bgra"], err_msg=f"{what}: bgra")


def same_rays(got, ref, what):
    for k in ("primary", "reflection", "shadow"):
        assert got["stats"][k] == ref["stats"][k], (what, k, got["stats"][k], ref["stats"][k])
    assert got["stats"]["stack_overflows"] == 0


def pool_bit(variant):
    return "pool_all" if variant == "shdefer" else "pool_level"


LISTED = {("dragon", "shdefer"), ("dragon", "shpool"), ("car_boxed", "shpool"), ("two_cars", "shpool")}


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["dragon", "car_boxed", "sportscar"])
def test_pool_vs_strict(name, W, H, variant):
    got = render(name, W, H, "fast", variant)
    if (name, variant) != ("sportscar", "shdefer"):  # (no room for its all-levels pool: PERSIST4)
        assert pool_bit(variant) in got["launch"]["build_bits"], got["launch"]
    assert ("pool_list" in got["launch"]["build_bits"]) == ((name, variant) in LISTED), got["launch"]
    ref = strict(name, W, H)
    same_frames(got, ref, (name, W, H, variant))
    same_rays(got, ref, (name, W, H, variant))


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
@pytest.mark.parametrize("regroup", [1, 16, 63, 64])
def test_pool_regroup(regroup, variant):
    for name, (W, H) in (("dragon", SIZES[1]), ("sportscar", SIZES[0])):
        got = render(name, W, H, "fast", variant, regroup=regroup)
        ref = strict(name, W, H)
        same_frames(got, ref, (name, regroup, variant))
        same_rays(got, ref, (name, regroup, variant))


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
def test_pool_one_bounce(variant):
    for W, H in SIZES:
        got = render("dragon", W, H, "fast", variant, bounces=1)
        ref = strict("dragon", W, H, bounces=1)
        same_frames(got, ref, (W, H, variant))
        same_rays(got, ref, (W, H, variant))


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
def test_pool_bounce_hit(variant):
    W, H = SIZES[1]
    got = render("dragon", W, H, "fast", variant, want_bounce_hit=True)
    ref = strict("dragon", W, H, want_bounce_hit=True)
    same_frames(got, ref, variant)
    np.testing.assert_array_equal(got["bounce_hit"], ref["bounce_hit"])
    same_rays(got, ref, variant)


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
def test_pool_spp4(variant):
    W, H = SIZES[1]
    # (the sample-sum slots take 4 KB: dragon's all-levels pool then runs the cursor, its per-level pool the list)
    got = render("dragon", W, H, "fast", variant, spp=4)
    assert pool_bit(variant) in got["launch"]["build_bits"], got["launch"]
    assert ("pool_list" in got["launch"]["build_bits"]) == (variant == "shpool"), got["launch"]
    ref = strict("dragon", W, H, spp=4)
    same_frames(got, ref, variant)
    same_rays(got, ref, variant)


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
@pytest.mark.parametrize("name", ["dragon", "sportscar"])
def test_pool_batch_of_4(name, variant):
    """one persistent launch of 4 frames: every frame equals the strict kernel's frame of its camera"""
    W, H = SIZES[1]
    got = render(name, W, H, "fast", variant, n=4)
    ref = strict(name, W, H, n=4)
    same_frames(got, ref, (name, variant))
    same_rays(got, ref, (name, variant))


@pytest.mark.parametrize("name", ["dragon", "car_boxed", "two_cars"])
def test_list_is_taken(name):
    """the scenes of the benchmark configurations run the list hand-out where LISTED says so (their lists fit 4
    workgroups per CU), single frames and batches; with the cursor forced none does"""
    from prt import device
    W, H = SIZES[1]
    for variant in ("shdefer", "shpool"):
        for kw in ({}, {"n": 4}):
            li = render(name, W, H, "fast", variant, **kw)["launch"]
            assert pool_bit(variant) in li["build_bits"], (variant, kw, li)
            assert ("pool_list" in li["build_bits"]) == ((name, variant) in LISTED), (variant, kw, li)
        li = render(name, W, H, "fast", variant, flags=device.FLAG_POOL_CURSOR)["launch"]
        assert pool_bit(variant) in li["build_bits"] and "pool_list" not in li["build_bits"], (variant, li)


@pytest.mark.parametrize("variant", ["shdefer", "shpool"])
@pytest.mark.parametrize("name,W,H,n", [("dragon", 64, 40, 1), ("car_boxed", 36, 20, 1), ("dragon", 36, 20, 4)])
def test_cursor_forced_same_walks(name, W, H, n, variant):
    """the cursor hand-out forced: the same frames as the strict kernel and as the list form, and -- the same ray to
    the same lane in the same round -- the counting builds' wave steps, histogram and per-ray work equal the list
    form's exactly"""
    from prt import device
    cur = render(name, W, H, "fast", variant, n=n, flags=device.FLAG_POOL_CURSOR, counters=True)
    lst = render(name, W, H, "fast", variant, n=n, counters=True)
    assert "pool_list" not in cur["launch"]["build_bits"], cur["launch"]
    ref = strict(name, W, H, n=n)
    same_frames(cur, ref, (name, variant, "cursor"))
    same_frames(lst, ref, (name, variant, "list"))
    same_rays(cur, ref, (name, variant))
    for k in STEP_KEYS + RAY_KEYS:
        assert cur["stats"][k] == lst["stats"][k], (name, variant, k, cur["stats"][k], lst["stats"][k])
    assert lst["stats"]["shadow_wave_steps"] > 0
