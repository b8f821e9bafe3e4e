"""The frame and shade kernels across light counts (tests/lit_scenes.py: a generated room with a bumpy sphere, fourteen
materials and L lights), L in {0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 40}: on both sides of every range the shading path
branches on -- the per-level shadow pool's 1..32 (one 32-bit visibility word per pixel), the all-levels pool's and the
shade query's pool form's 1..8 (8 bits per level), the forced variants' fall-back to PERSIST4 outside them, the job
lists' LDS size of 32 * levels * lights ints per wave, the default rule's pool for 2+ lights.

The yardstick is the oracle (tests/oracle_bind.py, CPU) at the camera it has; where the camera must move (batches) it
is the strict kernel, which this file holds to the oracle first. Equality is test_scaled_scene_vs_oracle's: hit equal,
t and rgb bit for bit, bgra equal to the strict kernel's, the ray counters equal to the oracle's, no stack overflow.
Frames are 64x40 (whole tiles) and 36x20 (partial tiles: lanes without a pixel that still work in the pool); every
scene and every oracle frame is made once per module.

LISTED is what an MI355X reported: the forced pool launches that took the job-list hand-out."""
import numpy as np
import pytest

from prt import host
from tests import lit_scenes as ls
from tests import test_gpu_pool_handout as ph
from tests.test_gpu_parity import KERNELS
from tests.test_gpu_shade import FORMS as SHADE_FORMS

pytestmark = pytest.mark.gpu
COUNTS = ls.LIGHT_COUNTS
SIZES = ph.SIZES  # 64x40, 36x20
POOLS = ("shpool", "shdefer")
RAYS = ("primary", "reflection", "shadow", "shadow_skipped", "hits")
# (form, L, bounces, variant) of the forced pool launches that ran the job-list hand-out on an MI355X; every other
# forced pool launch of cases() ran the cursor (shdefer at 7 and 8 lights, shpool at 31 and 32) or PERSIST4 (outside
# the variant's range of lights, and every 8-level launch: neither pool's 8-level LDS layout fits 4 workgroups per CU)
LISTED = {(form, L, 4, "shdefer") for form in ls.FORMS for L in (1, 2, 3)} | \
         {(form, L, 4, "shpool") for form in ls.FORMS for L in (1, 2, 3, 7, 8, 9)}


def cases():
    """(form, bounces) of section (a): 4 bounces in both forms, 8 in the hall"""
    return [("open", 4), ("hall", 4), ("hall", 8)]


def sizes(bounces):
    return SIZES if bounces == 4 else SIZES[:1]


@pytest.fixture(scope="module")
def lit(tmp_path_factory):
    return ls.Lit(tmp_path_factory.mktemp("lit"))


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


class Ctx:
    """one Renderer on one uploaded scene"""

    def __init__(self, dev, scene, counters=False, flags=0):
        self.r = dev.Renderer(0, counters=counters, flags=flags)
        self.r.upload(scene)

    def render(self, W, H, kernel, bounces=4, spp=1, cam=None, cams=None):
        """rt_render at `cam` (None: host.camera), or one rt_render_frames batch at `cams` -> numpy [n, H, W, ..]"""
        import torch
        n = 1 if cams is None else len(cams)
        b = {"rgb": torch.zeros((n, H, W, 3), dtype=torch.float32, device="cuda"),
             "hit": torch.zeros((n, H, W), dtype=torch.int32, device="cuda"),
             "t": torch.zeros((n, H, W), dtype=torch.float32, device="cuda"),
             "bgra": torch.zeros((n, H, W), dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        if cams is None:
            cam = cam if cam is not None else host.camera(W, H)
            self.r.render(cam, W, H, bounces=bounces, spp=spp, kernel=kernel, **b)
        else:
            self.r.render_frames(cams, W, H, bounces=bounces, spp=spp, kernel=kernel, **b)
        self.r.sync()
        out = {k: v.cpu().numpy() for k, v in b.items()}
        out["stats"], out["launch"] = self.r.stats(), self.r.launch_info()
        return out

    def close(self):
        self.r.close()


def same_as_oracle(got, ref, bgra, what):
    """got: a one-frame render; ref: the oracle's frame; bgra: the strict kernel's pixels"""
    np.testing.assert_array_equal(got["hit"][0], ref["hit"], err_msg=f"{what}: hit")
    assert np.array_equal(ph.bits(got["t"][0]), ph.bits(ref["t"])), f"{what}: t"
    diff = ph.bits(got["rgb"][0]) != ph.bits(ref["rgb"])
    assert not diff.any(), (what, "rgb", int(diff.any(-1).sum()), float(np.abs(got["rgb"][0] - ref["rgb"]).max()))
    np.testing.assert_array_equal(got["bgra"][0], bgra, err_msg=f"{what}: bgra")
    for k in RAYS:
        assert got["stats"][k] == ref["counters"][k], (what, k, got["stats"][k], ref["counters"][k])
    assert got["stats"]["stack_overflows"] == 0, what


def pool_facts(L, bounces, variant, li, what, boundary=True):
    """section (b): what a forced pool variant may and must have run (boundary: and, at 4 levels, that the pool ran
    wherever its range of lights allows it)"""
    bits = li["build_bits"]
    if "pool_all" in bits:
        assert 1 <= L <= 8 and variant == "shdefer", (what, li)
    if "pool_level" in bits:
        assert 1 <= L <= 32 and variant == "shpool", (what, li)
    if "pool_list" in bits:
        assert "pool_all" in bits or "pool_level" in bits, (what, li)
    if L == 0 or L >= 33 or (variant == "shdefer" and L >= 9):
        assert li["variant"] == "persist4" and not {"pool_all", "pool_level", "pool_list"} & set(bits), (what, li)
    if bounces == 4 and boundary:  # (this shallow scene's stacks leave room for both pools at 4 levels)
        if variant == "shdefer" and 1 <= L <= 8:
            assert "pool_all" in bits and li["variant"] == "shdefer", (what, li)
        if variant == "shpool" and 1 <= L <= 32:
            assert "pool_level" in bits and li["variant"] == "shpool", (what, li)


# ------------------------------------------------------------------ (a), (b): every kernel, every count; what ran
_TABLE = {}  # (form, L, bounces, variant) -> the launch infos of its sizes: section (b)'s record


@pytest.mark.parametrize("L", COUNTS)
def test_every_kernel_at_every_light_count(dev, lit, L):
    for form, bounces in cases():
        c = Ctx(dev, lit.scene(form, L))
        for W, H in sizes(bounces):
            ref = lit.frame(form, L, W, H, bounces)
            bgra = None
            for kernel in KERNELS:  # (strict first: its bgra is the others' yardstick, its rgb the oracle's)
                what = (form, L, bounces, W, H, kernel)
                got = c.render(W, H, kernel, bounces)
                if kernel == "strict":
                    bgra = got["bgra"][0]
                same_as_oracle(got, ref, bgra, what)
                if kernel in POOLS:
                    pool_facts(L, bounces, kernel, got["launch"], what)
                    _TABLE.setdefault((form, L, bounces, kernel), []).append(got["launch"])
        c.close()


def test_which_hand_out_ran(dev, lit):
    """the record of section (b): the forced pool launches' build and hand-out on this device against LISTED, the same
    at both frame sizes; each pool variant takes the list and the cursor at least once at 3+ lights"""
    for form, bounces in cases():
        for L in COUNTS:
            if all((form, L, bounces, v) in _TABLE for v in POOLS):
                continue
            c = Ctx(dev, lit.scene(form, L))  # (this test alone: the launches without the comparisons)
            for v in POOLS:
                _TABLE[form, L, bounces, v] = [c.render(W, H, v, bounces)["launch"] for W, H in sizes(bounces)]
            c.close()
    listed = set()
    for key in sorted(_TABLE):
        infos = _TABLE[key]
        for li in infos:
            pool_facts(key[1], key[2], key[3], li, key)
            assert li["build_bits"] == infos[0]["build_bits"] and li["variant"] == infos[0]["variant"], (key, infos)
        print("ran", *key, infos[0]["variant"], ",".join(infos[0]["build_bits"]))
        if "pool_list" in infos[0]["build_bits"]:
            listed.add(key)
    assert listed == LISTED, (sorted(listed - LISTED), sorted(LISTED - listed))
    for v in POOLS:
        pooled = {k for k in _TABLE if k[3] == v and k[1] >= 3 and
                  {"pool_all", "pool_level"} & set(_TABLE[k][0]["build_bits"])}
        assert pooled & LISTED, v
        assert pooled - LISTED, v


# ------------------------------------------------------------------ (c): list against cursor
@pytest.mark.parametrize("variant", POOLS)
def test_list_and_cursor_walk_alike(dev, lit, variant):
    """every listed launch again on counting contexts, with and without the cursor forced: the oracle's frames and
    counters, and wave steps, histogram and per-ray work equal between the two hand-outs
    (test_cursor_forced_same_walks' comparison, on its helpers)"""
    done = 0
    for form, L, bounces, v in sorted(LISTED):
        if v != variant:
            continue
        name = f"lit_{form}_{L}"
        ph._SCENES[name] = lit.scene(form, L)
        for W, H in sizes(bounces):
            what = (form, L, bounces, variant, W, H)
            cur = ph.render(name, W, H, "fast", variant, bounces=bounces, flags=dev.FLAG_POOL_CURSOR, counters=True)
            lst = ph.render(name, W, H, "fast", variant, bounces=bounces, counters=True)
            assert "pool_list" not in cur["launch"]["build_bits"], (what, cur["launch"])
            assert "pool_list" in lst["launch"]["build_bits"], (what, lst["launch"])
            assert ph.pool_bit(variant) in cur["launch"]["build_bits"], (what, cur["launch"])
            ref = lit.frame(form, L, W, H, bounces)
            for got, how in ((cur, "cursor"), (lst, "list")):
                same_as_oracle(got, ref, got["bgra"][0], what + (how,))
            ph.same_frames(cur, lst, what)
            for k in ph.STEP_KEYS + ph.RAY_KEYS:
                assert cur["stats"][k] == lst["stats"][k], (what, k, cur["stats"][k], lst["stats"][k])
            assert lst["stats"]["shadow_wave_steps"] > 0
            done += 1
        del ph._SCENES[name]
    assert done > 0, variant


# ------------------------------------------------------------------ (d): batches and samples
BATCH_COUNTS = (3, 8, 9, 32, 33)
BATCH_VARIANTS = ("default", "shpool", "shdefer", "persist4")


@pytest.mark.parametrize("L", BATCH_COUNTS)
def test_batches_of_4(dev, lit, L):
    """one rt_render_frames launch of 4 frames on test_gpu_pool_handout's moving camera: every frame equals the strict
    kernel's single frame of its camera (the first of which is the oracle's), the counters their sum"""
    for form in ls.FORMS:
        c = Ctx(dev, lit.scene(form, L))
        for W, H in SIZES:
            cams = ph.cams(W, H, 4)
            singles = [c.render(W, H, "strict", cam=cam) for cam in cams]
            same_as_oracle(singles[0], lit.frame(form, L, W, H), singles[0]["bgra"][0], (form, L, W, H, "strict"))
            assert not np.array_equal(singles[0]["rgb"], singles[3]["rgb"])  # (the camera moves)
            for variant in BATCH_VARIANTS:
                what = (form, L, W, H, variant)
                got = c.render(W, H, variant, cams=cams)
                for i, one in enumerate(singles):
                    ph.same_frames({k: got[k][i] for k in ("hit", "t", "rgb", "bgra")},
                                   {k: one[k][0] for k in ("hit", "t", "rgb", "bgra")}, what + (i,))
                for k in RAYS:
                    assert got["stats"][k] == sum(one["stats"][k] for one in singles), (what, k)
                assert got["stats"]["stack_overflows"] == 0
                if variant in POOLS:
                    pool_facts(L, 4, variant, got["launch"], what)
        c.close()


@pytest.mark.parametrize("L", BATCH_COUNTS)
def test_spp4(dev, lit, L):
    W, H = SIZES[0]
    for form in ls.FORMS:
        ref, counters = lit.frame_spp(form, L, W, H, 4)
        c = Ctx(dev, lit.scene(form, L))
        for variant in BATCH_VARIANTS:
            what = (form, L, variant)
            got = c.render(W, H, variant, spp=4)
            diff = ph.bits(got["rgb"][0]) != ph.bits(ref)
            assert not diff.any(), (what, int(diff.any(-1).sum()), float(np.abs(got["rgb"][0] - ref).max()))
            for k in RAYS:
                assert got["stats"][k] == counters[k], (what, k, got["stats"][k], counters[k])
            assert got["stats"]["primary"] == 4 * W * H and got["stats"]["stack_overflows"] == 0
            if variant in POOLS:  # (the sample sums take 4 KB of LDS more: which pool fits is the device's answer)
                pool_facts(L, 4, variant, got["launch"], what, boundary=False)
        c.close()


# ------------------------------------------------------------------ (e): the default rule
RULE_FRAMES = 24  # the measuring frame, 4 trial frames for each of 5 candidates at most, 3 more


@pytest.mark.parametrize("L", [2, 9, 33])
def test_the_default_rule(dev, lit, L):
    """consecutive single frames with kernel="fast" on one context, a sync after each: the hybrid rule's measuring
    frame, its trial frames (whose whole-frame kernel is the pool for 2+ lights) and its settled frames. Every frame
    equals the oracle's. Eight frames hold the measuring frame and trials only -- a shape's choice takes 4 trial
    frames per candidate -- so the loop goes on to RULE_FRAMES, by which the rule must have settled."""
    W, H = SIZES[0]
    for form in ls.FORMS:
        ref = lit.frame(form, L, W, H)
        c = Ctx(dev, lit.scene(form, L))
        bgra = c.render(W, H, "strict")["bgra"][0]
        seen = []
        for i in range(RULE_FRAMES):
            got = c.render(W, H, "fast")
            same_as_oracle(got, ref, bgra, (form, L, "frame", i, got["launch"]))
            seen.append(got["launch"])
        c.close()
        print(form, L, [(x["variant"], x["cold_variant"], x["trial"], x["settled"]) for x in seen])
        assert seen[0]["trial"] == 1 and seen[0]["variant"] == "persist", seen[0]  # the measuring frame
        assert any(x["trial"] for x in seen[1:8]), seen[:8]
        if L in (2, 9):  # the rule's pool kernel: the all-levels pool up to 8 lights, the per-level one up to 32
            pool = "shdefer" if L <= 8 else "shpool"
            assert any(pool in (x["variant"], x["cold_variant"]) and ph.pool_bit(pool) in x["build_bits"]
                       for x in seen), seen
            other = "pool_level" if pool == "shdefer" else "pool_all"
            assert not any(other in x["build_bits"] for x in seen), seen
        else:
            assert not any({"pool_all", "pool_level"} & set(x["build_bits"]) for x in seen), seen
        assert seen[-1]["settled"] == 1 and seen[-1]["trial"] == 0, seen[-1]


# ------------------------------------------------------------------ (f): shade queries
@pytest.mark.parametrize("L", [0, 1, 8, 9, 32, 33])
def test_shade_queries(dev, lit, L):
    """the 36x20 camera grid's own rays through rt_shade_rays in every form of test_gpu_shade.FORMS: the oracle's
    frame and counters; unclamped: the strict query's bits"""
    from prt import rays
    from tests.test_gpu_shade import Shader, equal
    W, H = SIZES[1]
    for form, bounces in cases():
        ref = lit.frame(form, L, W, H, bounces)
        want = {"rgb": ref["rgb"].reshape(-1, 3), "hit": ref["hit"].reshape(-1), "t": ref["t"].reshape(-1)}
        sh = Shader(dev, lit.scene(form, L))
        o, d = rays.pinhole(host.camera(W, H), W, H)
        strict = sh.render(host.camera(W, H), W, H, bounces=bounces)
        equal(strict, want, (form, L, bounces, "strict render"))
        np.testing.assert_array_equal(strict["bounce_hit"][:, :4], ref["bounce_hit"].reshape(-1, 4))
        want["bgra"] = strict["bgra"]
        raw = sh.shade(o, d, "strict", 0, bounces=bounces, unclamped=True)
        for kernel, regroup in SHADE_FORMS:
            what = (form, L, bounces, kernel, regroup)
            got = sh.shade(o, d, kernel, regroup, bounces=bounces)
            equal(got, want, what)
            np.testing.assert_array_equal(got["bounce_hit"][:, :4], ref["bounce_hit"].reshape(-1, 4), err_msg=str(what))
            np.testing.assert_array_equal(got["bounce_hit"], strict["bounce_hit"], err_msg=str(what))
            i = got["info"]
            for a, b in (("rays", "primary"), ("hits", "hits"), ("reflection", "reflection"), ("shadow", "shadow"),
                         ("shadow_skipped", "shadow_skipped")):
                assert i[a] == ref["counters"][b], (what, a, i[a], ref["counters"][b])
            assert i["stack_overflows"] == 0, (what, i)
            un = sh.shade(o, d, kernel, regroup, bounces=bounces, unclamped=True)
            equal(un, raw, what + ("unclamped",))
        clamped = np.minimum(np.maximum(raw["rgb"], np.float32(0)), np.float32(1))
        assert np.array_equal(ph.bits(clamped), ph.bits(want["rgb"])), (form, L, bounces)
        sh.r.close()


# ------------------------------------------------------------------ (g): changing lights on a live context
def test_lights_change_on_a_live_context(dev, lit):
    """one Renderer: the hall uploaded with 8, 9, 33 and 2 lights in turn (each resizes the LDS layout, the lists and
    rt_update_lights' pinned staging), after each upload every light moved -- light 0 from above the floor to below
    it; the moved set is a fourth file, so that the oracle reads the same floats"""
    W, H = SIZES[1]
    c = None
    for L in (8, 9, 33, 2):
        s = lit.scene("hall", L)
        moved = ls.moved(ls.lights(L, form="hall"))
        tag = (f"{L}_moved", moved)
        m = lit.scene("hall", tag)  # (the moved lights as the loader reads them)
        assert np.array_equal(m.lights.view(np.float32).reshape(-1, 6).view(np.int32), moved.view(np.int32))
        assert s.lights["pos"][0][2] > ls.FLOOR_Z > m.lights["pos"][0][2]
        if c is None:
            c = Ctx(dev, s)
        else:
            c.r.upload(s)
        before = lit.frame("hall", L, W, H)
        bgra = c.render(W, H, "strict")["bgra"][0]
        same_as_oracle(c.render(W, H, "fast"), before, bgra, (L, "before the update"))
        c.r.update_lights(m.lights)
        ref = lit.frame("hall", tag, W, H)
        assert not np.array_equal(ref["rgb"], before["rgb"])
        bgra = c.render(W, H, "strict")["bgra"][0]
        for kernel in ("strict", "shpool", "shdefer", "fast"):
            got = c.render(W, H, kernel)
            same_as_oracle(got, ref, bgra, (L, "moved", kernel))
            if kernel in POOLS:
                pool_facts(L, 4, kernel, got["launch"], (L, "moved", kernel))
    c.close()
