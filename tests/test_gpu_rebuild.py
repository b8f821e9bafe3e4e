"""View rebuilds (rt_rebuild_views: Renderer.rebuild_views / rebuild_info / _debug_build_tree). A rebuild keeps the
reference tree, so the yardstick is the vertex update's: a second Renderer freshly uploaded with the moved scene S'
(tests/test_gpu_refit.py moved_scene), compared bit for bit on rgb, hit, t and bounce_hit for the strict kernel and every
fast variant, and on closest-hit, occlusion and radiance queries; the round trip back to the original coordinates is
compared with the reference's own committed frame. The device path's words are held to the CPU mirror
(host.wbvh_build_greedy) run on the binary tree the device collapsed, bit for bit.

The motion is LARGE: for it, on the CPU, the greedy mirror's summed child-box area over S' is below the refitted host
tree's (checked in the fixture before any GPU work) -- the condition under which a rebuild is worth making."""
import os

import numpy as np
import pytest

from prt import host
from tests.test_gpu_refit import (GOLD, KERNELS, equal_frames, frame, hittable, inflation, moved_scene, rigid,
                                  same_bits, update)

pytestmark = pytest.mark.gpu

W, H = 64, 36
WSTACK = 16
LARGE = dict(angle=2.5, shift=(-4.0, 3.0, 2.0))
MODES = ["device", "host", "auto"]
VIEWS = ["full", "unit", "primary"]


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


def decoded_area(words):
    """rt_quant.hpp decoded_area summed over the nodes"""
    D = host.wbvh_decode(words)
    occ = (D["meta"] != 0) | (((D["imask"][:, None] >> np.arange(8)) & 1) != 0)
    d = D["hi"].astype(np.float64) - D["lo"].astype(np.float64)
    a = 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
    return float(a[occ].sum())


def cuda(coords):
    import torch
    return torch.from_numpy(np.ascontiguousarray(coords, np.float32)).cuda()


class Moved:
    """a scene, its LARGE motion, S' and the yardstick: a fresh upload of S' with its frames (made once, read-only)"""

    def __init__(self, dev, name):
        self.scene = s = host.Scene.named(name).build_bvh(3)
        self.coords, self.sel = rigid(s, **LARGE)
        c0 = s.triangles["coords"]
        for dmax in (1.0, 3.0):  # a rigid motion of this size flips hittable() for no triangle
            assert np.array_equal(hittable(self.coords, dmax), hittable(c0, dmax))
        self.s1 = moved_scene(s, self.coords)
        # the premise, on the CPU: the greedy mirror over S' is tighter than the refitted host tree
        n0, i0, _ = host.bvh_build(s.triangles, "binned_sah")
        w0, o0, _ = host.wbvh_build(n0, i0, s.triangles, inflation(c0))
        infl = inflation(self.coords)
        n1, i1, _ = host.bvh_build(self.s1.triangles, "binned_sah")
        refit = decoded_area(host.wbvh_refit(w0, o0, self.s1.triangles, infl))
        greedy = decoded_area(host.wbvh_build_greedy(n1, i1, self.s1.triangles, infl)[0])
        assert greedy < refit, (greedy, refit)
        self.fresh = dev.Renderer(0).upload(self.s1)
        self._want = {}

    def want(self, kernel):
        if kernel not in self._want:
            self._want[kernel] = frame(self.fresh, kernel)
            for v in self._want[kernel].values():
                v.setflags(write=False)
        return self._want[kernel]


@pytest.fixture(scope="module")
def moved(dev):
    out = {name: Moved(dev, name) for name in ("car_only", "car_boxed")}
    yield out
    for m in out.values():
        m.fresh.close()


@pytest.fixture(scope="module")
def rebuilt(dev, moved):
    """(scene, mode) -> a Renderer uploaded with the scene and rebuilt to the LARGE motion, made on first use"""
    made = {}

    def get(name, mode):
        if (name, mode) not in made:
            r = dev.Renderer(0).upload(moved[name].scene)
            assert r.scene_info()["accel_built"] == "gpu"
            r.rebuild_views(cuda(moved[name].coords), mode=mode)
            made[name, mode] = r
        return made[name, mode]

    yield get
    for r in made.values():
        r.close()


# ---------------------------------------------------------------- bits
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["car_only", "car_boxed"])
def test_rebuild_equals_a_fresh_upload(moved, rebuilt, name, mode, kernel):
    got = frame(rebuilt(name, mode), kernel)
    equal_frames(got, moved[name].want(kernel), f"{name} {mode} {kernel}")
    equal_frames(got, moved[name].want("strict"), f"{name} {mode} {kernel} vs strict")
    assert (got["hit"] >= 0).sum() > 200


def test_rebuild_info(moved, rebuilt):
    for name in ("car_only", "car_boxed"):
        fresh = moved[name].fresh.scene_info()
        for mode in MODES:
            r = rebuilt(name, mode)
            i, now = r.rebuild_info(), r.scene_info()
            assert i["mode_used"] == ("host" if mode == "host" else "device") and i["fell_back"] == 0, i
            assert i["views_built"] == sum(1 for k in range(3) if i["nodes"][k] > 0) >= 1, i
            assert i["nodes"] == [now["wide_nodes"], now["unit_nodes"], now["primary_nodes"]], (i, now)
            assert i["depth"][0] == now["wide_depth"] and all(0 <= d <= WSTACK for d in i["depth"]), i
            assert 0 < i["area_after"] < i["area_before"], i  # the LARGE motion's premise, on the device's own trees
            assert i["rebuild_ms"] > 0 and i["host_ms"] > 0 and i["ploc_ms"] > 0 and i["collapse_ms"] > 0, i
            # membership: the subset views hold the triangles a fresh upload's hold
            for f in ("n_triangles", "unit_triangles", "primary_triangles", "accel_built"):
                assert now[f] == fresh[f], (name, mode, f, now, fresh)


def rays(m, n=2048):
    rng = np.random.default_rng(11)
    c = m.s1.triangles["coords"].reshape(-1, 3)
    lo, hi = c.min(0) - 1, c.max(0) + 1
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = (c[rng.integers(0, len(c), n)] - o).astype(np.float32)  # aimed at a vertex
    d[n // 2:] /= np.linalg.norm(d[n // 2:], axis=1, keepdims=True).astype(np.float32)
    md2 = rng.uniform(0.5, 400.0, n).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), md2


def queries(r, o, d, md2):
    import torch
    got = {}
    for kernel in ("strict", "fast"):
        hit, t = r.trace_rays(o, d, kernel=kernel)
        occ = r.occluded(o, d, md2, kernel=kernel)
        bh = torch.empty((len(o), 4), dtype=torch.int32, device="cuda")
        rgb = torch.empty((len(o), 3), dtype=torch.float32, device="cuda")
        r.shade_rays(o, d, kernel=kernel, rgb=rgb, bounce_hit=bh)
        r.sync()
        got[kernel] = {"hit": hit.cpu().numpy(), "t": t.cpu().numpy(), "occluded": occ.cpu().numpy(),
                       "rgb": rgb.cpu().numpy(), "bounce_hit": bh.cpu().numpy()}
    return got


@pytest.mark.parametrize("name", ["car_only", "car_boxed"])
def test_queries_equal_a_fresh_upload(moved, rebuilt, name):
    m = moved[name]
    o, d, md2 = (cuda(x) for x in rays(m))
    want = queries(m.fresh, o, d, md2)
    hit = want["strict"]["hit"]
    assert (hit >= 0).sum() > 500 and np.isin(hit, m.sel).sum() > 50 and 50 < want["strict"]["occluded"].sum() < 2048
    for mode in MODES:
        got = queries(rebuilt(name, mode), o, d, md2)
        for kernel in ("strict", "fast"):
            for k, v in got[kernel].items():
                w = want[kernel][k]
                assert same_bits(v, w), (mode, kernel, k, int((v.view(np.int32) != w.view(np.int32)).sum()))


@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("name", ["car_only", "car_boxed"])
def test_round_trip_gives_the_reference_frame(dev, moved, name, mode):
    """rebuilt for the LARGE motion, then updated back to the original coordinates: the frame the reference itself
    rendered, from the strict kernel and from the fast one on the rebuilt (now refitted) views"""
    m = moved[name]
    r = dev.Renderer(0).upload(m.scene)
    r.rebuild_views(cuda(m.coords), mode=mode)
    assert not same_bits(frame(r, "strict")["rgb"], np.load(os.path.join(GOLD, f"{name}_64x36_strict.npz"))["rgb"])
    i = update(r, m.scene.triangles["coords"])
    assert i["views_rebuilt"] == 0 and i["views_refit"] == 3, i
    ref = np.load(os.path.join(GOLD, f"{name}_64x36_strict.npz"))
    for kernel in ("strict", "fast"):
        got = frame(r, kernel)
        np.testing.assert_array_equal(got["hit"], ref["hit"])
        assert same_bits(got["t"], ref["t"]) and same_bits(got["rgb"], ref["rgb"]), kernel
    r.close()


# ---------------------------------------------------------------- device == mirror
def mirror(r, view, s1):
    """host.wbvh_build_greedy over the binary tree the device collapsed for `view`, with S' -> (words, tri_orig)"""
    left, right, leaf, root = r._debug_build_tree(view)
    n = len(leaf)
    ids = np.unique(leaf)  # the view's triangles, rising: PLOC's input order
    assert len(ids) == n
    nodes, order = host.bvh_from_links(left, right, root, n)
    tri_idx = np.searchsorted(ids, leaf[order]).astype(np.int32)
    words, tri_order, info = host.wbvh_build_greedy(nodes, tri_idx, s1.triangles[ids], inflation(s1.triangles["coords"]))
    return words, ids[tri_order], info


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("name", ["car_only", "car_boxed"])
def test_device_rebuild_equals_the_mirror(moved, rebuilt, name, view):
    r = rebuilt(name, "device")
    words, orig = r._debug_wide(view)
    if words is None:  # the fresh upload has no such view either (test_rebuild_info: the same membership)
        assert moved[name].fresh._debug_wide(view)[0] is None and r._debug_build_tree(view) is None
        return
    want, want_orig, info = mirror(r, view, moved[name].s1)
    np.testing.assert_array_equal(orig, want_orig)
    np.testing.assert_array_equal(words, want)
    rc, ci = host.wbvh_check(words, np.argsort(np.argsort(orig)).astype(np.int32), WSTACK)
    assert rc == 0 and ci["depth"] == info["depth"], (rc, ci, info)
    assert r.rebuild_info()["depth"][VIEWS.index(view)] == info["depth"]


def test_full_view_exists_on_both_scenes(rebuilt):
    for name in ("car_only", "car_boxed"):
        assert rebuilt(name, "device")._debug_wide("full")[0] is not None
    assert rebuilt("car_boxed", "device")._debug_wide("unit")[0] is not None  # (car_boxed has both subset views)
    assert rebuilt("car_boxed", "device")._debug_wide("primary")[0] is not None


def test_two_rebuilds_give_identical_words(dev, moved):
    m = moved["car_boxed"]
    r = dev.Renderer(0).upload(m.scene)
    c = cuda(m.coords)
    r.rebuild_views(c, mode="device")
    first = {v: r._debug_wide(v) for v in VIEWS}
    r.rebuild_views(c, mode="device")
    for v in VIEWS:
        again = r._debug_wide(v)
        np.testing.assert_array_equal(again[0], first[v][0])
        np.testing.assert_array_equal(again[1], first[v][1])
    r.close()


# ---------------------------------------------------------------- membership
@pytest.mark.parametrize("mode", ["device", "host"])
def test_membership_follows_the_upload_rule(dev, mode):
    """tests/test_gpu_refit.py's member move: triangles scaled up join the subset views, others scaled down leave them"""
    s = host.Scene.named("car_boxed").build_bvh(3)
    c0 = s.triangles["coords"]
    c = c0.astype(np.float64)
    hu = hittable(c0, 1.0)
    up, down = np.nonzero(~hu)[0][::3], np.nonzero(hu)[0][::7]
    cen = c.mean(1, keepdims=True)
    c[up] = cen[up] + (c[up] - cen[up]) * 4.0
    c[down] = cen[down] + (c[down] - cen[down]) * 1e-3
    coords = np.ascontiguousarray(c.astype(np.float32))
    assert (hittable(coords, 1.0) & ~hu).sum() > 0 and (~hittable(coords, 1.0) & hu).sum() > 0
    s1 = moved_scene(s, coords)
    r = dev.Renderer(0).upload(s)
    before = r.scene_info()
    r.rebuild_views(cuda(coords), mode=mode)
    fresh = dev.Renderer(0).upload(s1)
    now, want = r.scene_info(), fresh.scene_info()
    assert now["unit_triangles"] == int(hittable(coords, 1.0).sum()) != before["unit_triangles"]
    for f in ("n_triangles", "unit_triangles", "primary_triangles", "accel_built"):
        assert now[f] == want[f], (f, now, want)
    for kernel in ("strict", "fast", "shpool"):
        equal_frames(frame(r, kernel), frame(fresh, "strict"), kernel)
    if mode == "device":
        for view in ("unit", "primary"):
            words, orig = r._debug_wide(view)
            w, o, _ = mirror(r, view, s1)
            np.testing.assert_array_equal(orig, o)
            np.testing.assert_array_equal(words, w)
    r.close()
    fresh.close()


# ---------------------------------------------------------------- small shapes
def one_centroid_scene(n=40):
    """triangles whose boxes all have the centre (1, 2, 3) exactly: every Morton code is equal"""
    rng = np.random.default_rng(3)
    e = rng.integers(1, 64, (n, 3)).astype(np.float64) / 16.0
    c = np.zeros((n, 3, 3))
    c[:, 0] = -e
    c[:, 1] = e * np.array([1.0, -1.0, 1.0])
    c[:, 2] = e * np.array([0.0, 1.0, 0.0])
    c += np.array([1.0, 2.0, 3.0])
    coords = c.astype(np.float32)
    assert ((coords.min(1) + coords.max(1)) == np.array([2.0, 4.0, 6.0], np.float32)).all()
    z = np.full((n, 3), 0.5, np.float32)
    s = host.Scene(host.triangle_init(coords, z, z, z), np.zeros(0, host.LIGHT_DTYPE))
    return s.build_bvh("binned_sah")  # (the reference builder's random splits never part centroids that differ on one axis only)


@pytest.mark.parametrize("n", [1, 2, 8, 9, 33, 2000, "one_centroid"])
def test_small_shapes(dev, n):
    s = one_centroid_scene() if n == "one_centroid" else host.Scene.random(n).build_bvh(3)
    c = s.triangles["coords"].astype(np.float64)
    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    coords = c.astype(np.float32) if n == "one_centroid" else np.ascontiguousarray((c @ R.T * 1.5).astype(np.float32))
    r = dev.Renderer(0).upload(s)
    built = r.scene_info()["accel_built"]
    r.rebuild_views(cuda(coords), mode="auto")
    i = r.rebuild_info()
    assert built == "gpu", built  # (these scenes all build on the device at upload)
    assert (i["mode_used"], i["fell_back"]) in (("device", 0), ("host", 1), ("host", 2)), i  # DEVICE, or as reported
    fresh = dev.Renderer(0).upload(moved_scene(s, coords))
    want = frame(fresh, "strict")
    equal_frames(frame(r, "strict"), want, "strict")
    equal_frames(frame(r, "fast"), want, "fast")
    if i["mode_used"] == "device":
        words, orig = r._debug_wide("full")
        w, o, info = mirror(r, "full", moved_scene(s, coords))
        np.testing.assert_array_equal(orig, o)
        np.testing.assert_array_equal(words, w)
        assert i["nodes"][0] == info["n_nodes"] and i["depth"][0] == info["depth"]
    r.close()
    fresh.close()


# ---------------------------------------------------------------- state and errors
def test_errors_and_state(dev, moved):
    m = moved["car_only"]
    s = m.scene
    r = dev.Renderer(0)
    c1 = cuda(m.coords)
    with pytest.raises(dev.RtError, match="status -5"):  # RT_E_STATE before an upload
        r.rebuild_views(c1)
    r.upload(s, accel="reference")
    with pytest.raises(dev.RtError, match="status -5"):  # no wide view
        r.rebuild_views(c1)
    r.upload(s, accel="host")
    with pytest.raises(dev.RtError, match="status -1"):  # DEVICE mode on a host-built scene
        r.rebuild_views(c1, mode="device")
    with pytest.raises(dev.RtError, match="status -5"):  # no rebuild yet
        r.rebuild_info()
    r.rebuild_views(c1, mode="auto")  # AUTO on a host-built scene: HOST
    i = r.rebuild_info()
    assert i["mode_used"] == "host" and i["fell_back"] == 0, i
    equal_frames(frame(r, "fast"), m.want("strict"), "host-built, rebuilt")
    r.upload(s)
    with pytest.raises(dev.RtError, match="status -5"):  # (an upload forgets the last rebuild)
        r.rebuild_info()
    with pytest.raises(dev.RtError, match="status -1"):  # a count mismatch
        r.rebuild_views(c1[:-1].contiguous())
    before = frame(r, "fast")
    words0 = r._debug_wide("full")[0]
    bad = c1.clone()
    bad[len(bad) // 2, 1, 2] = float("nan")
    for mode in MODES:
        with pytest.raises(dev.RtError, match="not finite"):
            r.rebuild_views(bad, mode=mode)
    equal_frames(frame(r, "fast"), before, "after a refused rebuild")
    equal_frames(frame(r, "strict"), before, "after a refused rebuild, strict")
    np.testing.assert_array_equal(r._debug_wide("full")[0], words0)
    with pytest.raises(dev.RtError, match="status -5"):  # (a refused rebuild is no rebuild, and no update either)
        r.rebuild_info()
    with pytest.raises(dev.RtError, match="status -5"):
        r.update_info()
    r.close()


def test_area_ratio_is_measured_against_the_rebuilt_view(dev, moved):
    m = moved["car_only"]
    r = dev.Renderer(0).upload(m.scene)
    grown = update(r, m.coords)["area_ratio"]
    assert grown > 1.2, grown
    r.rebuild_views(cuda(m.coords), mode="device")
    i = r.rebuild_info()
    assert i["area_after"] < i["area_before"] and abs(i["area_before"] / i["area_after"]) > 1.0
    again = update(r, m.coords)  # an identity update of the rebuilt views
    assert again["views_rebuilt"] == 0 and abs(again["area_ratio"] - 1.0) < 1e-6, again
    equal_frames(frame(r, "fast"), m.want("strict"), "rebuilt, then updated")
    r.close()


def test_launch_decisions_survive_a_rebuild(dev, moved):
    import torch
    m = moved["car_only"]
    r = dev.Renderer(0).upload(m.scene)
    cams = [host.camera(W, H)] * 4
    rgb = torch.empty((4, H, W, 3), dtype=torch.float32, device="cuda")
    for _ in range(8):
        r.render_frames(cams, W, H, rgb=rgb)
        r.sync()
        if r.launch_info()["settled"]:
            break
    li = r.launch_info()
    assert li["settled"] == 1 and li["trial"] == 0, li
    r.rebuild_views(cuda(m.coords), mode="device")
    r.render_frames(cams, W, H, rgb=rgb)
    r.sync()
    lj = r.launch_info()
    assert lj["settled"] == 1 and lj["trial"] == 0 and lj["variant"] == li["variant"], (li, lj)
    got = rgb.cpu().numpy()
    for f in range(4):
        assert same_bits(got[f], m.want("strict")["rgb"]), f
    r.close()
