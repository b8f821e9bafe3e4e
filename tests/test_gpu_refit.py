"""Vertex updates (rt_update_vertices: Renderer.update_vertices / update_info / update_lights). The yardstick is always a
second Renderer freshly uploaded with the moved scene S' -- host.triangle_init of the new coordinates with the old
materials, the uploaded reference tree with every box regrown in numpy from +-1e10 -- compared bit for bit on rgb, hit,
t and bounce_hit, for the strict kernel and the fast variants; the round trip back to the original coordinates is
compared with the reference's own committed frame. Whether a move changes a subset view's membership is decided here on
the CPU with hittable()'s own arithmetic, so what each test expects of views_rebuilt is a property of its input."""
import os

import numpy as np
import pytest

from prt import host
from tests.test_refit_host import regrow

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 64, 36
KERNELS = ["strict", "fast", "persist4", "coop4", "shpool", "shdefer"]
OUTS = ("rgb", "hit", "t", "bounce_hit")


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


@pytest.fixture(scope="module")
def scenes():
    return {name: host.Scene.named(name).build_bvh(3) for name in ("car_boxed", "car_only")}


# ---------------------------------------------------------------- S' on the CPU
def hittable(coords, dmax):
    """rt_hip.hip hittable(): the record normal in float32 (tri_records' roundings), its length in float64 against
    EPSILON (1 - 1e-5) / dmax"""
    c = np.asarray(coords, np.float32)
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    nx, ny, nz = (v.astype(np.float64) for v in (nx, ny, nz))
    return np.sqrt(nx * nx + ny * ny + nz * nz) >= (1.0 - 1e-5) * float(np.float32(1e-3)) / dmax


def moved_scene(scene, coords):
    t = scene.triangles
    s = host.Scene(host.triangle_init(coords, t["ks"], t["kd"], t["kr"]), scene.lights.copy())
    s.nodes, s.tri_idx, s.amb = regrow(scene.nodes, scene.tri_idx, coords), scene.tri_idx, scene.amb
    return s


def rigid(scene, angle=0.1, shift=(0.5, -0.25, 0.125), scale=None):
    """the triangles with centroid x > 0 rotated about z and translated -> (coords' float32, their indices)"""
    c = scene.triangles["coords"].astype(np.float64)
    sel = np.nonzero(scene.triangles["centroid"][:, 0] > 0)[0]
    R = np.array([[np.cos(angle), -np.sin(angle), 0.0], [np.sin(angle), np.cos(angle), 0.0], [0.0, 0.0, 1.0]])
    c[sel] = c[sel] @ R.T + np.array(shift)
    return np.ascontiguousarray(c.astype(np.float32)), sel


def inflation(coords):
    return float(np.ldexp(np.float32(max(np.float32(16.0), np.abs(coords).max())), -16))


# ---------------------------------------------------------------- renderers
def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def frame(r, kernel, bounces=4):
    import torch
    b = {"rgb": torch.empty((H, W, 3), dtype=torch.float32, device="cuda"),
         "hit": torch.empty((H, W), dtype=torch.int32, device="cuda"),
         "t": torch.empty((H, W), dtype=torch.float32, device="cuda"),
         "bounce_hit": torch.empty((H, W, bounces), dtype=torch.int32, device="cuda")}
    r.render(host.camera(W, H), W, H, bounces=bounces, kernel=kernel, **b)
    r.sync()
    return {k: v.cpu().numpy() for k, v in b.items()}


def equal_frames(got, want, what=""):
    for k in OUTS:
        assert same_bits(got[k], want[k]), (what, k, int((got[k].view(np.int32) != want[k].view(np.int32)).sum()))


def update(r, coords):
    import torch
    r.update_vertices(torch.from_numpy(np.ascontiguousarray(coords, np.float32)).cuda())
    return r.update_info()


class Pair:
    """a Renderer uploaded with `scene` and updated to `coords`, and the yardstick: a fresh upload of S'"""

    def __init__(self, dev, scene, coords, accel="auto"):
        self.s1 = moved_scene(scene, coords)
        self.upd = dev.Renderer(0).upload(scene, accel=accel)
        self.before = {v: self.upd._debug_wide(v) for v in ("full", "unit", "primary")}
        self.info0 = self.upd.scene_info()
        self.info = update(self.upd, coords)
        self.after = {v: self.upd._debug_wide(v) for v in ("full", "unit", "primary")}
        self.fresh = dev.Renderer(0).upload(self.s1, accel=accel)
        self._want = {}

    def want(self, kernel):
        """the yardstick's frames: the strict kernel's once, shared; a fast variant's own render of the fresh upload"""
        if kernel not in self._want:
            self._want[kernel] = frame(self.fresh, kernel)
            for v in self._want[kernel].values():
                v.setflags(write=False)
        return self._want[kernel]

    def close(self):
        self.upd.close()
        self.fresh.close()


# ---------------------------------------------------------------- rigid motion
@pytest.fixture(scope="module")
def rigid_pair(dev, scenes):
    s = scenes["car_boxed"]
    coords, sel = rigid(s)
    # the condition of views_rebuilt == 0, as a property of the input: hittable() flips for no triangle
    c0 = s.triangles["coords"]
    for dmax in (1.0, 3.0):
        assert np.array_equal(hittable(coords, dmax), hittable(c0, dmax))
    assert len(sel) > 10000 and not np.array_equal(coords[sel], c0[sel])
    p = Pair(dev, s, coords)
    yield p
    p.close()


def test_rigid_motion_refits_every_view(rigid_pair):
    i, i0 = rigid_pair.info, rigid_pair.info0
    assert i0["unit_nodes"] > 0 and i0["primary_nodes"] > 0  # car_boxed has both subset views
    assert i["views_rebuilt"] == 0 and i["views_refit"] == 3 and i["joined_unit"] == 0 and i["joined_primary"] == 0, i
    assert i["scene_magnitude"] == np.float32(max(16.0, np.abs(rigid_pair.s1.triangles["coords"]).max()))
    assert i["update_ms"] > 0 and 0.5 < i["area_ratio"] < 50.0, i
    now = rigid_pair.upd.scene_info()
    for f in ("n_triangles", "wide_nodes", "wide_depth", "unit_triangles", "unit_nodes", "primary_triangles",
              "primary_nodes", "accel_built"):
        assert now[f] == i0[f], f


@pytest.mark.parametrize("kernel", KERNELS)
def test_rigid_motion_equals_a_fresh_upload(rigid_pair, kernel):
    got = frame(rigid_pair.upd, kernel)
    equal_frames(got, rigid_pair.want(kernel), kernel)
    equal_frames(got, rigid_pair.want("strict"), kernel + " vs strict")
    assert (got["hit"] >= 0).sum() > 1000


@pytest.mark.parametrize("view", ["full", "unit", "primary"])
def test_device_refit_equals_the_host_refit(rigid_pair, view):
    """the words the device refit left, read back (test-only), against host.wbvh_refit of the words before"""
    words0, orig = rigid_pair.before[view]
    words1, orig1 = rigid_pair.after[view]
    assert words0 is not None and np.array_equal(orig, orig1)
    s1 = rigid_pair.s1
    want = host.wbvh_refit(words0, orig, s1.triangles, inflation(s1.triangles["coords"]))
    assert not np.array_equal(words0, words1)
    np.testing.assert_array_equal(words1, want)


def test_round_trip_gives_the_reference_frames(dev, scenes):
    """moved, then updated again with the original coordinates: the frame the reference itself rendered
    (car_boxed_64x36_strict.npz), from the strict kernel and from the fast one. car_boxed_64x36_fast.npz is the
    reference built with -ffast-math, whose bits no kernel of this library renders, fresh upload or not: the fast
    kernel's frame differs from it exactly where a fresh upload's does."""
    s = scenes["car_boxed"]
    r = dev.Renderer(0).upload(s)
    fresh = {k: frame(r, k) for k in ("strict", "fast")}
    update(r, rigid(s)[0])
    moved = frame(r, "strict")
    assert not same_bits(moved["rgb"], fresh["strict"]["rgb"])
    i = update(r, s.triangles["coords"])
    assert i["views_rebuilt"] == 0 and abs(i["area_ratio"] - 1.0) < 1e-6, i
    ref = np.load(os.path.join(GOLD, "car_boxed_64x36_strict.npz"))
    ref_fast = np.load(os.path.join(GOLD, "car_boxed_64x36_fast.npz"))
    for kernel in ("strict", "fast"):
        got = frame(r, kernel)
        np.testing.assert_array_equal(got["hit"], ref["hit"])
        assert same_bits(got["t"], ref["t"]) and same_bits(got["rgb"], ref["rgb"]), kernel
        equal_frames(got, fresh[kernel], kernel)
        for k in ("hit", "t", "rgb"):  # against the -ffast-math fixture: what a fresh upload's frame gives
            np.testing.assert_array_equal(got[k].view(np.int32) != ref_fast[k].view(np.int32),
                                          fresh[kernel][k].view(np.int32) != ref_fast[k].view(np.int32))
    r.close()


# ---------------------------------------------------------------- membership
@pytest.fixture(scope="module")
def member_pair(dev, scenes):
    s = scenes["car_boxed"]
    c0 = s.triangles["coords"]
    c = c0.astype(np.float64)
    hu, hp = hittable(c0, 1.0), hittable(c0, 3.0)
    up = np.nonzero(~hu)[0][::3]      # every third triangle no unit ray can hit (those no primary ray can, among them)
    down = np.nonzero(hu)[0][::7]     # every seventh one they can
    cen = c.mean(1, keepdims=True)
    c[up] = cen[up] + (c[up] - cen[up]) * 4.0
    c[down] = cen[down] + (c[down] - cen[down]) * 1e-3
    coords = np.ascontiguousarray(c.astype(np.float32))
    p = Pair(dev, s, coords)
    p.joins = (int((hittable(coords, 1.0) & ~hu).sum()), int((hittable(coords, 3.0) & ~hp).sum()))
    p.leaves = int((~hittable(coords, 1.0) & hu).sum())
    yield p
    p.close()


def test_membership_change_rebuilds_the_views(member_pair):
    i = member_pair.info
    assert member_pair.joins[0] > 0 and member_pair.joins[1] > 0 and member_pair.leaves > 0  # the input's property
    assert i["joined_unit"] == member_pair.joins[0] and i["joined_primary"] == member_pair.joins[1], i
    assert i["views_rebuilt"] == 2 and i["views_refit"] == 1, i
    now, fresh = member_pair.upd.scene_info(), member_pair.fresh.scene_info()
    for f in ("n_triangles", "n_lights", "accel_built", "unit_triangles", "unit_nodes", "unit_depth",
              "primary_triangles", "primary_nodes"):
        assert now[f] == fresh[f], (f, now, fresh)
    assert now["unit_triangles"] != member_pair.info0["unit_triangles"]
    assert now["wide_nodes"] == member_pair.info0["wide_nodes"]  # the full view keeps its topology


@pytest.mark.parametrize("kernel", KERNELS)
def test_membership_change_equals_a_fresh_upload(member_pair, kernel):
    got = frame(member_pair.upd, kernel)
    equal_frames(got, member_pair.want(kernel), kernel)
    equal_frames(got, member_pair.want("strict"), kernel + " vs strict")


# ---------------------------------------------------------------- far move: magnitude, inflation, query domain, faces
@pytest.fixture(scope="module")
def far_pair(dev, scenes):
    s = scenes["car_boxed"]
    coords, sel = rigid(s, angle=0.0, shift=(0.0, 50.0, 0.0))
    for dmax in (1.0, 3.0):  # (a translation by an integer: no flips either)
        assert np.array_equal(hittable(coords, dmax), hittable(s.triangles["coords"], dmax))
    p = Pair(dev, s, coords)
    p.sel = sel
    yield p
    p.close()


def test_far_move_changes_the_magnitude(far_pair):
    i = far_pair.info
    mx = np.float32(np.abs(far_pair.s1.triangles["coords"]).max())
    assert mx > 59 and i["scene_magnitude"] == mx and i["views_rebuilt"] == 0, i
    assert i["area_ratio"] > 1.0, i  # boxes that span the gap
    w0, w1 = far_pair.before["full"][0], far_pair.after["full"][0]
    assert ((w0[:, 3] ^ w1[:, 3]) & 0xFFFFFF).any()  # other exponents
    s1 = far_pair.s1
    np.testing.assert_array_equal(w1, host.wbvh_refit(w0, far_pair.before["full"][1], s1.triangles,
                                                      inflation(s1.triangles["coords"])))


@pytest.mark.parametrize("kernel", KERNELS)
def test_far_move_equals_a_fresh_upload(far_pair, kernel):
    equal_frames(frame(far_pair.upd, kernel), far_pair.want(kernel), kernel)


def far_rays(p):
    """4096 rays on the moved scene: 2048 random ones between the two parts, 1024 unit-length ones, and 1024
    axis-parallel ones whose origins sit on a box face of the NEW reference tree along a zero axis of the direction
    (half of them a float off that face) -- the walks consult the rebuilt face lists for these"""
    rng = np.random.default_rng(7)
    s1 = p.s1
    lo, hi = np.array([-11, -11, -11], np.float32), np.array([11, 61, 11], np.float32)
    o = rng.uniform(lo, hi, (3072, 3)).astype(np.float32)
    d = rng.normal(size=(3072, 3)).astype(np.float32)
    d[2048:] /= np.linalg.norm(d[2048:], axis=1, keepdims=True).astype(np.float32)
    inner = np.nonzero((s1.nodes["tr_len"] > 0) | (s1.nodes["child"] != 0))[0]
    pick = rng.choice(inner, 1024)
    fo = rng.uniform(lo, hi, (1024, 3)).astype(np.float32)
    fd = rng.normal(size=(1024, 3)).astype(np.float32)
    for k in range(1024):
        ax = k % 3
        face = s1.nodes["min" if k & 4 else "max"][pick[k]][ax]
        fo[k, ax] = face if k & 8 else np.nextafter(face, np.float32(np.inf))
        fd[k, ax] = 0.0
        if k & 16:
            fd[k, (ax + 1) % 3] = 0.0  # two zero components
            fo[k, (ax + 1) % 3] = s1.nodes["min"][pick[k]][(ax + 1) % 3]
    # aim the face rays at the geometry: towards a random vertex, keeping the zero components
    tgt = s1.triangles["coords"].reshape(-1, 3)[rng.integers(0, 3 * len(s1.triangles), 1024)]
    aim = (tgt - fo).astype(np.float32)
    fd = np.where(fd == 0.0, np.float32(0.0), aim).astype(np.float32)
    o, d = np.concatenate([o, fo]), np.concatenate([d, fd])
    md2 = rng.uniform(0.5, 4000.0, len(o)).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), md2


def test_far_move_queries_equal_a_fresh_upload(far_pair):
    import torch
    o, d, md2 = far_rays(far_pair)
    assert len(o) == 4096 and ((d == 0).sum(1) >= 1).sum() >= 1024
    to, td, tm = (torch.from_numpy(x).cuda() for x in (o, d, md2))
    want = None
    for r, name in ((far_pair.fresh, "fresh"), (far_pair.upd, "updated")):
        got = {}
        for kernel in ("strict", "fast"):
            hit, t = r.trace_rays(to, td, kernel=kernel)
            occ = r.occluded(to, td, tm, kernel=kernel)
            bh = torch.empty((len(o), 4), dtype=torch.int32, device="cuda")
            rgb = torch.empty((len(o), 3), dtype=torch.float32, device="cuda")
            r.shade_rays(to, td, kernel=kernel, rgb=rgb, bounce_hit=bh)
            r.sync()
            got[kernel] = {"hit": hit.cpu().numpy(), "t": t.cpu().numpy(), "occluded": occ.cpu().numpy(),
                           "rgb": rgb.cpu().numpy(), "bounce_hit": bh.cpu().numpy()}
            if kernel == "fast":
                qi = r.query_info()
                assert qi["stack_overflows"] == 0
        if want is None:
            want = got
            hit = want["strict"]["hit"]
            assert (hit >= 0).sum() > 500 and (hit < 0).sum() > 100
            assert 100 < want["strict"]["occluded"].sum() < 4000
            assert np.isin(hit, far_pair.sel).sum() > 100 and (hit[3072:] >= 0).sum() > 50  # the moved part; the face rays
            # (the fresh upload's fast answers are its strict ones except on rays with two zero components whose origin
            # lies on box faces along both: one of these 4096, where the reference walk itself loses the nearer
            # triangle to its 0 / 0 slabs -- the walks' business, not the update's: each kernel is held to its own
            # answers on the fresh upload)
            assert (want["fast"]["hit"] != hit).sum() <= 4
        else:
            for kernel in ("strict", "fast"):
                for k, v in got[kernel].items():
                    w = want[kernel][k]
                    assert same_bits(v, w), (kernel, k, int((v.view(np.int32) != w.view(np.int32)).sum()))


# ---------------------------------------------------------------- accel modes: a binary acceleration view, no PLOC
@pytest.mark.parametrize("accel", ["host", "reference"])
def test_accel_modes(dev, scenes, accel):
    s = scenes["car_only"]
    coords, _ = rigid(s)
    for dmax in (1.0, 3.0):
        assert np.array_equal(hittable(coords, dmax), hittable(s.triangles["coords"], dmax))
    p = Pair(dev, s, coords, accel=accel)
    assert p.info["views_rebuilt"] == 0 and p.info["views_refit"] == (3 if accel == "host" else 0), p.info
    assert p.upd.scene_info()["accel_built"] == accel
    if accel == "reference":
        assert p.info["area_ratio"] == 1.0
    # (without a wide view the variants all run the binary fast walk: the strict and the fast kernel cover it)
    for kernel in ("strict", "fast", "persist4", "shpool") if accel == "host" else ("strict", "fast"):
        equal_frames(frame(p.upd, kernel), p.want(kernel), f"{accel} {kernel}")
        equal_frames(p.want(kernel), p.want("strict"), f"{accel} {kernel} vs strict")
    p.close()


# ---------------------------------------------------------------- errors and state
def test_errors_and_state(dev, scenes):
    import torch
    s = scenes["car_only"]
    r = dev.Renderer(0)
    c0 = torch.from_numpy(np.ascontiguousarray(s.triangles["coords"])).cuda()
    with pytest.raises(dev.RtError, match="status -5"):  # RT_E_STATE before an upload
        r.update_vertices(c0)
    r.upload(s)
    with pytest.raises(dev.RtError, match="status -5"):  # no update yet
        r.update_info()
    with pytest.raises(dev.RtError, match="status -1"):  # a count mismatch
        r.update_vertices(c0[:-1].contiguous())
    before = frame(r, "fast")
    bad = c0.clone()
    bad[len(bad) // 2, 1, 2] = float("nan")
    with pytest.raises(dev.RtError, match="not finite"):
        r.update_vertices(bad)
    bad[len(bad) // 2, 1, 2] = float("inf")
    with pytest.raises(dev.RtError, match="not finite"):
        r.update_vertices(bad)
    with pytest.raises(dev.RtError, match="status -5"):  # (a refused update is no update)
        r.update_info()
    equal_frames(frame(r, "fast"), before, "after a refused update")
    equal_frames(frame(r, "strict"), before, "after a refused update, strict")
    r.close()


def test_launch_decisions_survive_an_update(dev, scenes):
    """a frame batch's default rule (three trial launches per candidate, then its choice) is decided per shape and
    upload: an update keeps the decision, a new upload would start the trials again"""
    import torch
    s = scenes["car_only"]
    r = dev.Renderer(0).upload(s)
    cams = [host.camera(W, H)] * 4
    rgb = torch.empty((4, H, W, 3), dtype=torch.float32, device="cuda")
    for _ in range(8):
        r.render_frames(cams, W, H, rgb=rgb)
        r.sync()
        if r.launch_info()["settled"]:
            break
    li = r.launch_info()
    assert li["settled"] == 1 and li["trial"] == 0, li
    before = rgb.cpu().numpy()
    coords = rigid(s)[0]
    update(r, coords)
    r.render_frames(cams, W, H, rgb=rgb)
    r.sync()
    lj = r.launch_info()
    assert lj["settled"] == 1 and lj["trial"] == 0 and lj["variant"] == li["variant"], (li, lj)
    fresh = dev.Renderer(0).upload(moved_scene(s, coords))
    want = frame(fresh, "strict")
    got = rgb.cpu().numpy()
    assert not same_bits(got, before)
    for f in range(4):
        assert same_bits(got[f], want["rgb"]), f
    r.close()
    fresh.close()


def test_update_lights(dev, scenes):
    s = scenes["car_boxed"]
    assert len(s.lights) >= 1
    lights = s.lights.copy()
    lights["pos"][0] += np.array([1.5, -2.0, 0.75], np.float32)
    lights["kl"][0] *= np.float32(0.5)
    r = dev.Renderer(0).upload(s)
    before = frame(r, "strict")
    r.update_lights(lights)
    s1 = host.Scene(s.triangles, lights)
    s1.nodes, s1.tri_idx, s1.amb = s.nodes, s.tri_idx, s.amb
    fresh = dev.Renderer(0).upload(s1)
    want = frame(fresh, "strict")
    assert not same_bits(want["rgb"], before["rgb"])
    for kernel in ("strict", "fast"):
        equal_frames(frame(r, kernel), want, kernel)
    with pytest.raises(dev.RtError, match="status -1"):
        r.update_lights(np.concatenate([lights, lights]))
    with pytest.raises(dev.RtError, match="status -1"):
        r.update_lights(lights[:0])
    equal_frames(frame(r, "fast"), want, "after refused light updates")
    fresh.close()
    # a new upload with more lights on the same context, then an update of those: the staging follows the scene
    more = np.concatenate([lights, s.lights, lights])
    more["pos"][1] += np.array([-3.0, 1.0, 0.5], np.float32)
    more["kl"] *= np.float32(0.4)
    s3 = host.Scene(s.triangles, more.copy())
    s3.nodes, s3.tri_idx, s3.amb = s.nodes, s.tri_idx, s.amb
    r.upload(s3)
    moved = more.copy()
    moved["pos"] += np.array([0.25, 0.5, -0.75], np.float32)
    r.update_lights(moved)
    s4 = host.Scene(s.triangles, moved)
    s4.nodes, s4.tri_idx, s4.amb = s.nodes, s.tri_idx, s.amb
    fresh = dev.Renderer(0).upload(s4)
    want = frame(fresh, "strict")
    for kernel in ("strict", "fast"):
        equal_frames(frame(r, kernel), want, "three lights " + kernel)
    r.close()
    fresh.close()


def test_update_info_after_a_refused_update(dev, scenes):
    """a refused update leaves the last good update's report, update_ms included, as it was"""
    import torch
    s = scenes["car_only"]
    r = dev.Renderer(0).upload(s)
    good = update(r, rigid(s)[0])
    assert 0 < good["update_ms"] < 1000
    bad = torch.from_numpy(np.ascontiguousarray(s.triangles["coords"])).cuda()
    bad[7, 0, 0] = float("nan")
    with pytest.raises(dev.RtError, match="not finite"):
        r.update_vertices(bad)
    assert r.update_info() == good
    r.close()
