"""Nearest-surface queries (rt_nearest_points: Renderer.nearest / nearest_info) against tests/nearest_ref.py, the numpy
float32 restatement of D and P over every (point, triangle) pair, which tests/test_nearest_abi.py holds against a
float64 brute force on the CPU. A point's answer is the first triangle by (D, original index), so every comparison is
bit for bit (same_bits on d2 and point, array_equal on tri) and no case is excluded. The expectations are computed once
per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import nearest_ref
from tests.nearest_ref import same_bits
from tests.test_gpu_query import cam_rays

pytestmark = pytest.mark.gpu

FMAX = np.float32(3.402823466e+38)
KERNELS = ["strict", "fast"]
W, H = 64, 36
N = 1024


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


@pytest.fixture(scope="module")
def scenes():
    return {name: host.Scene.named(name).build_bvh(3) for name in ("car_boxed", "car_only")}


def cuda(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def nearest(r, pts, kernel, max_dist2=None):
    tri, d2, point = r.nearest(cuda(pts), kernel=kernel, max_dist2=None if max_dist2 is None else cuda(max_dist2))
    info = r.nearest_info()
    return tri.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy(), info


def check(got, want, what=""):
    tri, d2, point, info = got
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    assert same_bits(d2, want[1]), what
    assert same_bits(point, want[2]), what
    found = int((want[0] >= 0).sum())
    assert info["points"] == len(tri) and info["found"] == found and info["empty_points"] == len(tri) - found, (what, info)
    assert info["stack_overflows"] == 0


def scene_points(r, coords, seed):
    """1,024 points: 256 at triangle centroids with 0.02 noise, 256 exactly on vertices, 256 uniform in the scene's box
    grown by a quarter, 256 of the 64x36 camera's hit points"""
    rng = np.random.default_rng(seed)
    c = np.asarray(coords, np.float32)
    cen = c[rng.integers(0, len(c), 256)].astype(np.float64).mean(1) + rng.normal(0, 0.02, (256, 3))
    vert = c[rng.integers(0, len(c), 256), rng.integers(0, 3, 256)]
    lo, hi = c.reshape(-1, 3).min(0).astype(np.float64), c.reshape(-1, 3).max(0).astype(np.float64)
    g = (hi - lo) / 4
    uni = rng.random((256, 3)) * (hi - lo + 2 * g) + (lo - g)
    o, d = cam_rays(host.camera_array(host.camera(W, H)), W, H)
    h, t = r.trace_rays(cuda(o), cuda(d), kernel="fast")
    r.sync()
    h, t = h.cpu().numpy(), t.cpu().numpy()
    sel = np.flatnonzero(h >= 0)
    assert len(sel) >= 256
    sel = sel[np.linspace(0, len(sel) - 1, 256).astype(int)]
    hitp = o[sel] + d[sel] * t[sel, None]
    pts = np.concatenate([cen, vert, uni, hitp]).astype(np.float32)
    assert pts.shape == (N, 3) and np.isfinite(pts).all()
    return np.ascontiguousarray(pts)


class Fix:
    """one fixture scene: a Renderer, its 1,024 points and the mirror's expectation for them"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.pts = scene_points(self.r, self.coords, seed)
        self.tri, self.d2, self.point, self.ties = nearest_ref.expected(self.pts, self.coords, ties=True)
        self.want = (self.tri, self.d2, self.point)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, 3 + k) for k, (name, s) in enumerate(scenes.items())}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture points
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_points(fix, scene, kernel):
    f = fix[scene]
    assert (f.tri >= 0).all()
    assert int((f.ties >= 2).sum()) >= 100  # exact ties at the minimum: the index rule decides on ordinary input
    p = np.random.default_rng(11).permutation(N)
    for order in (np.arange(N), p):
        got = nearest(f.r, f.pts[order], kernel)
        check(got, tuple(x[order] for x in f.want), what=(scene, kernel, order[0]))
        info = got[3]
        if kernel == "fast":
            assert info["walked_points"] == N and info["exhaustive_points"] == 0, info
        else:
            assert info["exhaustive_points"] == N and info["walked_points"] == 0, info
            assert info["tris_tested"] == N * len(f.coords) and info["nodes_visited"] == 0, info


# ------------------------------------------------------------------ 2. ties take the lower index
def test_ties_take_the_lower_index(dev, fix):
    base = host.Scene.named("car_only")
    t = base.triangles
    n = len(t)
    f = fix["car_only"]
    pts = f.pts[::4]
    doubled = host.Scene(np.concatenate([t, t]), base.lights).build_bvh(3)
    mirrored = host.Scene(np.concatenate([t[::-1], t]), base.lights).build_bvh(3)
    for name, s in (("doubled", doubled), ("copy first, reversed", mirrored)):
        want = nearest_ref.expected(pts, s.triangles["coords"])
        r = dev.Renderer(0).upload(s)
        for kernel in KERNELS:
            got = nearest(r, pts, kernel)
            check(got, want, what=(name, kernel))
            assert same_bits(got[1], f.d2[::4])  # the single scene's bits
            if name == "doubled":
                assert (got[0] < n).all() and np.array_equal(got[0], f.tri[::4])
            else:  # triangle j is at 2n - 1 - j... and at n + j: the smaller of the two positions answers
                assert np.array_equal(got[0], want[0]) and (want[0] >= 0).all()
        r.close()


# ------------------------------------------------------------------ 3. bounds
@pytest.mark.parametrize("kernel", KERNELS)
def test_bounds(fix, kernel):
    f = fix["car_only"]
    n = N
    check(nearest(f.r, f.pts, kernel, None), f.want, what="NULL")
    k = np.arange(n) % 7
    on_vertex = (np.arange(n) >= 256) & (np.arange(n) < 512) & (f.d2 == 0)
    assert on_vertex.sum() > 200  # (fl(a + e1) is the vertex itself for most triangles)
    md = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5],
                   [np.float32(np.inf), f.d2, np.nextafter(f.d2, np.float32(-np.inf)), np.float32(0), np.float32(-1.0),
                    np.float32(np.nan)], np.float32(-0.0)).astype(np.float32)
    want = nearest_ref.expected(f.pts, f.coords, md)
    found = want[0] >= 0
    assert found[k == 0].all() and found[k == 1].all() and not found[k == 2].any()  # the bound is inclusive, to the bit
    assert np.array_equal(found[k == 3], f.d2[k == 3] == 0) and found[k == 3].any() and not found[k == 3].all()
    assert found[(k == 3) & on_vertex].all() and not found[k == 4].any() and not found[k == 5].any()
    assert np.array_equal(want[0][found], f.tri[found]) and same_bits(want[1][found], f.d2[found])
    got = nearest(f.r, f.pts, kernel, md)
    check(got, want, what="bounds")
    tri, d2, point, info = got
    assert (tri[~found] == -1).all() and (d2[~found] == FMAX).all() and same_bits(point[~found], f.pts[~found])
    assert info["found"] == int(found.sum()) and info["empty_points"] == int((~found).sum())
    # (from the bits, as tests/nearest_ref.py reads them; the float below D = 0 is negative: no walk either)
    valid = ~np.isnan(md) & ~(np.signbit(md) & ((md.view(np.int32) & 0x7FFFFFFF) != 0))
    assert not valid[(k == 4) | (k == 5)].any() and valid[k < 2].all()
    walked = info["walked_points"] if kernel == "fast" else info["exhaustive_points"]
    assert walked == int(valid.sum()), info


# ------------------------------------------------------------------ 4. non-finite and far points
def test_non_finite_and_far_points(fix):
    f = fix["car_boxed"]
    pts = f.pts[:140].copy()
    special = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, -3e38]
    for i, v in enumerate(special):
        for a in range(3):
            pts[20 * i + 3 * a, a] = v          # one component
        pts[20 * i + 10] = v                     # all three
    finite = np.isfinite(pts).all(1)
    want = nearest_ref.expected(pts, f.coords)
    assert (want[0][~finite] == -1).all() and same_bits(want[2][~finite], pts[~finite])
    far = finite & (np.abs(pts).max(1) >= 1e30)
    assert far.sum() >= 16 and (want[0][far] == -1).all()  # D overflows: the empty set
    gs, gf = nearest(f.r, pts, "strict"), nearest(f.r, pts, "fast")
    check(gs, want, "strict")
    check(gf, want, "fast")
    for a, b in zip(gs[:3], gf[:3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    nf = int(finite.sum())
    assert gf[3]["walked_points"] == nf and gf[3]["exhaustive_points"] == 0
    assert gs[3]["exhaustive_points"] == nf and gs[3]["walked_points"] == 0
    assert gf[3]["empty_points"] == int((want[0] < 0).sum()) >= len(pts) - nf


# ------------------------------------------------------------------ 5. degenerate triangles
def test_degenerate_triangles(dev):
    """the three degenerate kinds beside ordinary triangles; each degenerate triangle is moved to a place of its own,
    since the reference's bvh_build (build_bvh) does not terminate on triangles that share a centroid"""
    from tests.test_nearest_abi import degenerate_triangles
    rng = np.random.default_rng(21)
    deg = degenerate_triangles()
    deg = deg + (np.arange(len(deg), dtype=np.float32) * 0.75)[:, None, None] * np.array([1, -1, 0.5], np.float32)
    base = rng.uniform(-3, 7, (40, 1, 3))
    plain = (base + rng.normal(0, 0.4, (40, 3, 3))).astype(np.float32)
    far_deg = np.array([[[20, 20, 20]] * 3, [[-9, 12, 3], [-9, 12, 3], [-8, 12, 3]]], np.float32)
    coords = np.concatenate([plain[:20], deg, plain[20:], far_deg])
    tris = np.zeros(len(coords), host.TRI_DTYPE)
    tris["coords"] = coords
    tris["centroid"] = coords.mean(1)
    tris["kd"] = 0.5
    tris["norm"][:, 0] = [0, 0, 1]
    tris["norm"][:, 1] = [0, 0, -1]
    s = host.Scene(tris, np.zeros(0, host.LIGHT_DTYPE)).build_bvh(3)
    pts = np.concatenate([rng.uniform(-4, 8, (150, 3)), deg.reshape(-1, 3), deg.mean(1),
                          deg.mean(1) + rng.normal(0, 0.05, (len(deg), 3)),
                          far_deg.mean(1) + rng.normal(0, 0.5, (2, 3))]).astype(np.float32)
    want = nearest_ref.expected(pts, coords)
    is_deg = np.zeros(len(coords), bool)
    is_deg[20:20 + len(deg)] = True
    is_deg[-2:] = True
    assert is_deg[want[0]].sum() >= 10 and (~is_deg[want[0]]).sum() >= 10  # a degenerate member is the nearest, too
    assert np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    r = dev.Renderer(0).upload(s)
    for kernel in KERNELS:
        check(nearest(r, pts, kernel), want, what=kernel)
    r.close()


# ------------------------------------------------------------------ 6. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        got = nearest(r, f.pts, kernel)
        check(got, f.want, what=(accel, flags, kernel))
    info = got[3]  # (the fast kernel's)
    if accel == "reference":  # no wide view: the exhaustive loop
        assert info["exhaustive_points"] == N and info["walked_points"] == 0
    else:
        assert info["walked_points"] == N and info["exhaustive_points"] == 0
    r.close()


# ------------------------------------------------------------------ 7. the walk prunes
def test_the_walk_prunes(fix):
    f = fix["car_boxed"]
    info = nearest(f.r, f.pts, "fast")[3]
    wide = f.r.scene_info()["wide_nodes"]
    print(f"car_boxed, {N} points: tris_tested {info['tris_tested']} ({info['tris_tested'] / N:.1f} per point of "
          f"{len(f.coords)}), nodes_visited {info['nodes_visited']} ({info['nodes_visited'] / N:.1f} per point of {wide})")
    assert 0 < info["tris_tested"] < N * len(f.coords) / 4
    assert 0 < info["nodes_visited"] < N * wide
    assert info["stack_overflows"] == 0


# ------------------------------------------------------------------ 8. count edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_point_count_edges(fix, kernel):
    import torch
    from prt import _lib
    f = fix["car_boxed"]
    dp = cuda(f.pts[:257])
    for n in (0, 1, 63, 64, 65, 257):
        tri = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        d2 = torch.full((n + 3,), -77.0, dtype=torch.float32, device="cuda")
        point = torch.full((n + 3, 3), -77.0, dtype=torch.float32, device="cuda")
        f.r.nearest(dp[:n], kernel=kernel, tri=tri, d2=d2, point=point)
        assert f.r.nearest_info()["points"] == n
        tri, d2, point = tri.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy()
        np.testing.assert_array_equal(tri[:n], f.tri[:n], err_msg=str(n))
        assert same_bits(d2[:n], f.d2[:n]) and same_bits(point[:n], f.point[:n]), n
        assert (tri[n:] == -77).all() and (d2[n:] == -77.0).all() and (point[n:] == -77.0).all(), n
    # each single output left out in turn
    L = _lib.hip()
    n = 65
    for skip in range(3):
        tri = torch.full((n,), -77, dtype=torch.int32, device="cuda")
        d2 = torch.full((n,), -77.0, dtype=torch.float32, device="cuda")
        point = torch.full((n, 3), -77.0, dtype=torch.float32, device="cuda")
        ptrs = [tri.data_ptr(), d2.data_ptr(), point.data_ptr()]
        ptrs[skip] = None
        q = _lib.Points(dp.data_ptr(), None, n, dev_kernel(kernel))
        assert L.rt_nearest_points(f.r._ctx, ctypes.byref(q), ctypes.byref(_lib.NearestResults(*ptrs))) == 0
        assert f.r.nearest_info()["points"] == n
        tri, d2, point = tri.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy()
        assert (tri == -77).all() if skip == 0 else np.array_equal(tri, f.tri[:n])
        assert (d2 == -77.0).all() if skip == 1 else same_bits(d2, f.d2[:n])
        assert (point == -77.0).all() if skip == 2 else same_bits(point, f.point[:n])


def dev_kernel(name):
    return {"auto": 0, "strict": 1, "fast": 2}[name]


# ------------------------------------------------------------------ 9. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_hits.py's car_boxed scaled by 1.3 and sheared: after update_vertices, and again after
    rebuild_views(mode="device"), both kernels answer for the new coordinates"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    want = nearest_ref.expected(f.pts, coords)
    assert (want[0] != f.tri).sum() > 100 and not same_bits(want[1], f.d2)
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            got = nearest(r, f.pts, kernel)
            check(got, want, what=(step, kernel))
        assert got[3]["walked_points"] == N
    r.close()


# ------------------------------------------------------------------ 10. isolation
def test_a_nearest_query_leaves_every_other_state_alone(dev, scenes, fix):
    import torch
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    o, d = cam_rays(host.camera_array(cam), W, H)
    do, dd, dp = cuda(o), cuda(d), cuda(f.pts)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def state(r):
        li = r.launch_info()
        return r.download(hit=True), r.stats(), li

    def others(r):
        r.trace_rays(do[:300], dd[:300])
        r.shade_rays(do[:200], dd[:200])
        r.trace_hits(do[:250], dd[:250], max_hits=4)
        return r.query_info(), r.shade_info(), r.hits_info()

    def run(query):
        r = dev.Renderer(0).upload(scenes["car_boxed"])
        hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
        r.render(cam, W, H, kernel="fast", hit=hit)
        r.sync()
        infos = others(r)
        if query:
            before, times = state(r), r.kernel_times(8)
            for kernel in ("fast", "strict"):
                r.nearest(dp[:512], kernel=kernel)
                ni = r.nearest_info()
                assert ni["points"] == 512
            after = state(r)
            assert same_bits(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
            assert before[1:] == after[1:] and r.kernel_times(8) == times and r.sync() == r.sync()
            again = r.query_info(), r.shade_info(), r.hits_info()
            for a, b in zip(infos, again):
                assert strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4
            others(r)
        r.render(cam, W, H, kernel="fast", hit=hit)
        ms = r.sync()
        if query:  # ... and their calls leave nearest_info as it was
            nj = r.nearest_info()
            assert strip(nj) == strip(ni) and abs(nj["kernel_ms"] - ni["kernel_ms"]) < 1e-4
        out = state(r), len(r.kernel_times(8)), ms > 0
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_bits(a[0][0][0], b[0][0][0]) and np.array_equal(a[0][0][1], b[0][0][1])
    assert a[0][1:] == b[0][1:] and a[1:] == b[1:]


# ------------------------------------------------------------------ 11. errors
def test_nearest_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    dp = cuda(f.pts)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.nearest(dp)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no nearest query run yet
        r.nearest_info()
    r.nearest(dp[:100])
    info = r.nearest_info()
    assert info["points"] == 100
    with pytest.raises(dev.RtError, match="status -1"):
        r.nearest(dp, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.nearest((0, 16))  # null point
    L = _lib.hip()
    tri = torch.empty(16, dtype=torch.int32, device="cuda")
    p, t = dp.data_ptr(), tri.data_ptr()
    for pts, res in [
        (_lib.Points(None, None, 16, 0), _lib.NearestResults(t, None, None)),   # null point
        (_lib.Points(p, None, 16, 0), _lib.NearestResults(None, None, None)),   # all three outputs null
        (_lib.Points(p, None, 16, 3), _lib.NearestResults(t, None, None)),      # unknown kernel
        (_lib.Points(p, None, 16, -1), _lib.NearestResults(t, None, None)),
        (_lib.Points(p, None, -1, 0), _lib.NearestResults(t, None, None)),      # negative n
    ]:
        assert L.rt_nearest_points(r._ctx, ctypes.byref(pts), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_nearest_points(r._ctx, None, None) == -1
    assert L.rt_nearest_points(r._ctx, ctypes.byref(_lib.Points(p, None, 16, 0)), None) == -1
    after = r.nearest_info()  # a refused call leaves nearest_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_nearest_points(r._ctx, ctypes.byref(_lib.Points(None, None, 0, 0)),
                               ctypes.byref(_lib.NearestResults(None, None, None))) == 0
    assert r.nearest_info()["points"] == 0
    r.close()
