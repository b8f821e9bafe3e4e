"""Neighbour queries (rt_nearest_tris: Renderer.nearest_tris / neighbours_info) against tests/neighbours_ref.py, the
stable sort of tests/nearest_ref.py's D over every (point, triangle) pair, which tests/test_neighbours_abi.py holds
against a float64 brute force on the CPU. A point's answer is the first k triangles by (D, original index) and a count,
so every comparison is bit for bit (same_bits on d2 and point, array_equal on tri and count) and no case is excluded.
The expectations are computed once per module (one table per point set, neighbours_ref.table)."""
import ctypes
import itertools

import numpy as np
import pytest

from prt import host
from tests import neighbours_ref
from tests.nearest_ref import same_bits
from tests.test_gpu_nearest import scene_points
from tests.test_gpu_query import cam_rays

pytestmark = pytest.mark.gpu

FMAX = np.float32(3.402823466e+38)
KERNELS = ["strict", "fast"]
KERNEL_ID = {"auto": 0, "strict": 1, "fast": 2}
W, H = 64, 36
N = 1024
CHUNK = 256  # QUERY_CHUNK (rt_query.hpp)
RADIUS2 = np.float32(1e-3)


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


def query(r, pts, k, kernel, max_dist2=None, count_all=False):
    """(tri, d2, point, count, info), in the yardstick's order"""
    tri, d2, count, point = r.nearest_tris(cuda(pts), k=k, kernel=kernel, count_all=count_all, points_out=True,
                                           max_dist2=None if max_dist2 is None else cuda(max_dist2))
    info = r.neighbours_info()
    return tri.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy(), count.cpu().numpy(), info


def check(got, want, what=""):
    tri, d2, point, count, info = got
    np.testing.assert_array_equal(count, want[3], err_msg=str(what))
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    assert same_bits(d2, want[1]), what
    assert same_bits(point, want[2]), what
    assert info["points"] == len(tri) and info["stack_overflows"] == 0, (what, info)
    assert info["tris_stored"] == int((want[0] >= 0).sum()) and info["tris_counted"] == int(want[3].sum()), (what, info)
    assert info["found"] + info["empty_points"] == len(tri), (what, info)
    if tri.shape[1] > 0:
        assert info["found"] == int((want[0][:, 0] >= 0).sum()), (what, info)


class Fix:
    """one fixture scene: a Renderer, test_gpu_nearest.scene_points' 1,024 points and the yardstick's table for them"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.pts = scene_points(self.r, self.coords, seed)
        self.tab = neighbours_ref.table(self.pts, self.coords)

    def want(self, k, **kw):
        return neighbours_ref.answer(self.tab, k, **kw)


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
    p = np.random.default_rng(11).permutation(N)
    for k in (1, 4, 8, 16):
        *_, size, cut = f.want(k, stats=True)
        assert (size == len(f.coords)).all()
        if k > 1:  # exact ties across the cut: the index rule decides which of the tied triangles is kept
            print(f"{scene}: k = {k}: {int(cut.sum())} points tie across the cut")
            assert int(cut.sum()) >= 100
        for order in (np.arange(N), p):
            got = query(f.r, f.pts[order], k, kernel)
            check(got, f.want(k, rows=order), what=(scene, kernel, k, order[0]))
            info = got[4]
            assert info["found"] == N and info["tris_stored"] == N * k
            if kernel == "fast":
                assert info["walked_points"] == N and info["exhaustive_points"] == 0, info
                assert 0 < info["tris_tested"] and 0 < info["nodes_visited"]
            else:
                assert info["exhaustive_points"] == N and info["walked_points"] == 0, info
                assert info["tris_tested"] == N * len(f.coords) and info["nodes_visited"] == 0, info


# ------------------------------------------------------------------ 2. k = 1 is Renderer.nearest
def per_point_bounds(d2):
    """the kinds of bound tests/test_gpu_nearest.py::test_bounds mixes, around each point's own nearest D"""
    j = np.arange(len(d2)) % 7
    return np.select([j == 0, j == 1, j == 2, j == 3, j == 4, j == 5],
                     [np.float32(np.inf), d2, np.nextafter(d2, np.float32(-np.inf)), np.float32(0), np.float32(-1.0),
                      np.float32(np.nan)], np.float32(-0.0)).astype(np.float32)


@pytest.mark.parametrize("kernel", KERNELS)
def test_k1_equals_nearest(fix, kernel):
    f = fix["car_only"]
    dp = cuda(f.pts)
    base = f.want(1)
    for md in (None, per_point_bounds(base[1][:, 0])):
        dm = None if md is None else cuda(md)
        near = f.r.nearest(dp, max_dist2=dm, kernel=kernel)
        assert f.r.nearest_info()["points"] == N  # (synchronises)
        ntri, nd2, npoint = (x.cpu().numpy() for x in near)
        tri, d2, point, count, info = query(f.r, f.pts, 1, kernel, md)
        assert np.array_equal(tri[:, 0], ntri) and same_bits(d2[:, 0], nd2) and same_bits(point[:, 0], npoint)
        assert np.array_equal(count, (ntri >= 0).astype(np.int32))
        check((tri, d2, point, count, info), f.want(1, max_dist2=md), what=(kernel, md is None))
    assert 100 < int((ntri >= 0).sum()) < N - 100  # (the bounded round found some and refused some)


# ------------------------------------------------------------------ 3. radius
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_radius(fix, scene, kernel):
    """every triangle within sqrt(1e-3) of each point: the lists, the capped count, the full count and the pure count.
    The counts are exact in every arm: a triangle offered twice, or a slot pruned under count_all, shows here."""
    f = fix[scene]
    md = np.full(N, RADIUS2, np.float32)
    size = f.want(16, max_dist2=md, stats=True)[4]
    regimes = int((size == 0).sum()), int(((size >= 1) & (size <= 16)).sum()), int((size > 16).sum())
    print(f"{scene}: |S_i| = 0: {regimes[0]}, 1..16: {regimes[1]}, > 16: {regimes[2]} points; max {int(size.max())}")
    assert min(regimes) >= 100
    for k, count_all in ((16, False), (16, True), (0, True)):
        want = f.want(k, max_dist2=md, count_all=count_all)
        assert np.array_equal(want[3], size if count_all else np.minimum(size, 16))
        got = query(f.r, f.pts, k, kernel, md, count_all)
        check(got, want, what=(scene, kernel, k, count_all))
        info = got[4]
        assert info["found"] == int((size > 0).sum()) and info["empty_points"] == int((size == 0).sum()), info
        assert info["tris_counted"] == int(size.sum() if count_all else np.minimum(size, 16).sum())


# ------------------------------------------------------------------ 4. mixed bounds, non-finite and far points
def test_mixed_bounds(fix):
    f = fix["car_boxed"]
    n = 64
    pts = f.pts[256:256 + n].copy()  # (on vertices: D = 0 is common)
    j = np.arange(n) % 8
    md = np.select([j == 0, j == 1, j == 2, j == 3, j == 4, j == 5, j == 6],
                   [np.float32(np.nan), np.float32(-1.0), np.float32(-0.0), np.float32(0), np.float32(1e-42), RADIUS2,
                    np.float32(np.inf)], FMAX).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for i, v in enumerate(special):  # (a stride of 5 meets a different kind of bound every time)
        pts[24 + 5 * i, i % 3] = v    # one component
        pts[26 + 5 * i] = v           # all three
    finite = np.isfinite(pts).all(1)
    far = finite & (np.abs(pts).max(1) >= 1e30)
    assert (~finite).sum() >= 6 and far.sum() >= 4
    tab = neighbours_ref.table(pts, f.coords)
    for k, count_all in ((8, False), (8, True), (0, True)):
        want = neighbours_ref.answer(tab, k, md, count_all, stats=True)
        size = want[4]
        empty = ~finite | far | (j == 0) | (j == 1)  # where §3p says so: the whole row empty, count 0
        assert (size[empty] == 0).all() and (want[3][empty] == 0).all() and (want[0][empty] == -1).all()
        assert (size[(j >= 6) & ~empty] == len(f.coords)).all()  # +inf and FLT_MAX: no bound
        for kind in (2, 3, 4):  # -0.0, 0 and a subnormal are valid bounds: the triangles of the vertex the point is on
            assert (size[(j == kind) & ~empty] > 0).any(), kind
        assert ((size[(j == 5) & ~empty] > 0) & (size[(j == 5) & ~empty] < len(f.coords))).all()
        for kernel in KERNELS:
            got = query(f.r, pts, k, kernel, md, count_all)
            check(got, want, what=(kernel, k, count_all))
            if k:
                assert same_bits(got[2][empty], np.repeat(pts[:, None], k, 1)[empty])  # q's own bits, NaN included
            valid = finite & ~(j == 0) & ~(j == 1)
            walked = got[4]["walked_points"] if kernel == "fast" else got[4]["exhaustive_points"]
            assert walked == int(valid.sum()), got[4]


# ------------------------------------------------------------------ 5. ties across the cut by construction
def test_ties_across_the_cut_by_construction(dev, fix):
    """car_only twice over, as test_gpu_nearest.py::test_ties_take_the_lower_index builds it: every entry has an exact
    twin, and of two equal D the lower index comes first"""
    base = host.Scene.named("car_only")
    t = base.triangles
    n = len(t)
    f = fix["car_only"]
    pts = f.pts[::4]
    single = f.want(2, rows=np.arange(0, N, 4))
    doubled = host.Scene(np.concatenate([t, t]), base.lights).build_bvh(3)
    mirrored = host.Scene(np.concatenate([t[::-1], t]), base.lights).build_bvh(3)
    for name, s in (("doubled", doubled), ("copy first, reversed", mirrored)):
        want = neighbours_ref.expected(pts, s.triangles["coords"], 4)
        tri = want[0]
        assert (tri >= 0).all() and (want[1][:, 0] == want[1][:, 1]).all() and (want[1][:, 2] == want[1][:, 3]).all()
        assert (np.diff(tri.astype(np.int64), axis=1)[want[1][:, :-1] == want[1][:, 1:]] > 0).all()  # lower index first
        assert same_bits(want[1][:, ::2], single[1])  # the single scene's two nearest D, each twice
        if name == "doubled":  # (where the single scene's nearest two tie, both come before either twin)
            alone = single[1][:, 0] != single[1][:, 1]
            assert alone.sum() >= 50 and (~alone).sum() >= 50
            assert np.array_equal(tri[:, 0], single[0][:, 0]) and np.array_equal(tri[alone, 1], single[0][alone, 0] + n)
            assert np.array_equal(tri[~alone, :2], single[0][~alone])
        r = dev.Renderer(0).upload(s)
        for kernel in KERNELS:
            check(query(r, pts, 4, kernel), want, what=(name, kernel))
        r.close()


# ------------------------------------------------------------------ 6. degenerate triangles
def test_degenerate_triangles(dev):
    """tests/test_gpu_nearest.py::test_degenerate_triangles' scene: zero-area and repeated-vertex triangles beside
    ordinary ones, each degenerate one at a place of its own; they appear in the lists with the stated (clamped) P"""
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
    tab = neighbours_ref.table(pts, coords)
    is_deg = np.zeros(len(coords), bool)
    is_deg[20:20 + len(deg)] = True
    is_deg[-2:] = True
    r = dev.Renderer(0).upload(s)
    for k, md, count_all in ((8, None, False), (16, None, False), (16, np.full(len(pts), 4.0, np.float32), True)):
        want = neighbours_ref.answer(tab, k, md, count_all)
        listed = want[0][want[0] >= 0]
        assert is_deg[listed].sum() >= 100 and (~is_deg[listed]).sum() >= 100
        assert np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
        for kernel in KERNELS:
            check(query(r, pts, k, kernel, md, count_all), want, what=(kernel, k))
    r.close()


# ------------------------------------------------------------------ 7. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    f = fix["car_boxed"]
    md = np.full(N, RADIUS2, np.float32)
    want = f.want(8, max_dist2=md)
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        got = query(r, f.pts, 8, kernel, md)
        check(got, want, what=(accel, flags, kernel))
        info = got[4]
        if accel == "reference" or kernel == "strict":  # no wide view: the exhaustive loop under either kernel
            assert info["exhaustive_points"] == N and info["walked_points"] == 0, info
            assert info["tris_tested"] == N * len(f.coords) and info["nodes_visited"] == 0, info
        else:
            assert info["walked_points"] == N and info["exhaustive_points"] == 0, info
    r.close()


# ------------------------------------------------------------------ 8. the walk prunes
def test_the_walk_prunes(fix):
    """k = 16, unbounded, car_boxed: measured on an MI355X, the 1,024 points test 115.7 triangles per point of 45,999
    and decode 45.4 nodes per point of 5,070 (k = 1: 20.5 and 11.4); the bound is
    test_gpu_nearest.py::test_the_walk_prunes' quarter"""
    f = fix["car_boxed"]
    info = query(f.r, f.pts, 16, "fast")[4]
    wide = f.r.scene_info()["wide_nodes"]
    print(f"car_boxed, {N} points, k = 16: tris_tested {info['tris_tested']} ({info['tris_tested'] / N:.1f} per point "
          f"of {len(f.coords)}), nodes_visited {info['nodes_visited']} ({info['nodes_visited'] / N:.1f} per point of "
          f"{wide})")
    assert 0 < info["tris_tested"] < N * len(f.coords) / 4
    assert 0 < info["nodes_visited"] < N * wide
    assert info["stack_overflows"] == 0


# ------------------------------------------------------------------ 9. count edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_point_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    dp = cuda(f.pts[:CHUNK + 1])
    for k in (4, 16):
        want = f.want(k)
        for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK + 1):
            tri = torch.full((n * k + 3,), -77, dtype=torch.int32, device="cuda")
            d2 = torch.full((n * k + 3,), -77.0, dtype=torch.float32, device="cuda")
            point = torch.full((n * k + 3, 3), -77.0, dtype=torch.float32, device="cuda")
            count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
            f.r.nearest_tris((dp.data_ptr(), n), k=k, kernel=kernel, tri=tri.data_ptr(), d2=d2.data_ptr(),
                             point=point.data_ptr(), count=count.data_ptr())  # (raw pointers: the buffers are longer)
            assert f.r.neighbours_info()["points"] == n
            tri, d2, point, count = tri.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy(), count.cpu().numpy()
            np.testing.assert_array_equal(tri[:n * k].reshape(n, k), want[0][:n], err_msg=str(n))
            assert same_bits(d2[:n * k].reshape(n, k), want[1][:n]), n
            assert same_bits(point[:n * k].reshape(n, k, 3), want[2][:n]), n
            assert np.array_equal(count[:n], want[3][:n]), n
            assert (tri[n * k:] == -77).all() and (d2[n * k:] == -77.0).all() and (point[n * k:] == -77.0).all(), n
            assert (count[n:] == -77).all(), n


# ------------------------------------------------------------------ 10. nullable outputs
@pytest.mark.parametrize("kernel", KERNELS)
def test_nullable_outputs(fix, kernel):
    """every non-empty subset of the four pointers: the ones present get the same bits, the absent ones are not
    touched. count alone stores nothing at max_tris > 0 and is refused there (rt_hip.h); it is the pure count's form"""
    import torch
    from prt import _lib
    L = _lib.hip()
    f = fix["car_boxed"]
    n, k = 65, 8
    dp = cuda(f.pts[:n])
    md = cuda(np.full(n, RADIUS2, np.float32))
    want = neighbours_ref.answer(f.tab, k, np.full(n, RADIUS2, np.float32), True, rows=np.arange(n))
    assert (want[3] > k).any() and (want[3] == 0).any()
    for present in itertools.product((False, True), repeat=4):
        if not any(present):
            continue
        tri = torch.full((n, k), -77, dtype=torch.int32, device="cuda")
        d2 = torch.full((n, k), -77.0, dtype=torch.float32, device="cuda")
        point = torch.full((n, k, 3), -77.0, dtype=torch.float32, device="cuda")
        count = torch.full((n,), -77, dtype=torch.int32, device="cuda")
        ptrs = [x.data_ptr() if p else None for x, p in zip((tri, d2, point, count), present)]
        res = _lib.NeighbourResults(*ptrs)
        count_only = present == (False, False, False, True)
        q = _lib.Neighbours(dp.data_ptr(), md.data_ptr(), n, k, 1, KERNEL_ID[kernel])
        rc = L.rt_nearest_tris(f.r._ctx, ctypes.byref(q), ctypes.byref(res))
        if count_only:
            assert rc == -1
            q = _lib.Neighbours(dp.data_ptr(), md.data_ptr(), n, 0, 1, KERNEL_ID[kernel])
            rc = L.rt_nearest_tris(f.r._ctx, ctypes.byref(q), ctypes.byref(res))
        assert rc == 0, present
        assert f.r.neighbours_info()["points"] == n
        tri, d2, point, count = tri.cpu().numpy(), d2.cpu().numpy(), point.cpu().numpy(), count.cpu().numpy()
        assert np.array_equal(tri, want[0]) if present[0] else (tri == -77).all(), present
        assert same_bits(d2, want[1]) if present[1] else (d2 == -77.0).all(), present
        assert same_bits(point, want[2]) if present[2] else (point == -77.0).all(), present
        assert np.array_equal(count, want[3]) if present[3] else (count == -77).all(), present


# ------------------------------------------------------------------ 11. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_nearest.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="device"), both kernels answer for the new coordinates (every second fixture
    point; the first query builds the point output's index map before the motion, the later ones reuse it)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    pts = f.pts[rows]
    md = np.full(len(pts), 64 * RADIUS2, np.float32)  # (the moved car is 1.3 times the size: a radius of 0.25)
    want = neighbours_ref.expected(pts, coords, 8, md, count_all=True)
    still = f.want(8, max_dist2=md, count_all=True, rows=rows)
    assert (want[3] != still[3]).sum() > 100 and (want[3] > 8).sum() > 50 and (want[3] == 0).sum() > 50
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    check(query(r, pts, 8, "fast", md, True), still, what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            got = query(r, pts, 8, kernel, md, True)
            check(got, want, what=(step, kernel))
        assert got[4]["walked_points"] == len(pts)
    r.close()


# ------------------------------------------------------------------ 12. isolation
def test_a_neighbours_query_leaves_every_other_state_alone(dev, scenes, fix):
    import torch
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    o, d = cam_rays(host.camera_array(cam), W, H)
    do, dd, dp = cuda(o), cuda(d), cuda(f.pts)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def state(r):
        return r.download(hit=True), r.stats(), r.launch_info()

    def others(r):
        """a ray query, a shade query, a hits query and a nearest query: their results and their infos"""
        out = [r.trace_rays(do[:300], dd[:300]), (r.shade_rays(do[:200], dd[:200]),),
               r.trace_hits(do[:250], dd[:250], max_hits=4), r.nearest(dp[:300])]
        infos = r.query_info(), r.shade_info(), r.hits_info(), r.nearest_info()
        return [x.cpu().numpy() for group in out for x in group], infos

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    res0, infos0 = others(r)
    before, times = state(r), r.kernel_times(8)
    for kernel, k, count_all in (("fast", 16, False), ("strict", 4, True), ("fast", 0, True)):
        r.nearest_tris(dp[:512], k=k, kernel=kernel, count_all=count_all, points_out=True,
                       max_dist2=cuda(np.full(512, RADIUS2, np.float32)))
        ni = r.neighbours_info()
        assert ni["points"] == 512
    after = state(r)
    assert same_bits(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]
    # (two readings of one event pair were seen to differ by 1 ns: the times are compared as the infos' kernel_ms are)
    reread = r.kernel_times(8)
    assert len(reread) == len(times) and all(abs(a - b) < 1e-4 for a, b in zip(reread, times))
    assert abs(r.sync() - r.sync()) < 1e-4
    again = r.query_info(), r.shade_info(), r.hits_info(), r.nearest_info()
    for a, b in zip(infos0, again):
        assert strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4
    res1, infos1 = others(r)  # ... the same queries again: the same bits, the same counters
    for a, b in zip(res0, res1):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in zip(infos0, infos1):
        assert strip(a) == strip(b)
    r.render(cam, W, H, kernel="fast", hit=hit)
    assert r.sync() > 0
    final = state(r)
    assert same_bits(before[0][0], final[0][0]) and np.array_equal(before[0][1], final[0][1])
    nj = r.neighbours_info()  # ... and their calls leave neighbours_info as it was
    assert strip(nj) == strip(ni) and abs(nj["kernel_ms"] - ni["kernel_ms"]) < 1e-4
    r.close()


# ------------------------------------------------------------------ 13. errors
def test_neighbours_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    dp = cuda(f.pts)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.nearest_tris(dp)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no neighbours query run yet
        r.neighbours_info()
    r.nearest_tris(dp[:100], k=4)
    info = r.neighbours_info()
    assert info["points"] == 100 and info["tris_stored"] == 400
    with pytest.raises(dev.RtError, match="status -1"):
        r.nearest_tris(dp, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.nearest_tris((0, 16))  # null point
    L = _lib.hip()
    tri = torch.empty(16 * 16, dtype=torch.int32, device="cuda")
    cnt = torch.empty(16, dtype=torch.int32, device="cuda")
    p, t, c = dp.data_ptr(), tri.data_ptr(), cnt.data_ptr()
    Q, R = _lib.Neighbours, _lib.NeighbourResults
    for q, res in [
        (Q(None, None, 16, 4, 0, 0), R(t, None, None, c)),      # null point
        (Q(p, None, 16, -1, 0, 0), R(t, None, None, c)),        # max_tris outside 0..16
        (Q(p, None, 16, 17, 0, 0), R(t, None, None, c)),
        (Q(p, None, 16, 4, 0, 0), R(None, None, None, c)),      # max_tris > 0 with tri, d2 and point all null
        (Q(p, None, 16, 4, 0, 0), R(None, None, None, None)),
        (Q(p, None, 16, 0, 0, 0), R(t, None, None, c)),         # max_tris = 0 without count_all ...
        (Q(p, None, 16, 0, 1, 0), R(t, None, None, None)),      # ... or without a count pointer
        (Q(p, None, 16, 4, 2, 0), R(t, None, None, c)),         # count_all not 0 / 1
        (Q(p, None, 16, 4, -1, 0), R(t, None, None, c)),
        (Q(p, None, 16, 4, 0, 3), R(t, None, None, c)),         # unknown kernel
        (Q(p, None, 16, 4, 0, -1), R(t, None, None, c)),
        (Q(p, None, -1, 4, 0, 0), R(t, None, None, c)),         # negative n
    ]:
        assert L.rt_nearest_tris(r._ctx, ctypes.byref(q), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_nearest_tris(r._ctx, None, None) == -1
    assert L.rt_nearest_tris(r._ctx, ctypes.byref(Q(p, None, 16, 4, 0, 0)), None) == -1
    after = r.neighbours_info()  # a refused call leaves neighbours_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_nearest_tris(r._ctx, ctypes.byref(Q(None, None, 0, 4, 0, 0)), ctypes.byref(R(None, None, None, None))) == 0
    assert r.neighbours_info()["points"] == 0
    r.close()
