"""Multi-hit queries (rt_trace_hits: Renderer.trace_hits / hits_info) against tests/hits_ref.py, the numpy float32
restatement of the reference's hit_triangle over every (ray, triangle) pair, which tests/test_hits_abi.py pins to the
reference binary's fixtures on the CPU. A ray's answer is its whole hit set ordered by (t, original triangle index), so
every comparison is bit for bit and no tie rule is imitated. The expected lists are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import hits_ref
from tests.test_gpu_query import cam_rays, domain_sets, grid_cameras, same_bits

pytestmark = pytest.mark.gpu

FMAX = np.float32(3.402823466e+38)
KERNELS = ["strict", "fast"]
W, H = 64, 36


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


def hits(r, o, d, max_hits, kernel, t_max=None, count_all=False):
    tri, t, count = r.trace_hits(cuda(o), cuda(d), max_hits=max_hits, kernel=kernel, count_all=count_all,
                                 t_max=None if t_max is None else cuda(t_max))
    info = r.hits_info()
    return tri.cpu().numpy(), t.cpu().numpy(), count.cpu().numpy(), info


def check(got, lists, max_hits, count_all=False, what=""):
    tri, t, count, info = got
    wtri, wt, wcount, wtotal = hits_ref.expected(lists, max_hits)
    np.testing.assert_array_equal(tri, wtri, err_msg=str(what))
    assert same_bits(t, wt), what
    np.testing.assert_array_equal(count, wtotal if count_all else wcount, err_msg=str(what))
    assert info["rays"] == len(lists) and info["rays_hit"] == int((wtotal > 0).sum()), (what, info)
    assert info["hits_stored"] == int(wcount.sum()), (what, info)
    assert info["hits_counted"] == int((wtotal if count_all else wcount).sum()), (what, info)
    assert info["stack_overflows"] == 0


class Fix:
    """one fixture scene: its 64x36 camera rays, their expected lists, a Renderer"""

    def __init__(self, dev, scene):
        self.o, self.d = cam_rays(host.camera_array(host.camera(W, H)), W, H)
        self.lists = hits_ref.hit_lists(self.o, self.d, scene.triangles["coords"])
        self.total = np.array([len(i) for i, _ in self.lists])
        self.r = dev.Renderer(0).upload(scene)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s) for name, s in scenes.items()}
    yield out
    for f in out.values():
        f.r.close()


@pytest.fixture(scope="module")
def grids(dev, scenes):
    """the eight 16x16 cameras of test_gpu_query.grid_cameras on car_boxed and their expected lists"""
    cams = grid_cameras(scenes["car_boxed"])
    o, d = (np.concatenate(x) for x in zip(*[cam_rays(c, 16, 16) for c in cams]))
    out = {"o": o, "d": d, "lists": hits_ref.hit_lists(o, d, scenes["car_boxed"].triangles["coords"])}
    assert sum(len(i) > 0 for i, _ in out["lists"]) > 1000
    return out


# ------------------------------------------------------------------ 1. fixture camera rays
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_camera_rays(fix, scene, kernel):
    f = fix[scene]
    assert 8 < f.total.max() <= 16 and (f.total > 8).sum() >= 12  # max_hits = 8 truncates, 16 does not
    p = np.random.default_rng(11).permutation(W * H)
    for K in (1, 4, 8, 16):
        for order in (np.arange(W * H), p):
            got = hits(f.r, f.o[order], f.d[order], K, kernel)
            check(got, [f.lists[i] for i in order], K, what=(K, order[0]))
            info = got[3]
            if kernel == "fast":
                assert info["unit_rays"] + info["short_rays"] + info["full_rays"] + info["exhaustive_rays"] == W * H
                assert info["exhaustive_rays"] == 0
            else:
                assert info["exhaustive_rays"] == W * H
        assert (got[2] == np.minimum(f.total[p], K)).all()
    assert (hits_ref.expected(f.lists, 8)[2] < f.total).any() and (hits_ref.expected(f.lists, 16)[2] == f.total).all()
    for K in (0, 4):
        got = hits(f.r, f.o, f.d, K, kernel, count_all=True)
        check(got, f.lists, K, count_all=True, what=("count_all", K))
        assert got[0].shape == (W * H, K)


def test_a_view_holds_each_triangle_once(fix):
    """the list never sees a triangle twice: every wide view's position -> original index map is injective"""
    for f in fix.values():
        for view in ("full", "unit", "primary"):
            _, orig = f.r._debug_wide(view)
            if orig is not None:
                assert len(np.unique(orig)) == len(orig), view


# ------------------------------------------------------------------ 2. relation to the closest query
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_first_hit_is_the_closest_query(fix, scene):
    f = fix[scene]
    h, t = f.r.trace_rays(cuda(f.o), cuda(f.d), kernel="fast")
    f.r.sync()
    h, t = h.cpu().numpy(), t.cpu().numpy()
    tri, tt, count, _ = hits(f.r, f.o, f.d, 2, "fast")
    assert same_bits(tt[:, 0], t)
    tie = (count == 2) & (tt[:, 0] == tt[:, 1])
    np.testing.assert_array_equal(tri[~tie, 0], h[~tie])
    for r in np.flatnonzero(tie):
        i, ts = f.lists[r]
        assert h[r] in i[ts == tt[r, 0]]


# ------------------------------------------------------------------ 3. t_max
@pytest.mark.parametrize("kernel", KERNELS)
def test_t_max(fix, kernel):
    f = fix["car_boxed"]
    n = W * H
    two = f.total >= 2
    assert two.sum() > 500
    t0 = np.array([ts[0] if len(ts) > 0 else 1.0 for _, ts in f.lists], np.float32)
    t1 = np.array([ts[1] if len(ts) > 1 else 2.0 for _, ts in f.lists], np.float32)
    special = np.array([np.inf, FMAX, 0.0, -1.0, np.nan, -np.inf, -0.0], np.float32)[np.arange(n) % 7]
    bounds = {
        "second hit included": t1,
        "the float below it": np.nextafter(t1, np.float32(0)),
        "halfway": ((t0.astype(np.float64) + t1.astype(np.float64)) / 2).astype(np.float32),
        "specials": special,
    }
    for name, b in bounds.items():
        want = hits_ref.bounded(f.lists, b)
        for K, count_all in ((4, False), (1, False), (0, True), (2, True)):
            check(hits(f.r, f.o, f.d, K, kernel, t_max=b, count_all=count_all), want, K, count_all, what=(name, K))
    wc = np.array([len(i) for i, _ in hits_ref.bounded(f.lists, t1)])
    wb = np.array([len(i) for i, _ in hits_ref.bounded(f.lists, bounds["the float below it"])])
    assert (wc[two] >= 2).all() and (wb[two] < wc[two]).all()  # the bound is inclusive, to the bit
    ws = np.array([len(i) for i, _ in hits_ref.bounded(f.lists, special)])
    assert (ws[np.arange(n) % 7 >= 2] == 0).all() and (ws[np.arange(n) % 7 < 2] == f.total[np.arange(n) % 7 < 2]).all()


# ------------------------------------------------------------------ 4. ties at the bound
def test_ties_at_the_bound(dev):
    """car_only with every triangle twice (test_exact_ties_are_rewalked's scene): every hit comes as a pair (j, j + n)
    with equal t, the lower index first; max_hits = 3 cuts a pair at the bound"""
    base = host.Scene.named("car_only")
    n = len(base.triangles)
    s = host.Scene(np.concatenate([base.triangles, base.triangles]), base.lights).build_bvh(3)
    w, h = 96, 54
    o, d = cam_rays(host.camera_array(host.camera(w, h)), w, h)
    single = hits_ref.hit_lists(o, d, base.triangles["coords"])
    lists = []
    for i, t in single:  # the doubled scene's list: the same t for j and j + n, by the same operations
        i2, t2 = np.concatenate([i, i + n]).astype(np.int32), np.concatenate([t, t])
        k = np.lexsort((i2, t2))
        lists.append((i2[k], t2[k]))
    plain = np.array([len(t) > 0 and len(np.unique(t)) == len(t) for _, t in single])  # (no tie within car_only itself)
    assert plain.sum() > 1000
    r = dev.Renderer(0).upload(s)
    for K in (1, 2, 3, 4):
        gs = hits(r, o, d, K, "strict")
        gf = hits(r, o, d, K, "fast")
        check(gs, lists, K, what=("strict", K))
        check(gf, lists, K, what=("fast", K))
        tri, t = gf[0][plain], gf[1][plain]
        assert (tri[:, 0] < n).all()
        if K >= 2:
            assert (tri[:, 1] == tri[:, 0] + n).all() and same_bits(t[:, 0], t[:, 1])
        if K == 3:
            deep = gf[2][plain] == 3
            assert deep.sum() > 100 and (tri[deep, 2] < n).all()  # the pair's lower index; its twin is cut off
    r.close()


# ------------------------------------------------------------------ 5. views
def test_each_ray_walks_a_view_its_length_allows(dev):
    """test_gpu_query.test_each_ray_walks_a_view_its_length_allows' two triangles and six direction lengths: B (the
    sliver, |n| = 1e-4) is culled while |det| = 1e-4 L < EPSILON, so the lists are [A] for the short rays and [B, A]
    for L = 20 and 1000"""
    tris = np.zeros(2, host.TRI_DTYPE)
    tris["coords"][0] = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    tris["coords"][1] = [[1, 1, 1], [1.01, 1, 1], [1, 1.01, 1]]
    tris["centroid"] = tris["coords"].mean(1)
    tris["kd"] = 0.5
    tris["norm"][:, 0] = [0, 0, 1]
    tris["norm"][:, 1] = [0, 0, -1]
    s = host.Scene(tris, np.zeros(0, host.LIGHT_DTYPE)).build_bvh(3)
    L = np.array([1, 2.5, 3.5, 20, 1000, 0.9999], np.float64)
    u = np.array([1e-3, -5e-4, -1.0])
    u /= np.linalg.norm(u)
    d = (u[None, :] * L[:, None]).astype(np.float32)
    o = np.tile(np.array([1.004, 1.003, 3], np.float32), (len(L), 1))
    lists = hits_ref.hit_lists(o, d, tris["coords"])
    assert [list(i) for i, _ in lists] == [[0], [0], [0], [1, 0], [1, 0], [0]]
    r = dev.Renderer(0).upload(s)
    check(hits(r, o, d, 4, "strict"), lists, 4)
    got = hits(r, o, d, 4, "fast")
    check(got, lists, 4)
    info = got[3]
    assert info["unit_rays"] >= 1 and info["short_rays"] >= 1 and info["full_rays"] >= 1, info
    r.close()


# ------------------------------------------------------------------ 6. camera grids
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_camera_grids_on_every_acceleration_structure(dev, scenes, grids, accel, flags):
    """inside and outside the box, |d| ~ 4, the degenerate rows and columns, the origin-on-a-face camera (whose
    zero-component rays the reference's BVH walk loses and brute force finds)"""
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        got = hits(r, grids["o"], grids["d"], 8, kernel)
        check(got, grids["lists"], 8, what=(accel, flags, kernel))
    info = got[3]
    n = len(grids["o"])
    assert info["unit_rays"] + info["short_rays"] + info["full_rays"] + info["exhaustive_rays"] == n
    zero = int((grids["d"] == 0).any(1).sum())
    assert zero > 0
    if accel == "reference":  # no wide view: zero-component rays run the exhaustive loop (rt_hits.hpp)
        assert info["exhaustive_rays"] == zero and info["full_rays"] == n - zero
    else:  # they stay on the wide walk
        assert info["exhaustive_rays"] == 0 and info["short_rays"] > 0 and info["full_rays"] > 0
    r.close()


# ------------------------------------------------------------------ 7. domain
def test_rays_outside_the_fast_domain_run_the_exhaustive_loop(fix, scenes, grids):
    r = fix["car_boxed"].r
    mx = max(16.0, float(np.abs(scenes["car_boxed"].triangles["coords"]).max()))
    seen_out = 0
    for name, (o, d, leaves) in domain_sets(grids).items():
        with np.errstate(invalid="ignore"):
            dm, om = np.abs(d).max(1), np.abs(o).max(1)
            inside = (np.isfinite(o).all(1) & np.isfinite(d).all(1) & (dm >= np.float32(2.0 ** -20))
                      & (dm <= np.float32(2.0 ** 20)) & (om <= np.float32(4 * mx)))
        assert (not inside.all()) == leaves, name
        for K, count_all in ((8, False), (0, True)):
            gs = hits(r, o, d, K, "strict", count_all=count_all)
            gf = hits(r, o, d, K, "fast", count_all=count_all)
            np.testing.assert_array_equal(gf[0], gs[0], err_msg=name)
            assert same_bits(gf[1], gs[1]), name
            np.testing.assert_array_equal(gf[2], gs[2], err_msg=name)
            assert gf[3]["exhaustive_rays"] == int((~inside).sum()), (name, gf[3])
            assert gf[3]["stack_overflows"] == 0 and gs[3]["exhaustive_rays"] == len(o)
        seen_out += int((~inside).sum())
    assert seen_out > 1000


# ------------------------------------------------------------------ 8. count edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_ray_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    sel = np.flatnonzero(f.total > 0)[:257]  # rays that hit, so that a wrong slot shows
    o, d, lists = f.o[sel], f.d[sel], [f.lists[i] for i in sel]
    do, dd = cuda(o), cuda(d)
    K = 5
    for n in (0, 1, 63, 64, 65, 257):
        tri = torch.full((n + 3, K), -77, dtype=torch.int32, device="cuda")
        t = torch.full((n + 3, K), -77.0, dtype=torch.float32, device="cuda")
        count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        f.r.trace_hits(do[:n], dd[:n], max_hits=K, kernel=kernel, tri=tri, t=t, count=count)
        info = f.r.hits_info()
        assert info["rays"] == n
        tri, t, count = tri.cpu().numpy(), t.cpu().numpy(), count.cpu().numpy()
        wtri, wt, wcount, _ = hits_ref.expected(lists[:n], K)
        np.testing.assert_array_equal(tri[:n], wtri, err_msg=str(n))
        assert same_bits(t[:n], wt), n
        np.testing.assert_array_equal(count[:n], wcount)
        assert (tri[n:] == -77).all() and (t[n:] == -77.0).all() and (count[n:] == -77).all(), n
        unused = np.arange(K)[None, :] >= wcount[:, None]
        assert (tri[:n][unused] == -1).all() and (t[:n][unused] == FMAX).all()
    assert unused.any() and not unused.all()


# ------------------------------------------------------------------ 9. moving scene
def test_moving_scene(dev, scenes, fix):
    """car_boxed scaled by 1.3 and sheared: after update_vertices, and again after rebuild_views(mode="device"), the
    query answers for the new coordinates"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    lists = hits_ref.hit_lists(f.o, f.d, coords)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(lists, f.lists))
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            check(hits(r, f.o, f.d, 8, kernel), lists, 8, what=(step, kernel))
        check(hits(r, f.o, f.d, 0, "fast", count_all=True), lists, 0, True, what=(step, "count"))
    r.close()


# ------------------------------------------------------------------ 10. isolation
def test_a_hits_query_leaves_every_other_state_alone(dev, scenes, fix):
    import torch
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    do, dd = cuda(f.o), cuda(f.d)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def state(r):
        li = r.launch_info()
        return r.download(hit=True), r.stats(), li

    def run(query):
        r = dev.Renderer(0).upload(scenes["car_boxed"])
        hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
        r.render(cam, W, H, kernel="fast", hit=hit)
        r.sync()
        r.trace_rays(do[:300], dd[:300])
        r.shade_rays(do[:200], dd[:200])
        qi, si = r.query_info(), r.shade_info()
        if query:
            before, times = state(r), r.kernel_times(8)
            for kernel, K, count_all in (("fast", 8, False), ("strict", 16, False), ("fast", 0, True)):
                r.trace_hits(do, dd, max_hits=K, kernel=kernel, count_all=count_all)
                assert r.hits_info()["rays"] == len(do)
            after = state(r)
            assert same_bits(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
            assert before[1:] == after[1:] and r.kernel_times(8) == times and r.sync() == r.sync()
            qj, sj = r.query_info(), r.shade_info()
            assert strip(qj) == strip(qi) and strip(sj) == strip(si)
            assert abs(qj["kernel_ms"] - qi["kernel_ms"]) < 1e-4 and abs(sj["kernel_ms"] - si["kernel_ms"]) < 1e-4
        r.render(cam, W, H, kernel="fast", hit=hit)
        ms = r.sync()
        out = state(r), len(r.kernel_times(8)), ms > 0
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_bits(a[0][0][0], b[0][0][0]) and np.array_equal(a[0][0][1], b[0][0][1])
    assert a[0][1:] == b[0][1:] and a[1:] == b[1:]


# ------------------------------------------------------------------ handled overflow
def test_stack_overflow_fails_hits_info(dev, scenes):
    """test_gpu_query.test_stack_overflow_fails_query_info's 41-triangle, 40-level handed-over tree: the binary fast
    walk's 34-entry stack overflows, which the kernel counts (the library's own error flag, not a device fault) and
    hits_info reports as RT_E_KERNEL (-8); the exhaustive kernel walks no tree and answers"""
    base = scenes["car_only"]
    n = 41
    s = host.Scene(np.ascontiguousarray(base.triangles[:n]), base.lights)
    nodes = [None]
    big = ((-1e4, -1e4, -1e4), (1e4, 1e4, 1e4))
    cur, leaf = 0, 0
    for level in range(n - 1):
        c = len(nodes)
        nodes += [None, (big[0], big[1], 1, leaf)]
        leaf += 1
        nodes[cur] = (big[0], big[1], 0, c)
        if level == n - 2:
            nodes[c] = (big[0], big[1], 1, leaf)
            leaf += 1
        cur = c
    s.nodes = np.array(nodes, dtype=host.NODE_DTYPE)
    s.tri_idx = np.arange(n, dtype=np.int32)
    o, d = cam_rays(host.camera_array(host.camera(16, 16)), 16, 16)
    r = dev.Renderer(0).upload(s, accel="reference")
    r.trace_hits(cuda(o), cuda(d), max_hits=4, kernel="fast")
    with pytest.raises(dev.RtError, match="-8"):
        r.hits_info()
    check(hits(r, o, d, 4, "strict"), hits_ref.hit_lists(o, d, s.triangles["coords"]), 4)
    r.close()


# ------------------------------------------------------------------ 11. errors
def test_hits_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    do, dd = cuda(f.o), cuda(f.d)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.trace_hits(do, dd)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no hits query traced yet
        r.hits_info()
    r.trace_hits(do[:100], dd[:100], max_hits=3)
    info = r.hits_info()
    assert info["rays"] == 100
    with pytest.raises(dev.RtError, match="status -1"):
        r.trace_hits(do, dd, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.trace_hits((0, 16), dd.data_ptr())  # null origin
    L = _lib.hip()
    tri = torch.empty((16, 16), dtype=torch.int32, device="cuda")
    cnt = torch.empty(16, dtype=torch.int32, device="cuda")
    o, d, p = do.data_ptr(), dd.data_ptr(), tri.data_ptr()
    for rays, res in [
        (_lib.Hits(o, None, None, 16, 4, 0, 0), _lib.HitResults(p, None, None)),      # null dir
        (_lib.Hits(o, d, None, 16, -1, 0, 0), _lib.HitResults(p, None, None)),        # max_hits below 0
        (_lib.Hits(o, d, None, 16, 17, 0, 0), _lib.HitResults(p, None, None)),        # ... above RT_HITS_MAX
        (_lib.Hits(o, d, None, 16, 4, 0, 0), _lib.HitResults(None, None, cnt.data_ptr())),  # tri and t both null
        (_lib.Hits(o, d, None, 16, 0, 0, 0), _lib.HitResults(None, None, cnt.data_ptr())),  # max_hits 0, no count_all
        (_lib.Hits(o, d, None, 16, 0, 1, 0), _lib.HitResults(p, None, None)),         # counting without a count pointer
        (_lib.Hits(o, d, None, 16, 4, 2, 0), _lib.HitResults(p, None, None)),         # count_all not 0 / 1
        (_lib.Hits(o, d, None, 16, 4, 0, 3), _lib.HitResults(p, None, None)),         # unknown kernel
        (_lib.Hits(o, d, None, -1, 4, 0, 0), _lib.HitResults(p, None, None)),         # negative n
    ]:
        assert L.rt_trace_hits(r._ctx, ctypes.byref(rays), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_trace_hits(r._ctx, None, None) == -1
    after = r.hits_info()  # a refused call leaves hits_info() as it was (the event pair's time to its last digits)
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # either output alone is allowed
    only_t = _lib.HitResults(None, torch.empty((16, 4), dtype=torch.float32, device="cuda").data_ptr(), None)
    assert L.rt_trace_hits(r._ctx, ctypes.byref(_lib.Hits(o, d, None, 16, 4, 0, 0)), ctypes.byref(only_t)) == 0
    assert r.hits_info()["rays"] == 16
    r.close()
