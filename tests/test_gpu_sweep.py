"""Sweep queries (rt_sweep_spheres: Renderer.sweep / sweep_info) against tests/sweep_ref.py, the numpy float32
restatement of toi, which tests/test_sweep_abi.py holds against a float64 brute force on the CPU. An answer is a
triangle index, a time and a point with defined bits, so every comparison is array_equal / same_bits and no case is
excluded. Per scene the sweeps are 512 from sweep_ref.fixture_sweeps plus 128 of the 64 x 36 camera's primary rays with
radii from the fixture's set; the expectations are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import sweep_ref
from tests.sweep_ref import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
FMAX = sweep_ref.FMAX
KERNELS = ["strict", "fast"]
W, H = 64, 36
NS, NC = 512, 128
N = NS + NC
CHUNK = 256  # QUERY_CHUNK (rt_query.hpp)
# the negative float nearest zero and a negative subnormal near -1e-40, from their bits (a conversion from a Python float
# would flush them to -0 in a process whose flush-to-zero state a fast-math library has set)
NEG_TINY, NEG_SUB = np.array([0x80000001, 0x80011111], np.uint32).view(F)


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


def fixture_sweeps(coords, seed):
    from prt import rays
    c, d, r = sweep_ref.fixture_sweeps(coords, NS, seed)
    o, p = rays.pinhole(host.camera(W, H), W, H, device="cpu")
    rows = np.arange(NC) * ((W * H) // NC) + 7
    ext = sweep_ref.scene_extent(coords)
    rc = (ext * np.array([0.0, 1e-3, 1e-2, 5e-2])[np.arange(NC) % 4]).astype(F)
    return (np.concatenate([c, o.numpy()[rows]]), np.concatenate([d, p.numpy()[rows]]), np.concatenate([r, rc]))


def query(r, c, d, rad, kernel, t_max=None):
    """(tri, t, point, info)"""
    tri, t, point = r.sweep(cuda(c), cuda(d), cuda(rad), t_max=None if t_max is None else cuda(t_max), kernel=kernel)
    info = r.sweep_info()
    return tri.cpu().numpy(), t.cpu().numpy(), point.cpu().numpy(), info


def check(got, want, what=""):
    tri, t, point, info = got
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    bad = np.nonzero(t.view(np.int32) != want[1].view(np.int32))[0]
    assert len(bad) == 0, (what, bad[:8], t[bad[:8]], want[1][bad[:8]])
    assert same_bits(point, want[2]), what
    n = len(tri)
    assert info["spheres"] == n and info["stack_overflows"] == 0, (what, info)
    assert info["found"] == int((want[0] >= 0).sum()) and info["found"] + info["empty_spheres"] == n, (what, info)


def check_path(info, kernel, valid, n_tris, wide=True, outside=0):
    """which loop served the sweeps: the walk under "fast" on a scene with a wide view (but for the `outside` sweeps
    beyond its domain), else the exhaustive loop"""
    if kernel == "fast" and wide:
        assert info["walked_spheres"] == valid - outside and info["exhaustive_spheres"] == outside, info
        assert (info["nodes_visited"] > 0) == (valid > outside), info
    else:
        assert info["exhaustive_spheres"] == valid and info["walked_spheres"] == 0, info
        assert info["tris_tested"] == valid * n_tris and info["nodes_visited"] == 0, info


class Fix:
    """one fixture scene: a Renderer, the N sweeps and the yardstick's answers for them"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.c, self.d, self.rad = fixture_sweeps(self.coords, seed)
        self.want = sweep_ref.expected(self.c, self.d, self.rad, self.coords)
        self.mx = max(16.0, float(np.abs(self.coords).max()))  # the scene's coordinate magnitude (rt_hip.hip)

    def rows(self, rows):
        return tuple(x[rows] for x in self.want)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, 41 + k) for k, (name, s) in enumerate(scenes.items())}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture sweeps, both orders
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_sweeps(fix, scene, kernel):
    f = fix[scene]
    tri, t, point, ties = f.want
    found = tri >= 0
    print(f"{scene}: {int(found.sum())} of {N} found, {int((ties > 1).sum())} with an exact tie, "
          f"{int((t == 0).sum())} touching at the start")
    assert found.sum() >= N // 2 and (~found).sum() >= 16 and (ties > 1).sum() >= 8 and (t == 0).sum() >= 8
    assert (t[~found] == FMAX).all() and same_bits(point[~found], f.c[~found])
    p = np.random.default_rng(11).permutation(N)
    for order in (np.arange(N), p):
        got = query(f.r, f.c[order], f.d[order], f.rad[order], kernel)
        check(got, f.rows(order), what=(scene, kernel, order[0]))
        check_path(got[3], kernel, N, len(f.coords))


# ------------------------------------------------------------------ 2. ties take the lower index
def test_ties_take_the_lower_index(dev, scenes, fix):
    """the scene with every triangle twice: each contact ties with its copy, and the lower index answers"""
    s = scenes["car_only"]
    f = fix["car_only"]
    t = s.triangles
    twice = host.Scene(host.triangle_init(np.concatenate([f.coords, f.coords]), *(np.concatenate([t[k], t[k]])
                                                                                  for k in ("ks", "kd", "kr"))),
                       s.lights.copy())
    r = dev.Renderer(0).upload(twice.build_bvh(3))
    for kernel in KERNELS:
        got = query(r, f.c, f.d, f.rad, kernel)
        assert (got[0] < len(f.coords)).all(), kernel
        check(got, f.want, what=("twice", kernel))
    r.close()


# ------------------------------------------------------------------ 3. t_max
@pytest.mark.parametrize("kernel", KERNELS)
def test_t_max_at_and_below_the_answer(fix, kernel):
    f = fix["car_boxed"]
    at = f.want[1].copy()  # (FLT_MAX where nothing was found: no bound)
    got = query(f.r, f.c, f.d, f.rad, kernel, t_max=at)
    check(got, f.want, what=("at", kernel))
    below = np.nextafter(at, F(-1))  # (an answer at t = 0: a negative bound, the empty set)
    want = sweep_ref.expected(f.c, f.d, f.rad, f.coords, t_max=below)
    assert (want[0] == -1).all()  # (the answer is the set's least toi: one float below it the set is empty)
    check(query(f.r, f.c, f.d, f.rad, kernel, t_max=below), want, what=("below", kernel))
    with np.errstate(over="ignore"):
        later = np.fmin(at * F(1.5), FMAX)  # a bound past the answer: the same answer; half of it: nothing
    check(query(f.r, f.c, f.d, f.rad, kernel, t_max=later), f.want, what=("later", kernel))
    half = np.where(at > 0, at * F(0.5), F(-1))
    check(query(f.r, f.c, f.d, f.rad, kernel, t_max=half), want, what=("half", kernel))
    inf = np.full(N, np.inf, F)
    check(query(f.r, f.c, f.d, f.rad, kernel, t_max=inf), f.want, what=("inf", kernel))
    zero = np.zeros(N, F)
    want = sweep_ref.expected(f.c, f.d, f.rad, f.coords, t_max=zero)
    assert np.array_equal(want[0] >= 0, f.want[1] == 0)
    check(query(f.r, f.c, f.d, f.rad, kernel, t_max=zero), want, what=("zero", kernel))


# ------------------------------------------------------------------ 4. special inputs
def special_sweeps(f):
    """(c, d, r, t_max, kind): invalid sweeps, d = 0, a radius that covers the scene, sweeps outside the walk's domain
    (max|c| or r above 2^20 mx, a nonzero |d.k| outside [2^-64, 2^64]) and at its edges"""
    found = np.nonzero((f.want[0] >= 0) & (f.want[1] > 0) & (f.rad > 0) & (f.d != 0).all(axis=1))[0][:8]
    ext = F(sweep_ref.scene_extent(f.coords))
    v = f.coords.reshape(-1, 3)
    mid = ((v.min(0) + v.max(0)) / 2).astype(F)
    cmax = F(f.mx * 2.0 ** 20)
    c, d, r, tm, kind = [], [], [], [], []

    def add(ci, di, ri, ti, k):
        c.append(np.array(ci, F)), d.append(np.array(di, F)), r.append(F(ri)), tm.append(F(ti)), kind.append(k)
    for i in found:
        ci, di, ri = f.c[i], f.d[i], f.rad[i]
        for bad in (np.nan, np.inf, -np.inf):
            for k in range(3):
                x = ci.copy()
                x[k] = bad
                add(x, di, ri, np.inf, "invalid")
                x = di.copy()
                x[k] = bad
                add(ci, x, ri, np.inf, "invalid")
            add(ci, di, bad, np.inf, "invalid")
        add(ci, di, -ri, np.inf, "invalid")
        add(ci, di, NEG_TINY, np.inf, "invalid")
        add(ci, di, ri, np.nan, "invalid")
        add(ci, di, ri, -1.0, "invalid")
        add(ci, di, ri, NEG_TINY, "invalid")
        add(ci, di, ri, -0.0, "valid")  # (-0 is the bound 0)
        add(ci, di, ri, np.inf, "valid")
        hit = ci + di * f.want[1][i]
        add(hit, [0, 0, 0], ri, np.inf, "still")           # d = 0 at the contact: within rounding of touching
        add(hit, [0, 0, 0], ri * F(1.01), np.inf, "still")  # ... and touching
        add(ci, [0, 0, 0], F(0), np.inf, "still")
        add(ci, di, ext * F(10), np.inf, "huge")
        add(mid, [0, 0, 0], ext * F(10), np.inf, "huge")
        add(ci, di, FMAX, np.inf, "outside")                # r above 2^20 mx (finite: valid)
        add(ci, di, np.nextafter(cmax, F(np.inf)), np.inf, "outside")
        add(ci, di, cmax, np.inf, "edge")
        far = ci.copy()
        far[0] = np.nextafter(cmax, F(np.inf))
        add(far, (mid - far) * F(1.5), ri, np.inf, "outside")  # max|c| above 2^20 mx
        far[0] = -cmax
        add(far, (mid - far) * F(1.5), ri, np.inf, "edge")
        for k in range(3):
            for tiny, what in ((1e-30, "outside"), (NEG_SUB, "outside"), (np.nextafter(F(2.0 ** -64), F(0)), "outside"),
                               (2.0 ** -64, "edge"), (-2.0 ** 64, "edge")):
                x = di.copy()
                x[k] = tiny
                add(ci, x, ri, np.inf, what)
            x = di * F(2.0 ** 40)
            add(ci, x, ri, np.inf, "edge")
            x = di.copy()
            x[k] = np.nextafter(F(2.0 ** 64), F(np.inf)) * np.sign(di[k])
            add(ci, x, ri, np.inf, "outside")
    return np.array(c), np.array(d), np.array(r), np.array(tm), np.array(kind)


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_special_inputs(fix, scene):
    f = fix[scene]
    c, d, r, tm, kind = special_sweeps(f)
    want = sweep_ref.expected(c, d, r, f.coords, t_max=tm)
    inv = kind == "invalid"
    assert inv.sum() >= 100 and (want[0][inv] == -1).all() and (want[1][inv] == FMAX).all()
    assert same_bits(want[2][inv], c[inv])
    assert (want[0][kind == "valid"] >= 0).any() and (want[0][kind == "valid"] == -1).any()  # (the bound -0 is 0)
    assert (want[0][kind == "huge"] == 0).all() and (want[1][kind == "huge"] == 0).all()  # every triangle ties at 0
    assert (want[0][kind == "still"] >= 0).any() and (want[0][kind == "still"] == -1).any()
    assert (want[0][kind == "outside"] >= 0).sum() >= 16
    valid, outside = int((~inv).sum()), int((kind == "outside").sum())
    for kernel in KERNELS:
        got = query(f.r, c, d, r, kernel, t_max=tm)
        check(got, want, what=(scene, kernel))
        check_path(got[3], kernel, valid, len(f.coords), outside=outside)
        assert (got[0][inv] == -1).all() and (got[1][inv] == FMAX).all() and same_bits(got[2][inv], c[inv])


# ------------------------------------------------------------------ 5. sphere count edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_sphere_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    c, d, r = cuda(f.c[:CHUNK + 1]), cuda(f.d[:CHUNK + 1]), cuda(f.rad[:CHUNK + 1])
    for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK + 1):
        tri = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        t = torch.full((n + 3,), -77.0, dtype=torch.float32, device="cuda")
        point = torch.full((3 * n + 3,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the fills are torch's work; the query runs on the renderer's stream)
        f.r.sweep((c.data_ptr(), n), d.data_ptr(), r.data_ptr(), kernel=kernel, tri=tri.data_ptr(), t=t.data_ptr(),
                  point=point.data_ptr())  # (raw pointers: the buffers are longer)
        assert f.r.sweep_info()["spheres"] == n
        tri, t, point = tri.cpu().numpy(), t.cpu().numpy(), point.cpu().numpy()
        np.testing.assert_array_equal(tri[:n], f.want[0][:n], err_msg=str(n))
        assert same_bits(t[:n], f.want[1][:n]) and same_bits(point[:3 * n].reshape(n, 3), f.want[2][:n]), n
        assert (tri[n:] == -77).all() and (t[n:] == -77).all() and (point[3 * n:] == -77).all(), n
    # a scalar radius, and single outputs
    rows = np.nonzero(f.rad == f.rad[1])[0]
    tri, t, point = f.r.sweep(cuda(f.c[rows]), cuda(f.d[rows]), float(f.rad[1]), kernel=kernel)
    f.r.sync()
    np.testing.assert_array_equal(tri.cpu().numpy(), f.want[0][rows])
    assert same_bits(t.cpu().numpy(), f.want[1][rows]) and same_bits(point.cpu().numpy(), f.want[2][rows])


# ------------------------------------------------------------------ 6. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        got = query(r, f.c, f.d, f.rad, kernel)
        check(got, f.want, what=(accel, flags, kernel))
        check_path(got[3], kernel, N, len(f.coords), wide=accel != "reference")
    r.close()


# ------------------------------------------------------------------ 7. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_nearest.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="auto"), both kernels answer as the yardstick does on the moved coordinates (every
    second fixture sweep)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    c, d, rad = f.c[rows], f.d[rows], f.rad[rows]
    want = sweep_ref.expected(c, d, rad, coords)
    still = f.rows(rows)
    assert (want[0] != still[0]).sum() > 100 and (want[0] >= 0).sum() > 100
    r = dev.Renderer(0).upload(s)
    check(query(r, c, d, rad, "fast"), still, what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="auto")
        for kernel in KERNELS:
            got = query(r, c, d, rad, kernel)
            check(got, want, what=(step, kernel))
        assert got[3]["walked_spheres"] == len(rows)
    r.close()


# ------------------------------------------------------------------ 8. isolation
def test_a_sweep_query_leaves_renders_and_other_queries_alone(dev, scenes, fix):
    import torch
    from prt import rays
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    pts = cuda(f.coords[::97, 0])
    o, p = rays.pinhole(cam, W, H)
    c, d, rad = cuda(f.c), cuda(f.d), cuda(f.rad)
    lo, hi = (pts - 0.05).contiguous(), (pts + 0.05).contiguous()
    torch.cuda.synchronize()  # (these tensors are torch's work; the queries run on the renderer's stream)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def others(r):
        hit, t = r.trace_rays(o, p)
        near = r.nearest(pts)
        nb = r.nearest_tris(pts, k=4)
        ov = r.overlaps(lo, hi, k=4)
        hits = r.trace_hits(o, p, max_hits=2)
        r.sync()
        out = [x.cpu().numpy() for x in (hit, t, *near, *nb[:3], *ov, *hits)]
        infos = [r.query_info(), r.nearest_info(), r.neighbours_info(), r.overlaps_info(), r.hits_info()]
        return out, infos

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    bgra = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", bgra=bgra)
    r.sync()
    bgra0 = bgra.cpu().numpy().copy()
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    frame0, stats0, launch0 = r.download(hit=True), r.stats(), r.launch_info()
    out0, infos0 = others(r)
    for kernel in ("fast", "strict", "fast"):
        r.sweep(c, d, rad, kernel=kernel)
        si = r.sweep_info()
        assert si["spheres"] == N
    frame1 = r.download(hit=True)
    assert same_bits(frame0[0], frame1[0]) and np.array_equal(frame0[1], frame1[1]) and r.stats() == stats0
    assert np.array_equal(bgra.cpu().numpy(), bgra0) and r.launch_info() == launch0
    infos = [r.query_info(), r.nearest_info(), r.neighbours_info(), r.overlaps_info(), r.hits_info()]
    for a, b in zip(infos, infos0):  # the other queries' counters as they were
        assert strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4
    out1, infos1 = others(r)  # ... and the same queries again: the same bits
    for a, b in zip(out0, out1):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in zip(infos1, infos0):
        assert strip(a) == strip(b)
    r.render(cam, W, H, kernel="fast", bgra=bgra)
    r.sync()
    assert np.array_equal(bgra.cpu().numpy(), bgra0)
    r.render(cam, W, H, kernel="fast", hit=hit)
    assert r.sync() > 0
    frame2 = r.download(hit=True)
    assert same_bits(frame0[0], frame2[0]) and np.array_equal(frame0[1], frame2[1])
    sj = r.sweep_info()  # ... and none of them touched the sweep query's own counters
    assert strip(sj) == strip(si) and abs(sj["kernel_ms"] - si["kernel_ms"]) < 1e-4
    r.close()


# ------------------------------------------------------------------ 9. errors
def test_sweep_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    c, d, rad = cuda(f.c), cuda(f.d), cuda(f.rad)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.sweep(c, d, rad)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no sweep query run yet
        r.sweep_info()
    r.sweep(c[:100], d[:100], rad[:100])
    info = r.sweep_info()
    assert info["spheres"] == 100 and info["found"] == int((f.want[0][:100] >= 0).sum())
    with pytest.raises(dev.RtError, match="status -1"):
        r.sweep(c, d, rad, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.sweep((0, 16), d.data_ptr(), rad.data_ptr())  # null centre
    L = _lib.hip()
    tri = torch.empty(16, dtype=torch.int32, device="cuda")
    tt = torch.empty(16, dtype=torch.float32, device="cuda")
    pt = torch.empty(48, dtype=torch.float32, device="cuda")
    pc, pd, pr, t, u, p = c.data_ptr(), d.data_ptr(), rad.data_ptr(), tri.data_ptr(), tt.data_ptr(), pt.data_ptr()
    Q, R = _lib.Spheres, _lib.SweepResults
    for q, res in [
        (Q(None, pd, pr, None, 16, 0), R(t, u, p)),      # null centre, motion, radius
        (Q(pc, None, pr, None, 16, 0), R(t, u, p)),
        (Q(pc, pd, None, None, 16, 0), R(t, u, p)),
        (Q(pc, pd, pr, None, 16, 0), R(None, None, None)),  # all outputs NULL
        (Q(pc, pd, pr, None, 16, 3), R(t, u, p)),        # unknown kernel
        (Q(pc, pd, pr, None, 16, -1), R(t, u, p)),
        (Q(pc, pd, pr, None, -1, 0), R(t, u, p)),        # negative n
    ]:
        assert L.rt_sweep_spheres(r._ctx, ctypes.byref(q), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_sweep_spheres(r._ctx, None, None) == -1
    assert L.rt_sweep_spheres(r._ctx, ctypes.byref(Q(pc, pd, pr, None, 16, 0)), None) == -1
    after = r.sweep_info()  # a refused call leaves sweep_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # one output alone is enough
    for res in (R(t, None, None), R(None, u, None), R(None, None, p)):
        assert L.rt_sweep_spheres(r._ctx, ctypes.byref(Q(pc, pd, pr, None, 16, 0)), ctypes.byref(res)) == 0
    r.sync()
    assert np.array_equal(tri.cpu().numpy(), f.want[0][:16]) and same_bits(tt.cpu().numpy(), f.want[1][:16])
    assert same_bits(pt.cpu().numpy().reshape(16, 3), f.want[2][:16])
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_sweep_spheres(r._ctx, ctypes.byref(Q(None, None, None, None, 0, 0)),
                              ctypes.byref(R(None, None, None))) == 0
    assert r.sweep_info()["spheres"] == 0
    r.close()
