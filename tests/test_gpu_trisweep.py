"""Triangle sweep queries (rt_sweep_triangles: Renderer.sweep_tris / trisweep_info) against tests/trisweep_ref.py, the
numpy float32 restatement of toi, which tests/test_trisweep_abi.py holds against geometry in float64 on the CPU. An
answer is a triangle index, a time, a point and a kind with defined bits, so every comparison is array_equal /
same_bits and no case is excluded. Per scene the queries are trisweep_ref.fixture's 512 seeded and 128 camera
triangles; the expectations are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import trisweep_ref as tr
from tests.trisweep_ref import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
FMAX = tr.FMAX
KERNELS = ["strict", "fast"]
N = tr.NS + tr.NC
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


def query(r, q, d, kernel, t_max=None):
    """(tri, t, point, kind, info)"""
    import torch
    kind = torch.empty(len(q), dtype=torch.int32, device="cuda")
    tri, t, point = r.sweep_tris(cuda(q), cuda(d), t_max=None if t_max is None else cuda(t_max), kernel=kernel,
                                 kind=kind)
    info = r.trisweep_info()
    return tri.cpu().numpy(), t.cpu().numpy(), point.cpu().numpy(), kind.cpu().numpy(), info


def check(got, want, what=""):
    tri, t, point, kind, info = got
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    bad = np.nonzero(t.view(np.int32) != want[1].view(np.int32))[0]
    assert len(bad) == 0, (what, bad[:8], t[bad[:8]], want[1][bad[:8]])
    assert same_bits(point, want[2]), what
    np.testing.assert_array_equal(kind, want[3], err_msg=str(what))
    n = len(tri)
    assert info["triangles"] == n and info["stack_overflows"] == 0, (what, info)
    assert info["found"] == int((want[0] >= 0).sum()) and info["found"] + info["empty"] == n, (what, info)


def check_path(info, kernel, valid, n_tris, wide=True, outside=0):
    """which loop served the queries: the walk under "fast" on a scene with a wide view (but for the `outside` queries
    beyond its domain), else the exhaustive loop"""
    if kernel == "fast" and wide:
        assert info["walked"] == valid - outside and info["exhaustive"] == outside, info
        assert (info["nodes_visited"] > 0) == (valid > outside), info
        if outside == 0:
            assert info["pairs_tested"] < valid * n_tris, info
    else:
        assert info["exhaustive"] == valid and info["walked"] == 0, info
        assert info["pairs_tested"] == valid * n_tris and info["nodes_visited"] == 0 and info["pairs_gated"] == 0, info


class Fix:
    """one fixture scene: a Renderer, the N queries and the yardstick's answers for them"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.q, self.d = tr.fixture(self.coords, seed)
        self.want = tr.expected(self.q, self.d, self.coords)
        self.mx = max(16.0, float(np.abs(self.coords).max()))  # the scene's coordinate magnitude (rt_hip.hip)

    def rows(self, rows):
        return tuple(x[rows] for x in self.want)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, tr.SEED[name]) for name, s in scenes.items()}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture queries, both orders
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_queries(fix, scene, kernel):
    f = fix[scene]
    print(scene, tr.check_fixture(f.want))
    tri, t, point, kind, ties = f.want
    none = tri < 0
    assert (t[none] == FMAX).all() and same_bits(point[none], f.q[none, 0]) and (kind[none] == -1).all()
    p = np.random.default_rng(11).permutation(N)
    for order in (np.arange(N), p):
        got = query(f.r, f.q[order], f.d[order], kernel)
        check(got, f.rows(order), what=(scene, kernel, order[0]))
        check_path(got[4], kernel, N, len(f.coords))


# ------------------------------------------------------------------ 2. ties take the lower index
def tie_queries(coords, n, seed):
    """queries that meet a shared mesh edge or corner head on, from the mesh's own coordinates: the corner v of a
    random triangle (even rows) or the midpoint of its first edge (odd rows) is met by the middle of a query edge that
    crosses it, coming down the triangle's normal from 5 % of the extent away at t = 1/2"""
    rng = np.random.default_rng(seed)
    c = np.asarray(coords, np.float64)
    ext = tr.scene_extent(coords)
    t = c[rng.integers(0, len(c), n)]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ok = np.linalg.norm(nrm, axis=1) > 0
    t, nrm = t[ok], nrm[ok]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    e = t[:, 1] - t[:, 0]
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    x = np.cross(nrm, e)  # across the first edge, in the triangle's plane
    at = np.where((np.arange(len(t)) % 2 == 0)[:, None], t[:, 0], 0.5 * (t[:, 0] + t[:, 1]))
    s = 0.01 * ext
    start = at + 0.05 * ext * nrm
    q = np.stack([start - s * x, start + s * x, start + s * nrm], axis=1)
    d = np.broadcast_to(-0.1 * ext * nrm, (len(t), 3))
    return np.ascontiguousarray(q.astype(F)), np.ascontiguousarray(d.astype(F))


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_ties_take_the_lower_index(fix, scene):
    f = fix[scene]
    q, d = tie_queries(f.coords, 128, 5)
    want = tr.expected(q, d, f.coords)
    tied = want[4] > 1
    print(f"{scene}: {int(tied.sum())} of {len(q)} head-on queries end in an exact tie")
    assert tied.sum() >= 16
    # the answer is the lowest index among the triangles that share its toi
    qi, ti, toi, _, _ = tr.pairs(q, d, f.coords)
    for i in np.flatnonzero(tied)[:32]:
        same = ti[(qi == i) & (toi.view(np.int32) == want[1][i].view(np.int32))]
        assert len(same) == want[4][i] and want[0][i] == same.min()
    for kernel in KERNELS:
        check(query(f.r, q, d, kernel), want, what=(scene, kernel))


def test_a_doubled_scene_answers_with_the_first_copy(dev, scenes, fix):
    """the scene with every triangle twice: each contact ties with its copy, and the lower index answers"""
    s = scenes["car_only"]
    f = fix["car_only"]
    t = s.triangles
    twice = host.Scene(host.triangle_init(np.concatenate([f.coords, f.coords]), *(np.concatenate([t[k], t[k]])
                                                                                  for k in ("ks", "kd", "kr"))),
                       s.lights.copy())
    r = dev.Renderer(0).upload(twice.build_bvh(3))
    rows = np.arange(0, N, 2)
    for kernel in KERNELS:
        got = query(r, f.q[rows], f.d[rows], kernel)
        assert (got[0] < len(f.coords)).all(), kernel
        check(got, f.rows(rows), what=("twice", kernel))
    r.close()


# ------------------------------------------------------------------ 3. t_max
@pytest.mark.parametrize("kernel", KERNELS)
def test_t_max_at_and_below_the_answer(fix, kernel):
    f = fix["car_boxed"]
    at = f.want[1].copy()  # (FLT_MAX where nothing was found: no bound)
    check(query(f.r, f.q, f.d, kernel, t_max=at), f.want, what=("at", kernel))
    below = np.nextafter(at, F(-1))  # (an answer at t = 0: a negative bound, the empty set)
    want = tr.expected(f.q, f.d, f.coords, t_max=below)
    assert (want[0] == -1).all()  # (the answer is the set's least toi: one float below it the set is empty)
    check(query(f.r, f.q, f.d, kernel, t_max=below), want, what=("below", kernel))
    zero = np.zeros(N, F)
    want = tr.expected(f.q, f.d, f.coords, t_max=zero)
    assert np.array_equal(want[0] >= 0, f.want[1] == 0) and (want[0] >= 0).sum() >= 8
    check(query(f.r, f.q, f.d, kernel, t_max=zero), want, what=("zero", kernel))
    check(query(f.r, f.q, f.d, kernel, t_max=np.full(N, np.inf, F)), f.want, what=("inf", kernel))
    mixed = np.array([np.nan, -1.0, NEG_TINY, NEG_SUB, -0.0, np.inf, 0.5, 1e-3], F)[np.arange(N) % 8]
    want = tr.expected(f.q, f.d, f.coords, t_max=mixed)
    assert (want[0][np.arange(N) % 8 < 4] == -1).all() and (want[0][np.arange(N) % 8 == 5] >= 0).any()
    check(query(f.r, f.q, f.d, kernel, t_max=mixed), want, what=("mixed", kernel))


# ------------------------------------------------------------------ 4. special inputs
def special_queries(f):
    """(q, d, t_max, kind): invalid queries, d = 0, a zero component of d with the box test on that axis passing and
    failing, zero-area queries, queries outside the walk's domain and at its edges"""
    found = np.nonzero((f.want[0] >= 0) & (f.want[1] > 0) & (f.d != 0).all(axis=1))[0][:8]
    cmax = F(f.mx * 2.0 ** 20)
    rec = tr.records(f.coords)
    q, d, tm, kind = [], [], [], []

    def add(qi, di, ti, k):
        q.append(np.array(qi, F)), d.append(np.array(di, F)), tm.append(F(ti)), kind.append(k)
    for i in found:
        qi, di, toi, j = f.q[i], f.d[i], f.want[1][i], f.want[0][i]
        for bad in (np.nan, np.inf, -np.inf):
            for k in range(9):
                x = qi.copy()
                x.reshape(-1)[k] = bad
                add(x, di, np.inf, "invalid")
            for k in range(3):
                x = di.copy()
                x[k] = bad
                add(qi, x, np.inf, "invalid")
        add(qi, di, np.nan, "invalid")
        add(qi, di, NEG_SUB, "invalid")
        hit = (qi + di * toi).astype(F)
        add(hit, [0, 0, 0], np.inf, "still")  # d = 0 at the contact: within rounding of touching
        add(qi, [0, 0, 0], np.inf, "still")
        add(f.coords[j] + (qi[0] - qi.mean(axis=0)) * F(0.1), [0, 0, 0], np.inf, "still")  # laid on a mesh triangle
        # one zero component of d: the query moved so that its box meets the answering triangle's on that axis, and
        # moved off it
        for k in range(3):
            x = di.copy()
            x[k] = 0
            on = qi.copy()
            on[:, k] += rec[5][j, k] - qi[:, k].min()
            add(on, x, np.inf, "axis on")
            off = qi.copy()
            off[:, k] += (rec[6][j, k] - qi[:, k].min()) + F(1e-3) * F(f.mx)
            add(off, x, np.inf, "axis")
        add([qi[0], qi[1], qi[1]], di, np.inf, "segment")
        add([qi[0], qi[0], qi[0]], di, np.inf, "point")
        far = qi.copy()
        far[2, 0] = np.nextafter(cmax, F(np.inf))
        add(far, di, np.inf, "outside")  # one |q| above 2^20 mx
        far[2, 0] = -cmax
        add(far, di, np.inf, "edge")
        for k in range(3):
            for tiny, what in ((1e-30, "outside"), (NEG_SUB, "outside"), (np.nextafter(F(2.0 ** -64), F(0)), "outside"),
                               (2.0 ** -64, "edge"), (-2.0 ** 64, "edge")):
                x = di.copy()
                x[k] = tiny
                add(qi, x, np.inf, what)
            add(qi, di * F(2.0 ** 40), np.inf, "edge")
            x = di.copy()
            x[k] = np.nextafter(F(2.0 ** 64), F(np.inf)) * np.sign(di[k])
            add(qi, x, np.inf, "outside")
    return np.array(q), np.array(d), np.array(tm), np.array(kind)


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_special_inputs(fix, scene):
    f = fix[scene]
    q, d, tm, kind = special_queries(f)
    want = tr.expected(q, d, f.coords, t_max=tm)
    inv = kind == "invalid"
    assert inv.sum() >= 100 and (want[0][inv] == -1).all() and (want[1][inv] == FMAX).all() and (want[3][inv] == -1).all()
    assert same_bits(want[2][inv], q[inv, 0])
    assert (want[0][kind == "still"] >= 0).any() and (want[0][kind == "still"] == -1).any()
    assert (want[0][kind == "axis on"] >= 0).any()
    assert (want[0][kind == "segment"] >= 0).any() and (want[0][kind == "point"] >= 0).any()
    assert (want[0][kind == "outside"] >= 0).sum() >= 16
    outside = ~tr.domain(q, d, f.mx) & ~inv
    assert np.array_equal(outside, kind == "outside")
    valid, outside = int((~inv).sum()), int(outside.sum())
    for kernel in KERNELS:
        got = query(f.r, q, d, kernel, t_max=tm)
        check(got, want, what=(scene, kernel))
        check_path(got[4], kernel, valid, len(f.coords), outside=outside)


# ------------------------------------------------------------------ 5. counts around chunk edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_query_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    q, d = cuda(f.q[:CHUNK + 1]), cuda(f.d[:CHUNK + 1])
    for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1):
        tri = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        kind = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        t = torch.full((n + 3,), -77.0, dtype=torch.float32, device="cuda")
        point = torch.full((3 * n + 3,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the fills are torch's work; the query runs on the renderer's stream)
        f.r.sweep_tris((q.data_ptr(), n), d.data_ptr(), kernel=kernel, tri=tri.data_ptr(), t=t.data_ptr(),
                       point=point.data_ptr(), kind=kind.data_ptr())  # (raw pointers: the buffers are longer)
        assert f.r.trisweep_info()["triangles"] == n
        tri, t, point, kind = tri.cpu().numpy(), t.cpu().numpy(), point.cpu().numpy(), kind.cpu().numpy()
        np.testing.assert_array_equal(tri[:n], f.want[0][:n], err_msg=str(n))
        np.testing.assert_array_equal(kind[:n], f.want[3][:n], err_msg=str(n))
        assert same_bits(t[:n], f.want[1][:n]) and same_bits(point[:3 * n].reshape(n, 3), f.want[2][:n]), n
        assert (tri[n:] == -77).all() and (t[n:] == -77).all() and (point[3 * n:] == -77).all(), n
        assert (kind[n:] == -77).all(), n


# ------------------------------------------------------------------ 6. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    rows = np.arange(0, N, 2)
    for kernel in KERNELS:
        got = query(r, f.q[rows], f.d[rows], kernel)
        check(got, f.rows(rows), what=(accel, flags, kernel))
        check_path(got[4], kernel, len(rows), len(f.coords), wide=accel != "reference")
    r.close()


# ------------------------------------------------------------------ 7. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_nearest.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="auto"), both kernels answer as the yardstick does on the moved coordinates (every
    second fixture query)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    q, d = f.q[rows], f.d[rows]
    want = tr.expected(q, d, coords)
    still = f.rows(rows)
    assert (want[0] != still[0]).sum() > 100 and (want[0] >= 0).sum() > 100
    r = dev.Renderer(0).upload(s)
    check(query(r, q, d, "fast"), still, what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="auto")
        for kernel in KERNELS:
            got = query(r, q, d, kernel)
            check(got, want, what=(step, kernel))
        assert got[4]["walked"] == len(rows)
    r.close()


# ------------------------------------------------------------------ 8. isolation
def test_a_triangle_sweep_leaves_renders_and_other_queries_alone(dev, scenes, fix):
    """tests/test_gpu_query_slots.py's pattern: a frame's BGRA and every other family's info are unchanged after
    triangle sweeps, and the triangle sweep's info after the others ran again"""
    import torch
    from prt import rays
    W, H = tr.CAM_W, tr.CAM_H
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    tris = cuda(f.coords[:: len(f.coords) // 300][:300])
    pts = tris.mean(dim=1).contiguous()
    lo, hi = (pts - 0.05).contiguous(), (pts + 0.05).contiguous()
    down = torch.zeros_like(pts)
    down[:, 1] = -1.0
    o, p = rays.pinhole(cam, W, H)
    q, d = cuda(f.q), cuda(f.d)
    torch.cuda.synchronize()  # (these tensors are torch's work; the queries run on the renderer's stream)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def same(a, b):
        return strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    run = [lambda: r.trace_rays(o[:65], p[:65]), lambda: r.shade_rays(o[:97], p[:97]),
           lambda: r.trace_hits(o[:131], p[:131], max_hits=2), lambda: r.nearest(pts[:163]),
           lambda: r.nearest_tris(pts[:197], k=4), lambda: r.overlaps(lo[:229], hi[:229], k=4),
           lambda: r.sweep(pts[:259], down[:259], 0.01), lambda: r.sweep_contacts(pts[:291], down[:291], 0.01, k=4),
           lambda: r.cuts(tris[:123], k=4), lambda: r.clearance(tris[:101]), lambda: r.proximity(tris[:67], k=4)]
    infos = [r.query_info, r.shade_info, r.hits_info, r.nearest_info, r.neighbours_info, r.overlaps_info,
             r.sweep_info, r.contacts_info, r.cuts_info, r.clearance_info, r.proximity_info]
    bgra = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", bgra=bgra)
    r.sync()
    bgra0, stats0, launch0 = bgra.cpu().numpy().copy(), r.stats(), r.launch_info()
    def others():
        for fn in run:
            out = fn()  # (held until the query has run: a dropped output's memory could serve the next call's inputs)
            r.sync()
            del out

    others()
    with pytest.raises(dev.RtError, match="status -5"):  # no triangle sweep run yet, whatever ran before
        r.trisweep_info()
    held = [i() for i in infos]
    for kernel in ("fast", "strict", "fast"):
        r.sweep_tris(q, d, kernel=kernel)
        si = r.trisweep_info()
        assert si["triangles"] == N and si["kernel_ms"] > 0
    assert np.array_equal(bgra.cpu().numpy(), bgra0) and r.stats() == stats0 and r.launch_info() == launch0
    for i, h in zip(infos, held):  # the other queries' counters as they were
        assert same(i(), h), (i(), h)
    others()  # ... and the other way round: none of them touches the triangle sweep's own counters
    r.render(cam, W, H, kernel="fast", bgra=bgra)
    r.sync()
    assert np.array_equal(bgra.cpu().numpy(), bgra0)
    assert same(r.trisweep_info(), si)
    for i, h in zip(infos, held):
        assert strip(i()) == strip(h)
    r.close()


# ------------------------------------------------------------------ 9. errors
def test_trisweep_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    q, d = cuda(f.q), cuda(f.d)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.sweep_tris(q, d)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no triangle sweep query run yet
        r.trisweep_info()
    r.sweep_tris(q[:100], d[:100])
    info = r.trisweep_info()
    assert info["triangles"] == 100 and info["found"] == int((f.want[0][:100] >= 0).sum())
    with pytest.raises(dev.RtError, match="bad kernel"):
        r.sweep_tris(q, d, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.sweep_tris((0, 16), d.data_ptr())  # null tris
    with pytest.raises(dev.RtError, match="motions: 297 elements"):
        r.sweep_tris(q[:100], d[:99])
    L = _lib.hip()
    tri = torch.empty(16, dtype=torch.int32, device="cuda")
    kd = torch.empty(16, dtype=torch.int32, device="cuda")
    tt = torch.empty(16, dtype=torch.float32, device="cuda")
    pt = torch.empty(48, dtype=torch.float32, device="cuda")
    pq, pd, t, u, p, k = q.data_ptr(), d.data_ptr(), tri.data_ptr(), tt.data_ptr(), pt.data_ptr(), kd.data_ptr()
    Q, R = _lib.SweepTris, _lib.TrisweepResults
    for qq, res in [
        (Q(None, pd, None, 16, 0), R(t, u, p, k)),         # null tris, null motion
        (Q(pq, None, None, 16, 0), R(t, u, p, k)),
        (Q(pq, pd, None, 16, 0), R(None, None, None, None)),  # all outputs NULL
        (Q(pq, pd, None, 16, 3), R(t, u, p, k)),           # unknown kernel
        (Q(pq, pd, None, 16, -1), R(t, u, p, k)),
        (Q(pq, pd, None, -1, 0), R(t, u, p, k)),           # negative n
    ]:
        assert L.rt_sweep_triangles(r._ctx, ctypes.byref(qq), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_sweep_triangles(r._ctx, None, None) == -1
    assert L.rt_sweep_triangles(r._ctx, ctypes.byref(Q(pq, pd, None, 16, 0)), None) == -1
    after = r.trisweep_info()  # a refused call leaves trisweep_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # one output alone is enough
    for res in (R(t, None, None, None), R(None, u, None, None), R(None, None, p, None), R(None, None, None, k)):
        assert L.rt_sweep_triangles(r._ctx, ctypes.byref(Q(pq, pd, None, 16, 0)), ctypes.byref(res)) == 0
    r.sync()
    assert np.array_equal(tri.cpu().numpy(), f.want[0][:16]) and same_bits(tt.cpu().numpy(), f.want[1][:16])
    assert same_bits(pt.cpu().numpy().reshape(16, 3), f.want[2][:16])
    assert np.array_equal(kd.cpu().numpy(), f.want[3][:16])
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_sweep_triangles(r._ctx, ctypes.byref(Q(None, None, None, 0, 0)),
                                ctypes.byref(R(None, None, None, None))) == 0
    assert r.trisweep_info()["triangles"] == 0
    r.close()
