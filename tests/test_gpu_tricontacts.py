"""Triangle contact queries (rt_sweep_tri_contacts: Renderer.sweep_tri_contacts / tricontacts_info) against
tests/tricontacts_ref.py, the lists of tests/trisweep_ref.py's pairs, which tests/test_tricontacts_abi.py holds against
geometry in float64 on the CPU. An answer is a list of triangle indices, times, points and kinds and a count, all with
defined bits, so every comparison is array_equal / same_bits and no case is excluded. Per scene the queries are
trisweep_ref.fixture's 512 seeded and 128 camera triangles; the members are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import tricontacts_ref as tc
from tests import trisweep_ref as tr
from tests.test_gpu_trisweep import NEG_SUB, NEG_TINY, check_path, special_queries
from tests.tricontacts_ref import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
FMAX = tc.FMAX
KERNELS = ["strict", "fast"]
N = tr.NS + tr.NC
KS = [1, 3, 4, 5, 8, 9, 16]  # both sides of every capacity (4, 8, 16) and of the register / LDS key boundaries
SCENES = ["car_boxed", "car_only"]


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


@pytest.fixture(scope="module")
def scenes():
    return {name: host.Scene.named(name).build_bvh(3) for name in SCENES}


def cuda(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def query(r, q, d, k, kernel, t_max=None, count_all=False):
    """(tri, t, point, kind, count, info); k = 0: the lists are empty"""
    import torch
    n = len(q)
    kind = torch.empty((n, k), dtype=torch.int32, device="cuda")
    out = r.sweep_tri_contacts(cuda(q), cuda(d), k=k, t_max=None if t_max is None else cuda(t_max), count_all=count_all,
                               points_out=True, kernel=kernel, kind=kind if k else None)
    info = r.tricontacts_info()
    tri, t, count, point = (x.cpu().numpy() for x in out)
    return tri, t, point, kind.cpu().numpy(), count, info


def check(got, mem, q, k, count_all, rows=None, what=""):
    """the five outputs against the yardstick's lists of the members mem (of the queries `rows` of q), and the info"""
    want = tc.lists(mem, q, k, count_all)
    total = mem.total
    if rows is not None:
        want, total = tuple(x[rows] for x in want), total[rows]
    tri, t, point, kind, count, info = got
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    bad = np.argwhere(t.view(np.int32) != want[1].view(np.int32))
    assert len(bad) == 0, (what, bad[:8])
    assert same_bits(point, want[2]), what
    np.testing.assert_array_equal(kind, want[3], err_msg=str(what))
    np.testing.assert_array_equal(count, want[4], err_msg=str(what))
    n = len(tri)
    assert info["triangles"] == n and info["stack_overflows"] == 0, (what, info)
    assert info["found"] == int((total > 0).sum()) and info["found"] + info["empty"] == n, (what, info)
    assert info["stored"] == int(np.minimum(total, k).sum()), (what, info)
    assert info["counted"] == int(want[4].astype(np.int64).sum()), (what, info)


class Fix:
    """one fixture scene: a Renderer, the N queries and their members without a bound and under t_max = 1"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.q, self.d = tr.fixture(self.coords, seed)
        self.mem = tc.members(self.q, self.d, self.coords)
        self.one = np.ones(N, F)
        self.mem1 = tc.members(self.q, self.d, self.coords, self.one)
        first = tc.lists(self.mem, self.q, 1)
        self.want = (first[0][:, 0], first[1][:, 0])  # (the sweep's tri and t: what special_queries reads)
        self.mx = max(16.0, float(np.abs(self.coords).max()))  # the scene's coordinate magnitude (rt_hip.hip)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, tr.SEED[name]) for name, s in scenes.items()}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. the fixture tests something
@pytest.mark.parametrize("scene", SCENES)
def test_fixture(fix, scene):
    f = fix[scene]
    many = int((f.mem.total > 16).sum())
    ties = [int(tc.boundary_ties(f.mem, k).sum()) for k in (4, 8, 16)]
    empty = int((f.mem.total == 0).sum())
    print(scene, "members", int(f.mem.total.sum()), "queries with more than 16", many, "boundary ties at 4 / 8 / 16", ties,
          "empty", empty, "under t_max = 1:", int(f.mem1.total.sum()))
    assert many >= 64 and min(ties) >= 16 and empty >= 16
    assert 0 < f.mem1.total.sum() < f.mem.total.sum()


# ------------------------------------------------------------------ 2. all variants
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", SCENES)
def test_variants(fix, scene, kernel, k):
    """count_all x bound (none, 1) x order (in order, permuted) at one k: all five outputs and the counters"""
    f = fix[scene]
    p = np.random.default_rng(13).permutation(N)
    for count_all in (False, True):
        for mem, tm in ((f.mem, None), (f.mem1, f.one)):
            for order in (None, p):
                q, d = (f.q, f.d) if order is None else (f.q[order], f.d[order])
                got = query(f.r, q, d, k, kernel, t_max=None if tm is None else tm[:len(q)], count_all=count_all)
                check(got, mem, f.q, k, count_all, rows=order,
                      what=(scene, kernel, k, count_all, tm is not None, order is not None))
                check_path(got[5], kernel, N, len(f.coords))


# ------------------------------------------------------------------ 3. fast against strict, the pure count included
@pytest.mark.parametrize("bound", ["none", "one"])
@pytest.mark.parametrize("scene", SCENES)
def test_fast_is_strict(fix, scene, bound):
    f = fix[scene]
    for k, count_all in ((0, True), (1, False), (4, False), (4, True), (8, False), (16, False), (16, True)):
        for tm in ((None,) if bound == "none" else (f.one,)):
            a = query(f.r, f.q, f.d, k, "strict", t_max=tm, count_all=count_all)
            b = query(f.r, f.q, f.d, k, "fast", t_max=tm, count_all=count_all)
            for x, y in zip(a[:5], b[:5]):
                assert x.shape == y.shape and same_bits(x, y), (scene, k, count_all)
            for key in ("triangles", "found", "stored", "counted", "empty"):
                assert a[5][key] == b[5][key], (key, a[5], b[5])
            if k == 0:  # the swept-volume count: no list, every member counted
                mem = f.mem if tm is None else f.mem1
                np.testing.assert_array_equal(b[4], mem.total.astype(np.int32))
                assert b[0].shape == (N, 0) and b[5]["stored"] == 0 and b[5]["counted"] == int(mem.total.sum())


# ------------------------------------------------------------------ 4. k = 1 is the sweep
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", SCENES)
def test_k1_is_sweep_tris(fix, scene, kernel):
    import torch
    f = fix[scene]
    for tm in (None, f.one):
        kind = torch.empty(N, dtype=torch.int32, device="cuda")
        tri, t, point = f.r.sweep_tris(cuda(f.q), cuda(f.d), t_max=None if tm is None else cuda(tm), kernel=kernel,
                                       kind=kind)
        f.r.sync()
        got = query(f.r, f.q, f.d, 1, kernel, t_max=tm)
        np.testing.assert_array_equal(got[0][:, 0], tri.cpu().numpy())
        assert same_bits(got[1][:, 0], t.cpu().numpy()) and same_bits(got[2][:, 0], point.cpu().numpy())
        np.testing.assert_array_equal(got[3][:, 0], kind.cpu().numpy())
        assert (got[0] >= 0).sum() > 100


# ------------------------------------------------------------------ 5. every triangle twice
def test_doubled(dev, scenes, fix):
    """the scene with every triangle twice: each member comes with its copy at the same toi, the lower index first, and
    every count is exactly twice the single scene's -- no record is offered twice, none is lost"""
    s = scenes["car_only"]
    f = fix["car_only"]
    t = s.triangles
    n = len(f.coords)
    twice = host.Scene(host.triangle_init(np.concatenate([f.coords, f.coords]), *(np.concatenate([t[k], t[k]])
                                                                                  for k in ("ks", "kd", "kr"))),
                       s.lights.copy())
    r = dev.Renderer(0).upload(twice.build_bvh(3))
    rows = np.arange(0, N, 2)
    m = f.mem
    # the doubled scene's members: every member (toi, j) and its copy (toi, j + n); in the order a tie puts the copies
    # after every original that shares the toi
    both = tc.Members(N, np.tile(m.qi, 2), np.concatenate([m.ti, m.ti + n]), np.tile(m.toi, 2),
                      np.tile(m.pt, (2, 1)), np.tile(m.kind, 2))
    assert (both.total == 2 * m.total).all()
    whole = np.flatnonzero(2 * m.total[rows] <= 16)  # the rows whose whole set fits the list
    assert len(whole) >= 64
    for kernel in KERNELS:
        got = query(r, f.q[rows], f.d[rows], 16, kernel, count_all=True)
        check(got, both, f.q, 16, True, rows=rows, what=("twice", kernel))
        tri, tt, point, kind, count, info = got
        np.testing.assert_array_equal(count, 2 * m.total[rows].astype(np.int32), err_msg=kernel)
        assert info["counted"] == 2 * int(m.total[rows].sum())
        for i in whole:  # entries come in pairs (j, j + n) with equal toi, point and kind
            c = count[i]
            order = np.lexsort((tri[i, :c] // n, tri[i, :c] % n))
            a, b = order[0::2], order[1::2]
            assert np.array_equal(tri[i, a] + n, tri[i, b]) and same_bits(tt[i, a], tt[i, b]), (kernel, i)
            assert same_bits(point[i, a], point[i, b]) and np.array_equal(kind[i, a], kind[i, b]), (kernel, i)
        pure = query(r, f.q[rows], f.d[rows], 0, kernel, count_all=True)
        np.testing.assert_array_equal(pure[4], count)
    r.close()


# ------------------------------------------------------------------ 5b. the closed-form lists, on the device
def test_hand_cases(dev, scenes):
    """tests/test_tricontacts_abi.py's hand cases through both kernels: two stacked sheets, a shared edge met head on,
    a start in contact with two triangles, and the bound on the k-th toi to the bit"""
    from tests.test_tricontacts_abi import PLATE, SHEETS
    s = scenes["car_only"]
    mat = [s.triangles[k][:2] for k in ("ks", "kd", "kr")]
    edge = np.array([[[0, 0, 0], [4, 0, -1], [0, 4, 0]], [[0, 0, 0], [0, 4, 0], [-4, 0, -1]]], F)
    half, quarter = F(0.5), F(0.25)
    cases = [  # (mesh, q, d, t_max, tri, t, kind, count with count_all)
        (SHEETS, PLATE, [0, 0, -4], np.inf, [1, 0, -1, -1], [0.25, 0.5, FMAX, FMAX], [0, 0, -1, -1], 2),
        (edge, [[-1, 2, 3], [1, 2, 3], [0, 2, 5]], [0, 0, -1], np.inf, [0, 1, -1, -1], [3, 3, FMAX, FMAX], None, 2),
        (SHEETS, [[1, 1, -2], [2, 1, 1], [1, 1, 1]], [1, 2, 3], np.inf, [0, 1, -1, -1], [0, 0, FMAX, FMAX],
         [15, 15, -1, -1], 2),
        (SHEETS, [[1, 1, -2], [2, 1, 1], [1, 1, 1]], [0, 0, 0], 0.0, [0, 1, -1, -1], [0, 0, FMAX, FMAX],
         [15, 15, -1, -1], 2),
        (SHEETS, PLATE, [0, 0, -4], half, [1, 0, -1, -1], [0.25, 0.5, FMAX, FMAX], [0, 0, -1, -1], 2),
        (SHEETS, PLATE, [0, 0, -4], np.nextafter(half, F(0)), [1, -1, -1, -1], [0.25, FMAX, FMAX, FMAX],
         [0, -1, -1, -1], 1),
        (SHEETS, PLATE, [0, 0, -4], quarter, [1, -1, -1, -1], [0.25, FMAX, FMAX, FMAX], [0, -1, -1, -1], 1),
        (SHEETS, PLATE, [0, 0, -4], np.nextafter(quarter, F(0)), [-1] * 4, [FMAX] * 4, [-1] * 4, 0),
    ]
    for mesh, q, d, tm, tri, t, kind, count in cases:
        mesh, q, d, tm = np.asarray(mesh, F), np.array([q], F), np.array([d], F), np.array([tm], F)
        r = dev.Renderer(0).upload(host.Scene(host.triangle_init(mesh, *mat), s.lights.copy()).build_bvh(3))
        mem = tc.members(q, d, mesh, tm)
        for kernel in KERNELS:
            got = query(r, q, d, 4, kernel, t_max=tm, count_all=True)
            check(got, mem, q, 4, True, what=(kernel, tri))
            assert got[0][0].tolist() == tri and got[1][0].tolist() == t and got[4][0] == count, (kernel, got[:5])
            assert kind is None or got[3][0].tolist() == kind, (kernel, got[3])
        r.close()


# ------------------------------------------------------------------ 6. t_max around the k-th toi
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", [1, 4])
def test_bound_at_kth(fix, k, kernel):
    f = fix["car_boxed"]
    rows, kth = tc.kth_toi(f.mem, k)
    assert tc.boundary_ties(f.mem, k)[rows].sum() >= 16  # (rows whose (k+1)-th ties the k-th are included)
    at = np.full(N, np.inf, F)
    at[rows] = kth
    below = at.copy()
    below[rows] = np.nextafter(kth, F(-1))  # (a k-th toi of 0: a negative bound, the empty set)
    above = at.copy()
    above[rows] = np.nextafter(kth, F(np.inf))
    for tm, what in ((at, "at"), (below, "below"), (above, "above")):
        mem = tc.members(f.q, f.d, f.coords, tm)
        if what == "at":  # the k-th itself is kept, and so is everything that ties it
            assert (mem.total[rows] >= k).all()
        if what == "below":
            assert (mem.total[rows] < k).all()
        for count_all in (False, True):
            got = query(f.r, f.q, f.d, k, kernel, t_max=tm, count_all=count_all)
            check(got, mem, f.q, k, count_all, what=(what, k, kernel, count_all))


# ------------------------------------------------------------------ 7. special inputs, 9. outside the walk's domain
@pytest.mark.parametrize("scene", SCENES)
def test_special_inputs(fix, scene):
    """tests/test_gpu_trisweep.py's special queries: non-finite corners and motions, NaN / negative-subnormal t_max,
    d = 0, zero components of d, zero-area queries, queries outside tsw_domain and at its edges; then t_max = 0 and the
    bounds built from bits on the fixture"""
    f = fix[scene]
    q, d, tm, kind = special_queries(f)
    mem = tc.members(q, d, f.coords, tm)
    inv = kind == "invalid"
    assert inv.sum() >= 100 and (mem.total[inv] == 0).all()
    empty = tc.lists(mem, q, 4)
    assert (empty[0][inv] == -1).all() and (empty[1][inv] == FMAX).all() and (empty[3][inv] == -1).all()
    assert same_bits(empty[2][inv], np.repeat(q[inv, :1], 4, axis=1)) and (empty[4][inv] == 0).all()
    assert (mem.total[kind == "still"] > 1).any() and (mem.total[kind == "still"] == 0).any()
    assert (mem.total[kind == "segment"] > 0).any() and (mem.total[kind == "point"] > 0).any()
    assert (mem.total[kind == "outside"] > 0).sum() >= 16
    outside = ~tr.domain(q, d, f.mx) & ~inv
    assert np.array_equal(outside, kind == "outside")
    valid, outside = int((~inv).sum()), int(outside.sum())
    for kernel in KERNELS:
        for k, count_all in ((4, False), (16, True)):
            got = query(f.r, q, d, k, kernel, t_max=tm, count_all=count_all)
            check(got, mem, q, k, count_all, what=(scene, kernel, k))
            check_path(got[5], kernel, valid, len(f.coords), outside=outside)
    zero = np.zeros(N, F)
    mixed = np.array([np.nan, -1.0, NEG_TINY, NEG_SUB, -0.0, np.inf, 0.5, 1e-3], F)[np.arange(N) % 8]
    for bound in (zero, mixed):
        mem = tc.members(f.q, f.d, f.coords, bound)
        if bound is zero:
            assert (mem.toi == 0).all() and (mem.total > 1).sum() >= 8  # starts in contact with several triangles
        else:
            assert (mem.total[np.arange(N) % 8 < 4] == 0).all() and (mem.total[np.arange(N) % 8 == 4] > 0).any()
        for kernel in KERNELS:
            got = query(f.r, f.q, f.d, 8, kernel, t_max=bound, count_all=True)
            check(got, mem, f.q, 8, True, what=(scene, kernel, "bounds"))


# ------------------------------------------------------------------ 8. count and output edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_query_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    k = 5
    want = tc.lists(f.mem, f.q, k)
    q, d = cuda(f.q[:258]), cuda(f.d[:258])
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        m = n * k
        tri = torch.full((m + 3,), -77, dtype=torch.int32, device="cuda")
        kind = torch.full((m + 3,), -77, dtype=torch.int32, device="cuda")
        t = torch.full((m + 3,), -77.0, dtype=torch.float32, device="cuda")
        point = torch.full((3 * m + 3,), -77.0, dtype=torch.float32, device="cuda")
        count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the fills are torch's work; the query runs on the renderer's stream)
        f.r.sweep_tri_contacts((q.data_ptr(), n), d.data_ptr(), k=k, kernel=kernel, tri=tri.data_ptr(), t=t.data_ptr(),
                               point=point.data_ptr(), kind=kind.data_ptr(), count=count.data_ptr())
        assert f.r.tricontacts_info()["triangles"] == n
        tri, t, point, kind, count = (x.cpu().numpy() for x in (tri, t, point, kind, count))
        np.testing.assert_array_equal(tri[:m].reshape(n, k), want[0][:n], err_msg=str(n))
        np.testing.assert_array_equal(kind[:m].reshape(n, k), want[3][:n], err_msg=str(n))
        np.testing.assert_array_equal(count[:n], want[4][:n], err_msg=str(n))
        assert same_bits(t[:m].reshape(n, k), want[1][:n]) and same_bits(point[:3 * m].reshape(n, k, 3), want[2][:n]), n
        assert (tri[m:] == -77).all() and (t[m:] == -77).all() and (point[3 * m:] == -77).all(), n
        assert (kind[m:] == -77).all() and (count[n:] == -77).all(), n


def test_each_output_alone(fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    L = _lib.hip()
    n, k = 100, 6
    want = tc.lists(f.mem, f.q, k)
    q, d = cuda(f.q[:n]), cuda(f.d[:n])
    i32, f32 = torch.int32, torch.float32
    tri, kd = (torch.full((n, k), -77, dtype=i32, device="cuda") for _ in range(2))
    tt = torch.full((n, k), -77.0, dtype=f32, device="cuda")
    pt = torch.full((n, k, 3), -77.0, dtype=f32, device="cuda")
    cnt = torch.full((n,), -77, dtype=i32, device="cuda")
    torch.cuda.synchronize()
    Q, R = _lib.TriContacts, _lib.TricontactResults
    for kernel in (1, 2):  # RT_KERNEL_STRICT, RT_KERNEL_FAST
        for res in (R(tri.data_ptr(), None, None, None, None), R(None, tt.data_ptr(), None, None, None),
                    R(None, None, pt.data_ptr(), None, None), R(None, None, None, kd.data_ptr(), None),
                    R(None, None, None, kd.data_ptr(), cnt.data_ptr())):
            qq = Q(q.data_ptr(), d.data_ptr(), None, n, k, 0, kernel)
            assert L.rt_sweep_tri_contacts(f.r._ctx, ctypes.byref(qq), ctypes.byref(res)) == 0
        f.r.sync()
        np.testing.assert_array_equal(tri.cpu().numpy(), want[0][:n])
        assert same_bits(tt.cpu().numpy(), want[1][:n]) and same_bits(pt.cpu().numpy(), want[2][:n])
        np.testing.assert_array_equal(kd.cpu().numpy(), want[3][:n])
        np.testing.assert_array_equal(cnt.cpu().numpy(), want[4][:n])
    # only the count is looked at, k = 16, through the Python method
    mine = torch.full((n,), -77, dtype=i32, device="cuda")
    torch.cuda.synchronize()
    out = f.r.sweep_tri_contacts(q, d, k=16, count=mine)
    f.r.sync()
    assert out[2] is mine and len(out) == 3
    np.testing.assert_array_equal(mine.cpu().numpy(), np.minimum(f.mem.total[:n], 16).astype(np.int32))
    out = f.r.sweep_tri_contacts(q, d, k=0, count_all=True, count=mine)
    f.r.sync()
    assert tuple(out[0].shape) == (n, 0) and tuple(out[1].shape) == (n, 0)
    np.testing.assert_array_equal(mine.cpu().numpy(), f.mem.total[:n].astype(np.int32))


# ------------------------------------------------------------------ 10. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    rows = np.arange(0, N, 2)
    for kernel in KERNELS:
        for k, count_all in ((5, False), (16, True)):
            got = query(r, f.q[rows], f.d[rows], k, kernel, count_all=count_all)
            check(got, f.mem, f.q, k, count_all, rows=rows, what=(accel, flags, kernel, k))
            check_path(got[5], kernel, len(rows), len(f.coords), wide=accel != "reference")
    r.close()


# ------------------------------------------------------------------ 11. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_trisweep.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="auto"), both kernels answer as the yardstick does on the moved coordinates (every
    second fixture query)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    q, d = f.q[rows], f.d[rows]
    mem = tc.members(q, d, coords)
    assert (tc.lists(mem, q, 1)[0][:, 0] != f.want[0][rows]).sum() > 100 and (mem.total > 0).sum() > 100
    r = dev.Renderer(0).upload(s)
    check(query(r, q, d, 8, "fast", count_all=True), f.mem, f.q, 8, True, rows=rows, what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="auto")
        for kernel in KERNELS:
            got = query(r, q, d, 8, kernel, count_all=True)
            check(got, mem, q, 8, True, what=(step, kernel))
        assert got[5]["walked"] == len(rows)
    r.close()


# ------------------------------------------------------------------ 12. isolation
def test_a_contact_query_leaves_renders_and_other_queries_alone(dev, scenes, fix):
    """a frame, sweep_tris' answer and its info are unchanged after triangle contact queries, and a sweep_tris call in
    between does not disturb tricontacts_info"""
    import torch
    W, H = tr.CAM_W, tr.CAM_H
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    q, d = cuda(f.q), cuda(f.d)
    torch.cuda.synchronize()

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def same(a, b):
        return strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    bgra = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", bgra=bgra)
    r.sync()
    bgra0, stats0, launch0 = bgra.cpu().numpy().copy(), r.stats(), r.launch_info()
    kind = torch.empty(N, dtype=torch.int32, device="cuda")
    out = r.sweep_tris(q, d, kind=kind)
    si = r.trisweep_info()  # (synchronises: the outputs are read after it)
    sweep0 = [x.cpu().numpy().copy() for x in (*out, kind)]
    with pytest.raises(dev.RtError, match="status -5"):  # no triangle contact query run yet, whatever ran before
        r.tricontacts_info()
    for kernel, k, count_all in (("fast", 8, False), ("strict", 16, True), ("fast", 0, True), ("fast", 3, True)):
        out = r.sweep_tri_contacts(q, d, k=k, count_all=count_all, points_out=True, kernel=kernel)
        ci = r.tricontacts_info()
        assert ci["triangles"] == N and ci["kernel_ms"] > 0
        del out
    assert ci["counted"] == int(f.mem.total.sum()) and ci["stored"] == int(np.minimum(f.mem.total, 3).sum())
    assert np.array_equal(bgra.cpu().numpy(), bgra0) and r.stats() == stats0 and r.launch_info() == launch0
    assert same(r.trisweep_info(), si)
    kind2 = torch.empty(N, dtype=torch.int32, device="cuda")
    out = r.sweep_tris(q, d, kind=kind2)
    assert strip(r.trisweep_info()) == strip(si)
    sweep1 = [x.cpu().numpy() for x in (*out, kind2)]
    for a, b in zip(sweep0, sweep1):
        assert same_bits(a, b)
    r.render(cam, W, H, kernel="fast", bgra=bgra)
    r.sync()
    assert np.array_equal(bgra.cpu().numpy(), bgra0)
    assert same(r.tricontacts_info(), ci)  # the sweep and the frame in between touched none of its counters
    r.close()


# ------------------------------------------------------------------ 13. errors
def test_tricontacts_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    q, d = cuda(f.q), cuda(f.d)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.sweep_tri_contacts(q, d)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no triangle contact query run yet
        r.tricontacts_info()
    r.sweep_tri_contacts(q[:100], d[:100], k=4)
    info = r.tricontacts_info()
    assert info["triangles"] == 100 and info["found"] == int((f.mem.total[:100] > 0).sum())
    with pytest.raises(dev.RtError, match="bad kernel"):
        r.sweep_tri_contacts(q, d, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.sweep_tri_contacts((0, 16), d.data_ptr())  # null tris
    with pytest.raises(dev.RtError, match="motions: 297 elements"):
        r.sweep_tri_contacts(q[:100], d[:99])
    L = _lib.hip()
    i32, f32 = torch.int32, torch.float32
    tri, kd = torch.empty(64, dtype=i32, device="cuda"), torch.empty(64, dtype=i32, device="cuda")
    tt, pt = torch.empty(64, dtype=f32, device="cuda"), torch.empty(192, dtype=f32, device="cuda")
    cnt = torch.empty(16, dtype=i32, device="cuda")
    pq, pd = q.data_ptr(), d.data_ptr()
    t, u, p, k, c = tri.data_ptr(), tt.data_ptr(), pt.data_ptr(), kd.data_ptr(), cnt.data_ptr()
    Q, R = _lib.TriContacts, _lib.TricontactResults
    full = R(t, u, p, k, c)
    for qq, res, msg in [
        (Q(None, pd, None, 16, 4, 0, 0), full, "rt_sweep_tri_contacts: null tris / motion"),
        (Q(pq, None, None, 16, 4, 0, 0), full, "rt_sweep_tri_contacts: null tris / motion"),
        (Q(pq, pd, None, 16, -1, 0, 0), full, "rt_sweep_tri_contacts: max_tris must be 0..16"),
        (Q(pq, pd, None, 16, 17, 0, 0), full, "rt_sweep_tri_contacts: max_tris must be 0..16"),
        (Q(pq, pd, None, 16, 4, 0, 0), R(None, None, None, None, c),
         "rt_sweep_tri_contacts: max_tris > 0 needs a tri, a t, a point or a kind output"),
        (Q(pq, pd, None, 16, 4, 0, 0), R(None, None, None, None, None),
         "rt_sweep_tri_contacts: max_tris > 0 needs a tri, a t, a point or a kind output"),
        (Q(pq, pd, None, 16, 0, 0, 0), full, "rt_sweep_tri_contacts: max_tris = 0 needs count_all"),
        (Q(pq, pd, None, 16, 0, 1, 0), R(t, u, p, k, None), "rt_sweep_tri_contacts: a counting query needs a count output"),
        (Q(pq, pd, None, 16, 4, 2, 0), full, "rt_sweep_tri_contacts: count_all must be 0 or 1"),
        (Q(pq, pd, None, 16, 4, -1, 0), full, "rt_sweep_tri_contacts: count_all must be 0 or 1"),
        (Q(pq, pd, None, 16, 4, 0, 3), full, "rt_sweep_tri_contacts: bad kernel"),
        (Q(pq, pd, None, 16, 4, 0, -1), full, "rt_sweep_tri_contacts: bad kernel"),
        (Q(pq, pd, None, -1, 4, 0, 0), full, "rt_sweep_tri_contacts: negative triangle count"),
    ]:
        assert L.rt_sweep_tri_contacts(r._ctx, ctypes.byref(qq), ctypes.byref(res)) == -1, msg
        assert L.rt_last_error(r._ctx).decode() == msg
    assert L.rt_sweep_tri_contacts(r._ctx, None, None) == -1
    assert L.rt_last_error(r._ctx).decode() == "rt_sweep_tri_contacts: null tris / results"
    assert L.rt_sweep_tri_contacts(r._ctx, ctypes.byref(Q(pq, pd, None, 16, 4, 0, 0)), None) == -1
    after = r.tricontacts_info()  # a refused call leaves tricontacts_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all, and launches nothing
    assert L.rt_sweep_tri_contacts(r._ctx, ctypes.byref(Q(None, None, None, 0, 4, 0, 0)),
                                   ctypes.byref(R(None, None, None, None, None))) == 0
    zero = r.tricontacts_info()
    assert zero["triangles"] == 0 and zero["kernel_ms"] == 0
    r.close()
