"""Overlap queries (rt_overlap_boxes: Renderer.overlaps / overlaps_csr / overlaps_info) against tests/overlap_ref.py, the
numpy float32 restatement of the triangle-box test T, which tests/test_overlap_abi.py holds against a float64
separating-axis test on the CPU. A box's answer is a set of triangle indices in index order and a count, so every
comparison is array_equal and no case is excluded. Per scene the boxes are 512 from overlap_ref.surface_boxes plus an
8 x 8 x 8 prt.boxes.grid over the scene's box; their full sets are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import overlap_ref
from tests.nearest_ref import same_bits
from tests.test_overlap_abi import invalid_boxes

pytestmark = pytest.mark.gpu

KERNELS = ["strict", "fast"]
KERNEL_ID = {"auto": 0, "strict": 1, "fast": 2}
W, H = 64, 36
NS, G = 512, 8
N = NS + G ** 3
CHUNK = 256  # QUERY_CHUNK (rt_query.hpp)


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


def scene_box(coords):
    v = coords.reshape(-1, 3)
    return v.min(0), v.max(0)


def fixture_boxes(coords, seed):
    from prt import boxes
    lo, hi = overlap_ref.surface_boxes(coords, NS, seed)
    glo, ghi = boxes.grid(*scene_box(coords), (G, G, G))
    return np.concatenate([lo, glo.cpu().numpy()]), np.concatenate([hi, ghi.cpu().numpy()])


def query(r, lo, hi, k, kernel, count_all=False):
    """(tri, count, info)"""
    tri, count = r.overlaps(cuda(lo), cuda(hi), k=k, kernel=kernel, count_all=count_all)
    info = r.overlaps_info()
    return tri.cpu().numpy(), count.cpu().numpy(), info


def check(got, want, size, what=""):
    """the answer, and the info counters against it (size: |S_i| per box)"""
    tri, count, info = got
    np.testing.assert_array_equal(count, want[1], err_msg=str(what))
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    assert info["boxes"] == len(tri) and info["stack_overflows"] == 0, (what, info)
    assert info["tris_stored"] == int((want[0] >= 0).sum()) and info["tris_counted"] == int(want[1].sum()), (what, info)
    assert info["found"] + info["empty_boxes"] == len(tri), (what, info)
    assert info["found"] == int((size > 0).sum()) and info["tris_listed"] == 0, (what, info)


def check_path(info, kernel, valid, n_tris, wide=True):
    """which loop served the boxes: the walk under "fast" on a scene with a wide view, else the exhaustive loop"""
    if kernel == "fast" and wide:
        assert info["walked_boxes"] == valid and info["exhaustive_boxes"] == 0, info
        assert (info["nodes_visited"] > 0) == (valid > 0), info
    else:
        assert info["exhaustive_boxes"] == valid and info["walked_boxes"] == 0, info
        assert info["tris_tested"] == valid * n_tris and info["nodes_visited"] == 0, info


class Fix:
    """one fixture scene: a Renderer, the N boxes and the yardstick's full sets for them"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.lo, self.hi = fixture_boxes(self.coords, seed)
        self.csr = overlap_ref.sets(self.lo, self.hi, self.coords)
        self.size = np.diff(self.csr[0])

    def want(self, k, count_all=False, rows=None):
        return overlap_ref.answer(self.csr, k, count_all, rows)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, 41 + k) for k, (name, s) in enumerate(scenes.items())}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture boxes, every k, both orders
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_boxes(fix, scene, kernel):
    f = fix[scene]
    regimes = int((f.size == 0).sum()), int(((f.size >= 1) & (f.size <= 16)).sum()), int((f.size > 16).sum())
    print(f"{scene}: |S_i| = 0: {regimes[0]}, 1..16: {regimes[1]}, > 16: {regimes[2]} boxes; max {int(f.size.max())}")
    assert min(regimes) >= 50  # the empty answer, the short list and the cut at k are all exercised
    p = np.random.default_rng(11).permutation(N)
    for k in (1, 4, 8, 16):
        for order in (np.arange(N), p):
            got = query(f.r, f.lo[order], f.hi[order], k, kernel)
            check(got, f.want(k, rows=order), f.size[order], what=(scene, kernel, k, order[0]))
            check_path(got[2], kernel, N, len(f.coords))


# ------------------------------------------------------------------ 2. counts
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_counts(fix, scene, kernel):
    """the pure count and count_all beside a list: exact on every box -- a triangle offered twice, or a slot dropped
    that holds a member, shows here"""
    f = fix[scene]
    for k in (0, 4, 16):
        want = f.want(k, count_all=True)
        assert np.array_equal(want[1], f.size) and want[0].shape == (N, k)
        got = query(f.r, f.lo, f.hi, k, kernel, count_all=True)
        check(got, want, f.size, what=(scene, kernel, k))
        assert got[2]["tris_counted"] == int(f.size.sum())
        if kernel == "fast":  # the walk prunes: fewer tests than the exhaustive loop's by far
            assert got[2]["tris_tested"] < N * len(f.coords) / 4, got[2]


# ------------------------------------------------------------------ 3. the list form
def c_query(r, lo, hi, k, count_all, kernel, offsets=None, tri=None, count=None, lst=None):
    """rt_overlap_boxes itself, on torch tensors or None -> the status"""
    from prt import _lib
    ptr = lambda x: None if x is None else x.data_ptr()
    q = _lib.Boxes(ptr(lo), ptr(hi), ptr(offsets), 0 if lo is None else len(lo), k, count_all, KERNEL_ID[kernel])
    res = _lib.OverlapResults(ptr(tri), ptr(count), ptr(lst))
    return _lib.hip().rt_overlap_boxes(r._ctx, ctypes.byref(q), ctypes.byref(res))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_csr(fix, scene, kernel):
    import torch
    f = fix[scene]
    lo, hi = cuda(f.lo), cuda(f.hi)
    offsets, tris = f.r.overlaps_csr(lo, hi, kernel=kernel)
    assert offsets.dtype == tris.dtype == torch.int32
    np.testing.assert_array_equal(offsets.cpu().numpy(), f.csr[0])
    np.testing.assert_array_equal(tris.cpu().numpy(), f.csr[1])
    info = f.r.overlaps_info()
    assert info["tris_listed"] == info["tris_counted"] == len(f.csr[1]) and info["tris_stored"] == 0, info
    # the C form: box `short` gets 3 entries fewer than it has members, every fourth box 2 more, beside k = 4 lists
    segs = overlap_ref.segments(f.csr)
    short = int(np.argmax((f.size >= 8) & (f.size <= 64)))
    assert 8 <= f.size[short] <= 64
    room = f.size + np.where(np.arange(N) % 4 == 0, 2, 0)
    room[short] = f.size[short] - 3
    off = np.zeros(N + 1, np.int64)
    np.cumsum(room, out=off[1:])
    lst = torch.full((int(off[-1]) + 5,), -77, dtype=torch.int32, device="cuda")
    tri = torch.full((N, 4), -77, dtype=torch.int32, device="cuda")
    count = torch.full((N,), -77, dtype=torch.int32, device="cuda")
    assert c_query(f.r, lo, hi, 4, 1, kernel, cuda(off, np.int32), tri, count, lst) == 0
    info = f.r.overlaps_info()
    want = f.want(4, count_all=True)
    np.testing.assert_array_equal(count.cpu().numpy(), f.size)  # count stays true, the short segment's too
    np.testing.assert_array_equal(tri.cpu().numpy(), want[0])
    got = lst.cpu().numpy()
    for i in range(N):
        seg = got[off[i]:off[i + 1]]
        if i == short:  # only that segment is written, all of it, with members of S_i, none twice
            assert len(seg) == f.size[i] - 3 and np.isin(seg, segs[i]).all() and len(np.unique(seg)) == len(seg)
        else:  # the first |S_i| entries are S_i as a set; the rest is not written
            assert np.array_equal(np.sort(seg[:f.size[i]]), segs[i]), i
            assert (seg[f.size[i]:] == -77).all(), i
    assert (got[off[-1]:] == -77).all()
    assert info["tris_listed"] == int(np.minimum(room, f.size).sum()) == len(f.csr[1]) - 3, info
    assert info["tris_counted"] == len(f.csr[1]) and info["tris_stored"] == int((want[0] >= 0).sum()), info


# ------------------------------------------------------------------ 4. special boxes, mixed into one call
def special_boxes(coords):
    """(lo, hi, kind, tri): point, line and plane boxes on vertices and faces, boxes that equal a triangle's corner box
    or touch it from outside, the whole-scene box, and invalid boxes -- interleaved, so that a wave holds every kind"""
    rec = overlap_ref.records(coords)
    tlo, thi = rec[5], rec[6]
    slo, shi = scene_box(coords)
    rows = np.arange(0, len(coords), max(len(coords) // 24, 1))[:24]
    one = np.float32(0.125)
    lo, hi, kind, tri = [], [], [], []

    def put(l, h, what, j=-1):
        lo.append(np.array(l, np.float32))
        hi.append(np.array(h, np.float32))
        kind.append(what)
        tri.append(j)

    bad = invalid_boxes(coords[rows[0], 0].copy())
    for n, j in enumerate(rows):
        v0, v1 = coords[j, 0], coords[j, 1]
        face = coords[j].astype(np.float64).mean(0).astype(np.float32)
        put(v0, v0, "point_v0", j)
        put(v1, v1, "point_v1", j)
        put(face, face, "point_face", j)
        put([slo[0], v0[1], v0[2]], [shi[0], v0[1], v0[2]], "line_vertex", j)        # along x through v0
        put([face[0], slo[1], face[2]], [face[0], shi[1], face[2]], "line_face", j)  # along y through the face
        put([slo[0], slo[1], v0[2]], [shi[0], shi[1], v0[2]], "plane_vertex", j)     # z = v0.z
        put([face[0], slo[1], slo[2]], [face[0], shi[1], shi[2]], "plane_face", j)   # x = the face's
        put(tlo[j], thi[j], "corner_box", j)                                         # closed: step 2 by equality
        put(tlo[j] - one, [tlo[j, 0], thi[j, 1] + one, thi[j, 2] + one], "touching", j)  # its face x = tlo.x, outside
        put(slo, shi, "scene")
        put(bad[0][n % len(bad[0])], bad[1][n % len(bad[0])], "invalid")
    return np.array(lo), np.array(hi), np.array(kind), np.array(tri)


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_special_boxes(fix, scene):
    f = fix[scene]
    lo, hi, kind, tj = special_boxes(f.coords)
    n, nt = len(lo), len(f.coords)
    csr = overlap_ref.sets(lo, hi, f.coords)
    size = np.diff(csr[0])
    segs = overlap_ref.segments(csr)
    # what the definition promises, on the yardstick: v0's point box and the corner box hold their triangle, the scene
    # box every triangle, an invalid box none
    for i in np.nonzero((kind == "point_v0") | (kind == "corner_box"))[0]:
        assert tj[i] in segs[i], (kind[i], tj[i])
    assert (size[kind == "scene"] == nt).all() and (size[kind == "invalid"] == 0).all()
    # (a point box at a float32 point of a face lies off the face's plane as a rule and reports nothing; at v1 it meets
    # fl(a + e1), a neighbouring float of v1: both are in the call for the yardstick to decide)
    for what in ("point_v1", "line_vertex", "line_face", "plane_vertex", "plane_face", "touching"):
        assert (size[kind == what] > 0).any(), what
    assert (size[kind == "plane_vertex"] > 16).any()
    valid = int((kind != "invalid").sum())
    for kernel in KERNELS:
        for k, count_all in ((16, True), (8, False), (0, True)):
            want = overlap_ref.answer(csr, k, count_all)
            got = query(f.r, lo, hi, k, kernel, count_all)
            check(got, want, size, what=(scene, kernel, k))
            check_path(got[2], kernel, valid, nt)
            if k:
                assert (got[0][kind == "invalid"] == -1).all() and (got[1][kind == "invalid"] == 0).all()
            if count_all:
                assert (got[1][kind == "scene"] == nt).all()
        off, tris = f.r.overlaps_csr(cuda(lo), cuda(hi), kernel=kernel)
        np.testing.assert_array_equal(off.cpu().numpy(), csr[0])
        np.testing.assert_array_equal(tris.cpu().numpy(), csr[1])


# ------------------------------------------------------------------ 5. box count edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_box_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    lo, hi = cuda(f.lo[:CHUNK + 1]), cuda(f.hi[:CHUNK + 1])
    for k in (4, 16):
        want = f.want(k)
        for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK + 1):
            tri = torch.full((n * k + 3,), -77, dtype=torch.int32, device="cuda")
            count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
            f.r.overlaps((lo.data_ptr(), n), hi.data_ptr(), k=k, kernel=kernel, tri=tri.data_ptr(),
                         count=count.data_ptr())  # (raw pointers: the buffers are longer)
            assert f.r.overlaps_info()["boxes"] == n
            tri, count = tri.cpu().numpy(), count.cpu().numpy()
            np.testing.assert_array_equal(tri[:n * k].reshape(n, k), want[0][:n], err_msg=str(n))
            assert np.array_equal(count[:n], want[1][:n]), n
            assert (tri[n * k:] == -77).all() and (count[n:] == -77).all(), n
    o, t = f.r.overlaps_csr(lo[:0], hi[:0], kernel=kernel)
    assert o.cpu().numpy().tolist() == [0] and t.numel() == 0
    o, t = f.r.overlaps_csr(lo[:1], hi[:1], kernel=kernel)
    assert np.array_equal(o.cpu().numpy(), f.csr[0][:2]) and np.array_equal(t.cpu().numpy(), f.csr[1][:f.csr[0][1]])


# ------------------------------------------------------------------ 6. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        for k, count_all in ((8, True), (0, True)):
            got = query(r, f.lo, f.hi, k, kernel, count_all)
            check(got, f.want(k, count_all), f.size, what=(accel, flags, kernel, k))
            check_path(got[2], kernel, N, len(f.coords), wide=accel != "reference")
    r.close()


# ------------------------------------------------------------------ 7. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_nearest.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="device"), both kernels answer as a fresh upload of the moved scene does and as the
    yardstick does on the moved coordinates (every second fixture box)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    lo, hi = f.lo[rows], f.hi[rows]
    csr = overlap_ref.sets(lo, hi, coords)
    size = np.diff(csr[0])
    want = overlap_ref.answer(csr, 8, True)
    still = f.want(8, True, rows=rows)
    assert (want[1] != still[1]).sum() > 100 and (want[1] > 8).sum() > 50 and (want[1] == 0).sum() > 50
    t = s.triangles
    moved = host.Scene(host.triangle_init(coords, t["ks"], t["kd"], t["kr"]), s.lights.copy())
    fresh = dev.Renderer(0).upload(moved.build_bvh(3))
    for kernel in KERNELS:
        check(query(fresh, lo, hi, 8, kernel, True), want, size, what=("fresh", kernel))
    fresh.close()
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    check(query(r, lo, hi, 8, "fast", True), still, f.size[rows], what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            got = query(r, lo, hi, 8, kernel, True)
            check(got, want, size, what=(step, kernel))
        assert got[2]["walked_boxes"] == len(rows)
        off, tris = r.overlaps_csr(cuda(lo), cuda(hi))
        assert np.array_equal(off.cpu().numpy(), csr[0]) and np.array_equal(tris.cpu().numpy(), csr[1]), step
    r.close()


# ------------------------------------------------------------------ 8. isolation
def test_an_overlap_query_leaves_renders_and_neighbour_queries_alone(dev, scenes, fix):
    import torch
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    pts = cuda(f.coords[::97, 0])
    lo, hi = cuda(f.lo), cuda(f.hi)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def neighbours(r):
        out = r.nearest_tris(pts, k=8, points_out=True)
        info = r.neighbours_info()
        return [x.cpu().numpy() for x in out], info

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    frame0, stats0 = r.download(hit=True), r.stats()
    nb0, ni0 = neighbours(r)
    for kernel, k, count_all in (("fast", 16, False), ("strict", 4, True), ("fast", 0, True)):
        r.overlaps(lo, hi, k=k, kernel=kernel, count_all=count_all)
        oi = r.overlaps_info()
        assert oi["boxes"] == N
    r.overlaps_csr(lo[:300], hi[:300])
    oi = r.overlaps_info()
    frame1 = r.download(hit=True)
    assert same_bits(frame0[0], frame1[0]) and np.array_equal(frame0[1], frame1[1]) and r.stats() == stats0
    ni = r.neighbours_info()  # the neighbours query's counters as they were
    assert strip(ni) == strip(ni0) and abs(ni["kernel_ms"] - ni0["kernel_ms"]) < 1e-4
    nb1, ni1 = neighbours(r)  # ... and the same query again: the same bits
    for a, b in zip(nb0, nb1):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert strip(ni1) == strip(ni0)
    r.render(cam, W, H, kernel="fast", hit=hit)
    assert r.sync() > 0
    frame2 = r.download(hit=True)
    assert same_bits(frame0[0], frame2[0]) and np.array_equal(frame0[1], frame2[1])
    oj = r.overlaps_info()  # ... and neither touched the overlap query's own counters
    assert strip(oj) == strip(oi) and abs(oj["kernel_ms"] - oi["kernel_ms"]) < 1e-4
    r.close()


# ------------------------------------------------------------------ 9. errors
def test_overlap_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    lo, hi = cuda(f.lo), cuda(f.hi)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.overlaps(lo, hi)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no overlap query run yet
        r.overlaps_info()
    r.overlaps(lo[:100], hi[:100], k=4)
    info = r.overlaps_info()
    assert info["boxes"] == 100 and info["tris_stored"] == int(np.minimum(f.size[:100], 4).sum())
    with pytest.raises(dev.RtError, match="status -1"):
        r.overlaps(lo, hi, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.overlaps((0, 16), hi.data_ptr())  # null lo
    L = _lib.hip()
    tri = torch.empty(16 * 16, dtype=torch.int32, device="cuda")
    cnt = torch.empty(16, dtype=torch.int32, device="cuda")
    off = torch.zeros(17, dtype=torch.int32, device="cuda")
    l, h, t, c, o = lo.data_ptr(), hi.data_ptr(), tri.data_ptr(), cnt.data_ptr(), off.data_ptr()
    Q, R = _lib.Boxes, _lib.OverlapResults
    for q, res in [
        (Q(None, h, None, 16, 4, 0, 0), R(t, c, None)),    # null lo, null hi
        (Q(l, None, None, 16, 4, 0, 0), R(t, c, None)),
        (Q(l, h, None, 16, -1, 0, 0), R(t, c, None)),      # max_tris outside 0..16
        (Q(l, h, None, 16, 17, 0, 0), R(t, c, None)),
        (Q(l, h, None, 16, 4, 0, 0), R(None, c, None)),    # max_tris > 0 without tri
        (Q(l, h, None, 16, 0, 0, 0), R(t, c, None)),       # max_tris = 0 without count_all ...
        (Q(l, h, None, 16, 0, 1, 0), R(t, None, None)),    # ... or without a count pointer
        (Q(l, h, None, 16, 4, 2, 0), R(t, c, None)),       # count_all not 0 / 1
        (Q(l, h, None, 16, 4, -1, 0), R(t, c, None)),
        (Q(l, h, None, 16, 4, 0, 3), R(t, c, None)),       # unknown kernel
        (Q(l, h, None, 16, 4, 0, -1), R(t, c, None)),
        (Q(l, h, None, -1, 4, 0, 0), R(t, c, None)),       # negative n
        (Q(l, h, o, 16, 4, 0, 0), R(t, c, None)),          # offsets without list
        (Q(l, h, None, 16, 4, 0, 0), R(t, c, t)),          # list without offsets
        (Q(l, h, o, 0, 4, 0, 0), R(t, c, None)),           # ... at n = 0 too
    ]:
        assert L.rt_overlap_boxes(r._ctx, ctypes.byref(q), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_overlap_boxes(r._ctx, None, None) == -1
    assert L.rt_overlap_boxes(r._ctx, ctypes.byref(Q(l, h, None, 16, 4, 0, 0)), None) == -1
    after = r.overlaps_info()  # a refused call leaves overlaps_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_overlap_boxes(r._ctx, ctypes.byref(Q(None, None, None, 0, 4, 0, 0)), ctypes.byref(R(None, None, None))) == 0
    assert r.overlaps_info()["boxes"] == 0
    r.close()
