"""Cut queries (rt_cut_triangles: Renderer.cuts / cuts_csr / cuts_info) against tests/cut_ref.py, the numpy float32
restatement of the triangle-triangle test X and its cut segment, which tests/test_cut_abi.py holds against float64 on
the CPU. A query's answer is a set of triangle indices in index order, a count and one segment per member, so every
comparison is array_equal (segments by their bits) and no case is excluded. Per scene the queries are 512 from
cut_ref.surface_tris plus 128 faces of the other scene's mesh; their full sets are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import cut_ref
from tests.nearest_ref import same_bits

pytestmark = pytest.mark.gpu

KERNELS = ["strict", "fast"]
KERNEL_ID = {"auto": 0, "strict": 1, "fast": 2}
W, H = 64, 36
NS, NF = 512, 128
N = NS + NF
CHUNK = 256  # QUERY_CHUNK (rt_query.hpp)
OTHER = {"car_boxed": "car_only", "car_only": "car_boxed"}


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


def fixture_tris(coords, other, seed):
    faces = other[np.linspace(0, len(other) - 1, NF).astype(np.int64)]
    return np.concatenate([cut_ref.surface_tris(coords, NS, seed), faces]).astype(np.float32)


def query(r, q, k, kernel, count_all=False):
    """(tri, count, info)"""
    tri, count = r.cuts(cuda(q), k=k, kernel=kernel, count_all=count_all)
    info = r.cuts_info()
    return tri.cpu().numpy(), count.cpu().numpy(), info


def check(got, want, size, what="", listed=0):
    """the answer, and the info counters against it (size: |S_i| per query)"""
    tri, count, info = got
    np.testing.assert_array_equal(count, want[1], err_msg=str(what))
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    assert info["triangles"] == len(tri) and info["stack_overflows"] == 0, (what, info)
    assert info["stored"] == int((want[0] >= 0).sum()) and info["counted"] == int(want[1].sum()), (what, info)
    assert info["found"] + info["empty"] == len(tri), (what, info)
    assert info["found"] == int((size > 0).sum()) and info["listed"] == listed, (what, info)


def check_path(info, kernel, valid, n_tris, wide=True):
    """which loop served the queries: the walk under "fast" on a scene with a wide view, else the exhaustive loop"""
    assert info["walked"] + info["exhaustive"] == valid, info
    if kernel == "fast" and wide:
        assert info["walked"] == valid and info["exhaustive"] == 0, info
        assert (info["nodes_visited"] > 0) == (valid > 0), info
    else:
        assert info["exhaustive"] == valid and info["walked"] == 0, info
        assert info["pairs_tested"] == valid * n_tris and info["nodes_visited"] == 0, info


class Fix:
    """one fixture scene: a Renderer, the N queries and the yardstick's full sets and segments for them"""

    def __init__(self, dev, scene, other, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.q = fixture_tris(self.coords, other.triangles["coords"], seed)
        self.off, self.idx, self.seg = cut_ref.sets(self.q, self.coords)
        self.csr = (self.off, self.idx)
        self.size = np.diff(self.off)

    def want(self, k, count_all=False, rows=None):
        return cut_ref.answer(self.csr, k, count_all, rows)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, scenes[OTHER[name]], 51 + k) for k, (name, s) in enumerate(scenes.items())}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture queries, every k, both orders
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_queries(fix, scene, kernel):
    f = fix[scene]
    regimes = int((f.size == 0).sum()), int(((f.size >= 1) & (f.size <= 16)).sum()), int((f.size > 16).sum())
    print(f"{scene}: |S_i| = 0: {regimes[0]}, 1..16: {regimes[1]}, > 16: {regimes[2]} queries; max {int(f.size.max())}")
    assert min(regimes) >= 20  # the empty answer, the short list and the cut at k are all exercised
    p = np.random.default_rng(11).permutation(N)
    for k, count_all in ((0, True), (1, False), (1, True), (4, False), (4, True), (8, False), (8, True), (16, False),
                         (16, True)):
        for order in (np.arange(N), p):
            got = query(f.r, f.q[order], k, kernel, count_all)
            check(got, f.want(k, count_all, rows=order), f.size[order], what=(scene, kernel, k, count_all, order[0]))
            check_path(got[2], kernel, N, len(f.coords))
            if count_all:
                assert np.array_equal(got[1], f.size[order])
        if kernel == "fast":  # the walk prunes: fewer tests than the exhaustive loop's by far
            assert got[2]["pairs_tested"] < N * len(f.coords) / 4, got[2]


# ------------------------------------------------------------------ 2. the list form
def c_query(r, q, k, count_all, kernel, offsets=None, tri=None, count=None, lst=None, seg=None, n=None):
    """rt_cut_triangles itself, on torch tensors or None -> the status"""
    from prt import _lib
    ptr = lambda x: None if x is None else x.data_ptr()
    t = _lib.Tris(ptr(q), ptr(offsets), (0 if q is None else len(q)) if n is None else n, k, count_all,
                  KERNEL_ID[kernel])
    res = _lib.CutResults(ptr(tri), ptr(count), ptr(lst), ptr(seg))
    return _lib.hip().rt_cut_triangles(r._ctx, ctypes.byref(t), ctypes.byref(res))


def csr_of(r, q, kernel):
    off, idx, seg = r.cuts_csr(cuda(q), kernel=kernel)
    return off.cpu().numpy(), idx.cpu().numpy(), seg.cpu().numpy()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_csr(fix, scene, kernel):
    import torch
    f = fix[scene]
    q = cuda(f.q)
    off, idx, seg = f.r.cuts_csr(q, kernel=kernel)
    assert off.dtype == idx.dtype == torch.int32 and seg.dtype == torch.float32 and seg.shape == (len(f.idx), 2, 3)
    np.testing.assert_array_equal(off.cpu().numpy(), f.off)
    np.testing.assert_array_equal(idx.cpu().numpy(), f.idx)
    assert same_bits(seg.cpu().numpy(), f.seg)
    info = f.r.cuts_info()
    assert info["listed"] == info["counted"] == len(f.idx) and info["stored"] == 0, info
    off2, idx2, none = f.r.cuts_csr(q, segments=False, kernel=kernel)  # the indices alone
    assert none is None and np.array_equal(off2.cpu().numpy(), f.off) and np.array_equal(idx2.cpu().numpy(), f.idx)
    # the C form: query `short` gets 3 entries fewer than it has members, every fourth query 2 more, beside k = 4 lists;
    # 5 guard entries follow every output
    segs = cut_ref.segments(f.csr)
    short = int(np.argmax((f.size >= 8) & (f.size <= 64)))
    assert 8 <= f.size[short] <= 64
    room = f.size + np.where(np.arange(N) % 4 == 0, 2, 0)
    room[short] = f.size[short] - 3
    o = np.zeros(N + 1, np.int64)
    np.cumsum(room, out=o[1:])
    lst = torch.full((int(o[-1]) + 5,), -77, dtype=torch.int32, device="cuda")
    sg = torch.full((int(o[-1]) + 5, 2, 3), -77.0, dtype=torch.float32, device="cuda")
    tri = torch.full((N * 4 + 5,), -77, dtype=torch.int32, device="cuda")
    count = torch.full((N + 5,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert c_query(f.r, q, 4, 1, kernel, cuda(o, np.int32), tri, count, lst, sg) == 0
    info = f.r.cuts_info()
    want = f.want(4, count_all=True)
    count, tri, got, gseg = count.cpu().numpy(), tri.cpu().numpy(), lst.cpu().numpy(), sg.cpu().numpy()
    np.testing.assert_array_equal(count[:N], f.size)  # count stays true, the short segment's too
    np.testing.assert_array_equal(tri[:4 * N].reshape(N, 4), want[0])
    assert (count[N:] == -77).all() and (tri[4 * N:] == -77).all()
    for i in range(N):
        s, sseg = got[o[i]:o[i + 1]], gseg[o[i]:o[i + 1]]
        m = int(min(f.size[i], room[i]))
        if i == short:  # all of the segment is written, with members of S_i, none twice
            assert len(s) == f.size[i] - 3 and np.isin(s, segs[i]).all() and len(np.unique(s)) == len(s)
        else:  # the first |S_i| entries are S_i as a set; the rest is not written
            assert np.array_equal(np.sort(s[:m]), segs[i]), i
            assert (s[m:] == -77).all() and (sseg[m:] == -77.0).all(), i
        at = f.off[i] + np.searchsorted(segs[i], s[:m])  # every written entry has its own member's segment beside it
        assert same_bits(sseg[:m], f.seg[at]), i
    assert (got[o[-1]:] == -77).all() and (gseg[o[-1]:] == -77.0).all()
    assert info["listed"] == int(np.minimum(room, f.size).sum()) == len(f.idx) - 3, info
    assert info["counted"] == len(f.idx) and info["stored"] == int((want[0] >= 0).sum()), info
    # a list without segments
    lst2 = torch.full((int(o[-1]) + 5,), -77, dtype=torch.int32, device="cuda")
    cnt2 = torch.full((N,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert c_query(f.r, q, 0, 1, kernel, cuda(o, np.int32), None, cnt2, lst2, None) == 0
    assert f.r.cuts_info()["listed"] == len(f.idx) - 3 and np.array_equal(cnt2.cpu().numpy(), f.size)
    got2 = lst2.cpu().numpy()
    for i in range(0, N, 7):
        m = int(min(f.size[i], room[i]))
        assert np.isin(got2[o[i]:o[i] + m], segs[i]).all() and (got2[o[i] + m:o[i + 1]] == -77).all(), i
    assert (got2[o[-1]:] == -77).all()


# ------------------------------------------------------------------ 3. fast against strict
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fast_equals_strict_on_every_output(fix, scene):
    f = fix[scene]
    a, b = (query(f.r, f.q, 16, kernel, True) for kernel in KERNELS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    same = ("triangles", "found", "stored", "counted", "listed", "empty", "stack_overflows")
    assert {k: a[2][k] for k in same} == {k: b[2][k] for k in same}
    ca, cb = (csr_of(f.r, f.q, kernel) for kernel in KERNELS)
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and same_bits(ca[2], cb[2])


# ------------------------------------------------------------------ 4. every triangle twice
def test_a_doubled_scene_doubles_every_count(dev, scenes, fix):
    f = fix["car_only"]
    s = scenes["car_only"]
    t = s.triangles
    twice = lambda x: np.ascontiguousarray(np.concatenate([x, x]))
    n = len(f.coords)
    doubled = host.Scene(host.triangle_init(twice(t["coords"]), twice(t["ks"]), twice(t["kd"]), twice(t["kr"])),
                         s.lights.copy())
    r = dev.Renderer(0).upload(doubled.build_bvh(3))
    for kernel in KERNELS:
        tri, count, info = query(r, f.q, 16, kernel, True)
        np.testing.assert_array_equal(count, 2 * f.size)
        assert info["counted"] == 2 * int(f.size.sum()) and info["stack_overflows"] == 0
        off, idx, seg = csr_of(r, f.q, kernel)
        np.testing.assert_array_equal(off, 2 * f.off)
        for i in range(0, N, 5):  # S_i, then S_i again n higher, with the same segments
            a, b = f.off[i], f.off[i + 1]
            want = np.concatenate([f.idx[a:b], f.idx[a:b] + n])
            assert np.array_equal(idx[2 * a:2 * b], want), i
            assert same_bits(seg[2 * a:2 * b], np.concatenate([f.seg[a:b], f.seg[a:b]])), i
    r.close()


# ------------------------------------------------------------------ 5. special queries, mixed into one call
def special_tris(coords):
    """(q, kind): queries with a NaN or an infinity in each of the nine positions, zero-area queries, queries equal to a
    mesh face, triangles whose corner box spans the whole scene box, and coordinates of 1e30 -- interleaved, so that a
    wave holds every kind"""
    v = coords.reshape(-1, 3).astype(np.float64)
    ctr, ext = (v.min(0) + v.max(0)) / 2, float((v.max(0) - v.min(0)).max())
    rows = np.arange(0, len(coords), max(len(coords) // 27, 1))[:27]
    big = 1e30
    q, kind = [], []

    def put(t, what):
        q.append(np.array(t, np.float64).astype(np.float32))
        kind.append(what)

    for n, j in enumerate(rows):
        face = coords[j].astype(np.float64)
        mid, nrm = face.mean(0), np.cross(face[1] - face[0], face[2] - face[0])
        nrm = nrm / max(np.linalg.norm(nrm), 1e-30)
        through = np.array([mid - 0.01 * ext * nrm, mid + 0.01 * ext * nrm + 0.003 * ext, mid + 0.02 * ext * nrm])
        bad = through.copy()
        bad.reshape(-1)[n % 9] = (np.nan, np.inf, -np.inf)[n // 9]
        put(bad, "invalid")
        put(through, "through")
        up = np.array([0, 0, 0.01 * ext])
        put([mid - up, mid + up, mid], "needle")   # zero area: collinear corners, f1 x f2 = 0 exactly
        put([through[0], through[0], through[2]], "repeated")                    # ... a repeated corner
        put([mid, mid, mid], "point")
        put(face, "face")                                                         # a query equal to a mesh face
        tilt = (n % 3 - 1) * 0.3 * ext
        put([ctr + [-4 * ext, -4 * ext, -2 * ext + tilt], ctr + [4 * ext, -4 * ext, 2 * ext + tilt],
             ctr + [0, 4 * ext, tilt]], "scene")                                  # its corner box holds the scene's
        put([[big, big, big], [big, 0.5 * big, big], [0.5 * big, big, big]], "far")
        put([through[0], through[1], [big, 0, 0]], "long")                        # one corner at 1e30
        put([[-big, -big, tilt], [big, -big, tilt], [0, big, tilt]], "huge")      # every corner, around the scene
    return np.array(q), np.array(kind)


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_special_queries(fix, scene):
    f = fix[scene]
    q, kind = special_tris(f.coords)
    nt = len(f.coords)
    off, idx, seg = cut_ref.sets(q, f.coords)
    csr, size = (off, idx), np.diff(off)
    # what the definition promises, on the yardstick
    assert len(q) == 270 and (cut_ref.valid_tris(q) == (kind != "invalid")).all()
    for what in ("invalid", "needle", "repeated", "point", "far"):
        assert (size[kind == what] == 0).all(), what
    assert (size[kind == "through"] > 0).all() and (size[kind == "scene"] > 16).any()
    print(f"{scene}: |S_i| sums by kind: " + ", ".join(f"{w} {int(size[kind == w].sum())}" for w in np.unique(kind)) +
          f"; {int(np.isnan(seg).any(axis=(1, 2)).sum())} of {len(seg)} segments hold a NaN")
    valid = int((kind != "invalid").sum())
    for kernel in KERNELS:
        for k, count_all in ((16, True), (8, False), (0, True)):
            want = cut_ref.answer(csr, k, count_all)
            got = query(f.r, q, k, kernel, count_all)
            check(got, want, size, what=(scene, kernel, k))
            check_path(got[2], kernel, valid, nt)
            if k:
                assert (got[0][kind == "invalid"] == -1).all() and (got[1][kind == "invalid"] == 0).all()
        o, i, s = csr_of(f.r, q, kernel)
        np.testing.assert_array_equal(o, off)
        np.testing.assert_array_equal(i, idx)
        assert same_bits(s, seg)


# ------------------------------------------------------------------ 6. query count edges
@pytest.mark.parametrize("kernel", KERNELS)
def test_query_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    top = 2 * CHUNK + 1
    q = cuda(f.q[:top])
    for k in (4, 16):
        want = f.want(k)
        for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK + 1, top):
            tri = torch.full((n * k + 3,), -77, dtype=torch.int32, device="cuda")
            count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            f.r.cuts((q.data_ptr(), n), k=k, kernel=kernel, tri=tri.data_ptr(),
                     count=count.data_ptr())  # (raw pointers: the buffers are longer)
            assert f.r.cuts_info()["triangles"] == n
            tri, count = tri.cpu().numpy(), count.cpu().numpy()
            np.testing.assert_array_equal(tri[:n * k].reshape(n, k), want[0][:n], err_msg=str(n))
            assert np.array_equal(count[:n], want[1][:n]), n
            assert (tri[n * k:] == -77).all() and (count[n:] == -77).all(), n
    o, t, s = f.r.cuts_csr(q[:0], kernel=kernel)
    assert o.cpu().numpy().tolist() == [0] and t.numel() == 0 and tuple(s.shape) == (0, 2, 3)
    o, t, s = f.r.cuts_csr(q[:1], kernel=kernel)
    assert np.array_equal(o.cpu().numpy(), f.off[:2]) and np.array_equal(t.cpu().numpy(), f.idx[:f.off[1]])
    assert same_bits(s.cpu().numpy(), f.seg[:f.off[1]])


# ------------------------------------------------------------------ 7. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        for k, count_all in ((8, True), (0, True)):
            got = query(r, f.q, k, kernel, count_all)
            check(got, f.want(k, count_all), f.size, what=(accel, flags, kernel, k))
            check_path(got[2], kernel, N, len(f.coords), wide=accel != "reference")
    off, idx, seg = csr_of(r, f.q, "fast")
    assert np.array_equal(off, f.off) and np.array_equal(idx, f.idx) and same_bits(seg, f.seg)
    r.close()


# ------------------------------------------------------------------ 8. moving scene
def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_overlap.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="device"), both kernels answer as a fresh upload of the moved scene does and as the
    yardstick does on the moved coordinates (every second fixture query)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    q = f.q[rows]
    off, idx, seg = cut_ref.sets(q, coords)
    csr, size = (off, idx), np.diff(off)
    want = cut_ref.answer(csr, 8, True)
    still = f.want(8, True, rows=rows)
    assert (want[1] != still[1]).sum() > 100 and (want[1] > 0).sum() > 20
    t = s.triangles
    moved = host.Scene(host.triangle_init(coords, t["ks"], t["kd"], t["kr"]), s.lights.copy())
    fresh = dev.Renderer(0).upload(moved.build_bvh(3))
    for kernel in KERNELS:
        check(query(fresh, q, 8, kernel, True), want, size, what=("fresh", kernel))
    fresh.close()
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    check(query(r, q, 8, "fast", True), still, f.size[rows], what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            got = query(r, q, 8, kernel, True)
            check(got, want, size, what=(step, kernel))
        assert got[2]["walked"] == len(rows)
        o, i, sg = csr_of(r, q, "fast")
        assert np.array_equal(o, off) and np.array_equal(i, idx) and same_bits(sg, seg), step
    r.close()


# ------------------------------------------------------------------ 9. isolation
def test_a_cut_query_leaves_renders_and_other_queries_alone(dev, scenes, fix):
    import torch
    from prt import rays
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    pts = cuda(f.coords[::97, 0])
    o, p = rays.pinhole(cam, W, H)
    lo, hi = (pts - 0.05).contiguous(), (pts + 0.05).contiguous()
    d = torch.zeros_like(pts)
    d[:, 1] = -1.0
    far = torch.full((o.shape[0],), 1e30, dtype=torch.float32, device="cuda")
    q = cuda(f.q)
    torch.cuda.synchronize()  # (these tensors are torch's work; the queries run on the renderer's stream)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def infos_of(r):
        return [r.query_info(), r.shade_info(), r.nearest_info(), r.neighbours_info(), r.overlaps_info(),
                r.hits_info(), r.sweep_info()]

    def others(r):
        occ = r.occluded(o, p, far)
        hit, t = r.trace_rays(o, p)
        rgb = r.shade_rays(o, p)
        near = r.nearest(pts)
        nb = r.nearest_tris(pts, k=4)
        ov = r.overlaps(lo, hi, k=4)
        hits = r.trace_hits(o, p, max_hits=2)
        sw = r.sweep(pts, d, 0.01)
        r.sync()
        out = [x.cpu().numpy() for x in (occ, hit, t, rgb, *near, *nb[:3], *ov, *hits, *sw)]
        return out, infos_of(r)

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    frame0, stats0, launch0 = r.download(hit=True), r.stats(), r.launch_info()
    out0, infos0 = others(r)
    for kernel, k, count_all in (("fast", 16, False), ("strict", 4, True), ("fast", 0, True)):
        r.cuts(q, k=k, kernel=kernel, count_all=count_all)
        ci = r.cuts_info()
        assert ci["triangles"] == N
    r.cuts_csr(q[:300])
    ci = r.cuts_info()
    frame1 = r.download(hit=True)
    assert same_bits(frame0[0], frame1[0]) and np.array_equal(frame0[1], frame1[1]) and r.stats() == stats0
    assert r.launch_info() == launch0
    for a, b in zip(infos_of(r), infos0):  # the other queries' counters as they were
        assert strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4
    out1, infos1 = others(r)  # ... and the same queries again: the same bits
    for a, b in zip(out0, out1):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in zip(infos1, infos0):
        assert strip(a) == strip(b)
    r.render(cam, W, H, kernel="fast", hit=hit)
    assert r.sync() > 0
    frame2 = r.download(hit=True)
    assert same_bits(frame0[0], frame2[0]) and np.array_equal(frame0[1], frame2[1])
    cj = r.cuts_info()  # ... and none of them touched the cut query's own counters
    assert strip(cj) == strip(ci) and abs(cj["kernel_ms"] - ci["kernel_ms"]) < 1e-4
    r.close()


# ------------------------------------------------------------------ 10. errors
def test_cut_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    q = cuda(f.q)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.cuts(q)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no cut query run yet
        r.cuts_info()
    r.cuts(q[:100], k=4)
    info = r.cuts_info()
    assert info["triangles"] == 100 and info["stored"] == int(np.minimum(f.size[:100], 4).sum())
    with pytest.raises(dev.RtError, match="status -1"):
        r.cuts(q, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.cuts((0, 16))  # null tris
    L = _lib.hip()
    tri = torch.empty(16 * 16, dtype=torch.int32, device="cuda")
    cnt = torch.empty(16, dtype=torch.int32, device="cuda")
    off = torch.zeros(17, dtype=torch.int32, device="cuda")
    seg = torch.empty((16, 2, 3), dtype=torch.float32, device="cuda")
    p, t, c, o, s = q.data_ptr(), tri.data_ptr(), cnt.data_ptr(), off.data_ptr(), seg.data_ptr()
    Q, R = _lib.Tris, _lib.CutResults
    for t_, res in [
        (Q(None, None, 16, 4, 0, 0), R(t, c, None, None)),   # null tris
        (Q(p, None, 16, -1, 0, 0), R(t, c, None, None)),     # max_tris outside 0..16
        (Q(p, None, 16, 17, 0, 0), R(t, c, None, None)),
        (Q(p, None, 16, 4, 0, 0), R(None, c, None, None)),   # max_tris > 0 without tri
        (Q(p, None, 16, 0, 0, 0), R(t, c, None, None)),      # max_tris = 0 without count_all ...
        (Q(p, None, 16, 0, 1, 0), R(t, None, None, None)),   # ... or without a count pointer
        (Q(p, None, 16, 4, 2, 0), R(t, c, None, None)),      # count_all not 0 / 1
        (Q(p, None, 16, 4, -1, 0), R(t, c, None, None)),
        (Q(p, None, 16, 4, 0, 3), R(t, c, None, None)),      # unknown kernel
        (Q(p, None, 16, 4, 0, -1), R(t, c, None, None)),
        (Q(p, None, -1, 4, 0, 0), R(t, c, None, None)),      # negative n
        (Q(p, o, 16, 4, 0, 0), R(t, c, None, None)),         # offsets without list
        (Q(p, None, 16, 4, 0, 0), R(t, c, t, None)),         # list without offsets
        (Q(p, o, 0, 4, 0, 0), R(t, c, None, None)),          # ... at n = 0 too
        (Q(p, None, 16, 4, 0, 0), R(t, c, None, s)),         # list_seg without list
        (Q(p, None, 0, 4, 0, 0), R(t, c, None, s)),          # ... at n = 0 too
    ]:
        assert L.rt_cut_triangles(r._ctx, ctypes.byref(t_), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_cut_triangles(r._ctx, None, None) == -1
    assert L.rt_cut_triangles(r._ctx, ctypes.byref(Q(p, None, 16, 4, 0, 0)), None) == -1
    after = r.cuts_info()  # a refused call leaves cuts_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_cut_triangles(r._ctx, ctypes.byref(Q(None, None, 0, 4, 0, 0)),
                              ctypes.byref(R(None, None, None, None))) == 0
    assert r.cuts_info()["triangles"] == 0
    r.close()
