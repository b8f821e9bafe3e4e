"""Clearance queries (rt_clearance_triangles: Renderer.clearance / clearance_info) against tests/clearance_ref.py, the
numpy float32 restatement of D, the pair of points and the winning candidate, which tests/test_clearance_abi.py holds
against float64 on the CPU. A query's answer is the first triangle by (D, original index), so every comparison is bit
for bit (same_bits on d2 and both points, array_equal on tri and kind) and no case is excluded. Per scene the queries
are the 256 of clearance_ref.fixture_tris; the expectations are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import clearance_ref as cr
from tests import cut_ref
from tests.clearance_ref import same_bits

pytestmark = pytest.mark.gpu

FMAX = cr.FMAX
KERNELS = ["strict", "fast"]
KERNEL_ID = {"auto": 0, "strict": 1, "fast": 2}
W, H = 64, 36
N = 256
SEED = {"car_only": 71, "car_boxed": 72}  # (tests/test_clearance_abi.py's: the fixtures held against float64)


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


def query(r, q, kernel, md=None):
    """(tri, d2, on_query, on_mesh, kind, info)"""
    import torch
    kind = torch.empty(len(q), dtype=torch.int32, device="cuda")
    out = r.clearance(cuda(q), max_dist2=None if md is None else cuda(md), kernel=kernel, kind=kind)
    info = r.clearance_info()
    return tuple(x.cpu().numpy() for x in (*out, kind)) + (info,)


def check(got, want, what=""):
    tri, d2, oq, om, kind, info = got
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    np.testing.assert_array_equal(kind, want[4], err_msg=str(what))
    assert same_bits(d2, want[1]), what
    assert same_bits(oq, want[2]) and same_bits(om, want[3]), what
    found = int((want[0] >= 0).sum())
    assert info["triangles"] == len(tri) and info["found"] == found and info["empty"] == len(tri) - found, (what, info)
    assert info["stack_overflows"] == 0


def check_path(info, kernel, valid, n_tris, wide=True):
    """which loop served the queries: the walk under "fast" on a scene with a wide view, else the exhaustive loop"""
    assert info["walked"] + info["exhaustive"] == valid, info
    if kernel == "fast" and wide:
        assert info["walked"] == valid and info["exhaustive"] == 0, info
        assert (info["nodes_visited"] > 0) == (valid > 0), info
    else:
        assert info["exhaustive"] == valid and info["walked"] == 0, info
        assert info["pairs_tested"] == valid * n_tris and info["nodes_visited"] == 0 and info["pairs_gated"] == 0, info


class Fix:
    """one fixture scene: a Renderer, its 256 queries and the mirror's expectation for them"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.q = cr.fixture_tris(self.coords, N, seed)
        self.want = cr.expected(self.q, self.coords)
        self.tri, self.d2, self.oq, self.om, self.kind, self.ties = self.want

    def rows(self, rows):
        return tuple(x[rows] for x in self.want)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, SEED[name]) for name, s in scenes.items()}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture queries, both kernels, both orders
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_queries(fix, scene, kernel):
    f = fix[scene]
    groups = [int((f.kind == 15).sum()), int((f.kind <= 2).sum()), int(((f.kind >= 3) & (f.kind <= 5)).sum()),
              int(((f.kind >= 6) & (f.kind <= 14)).sum())]
    assert (f.tri >= 0).all() and groups[0] >= 32 and groups[1] >= 32 and groups[2] >= 32 and groups[3] >= 16, groups
    assert int((f.ties >= 2).sum()) >= 50  # exact ties at the minimum: the index rule decides on ordinary input
    p = np.random.default_rng(11).permutation(N)
    for order in (np.arange(N), p):
        got = query(f.r, f.q[order], kernel)
        check(got, f.rows(order), what=(scene, kernel, order[0]))
        check_path(got[5], kernel, N, len(f.coords))


# ------------------------------------------------------------------ 2. ties take the lower index
def test_ties_take_the_lower_index(dev, fix):
    base = host.Scene.named("car_only")
    t = base.triangles
    n = len(t)
    f = fix["car_only"]
    q = f.q[::4]
    doubled = host.Scene(np.concatenate([t, t]), base.lights).build_bvh(3)
    mirrored = host.Scene(np.concatenate([t[::-1], t]), base.lights).build_bvh(3)
    for name, s in (("doubled", doubled), ("copy first, reversed", mirrored)):
        want = cr.expected(q, s.triangles["coords"])
        assert (want[0] >= 0).all() and (want[5] >= 2).all()  # every minimum is shared now
        r = dev.Renderer(0).upload(s)
        for kernel in KERNELS:
            got = query(r, q, kernel)
            check(got, want, what=(name, kernel))
            assert same_bits(got[1], f.d2[::4])  # the single scene's bits
            if name == "doubled":
                assert (got[0] < n).all() and np.array_equal(got[0], f.tri[::4])
                assert np.array_equal(got[4], f.kind[::4]) and same_bits(got[2], f.oq[::4])
        r.close()


# ------------------------------------------------------------------ 3. bounds, invalid queries, counts
@pytest.mark.parametrize("kernel", KERNELS)
def test_bounds(fix, kernel):
    f = fix["car_only"]
    k = np.arange(N) % 7
    md = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5],
                   [np.float32(np.inf), f.d2, np.nextafter(f.d2, np.float32(-np.inf)), np.float32(0), np.float32(-1.0),
                    np.float32(np.nan)], np.float32(-0.0)).astype(np.float32)
    want = cr.expected(f.q, f.coords, md)
    found = want[0] >= 0
    assert found[k == 0].all() and found[k == 1].all() and not found[k == 2].any()  # the bound is inclusive, to the bit
    assert np.array_equal(found[k == 3], f.d2[k == 3] == 0) and found[k == 3].any() and not found[k == 3].all()
    assert not found[k == 4].any() and not found[k == 5].any() and np.array_equal(found[k == 6], f.d2[k == 6] == 0)
    for a, b in zip(want[:5], f.want[:5]):
        assert np.array_equal(a[found].view(np.int32), b[found].view(np.int32))
    got = query(f.r, f.q, kernel, md)
    check(got, want, what="bounds")
    tri, d2, oq, om, kind, info = got
    assert (tri[~found] == -1).all() and (d2[~found] == FMAX).all() and (kind[~found] == -1).all()
    assert same_bits(oq[~found], f.q[~found, 0]) and same_bits(om[~found], f.q[~found, 0])
    valid = cr.valid_queries(f.q, md)
    assert not valid[(k == 4) | (k == 5)].any() and valid[k < 2].all()
    check_path(info, kernel, int(valid.sum()), len(f.coords))


def test_non_finite_corners_in_a_batch(fix):
    f = fix["car_boxed"]
    q = f.q[:162].copy()
    for i in range(27):  # every one of the nine numbers as NaN, +inf and -inf, five good queries between each
        q[6 * i].reshape(-1)[i % 9] = (np.nan, np.inf, -np.inf)[i // 9]
    bad = ~np.isfinite(q).all(axis=(1, 2))
    assert bad.sum() == 27
    want = cr.expected(q, f.coords)
    assert (want[0][bad] == -1).all() and same_bits(want[2][bad], q[bad, 0]) and same_bits(want[3][bad], q[bad, 0])
    for a, b in zip(want[:5], f.want[:5]):
        assert np.array_equal(a[~bad].view(np.int32), b[:162][~bad].view(np.int32))
    for kernel in KERNELS:
        got = query(f.r, q, kernel)
        check(got, want, what=kernel)
        check_path(got[5], kernel, 162 - 27, len(f.coords))
        assert got[5]["empty"] == 27


@pytest.mark.parametrize("kernel", KERNELS)
def test_query_count_edges(fix, kernel):
    import torch
    from prt import _lib
    f = fix["car_boxed"]
    dq = cuda(f.q[:65])
    for n in (0, 1, 63, 65):
        tri = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        kind = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        d2 = torch.full((n + 3,), -77.0, dtype=torch.float32, device="cuda")
        oq = torch.full((n + 3, 3), -77.0, dtype=torch.float32, device="cuda")
        om = torch.full((n + 3, 3), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        f.r.clearance(dq[:n], kernel=kernel, tri=tri, d2=d2, on_query=oq, on_mesh=om, kind=kind)
        assert f.r.clearance_info()["triangles"] == n
        tri, kind, d2, oq, om = (x.cpu().numpy() for x in (tri, kind, d2, oq, om))
        np.testing.assert_array_equal(tri[:n], f.tri[:n], err_msg=str(n))
        np.testing.assert_array_equal(kind[:n], f.kind[:n], err_msg=str(n))
        assert same_bits(d2[:n], f.d2[:n]) and same_bits(oq[:n], f.oq[:n]) and same_bits(om[:n], f.om[:n]), n
        assert (tri[n:] == -77).all() and (kind[n:] == -77).all() and (d2[n:] == -77.0).all(), n
        assert (oq[n:] == -77.0).all() and (om[n:] == -77.0).all(), n
    # each single output alone
    L = _lib.hip()
    n = 65
    for only in range(5):
        bufs = [torch.full((n,), -77, dtype=torch.int32, device="cuda"),
                torch.full((n,), -77.0, dtype=torch.float32, device="cuda"),
                torch.full((n, 3), -77.0, dtype=torch.float32, device="cuda"),
                torch.full((n, 3), -77.0, dtype=torch.float32, device="cuda"),
                torch.full((n,), -77, dtype=torch.int32, device="cuda")]
        torch.cuda.synchronize()
        ptrs = [b.data_ptr() if i == only else None for i, b in enumerate(bufs)]
        t = _lib.ClearTris(dq.data_ptr(), None, n, KERNEL_ID[kernel])
        assert L.rt_clearance_triangles(f.r._ctx, ctypes.byref(t), ctypes.byref(_lib.ClearanceResults(*ptrs))) == 0
        assert f.r.clearance_info()["triangles"] == n
        want = (f.tri, f.d2, f.oq, f.om, f.kind)[only][:n]
        assert np.array_equal(bufs[only].cpu().numpy().view(np.int32), want.view(np.int32)), only


# ------------------------------------------------------------------ 4. against the cut query
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_crossings_are_the_cut_query_s(fix, scene):
    f = fix[scene]
    off, idx, _ = f.r.cuts_csr(cuda(f.q), segments=False)
    off, idx = off.cpu().numpy(), idx.cpu().numpy()
    size = np.diff(off)
    for kernel in KERNELS:
        tri, d2, _, _, kind, _ = query(f.r, f.q, kernel)
        assert (kind == 15).sum() >= 32
        for i in np.flatnonzero(kind == 15):  # a crossing's triangle is one the query cuts
            assert tri[i] in idx[off[i]:off[i + 1]], i
        assert (d2[size > 0] == 0).all() and (tri[size > 0] >= 0).all()
        assert ((kind == 15) <= (size > 0)).all()


# ------------------------------------------------------------------ 5. every structure, moving scene
@pytest.mark.parametrize("accel,flags", [("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        got = query(r, f.q, kernel)
        check(got, f.want, what=(accel, flags, kernel))
        check_path(got[5], kernel, N, len(f.coords), wide=accel != "reference")
    r.close()


def test_moving_scene(dev, scenes, fix):
    """tests/test_gpu_nearest.py's car_boxed scaled by 1.3 and sheared: after update_vertices, and again after
    rebuild_views(mode="device"), both kernels answer as the mirror does on the moved coordinates (every second
    fixture query)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    q = f.q[rows]
    want = cr.expected(q, coords)
    assert (want[0] != f.tri[rows]).sum() > 50 and not same_bits(want[1], f.d2[rows])
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    check(query(r, q, "fast"), f.rows(rows), what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            got = query(r, q, kernel)
            check(got, want, what=(step, kernel))
        assert got[5]["walked"] == len(rows)
    r.close()


# ------------------------------------------------------------------ 6. the walk prunes
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_the_walk_prunes(fix, scene):
    f = fix[scene]
    info = query(f.r, f.q, "fast")[5]
    wide = f.r.scene_info()["wide_nodes"]
    print(f"{scene}, {N} queries: pairs_tested {info['pairs_tested']} ({info['pairs_tested'] / N:.1f} per query of "
          f"{len(f.coords)}), pairs_gated {info['pairs_gated']} ({info['pairs_gated'] / N:.1f}), nodes_visited "
          f"{info['nodes_visited']} ({info['nodes_visited'] / N:.1f} per query of {wide})")
    assert 0 < info["pairs_tested"] < N * len(f.coords) / 4
    assert 0 < info["nodes_visited"] < N * wide
    assert info["pairs_gated"] > 0 and info["stack_overflows"] == 0


# ------------------------------------------------------------------ 7. isolation
def test_a_clearance_query_leaves_every_other_state_alone(dev, scenes, fix):
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
                r.hits_info(), r.sweep_info(), r.contacts_info(), r.cuts_info()]

    def others(r):
        occ = r.occluded(o, p, far)
        hit, t = r.trace_rays(o, p)
        rgb = r.shade_rays(o, p)
        near = r.nearest(pts)
        nb = r.nearest_tris(pts, k=4)
        ov = r.overlaps(lo, hi, k=4)
        hits = r.trace_hits(o, p, max_hits=2)
        sw = r.sweep(pts, d, 0.01)
        ct = r.sweep_contacts(pts, d, 0.01, k=4)
        cu = r.cuts(q, k=4)
        r.sync()
        out = [x.cpu().numpy() for x in (occ, hit, t, rgb, *near, *nb[:3], *ov, *hits, *sw, *ct[:2], *cu)]
        return out, infos_of(r)

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    frame0, stats0, launch0, times0 = r.download(hit=True), r.stats(), r.launch_info(), r.kernel_times(8)
    out0, infos0 = others(r)
    for kernel in ("fast", "strict"):
        r.clearance(q, kernel=kernel)
        ci = r.clearance_info()
        assert ci["triangles"] == N
    frame1 = r.download(hit=True)
    assert same_bits(frame0[0], frame1[0]) and np.array_equal(frame0[1], frame1[1]) and r.stats() == stats0
    assert r.launch_info() == launch0 and r.kernel_times(8) == times0
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
    cj = r.clearance_info()  # ... and none of them touched the clearance query's own counters
    assert strip(cj) == strip(ci) and abs(cj["kernel_ms"] - ci["kernel_ms"]) < 1e-4
    r.close()


# ------------------------------------------------------------------ 8. fast against strict, no mirror
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fast_equals_strict_on_4096_queries(fix, scene):
    f = fix[scene]
    q = cut_ref.surface_tris(f.coords, 4096, seed=97)
    a, b = (query(f.r, q, kernel) for kernel in KERNELS)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    same = ("triangles", "found", "empty", "stack_overflows")
    assert {k: a[5][k] for k in same} == {k: b[5][k] for k in same} and a[5]["found"] == 4096
    check_path(a[5], "strict", 4096, len(f.coords))
    check_path(b[5], "fast", 4096, len(f.coords))
    assert (a[4] == 15).sum() > 1000 and (a[4] < 15).sum() > 100


# ------------------------------------------------------------------ 9. errors
def test_clearance_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    q = cuda(f.q)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.clearance(q)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no clearance query run yet
        r.clearance_info()
    r.clearance(q[:100])
    info = r.clearance_info()
    assert info["triangles"] == 100 and info["found"] == 100
    with pytest.raises(dev.RtError, match="status -1"):
        r.clearance(q, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.clearance((0, 16))  # null tris
    L = _lib.hip()
    tri = torch.empty(16, dtype=torch.int32, device="cuda")
    p, t = q.data_ptr(), tri.data_ptr()
    Q, R = _lib.ClearTris, _lib.ClearanceResults
    for t_, res in [
        (Q(None, None, 16, 0), R(t, None, None, None, None)),   # null tris
        (Q(p, None, 16, 0), R(None, None, None, None, None)),   # all five outputs null
        (Q(p, None, 16, 3), R(t, None, None, None, None)),      # unknown kernel
        (Q(p, None, 16, -1), R(t, None, None, None, None)),
        (Q(p, None, -1, 0), R(t, None, None, None, None)),      # negative n
    ]:
        assert L.rt_clearance_triangles(r._ctx, ctypes.byref(t_), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_clearance_triangles(r._ctx, None, None) == -1
    assert L.rt_clearance_triangles(r._ctx, ctypes.byref(Q(p, None, 16, 0)), None) == -1
    after = r.clearance_info()  # a refused call leaves clearance_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_clearance_triangles(r._ctx, ctypes.byref(Q(None, None, 0, 0)),
                                    ctypes.byref(R(None, None, None, None, None))) == 0
    assert r.clearance_info()["triangles"] == 0
    r.close()
