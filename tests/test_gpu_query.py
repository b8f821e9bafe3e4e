"""Ray queries (rt_trace_rays: Renderer.trace_rays / occluded / query_info) against, in this order,
(a) the reference's committed fixtures, (b) the strict frame kernel through rt_render with a hand-filled camera --
which expresses any ray set o = pos, d = ((ul - pos) + inc_x * x) + inc_y * y -- and (c), only for rays no camera
can express, the strict query, which (a) and (b) pin first. Everything is compared bit for bit."""
import os

import numpy as np
import pytest

from prt import host
from prt._lib import Camera, Vec3

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMAX = np.float32(3.402823466e+38)
KERNELS = ["strict", "fast"]
# the occlusion query's kernel and form: the fast kernel on a wide view is the per-wave pool with refill threshold
# regroup (0: the default, 16), regroup = 64 the lockstep form; the closest-hit query has the lockstep form only
OCC_FORMS = [("strict", 0), ("fast", 0), ("fast", 64), ("fast", 1), ("fast", 63)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


@pytest.fixture(scope="module")
def scenes():
    return {name: host.Scene.named(name).build_bvh(3) for name in ("car_boxed", "car_only")}


def cam_of(a):
    return Camera(*[Vec3(*[float(v) for v in row]) for row in a])


def cam_rays(a, W, H):
    """the primary rays of camera a = [pos, ul, inc_x, inc_y] (float32), row-major: d formed in float32 in the
    kernels' order ((ul - pos) + inc_x * x) + inc_y * y"""
    a = np.asarray(a, np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    xs, ys = xs.reshape(-1, 1), ys.reshape(-1, 1)
    d = (a[1] - a[0])[None, :].astype(np.float32)
    d = d + a[2][None, :] * xs
    d = d + a[3][None, :] * ys
    o = np.broadcast_to(a[0], d.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def look(pos, target, W, H, step, rng):
    """a camera at pos looking at target whose directions are about |forward| = 1 long and `step` apart"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    f = target - pos
    f /= np.linalg.norm(f)
    up = rng.standard_normal(3)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ul = pos + f - r * step * W / 2 + u * step * H / 2
    return np.array([pos, ul, r * step, -u * step], np.float32)


def grid_cameras(scene):
    """eight seeded 16x16 cameras on car_boxed (its box is [-10.2, 10.2]^3): around and inside the box, short and
    long directions, one with rows / columns of degenerate directions, one whose origin lies on a box face of the
    reference tree along a zero axis of some of its directions"""
    rng = np.random.default_rng(20240611)
    cams = []
    for k in range(6):
        inside = k % 2 == 1
        pos = rng.uniform(-9, 9, 3) if inside else rng.uniform(-1, 1, 3) * 6 + np.array([0, -20, 6]) * (1 if k < 4 else -1)
        c = look(pos, rng.uniform(-3, 3, 3), 16, 16, [0.02, 0.1, 0.3][k % 3], rng)
        if k >= 4:
            c[1:] = c[1:] * np.float32(4.0) - np.array([c[0] * 3, 0 * c[0], 0 * c[0]], np.float32)  # |d| ~ 4: the full view
        cams.append(c)
    # degenerate directions: row 0 has d.z = 0 (ul - pos and inc_x have no z), column 8 d.x = -0.4 + 0.05 * 8 = 0
    cams.append(np.array([[0.3, -9, 3], [-0.1, -7, 3], [0.05, 0, 0], [0, -0.01, -0.05]], np.float32))
    # the face case: pos.x is a face coordinate of a reference-tree leaf box, and column 0 has d.x = 0
    leaves = scene.nodes[scene.nodes["tr_len"] > 0]
    fx = np.float32(leaves["min"][len(leaves) // 2][0])
    cams.append(np.array([[fx, -9, 3], [fx, -7, 3.5], [0.05, 0, 0], [0, -0.01, -0.05]], np.float32))
    return cams


class Bench:
    """one Renderer on one scene, the rays of the grid cameras and their strict-render answers"""

    def __init__(self, dev, scene, accel="auto", flags=0):
        self.dev = dev
        self.r = dev.Renderer(0, flags=flags)
        self.r.upload(scene, accel=accel)

    def strict_render(self, cam, W, H):
        import torch
        hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
        t = torch.empty((H, W), dtype=torch.float32, device="cuda")
        self.r.render(cam_of(cam), W, H, kernel="strict", hit=hit, t=t)
        self.r.sync()
        return hit.cpu().numpy().reshape(-1), t.cpu().numpy().reshape(-1)

    def trace(self, o, d, kernel, **kw):
        import torch
        h, t = self.r.trace_rays(torch.from_numpy(np.array(o, np.float32)).cuda(),
                                 torch.from_numpy(np.array(d, np.float32)).cuda(), kernel=kernel, **kw)
        info = self.r.query_info()
        return h.cpu().numpy(), t.cpu().numpy(), info

    def occluded(self, o, d, m, kernel, regroup=0):
        import torch
        out = self.r.occluded(torch.from_numpy(np.array(o, np.float32)).cuda(),
                              torch.from_numpy(np.array(d, np.float32)).cuda(),
                              torch.from_numpy(np.array(m, np.float32)).cuda(), kernel=kernel, regroup=regroup)
        info = self.r.query_info()
        return out.cpu().numpy(), info


@pytest.fixture(scope="module")
def grids(dev, scenes):
    """case 2's rays on car_boxed (8 cameras x 16 x 16) and the strict render's hit / t for them"""
    b = Bench(dev, scenes["car_boxed"])
    cams = grid_cameras(scenes["car_boxed"])
    O, D, HIT, T = [], [], [], []
    for c in cams:
        o, d = cam_rays(c, 16, 16)
        h, t = b.strict_render(c, 16, 16)
        O.append(o), D.append(d), HIT.append(h), T.append(t)
    out = {"bench": b, "cams": cams, "o": np.concatenate(O), "d": np.concatenate(D), "hit": np.concatenate(HIT),
           "t": np.concatenate(T)}
    for k in ("o", "d", "hit", "t"):
        out[k].setflags(write=False)
    assert (out["hit"] >= 0).sum() > 1000 and (out["hit"] < 0).sum() > 0  # (the cameras see the scene and past it)
    return out


# ------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_reference_fixture_rays(dev, scenes, scene, kernel):
    W, H = 64, 36
    ref = np.load(os.path.join(GOLD, f"{scene}_{W}x{H}_strict.npz"))
    o, d = cam_rays(host.camera_array(host.camera(W, H)), W, H)
    b = Bench(dev, scenes[scene])
    h, t, info = b.trace(o, d, kernel)
    np.testing.assert_array_equal(h, ref["hit"].reshape(-1))
    assert same_bits(t, ref["t"].reshape(-1))
    assert info["rays"] == W * H and info["hits"] == int((ref["hit"] >= 0).sum()) and info["stack_overflows"] == 0
    p = np.random.default_rng(7).permutation(W * H)
    h, t, _ = b.trace(o[p], d[p], kernel)
    np.testing.assert_array_equal(h, ref["hit"].reshape(-1)[p])
    assert same_bits(t, ref["t"].reshape(-1)[p])
    b.r.close()


# ------------------------------------------------------------------ 2. camera grids
@pytest.mark.parametrize("kernel", KERNELS)
def test_camera_grids_equal_the_strict_render(grids, kernel):
    h, t, info = grids["bench"].trace(grids["o"], grids["d"], kernel)
    np.testing.assert_array_equal(h, grids["hit"])
    assert same_bits(t, grids["t"])
    assert info["strict_rays"] == 0  # every one of these rays is inside the fast walks' domain
    if kernel == "fast":
        assert info["unit_rays"] + info["short_rays"] + info["full_rays"] == len(h)
        assert info["short_rays"] > 0 and info["full_rays"] > 0


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("accel,flags", [("reference", 0), ("host", 0), ("gpu", 0), ("auto", 2 | 4)])
def test_camera_grids_on_every_acceleration_structure(dev, scenes, grids, accel, flags, kernel):
    """accel = reference / host / gpu, and the unpacked builds (FLAG_UNPACKED_STACK | FLAG_UNPACKED_TRIS)"""
    b = Bench(dev, scenes["car_boxed"], accel=accel, flags=flags)
    h, t, info = b.trace(grids["o"], grids["d"], kernel)
    np.testing.assert_array_equal(h, grids["hit"])
    assert same_bits(t, grids["t"])
    assert info["strict_rays"] == 0
    b.r.close()


# ------------------------------------------------------------------ 3. edges of the ray count
@pytest.mark.parametrize("kernel", KERNELS)
def test_ray_count_edges(dev, grids, kernel):
    import torch
    C = dev.QUERY_CHUNK
    o, d = np.tile(grids["o"], (3, 1)), np.tile(grids["d"], (3, 1))
    hit, t = np.tile(grids["hit"], 3), np.tile(grids["t"], 3)
    do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    r = grids["bench"].r
    for n in (0, 1, 63, 64, 65, C - 1, C, C + 1, 4097):
        oh = torch.full((n + 8,), -77, dtype=torch.int32, device="cuda")
        ot = torch.full((n + 8,), -77.0, dtype=torch.float32, device="cuda")
        r.trace_rays(do[:n], dd[:n], kernel=kernel, hit=oh, t=ot)
        assert r.query_info()["rays"] == n
        oh, ot = oh.cpu().numpy(), ot.cpu().numpy()
        np.testing.assert_array_equal(oh[:n], hit[:n], err_msg=str(n))
        assert same_bits(ot[:n], t[:n]), n
        assert (oh[n:] == -77).all() and (ot[n:] == -77.0).all(), n  # nothing written past n


# ------------------------------------------------------------------ 4. ties
def test_exact_ties_are_rewalked(dev):
    """every triangle twice (as test_exact_ties_everywhere_match_strict builds it): the fast query equals the strict
    render (the reference's first-found rule)"""
    base = host.Scene.named("car_only")
    s = host.Scene(np.concatenate([base.triangles, base.triangles]), base.lights).build_bvh(3)
    W, H = 96, 54
    cam = host.camera_array(host.camera(W, H))
    b = Bench(dev, s)
    rh, rt = b.strict_render(cam, W, H)
    o, d = cam_rays(cam, W, H)
    for kernel in KERNELS:
        h, t, info = b.trace(o, d, kernel)
        np.testing.assert_array_equal(h, rh, err_msg=kernel)
        assert same_bits(t, rt), kernel
        if kernel == "fast":
            assert info["tie_rewalks"] > 0
            assert info["unit_rays"] + info["short_rays"] + info["full_rays"] + info["strict_rays"] == len(h)
    b.r.close()


# ------------------------------------------------------------------ 5. views
def test_each_ray_walks_a_view_its_length_allows(dev):
    """A = (0,0,0),(4,0,0),(0,4,0); B = (1,1,1),(1.01,1,1),(1,1.01,1) with |n| = 1e-4: B is in neither the unit nor
    the primary view. From (1.004, 1.003, 3) along normalize(1e-3, -5e-4, -1) * L the reference's hit_triangle culls
    B while |det| = 1e-4 L < EPSILON: L = 1, 2.5, 3.5 hit A at t = 3 / L; L = 20 and 1000 hit B (t = 2 / L) in front
    of it. (L = 0.9999 added: its computed length is below 1 whatever the rounding of the normalisation.)"""
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
    b = Bench(dev, s)
    want = np.array([0, 0, 0, 1, 1, 0], np.int32)
    hs, ts, st = b.trace(o, d, "strict")
    np.testing.assert_array_equal(hs, want)
    np.testing.assert_allclose(ts, np.where(want == 0, 3.0, 2.0) / L, rtol=1e-3)
    hf, tf, info = b.trace(o, d, "fast")
    np.testing.assert_array_equal(hf, want)
    assert same_bits(tf, ts)
    assert info["unit_rays"] >= 1 and info["short_rays"] >= 1 and info["full_rays"] >= 1, info
    b.r.close()


# ------------------------------------------------------------------ 6. domain
def domain_sets(grids):
    o, d = grids["o"][::4].copy(), grids["d"][::4].copy()
    sets = {}
    # (|d| 2^-17 .. 2^14 can still hit this scene: hit_triangle wants |det| >= 1e-3 and t > 1e-3)
    for k in (-60, -30, -17, -14, -10, 10, 14, 30, 60):
        sets[f"scale{k}"] = (o, (d * np.float32(2.0) ** k).astype(np.float32), abs(k) > 20)
    # the domain's edges: a direction whose largest component is exactly 2^+-20 is inside, the next float outside;
    # an origin whose largest component is 4 mx = 64 (car_boxed: mx = 16) is inside, the next float outside
    dm = np.abs(d).max(1, keepdims=True)
    unit_max = (d / dm).astype(np.float32)  # largest component exactly +-1
    for k in (-20, 20):
        sets[f"edge{k}_in"] = (o, (unit_max * np.float32(2.0) ** k).astype(np.float32), False)
    sets["edge20_out"] = (o, (unit_max * np.nextafter(np.float32(2.0 ** 20), np.float32(np.inf))).astype(np.float32), True)
    sets["edge-20_out"] = (o, (unit_max * np.nextafter(np.float32(2.0 ** -20), np.float32(0))).astype(np.float32), True)
    far_o = o.copy()
    far_o[:, 1] = np.where(np.arange(len(o)) % 2 == 0, 64.0, -64.0)
    sets["origin_edge_in"] = (far_o, d, False)
    sets["origin_edge_in_fast_d"] = (far_o, (unit_max * np.float32(2.0) ** 20).astype(np.float32), False)
    sets["origin_edge_in_slow_d"] = (far_o, (unit_max * np.float32(2.0) ** -20).astype(np.float32), False)
    out_o = far_o.copy()
    out_o[:, 1] = np.nextafter(np.abs(far_o[:, 1]), np.float32(np.inf)) * np.sign(far_o[:, 1])
    sets["origin_edge_out"] = (out_o.astype(np.float32), d, True)
    sets["far"] = ((o - d * np.float32(2.0 ** 20)).astype(np.float32), d, True)
    bad_o, bad_d = o.copy(), d.copy()
    bad_o[0::6, 0] = np.nan
    bad_o[1::6, 1] = np.inf
    bad_d[2::6, 2] = np.nan
    bad_d[3::6, 0] = -np.inf
    bad_d[4::6] = 0.0
    sets["nonfinite"] = (bad_o, bad_d, True)
    return sets


def test_rays_outside_the_fast_domain_walk_the_reference_tree(grids):
    """Yardstick (c): no camera expresses these rays (directions scaled by 2^k, origins 2^20 directions away, NaN and
    inf components, all-zero directions), so the fast query is compared with the strict query, which the fixture and
    camera-grid tests above pin to the reference's fixtures and the strict frame kernel. Nothing is an error."""
    b = grids["bench"]
    for name, (o, d, leaves) in domain_sets(grids).items():
        hs, ts, _ = b.trace(o, d, "strict")
        hf, tf, info = b.trace(o, d, "fast")
        np.testing.assert_array_equal(hf, hs, err_msg=name)
        assert same_bits(tf, ts), name
        assert info["stack_overflows"] == 0
        if leaves:
            assert info["strict_rays"] > 0, name
        else:
            assert info["strict_rays"] == 0, name  # inside: the domain is not an empty one


# ------------------------------------------------------------------ 7. occlusion
def occlusion_cases(hit, D):
    """(max_dist2, expected) per case for rays whose closest hit is at squared distance D (hit < 0: a miss)"""
    n = len(hit)
    h = hit >= 0
    f = lambda v: np.full(n, v, np.float32)
    return {
        "quarter": (np.where(h, 0.25 * D, 4.0).astype(np.float32), np.zeros(n, np.int32)),
        "four": (np.where(h, 4.0 * D, 4.0).astype(np.float32), h.astype(np.int32)),
        "inf": (f(np.inf), h.astype(np.int32)),
        "fltmax": (f(FMAX), h.astype(np.int32)),
        "zero": (f(0.0), np.zeros(n, np.int32)),
        "negative": (f(-1.0), np.zeros(n, np.int32)),
    }


@pytest.mark.parametrize("kernel,regroup", OCC_FORMS)
def test_occlusion_of_camera_rays(grids, kernel, regroup):
    """the strict render's closest hit at t is at squared distance D = |d|^2 t^2: nothing is nearer than 0.25 D,
    that hit is nearer than 4 D"""
    o, d, hit, t = grids["o"], grids["d"], grids["hit"], grids["t"]
    D = (d.astype(np.float64) ** 2).sum(1) * np.where(hit >= 0, t, 0).astype(np.float64) ** 2
    for name, (m, want) in occlusion_cases(hit, D).items():
        got, info = grids["bench"].occluded(o, d, m, kernel, regroup)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert info["hits"] == int(want.sum()) and info["stack_overflows"] == 0 and info["rays"] == len(o)


@pytest.mark.parametrize("kernel,regroup", OCC_FORMS)
def test_occlusion_of_unit_length_rays(grids, kernel, regroup):
    """the same origins with numpy-normalised directions, t from the strict query (yardstick (c): a camera's
    directions are not normalised; the strict query is pinned by the tests above)"""
    o, b = grids["o"], grids["bench"]
    d = grids["d"].astype(np.float32)
    d = (d / np.sqrt((d * d).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    hit, t, _ = b.trace(o, d, "strict")
    assert (hit >= 0).sum() > 1000
    D = (d.astype(np.float64) ** 2).sum(1) * np.where(hit >= 0, t, 0).astype(np.float64) ** 2
    for name, (m, want) in occlusion_cases(hit, D).items():
        got, info = b.occluded(o, d, m, kernel, regroup)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert info["hits"] == int(want.sum()) and info["rays"] == len(o)
        if kernel == "fast":
            assert info["unit_rays"] + info["full_rays"] + info["strict_rays"] == len(o), (name, info)
        if kernel == "fast" and name in ("quarter", "four", "fltmax"):
            assert info["unit_rays"] > 0, name
            print(f"unit share {name}: {info['unit_rays']} of {info['rays']} (strict {info['strict_rays']})")
    m = np.where(np.arange(len(o)) % 3 == 0, np.nan, 4.0).astype(np.float32)
    gs, _ = b.occluded(o, d, m, "strict")
    gf, _ = b.occluded(o, d, m, kernel, regroup)
    np.testing.assert_array_equal(gf, gs)


@pytest.mark.parametrize("regroup", [64, 0, 5])
def test_occlusion_ray_count_edges_and_domain(dev, grids, regroup):
    """both forms of the fast occlusion query on prefixes of the unit-length rays (a chunk's last pass partly filled,
    several chunks) and on the sets that leave the fast domain, against the strict query (yardstick (c): pinned by the
    occlusion tests above); nothing is written past n"""
    import torch
    C = dev.QUERY_CHUNK
    r = grids["bench"].r
    d = grids["d"].astype(np.float32)
    d = (d / np.sqrt((d * d).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    o = np.tile(grids["o"], (3, 1))
    d = np.tile(d, (3, 1))
    m = np.full(len(o), 900.0, np.float32)
    m[5::11] = np.inf  # rays outside the fast walk's domain among the others
    d[7::13] *= np.float32(1.5)
    do, dd, dm = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(m).cuda()
    want = r.occluded(do, dd, dm, kernel="strict")
    r.sync()  # (a query is asynchronous on the renderer's stream)
    want = want.cpu().numpy()
    assert 0 < want.sum() < len(want)
    for n in (0, 1, 63, 64, 65, C - 1, C, C + 1, 4097):
        out = torch.full((n + 8,), -77, dtype=torch.int32, device="cuda")
        r.occluded(do[:n], dd[:n], dm[:n], kernel="fast", out=out, regroup=regroup)
        info = r.query_info()
        out = out.cpu().numpy()
        np.testing.assert_array_equal(out[:n], want[:n], err_msg=str(n))
        assert (out[n:] == -77).all(), n
        assert info["rays"] == n and info["hits"] == int(want[:n].sum())
        assert info["unit_rays"] + info["full_rays"] + info["strict_rays"] == n and (n < 64 or info["strict_rays"] > 0)


# ------------------------------------------------------------------ 8. state
def test_a_query_leaves_the_render_state_alone(dev, scenes, grids):
    import torch
    W, H = 64, 36
    cam = host.camera(W, H)
    do, dd = torch.from_numpy(grids["o"].copy()).cuda(), torch.from_numpy(grids["d"].copy()).cuda()

    def state(r):
        li = r.launch_info()
        return r.download(hit=True), r.stats(), li

    def run(query):
        r = dev.Renderer(0)
        r.upload(scenes["car_boxed"])
        hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
        r.render(cam, W, H, kernel="fast", hit=hit)
        r.sync()
        if query:
            before, times = state(r), r.kernel_times(8)
            r.trace_rays(do, dd)
            r.occluded(do, dd, torch.full((len(do),), 4.0, device="cuda"))
            assert r.query_info()["rays"] == len(do)
            after = state(r)
            assert same_bits(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
            assert before[1:] == after[1:] and r.kernel_times(8) == times and r.sync() == r.sync()
        r.render(cam, W, H, kernel="fast", hit=hit)
        ms = r.sync()
        out = state(r), len(r.kernel_times(8)), ms > 0
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_bits(a[0][0][0], b[0][0][0]) and np.array_equal(a[0][0][1], b[0][0][1])
    assert a[0][1:] == b[0][1:] and a[1:] == b[1:]


def test_query_errors(dev, scenes, grids):
    import torch
    do, dd = torch.from_numpy(grids["o"].copy()).cuda(), torch.from_numpy(grids["d"].copy()).cuda()
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.trace_rays(do, dd)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no query traced yet
        r.query_info()
    with pytest.raises(dev.RtError, match="status -1"):
        r.trace_rays(do, dd, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.trace_rays(do, dd, regroup=65)
    with pytest.raises(dev.RtError, match="status -1"):
        r.trace_rays((0, 16), dd.data_ptr())  # null origin
    from prt import _lib
    L = _lib.hip()
    import ctypes
    hit = torch.empty(len(do), dtype=torch.int32, device="cuda")
    for rays, res in [
        (_lib.Rays(do.data_ptr(), dd.data_ptr(), None, 16, 2, 0, 0), _lib.RayResults(hit.data_ptr(), None, None)),
        (_lib.Rays(do.data_ptr(), dd.data_ptr(), None, 16, 1, 0, 0), _lib.RayResults(None, None, hit.data_ptr())),
        (_lib.Rays(do.data_ptr(), dd.data_ptr(), do.data_ptr(), 16, 1, 0, 0), _lib.RayResults(hit.data_ptr(), None, None)),
        (_lib.Rays(do.data_ptr(), dd.data_ptr(), None, 16, 0, 0, 0), _lib.RayResults(None, None, hit.data_ptr())),
        (_lib.Rays(do.data_ptr(), dd.data_ptr(), None, -1, 0, 0, 0), _lib.RayResults(hit.data_ptr(), None, None)),
    ]:  # a bad kind; OCCLUDED without max_dist2 / without occluded; CLOSEST with both outputs null; negative n
        assert L.rt_trace_rays(r._ctx, ctypes.byref(rays), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    h, t = r.trace_rays(do[:16], dd[:16])  # and the context still works
    assert r.query_info()["rays"] == 16
    r.close()


# ------------------------------------------------------------------ 9. handled overflow
def test_stack_overflow_fails_query_info(dev, scenes):
    """the 41-triangle, 40-level handed-over tree of test_kernel_errors_fail_sync_and_download: the walk's 34-entry
    stack overflows, which the kernel counts (the library's own error flag, not a device fault) and query_info
    reports as RT_E_KERNEL (-8); a later render of another scene is unaffected"""
    import torch
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
    do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    r = dev.Renderer(0)
    r.upload(s, accel="reference")
    for kernel in KERNELS:
        r.trace_rays(do, dd, kernel=kernel)
        with pytest.raises(dev.RtError, match="-8"):
            r.query_info()
    r.upload(base)
    hit = torch.empty((36, 64), dtype=torch.int32, device="cuda")
    r.render(host.camera(64, 36), 64, 36, kernel="fast", hit=hit)
    assert r.sync() > 0
    ref = np.load(os.path.join(GOLD, "car_only_64x36_strict.npz"))
    np.testing.assert_array_equal(hit.cpu().numpy(), ref["hit"])
    h, _ = r.trace_rays(*[torch.from_numpy(x).cuda() for x in cam_rays(host.camera_array(host.camera(64, 36)), 64, 36)])
    assert r.query_info()["stack_overflows"] == 0
    np.testing.assert_array_equal(h.cpu().numpy(), ref["hit"].reshape(-1))
    r.close()
