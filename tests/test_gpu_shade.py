"""Radiance queries (rt_shade_rays: Renderer.shade_rays / shade_info) against, in this order, (a) the reference's
committed fixtures, (b) the strict frame kernel through rt_render with hand-filled cameras and (c), only for rays no
16x16 camera grid reaches, the strict shade query, which is first pinned ray by ray to 2x1 strict renders. Everything is
compared bit for bit. Each test runs on the strict kernel and on the fast kernel's forms: regroup 0 (the library's
choice), 64 (lockstep), 1 and 63 (the shadow pool at its two extreme refill thresholds)."""
import os

import numpy as np
import pytest

from prt import host
from tests.test_gpu_query import cam_of, cam_rays, domain_sets, grid_cameras, same_bits

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMAX = np.float32(3.402823466e+38)
FORMS = [("strict", 0), ("fast", 0), ("fast", 64), ("fast", 1), ("fast", 63)]
FAST_FORMS = FORMS[1:]
OUTS = ("rgb", "bgra", "hit", "t", "bounce_hit")
COUNTS = (("rays", "primary"), ("hits", "hits"), ("reflection", "reflection"), ("shadow", "shadow"),
          ("shadow_skipped", "shadow_skipped"))  # rt_shade_info's name, rt_stats' name


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


@pytest.fixture(scope="module")
def scenes():
    return {name: host.Scene.named(name).build_bvh(3) for name in ("car_boxed", "car_only")}


def equal(got, want, what=""):
    """every output present in both, bit for bit"""
    for k in OUTS:
        if k in got and k in want:
            if k in ("rgb", "t"):
                assert same_bits(got[k], want[k]), (what, k, int((got[k].view(np.int32) != want[k].view(np.int32)).sum()))
            else:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")


def take(ref, idx):
    return {k: ref[k][idx] for k in OUTS if k in ref}


class Shader:
    """one Renderer on one scene: strict renders with every output, and shade queries with every output"""

    def __init__(self, dev, scene, accel="auto", flags=0):
        self.r = dev.Renderer(0, flags=flags)
        self.r.upload(scene, accel=accel)

    def bufs(self, n, bounces, fill=None):
        import torch
        mk = (lambda s, dt: torch.empty(s, dtype=dt, device="cuda")) if fill is None else \
             (lambda s, dt: torch.full(s, fill, dtype=dt, device="cuda"))
        return {"rgb": mk((n, 3), torch.float32), "bgra": mk((n,), torch.int32), "hit": mk((n,), torch.int32),
                "t": mk((n,), torch.float32), "bounce_hit": mk((n, bounces), torch.int32)}

    def render(self, cam, W, H, bounces=4, kernel="strict"):
        b = self.bufs(W * H, bounces)
        self.r.render(cam if not isinstance(cam, np.ndarray) else cam_of(cam), W, H, bounces=bounces, kernel=kernel, **b)
        self.r.sync()
        out = {k: v.cpu().numpy() for k, v in b.items()}
        out["stats"] = self.r.stats()
        return out

    def shade(self, o, d, kernel, regroup=0, bounces=4, unclamped=False):
        import torch
        do = o if isinstance(o, torch.Tensor) else torch.from_numpy(np.array(o, np.float32)).cuda()
        dd = d if isinstance(d, torch.Tensor) else torch.from_numpy(np.array(d, np.float32)).cuda()
        b = self.bufs(len(do), bounces)
        if unclamped:
            del b["bgra"]
        self.r.shade_rays(do, dd, bounces=bounces, kernel=kernel, regroup=regroup, unclamped=unclamped, **b)
        info = self.r.shade_info()
        out = {k: v.cpu().numpy() for k, v in b.items()}
        out["info"] = info
        return out

    def pin(self, o, d, bounces=4):
        """yardstick for single rays: ray k = pixel (1, 0) of a 2x1 strict render with pos = ul = o, inc_x = d,
        inc_y = 0, whose direction is (0 + d) + 0"""
        n = len(o)
        b = self.bufs(2 * n, bounces)
        for k in range(n):
            cam = np.array([o[k], o[k], d[k], [0, 0, 0]], np.float32)
            self.r.render(cam_of(cam), 2, 1, bounces=bounces, kernel="strict",
                          **{name: v[2 * k:2 * k + 2] for name, v in b.items()})
        self.r.sync()
        return {k: v.cpu().numpy()[1::2] for k, v in b.items()}


def concat(parts):
    out = {k: np.concatenate([p[k] for p in parts]) for k in OUTS}
    out["stats"] = {s: sum(p["stats"][s] for p in parts) for _, s in COUNTS}
    for k in OUTS:
        out[k].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def grids(dev, scenes):
    """yardstick (b): the rays of the eight 16x16 grid cameras of tests/test_gpu_query.py on car_boxed (the two last are
    hand-filled) and their strict renders' outputs and counters"""
    sh = Shader(dev, scenes["car_boxed"])
    cams = grid_cameras(scenes["car_boxed"])
    rays = [cam_rays(c, 16, 16) for c in cams]
    ref = concat([sh.render(c, 16, 16) for c in cams])
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    o.setflags(write=False), d.setflags(write=False)
    st = ref["stats"]
    # a check on the yardstick: its rays reach every part of raytrace()
    assert st["primary"] == 2048 and st["reflection"] > 0 and st["shadow"] > 0 and st["shadow_skipped"] > 0, st
    assert (ref["hit"] >= 0).sum() > 1000 and (ref["hit"] < 0).sum() > 0
    return {"sh": sh, "cams": cams, "o": o, "d": d, "ref": ref}


def check_counters(info, stats, what=""):
    for a, b in COUNTS:
        assert info[a] == stats[b], (what, a, info, {s: stats[s] for _, s in COUNTS})
    assert info["stack_overflows"] == 0


# ------------------------------------------------------------------ (a) the reference's fixtures
@pytest.mark.parametrize("kernel,regroup", FORMS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_reference_fixture_rays(dev, scenes, scene, kernel, regroup):
    W, H = 64, 36
    g = np.load(os.path.join(GOLD, f"{scene}_{W}x{H}_strict.npz"))
    ref = {"rgb": g["rgb"].reshape(-1, 3), "hit": g["hit"].reshape(-1), "t": g["t"].reshape(-1)}
    o, d = cam_rays(host.camera_array(host.camera(W, H)), W, H)
    sh = Shader(dev, scenes[scene])
    got = sh.shade(o, d, kernel, regroup)
    equal(got, ref, "row-major")
    nhit = int((ref["hit"] >= 0).sum())
    assert got["info"]["rays"] == W * H and got["info"]["hits"] >= nhit and got["info"]["stack_overflows"] == 0
    # (hits counts every level's, as rt_stats does: with one level it is the fixture's count)
    one = sh.shade(o, d, kernel, regroup, bounces=1)
    assert one["info"]["hits"] == nhit and one["info"]["reflection"] == 0 and one["info"]["rays"] == W * H
    np.testing.assert_array_equal(one["hit"], ref["hit"])
    p = np.random.default_rng(7).permutation(W * H)
    got = sh.shade(o[p], d[p], kernel, regroup)
    equal(got, take(ref, p), "permuted")
    sh.r.close()


# ------------------------------------------------------------------ (b) the strict frame kernel
@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_camera_grids_equal_the_strict_render(grids, kernel, regroup):
    got = grids["sh"].shade(grids["o"], grids["d"], kernel, regroup)
    equal(got, grids["ref"])
    check_counters(got["info"], grids["ref"]["stats"])
    assert got["info"]["strict_paths"] == 0  # every one of these rays is inside the fast walks' domain


@pytest.fixture(scope="module", params=[("reference", 0), ("host", 0), ("gpu", 0), ("auto", 2 | 4)],
                ids=["reference", "host", "gpu", "unpacked"])
def other_accel(request, dev, scenes):
    sh = Shader(dev, scenes["car_boxed"], accel=request.param[0], flags=request.param[1])
    yield sh
    sh.r.close()


@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_camera_grids_on_every_acceleration_structure(other_accel, grids, kernel, regroup):
    """accel = reference / host / gpu, and the unpacked builds (FLAG_UNPACKED_STACK | FLAG_UNPACKED_TRIS)"""
    got = other_accel.shade(grids["o"], grids["d"], kernel, regroup)
    equal(got, grids["ref"])
    check_counters(got["info"], grids["ref"]["stats"])
    assert got["info"]["strict_paths"] == 0


# ------------------------------------------------------------------ (c) rays the grids do not reach
@pytest.fixture(scope="module")
def domain(grids):
    """domain_sets' rays and, per set, the strict shade query's answer (pinned by the strict case below)"""
    sets = domain_sets(grids)
    return {name: (o, d, leaves, grids["sh"].shade(o, d, "strict")) for name, (o, d, leaves) in sets.items()}


@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_rays_outside_the_fast_domain(grids, domain, kernel, regroup):
    """strict: a seeded sample of at most 32 rays per set against 2x1 strict renders (a direction component of -0
    would become +0 in the pixel's (0 + d) + 0: such rays are left out of the sample). fast: the full sets against
    the strict query; strict_paths > 0 exactly for the sets that leave the domain. Nothing is an error."""
    sh = grids["sh"]
    rng = np.random.default_rng(31)
    for name, (o, d, leaves, ref) in domain.items():
        if kernel == "strict":
            ok = np.flatnonzero(~((d == 0) & np.signbit(d)).any(1))
            idx = np.sort(rng.choice(ok, size=min(32, len(ok)), replace=False))
            assert len(idx) >= 16, name
            want = sh.pin(o[idx], d[idx])
            equal(take(ref, idx), want, name)
            assert ref["info"]["strict_paths"] == 0 and ref["info"]["stack_overflows"] == 0
            continue
        got = sh.shade(o, d, kernel, regroup)
        equal(got, ref, name)
        for a, _ in COUNTS:
            assert got["info"][a] == ref["info"][a], (name, a)
        assert got["info"]["stack_overflows"] == 0
        if leaves:
            assert got["info"]["strict_paths"] > 0, name
        else:
            assert got["info"]["strict_paths"] == 0, name  # inside: the domain is not an empty one


# ------------------------------------------------------------------ bounces
BOUNCES = (1, 2, 4, 5, 8)


@pytest.fixture(scope="module")
def by_bounces(grids):
    """grid camera 1 (inside the box: mirrors face mirrors) rendered strictly at each number of levels"""
    cam = grids["cams"][1]
    ref = {b: grids["sh"].render(cam, 16, 16, bounces=b) for b in BOUNCES}
    # a check on the yardstick: paths reach the last level at every depth (bounces = 1: a reflective surface there)
    for b in BOUNCES:
        assert (ref[b]["bounce_hit"][:, b - 1] >= 0).any(), b
    assert ref[8]["stats"]["reflection"] > ref[4]["stats"]["reflection"] > ref[1]["stats"]["reflection"] == 0
    return ref


@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_bounces(grids, by_bounces, kernel, regroup):
    o, d = cam_rays(grids["cams"][1], 16, 16)
    for b in BOUNCES:
        got = grids["sh"].shade(o, d, kernel, regroup, bounces=b)
        equal(got, by_bounces[b], f"bounces {b}")
        check_counters(got["info"], by_bounces[b]["stats"], f"bounces {b}")


# ------------------------------------------------------------------ edges of the ray count
@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_ray_count_edges(dev, grids, kernel, regroup):
    import torch
    C = dev.QUERY_CHUNK
    sh = grids["sh"]
    do = torch.from_numpy(np.tile(grids["o"], (3, 1))).cuda()
    dd = torch.from_numpy(np.tile(grids["d"], (3, 1))).cuda()
    ref = {k: np.concatenate([grids["ref"][k]] * 3) for k in OUTS}
    for n in (0, 1, 63, 64, 65, C - 1, C, C + 1, 4097):
        b = sh.bufs(n + 8, 4, fill=-77)
        sh.r.shade_rays(do[:n], dd[:n], kernel=kernel, regroup=regroup, **b)
        assert sh.r.shade_info()["rays"] == n
        got = {k: v.cpu().numpy() for k, v in b.items()}
        equal({k: v[:n] for k, v in got.items()}, take(ref, slice(0, n)), str(n))
        for k, v in got.items():
            assert (v[n:] == -77).all(), (n, k)  # nothing written past n


# ------------------------------------------------------------------ exact ties
@pytest.fixture(scope="module")
def tied(dev):
    """car_only with every triangle twice (as test_exact_ties_are_rewalked builds it) and its strict render"""
    base = host.Scene.named("car_only")
    s = host.Scene(np.concatenate([base.triangles, base.triangles]), base.lights).build_bvh(3)
    W, H = 96, 54
    cam = host.camera_array(host.camera(W, H))
    sh = Shader(dev, s)
    out = {"sh": sh, "ref": sh.render(cam, W, H), "rays": cam_rays(cam, W, H)}
    yield out
    sh.r.close()


@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_exact_ties_are_rewalked(tied, kernel, regroup):
    got = tied["sh"].shade(*tied["rays"], kernel, regroup)
    equal(got, tied["ref"])
    check_counters(got["info"], tied["ref"]["stats"])
    if kernel == "fast":
        assert got["info"]["tie_rewalks"] > 0


# ------------------------------------------------------------------ lights
@pytest.fixture(scope="module")
def unlit(dev):
    """the two-triangle scene of test_each_ray_walks_a_view_its_length_allows: no light at all. Its rays, rays that
    miss, and 2x1 strict renders as their yardstick."""
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
    d = np.concatenate([(u[None, :] * L[:, None]), -(u[None, :] * L[:, None])]).astype(np.float32)  # (the last six miss)
    d = np.tile(d, (7, 1))  # 84 rays: more than a wave
    o = np.tile(np.array([1.004, 1.003, 3], np.float32), (len(d), 1))
    sh = Shader(dev, s)
    ref = sh.pin(o, d)
    assert (ref["hit"] >= 0).sum() == 42 and (ref["hit"] < 0).sum() == 42
    yield {"sh": sh, "o": o, "d": d, "ref": ref}
    sh.r.close()


@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_a_scene_without_lights(unlit, kernel, regroup):
    """(car_boxed's own lights: the camera-grid tests.) The pool form runs on an empty pool."""
    got = unlit["sh"].shade(unlit["o"], unlit["d"], kernel, regroup)
    equal(got, unlit["ref"])
    i = got["info"]
    assert i["rays"] == 84 and i["hits"] == 42 and i["shadow"] == 0 and i["shadow_skipped"] == 0 and i["reflection"] == 0


# ------------------------------------------------------------------ unclamped
@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_unclamped_is_raytraces_value(grids, scenes, kernel, regroup):
    sh, ref = grids["sh"], grids["ref"]
    got = sh.shade(grids["o"], grids["d"], kernel, regroup, unclamped=True)
    equal({k: got[k] for k in ("hit", "t", "bounce_hit")}, ref)
    clamped = np.minimum(np.maximum(got["rgb"], np.float32(0)), np.float32(1))  # vec_constrain(col, 0, 1)
    assert same_bits(clamped, ref["rgb"])
    miss = ref["hit"] < 0
    amb = np.float32(0) + np.asarray(scenes["car_boxed"].amb, np.float32)  # raytracer.c:132-135
    assert miss.any() and same_bits(got["rgb"][miss], np.tile(amb, (int(miss.sum()), 1)))
    print("unclamped values above 1:", int((got["rgb"] > 1).sum()), "max", float(got["rgb"].max()))


# ------------------------------------------------------------------ state
def test_a_shade_query_leaves_render_and_query_state_alone(dev, scenes, grids):
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
            r.trace_rays(do[:300], dd[:300])
            qi = r.query_info()
            before, times = state(r), r.kernel_times(8)
            for regroup in (64, 5):
                r.shade_rays(do, dd, regroup=regroup)
                assert r.shade_info()["rays"] == len(do)
            r.shade_rays(do, dd, kernel="strict", bounces=8)
            assert r.shade_info()["rays"] == len(do)
            after = state(r)
            assert same_bits(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
            assert before[1:] == after[1:] and r.kernel_times(8) == times and r.sync() == r.sync()
            # (hipEventElapsedTime of one event pair moves in its last digits from call to call: the counters exactly,
            # the time to 1e-4 ms -- the shade queries above ran 2,048 rays at up to 8 levels against the query's 300)
            qj = r.query_info()
            assert {k: v for k, v in qj.items() if k != "kernel_ms"} == {k: v for k, v in qi.items() if k != "kernel_ms"}
            assert abs(qj["kernel_ms"] - qi["kernel_ms"]) < 1e-4, (qi, qj)
        r.render(cam, W, H, kernel="fast", hit=hit)
        ms = r.sync()
        out = state(r), len(r.kernel_times(8)), ms > 0
        r.close()
        return out

    a, b = run(False), run(True)
    assert same_bits(a[0][0][0], b[0][0][0]) and np.array_equal(a[0][0][1], b[0][0][1])
    assert a[0][1:] == b[0][1:] and a[1:] == b[1:]


def test_shade_errors(dev, scenes, grids):
    import torch
    do, dd = torch.from_numpy(grids["o"].copy()).cuda(), torch.from_numpy(grids["d"].copy()).cuda()
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.shade_rays(do, dd)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # nothing shaded yet
        r.shade_info()
    for kw in ({"kernel": 7}, {"regroup": 65}, {"bounces": 0}, {"bounces": 9}):
        with pytest.raises(dev.RtError, match="status -1"):
            r.shade_rays(do, dd, **kw)
    with pytest.raises(dev.RtError, match="status -1"):
        r.shade_rays((0, 16), dd.data_ptr())  # null origin
    from prt import _lib
    import ctypes
    L = _lib.hip()
    rgb = torch.empty((16, 3), dtype=torch.float32, device="cuda")
    for q, res in [
        (_lib.Shade(do.data_ptr(), dd.data_ptr(), 16, 4, 0, 0, 0), _lib.ShadeResults(None, None, None, None, None)),
        (_lib.Shade(do.data_ptr(), dd.data_ptr(), -1, 4, 0, 0, 0), _lib.ShadeResults(rgb.data_ptr(), None, None, None, None)),
        (_lib.Shade(do.data_ptr(), dd.data_ptr(), 16, 4, 0, 0, 1),
         _lib.ShadeResults(rgb.data_ptr(), rgb.data_ptr(), None, None, None)),
        (_lib.Shade(do.data_ptr(), dd.data_ptr(), 16, 4, 0, 0, 2), _lib.ShadeResults(rgb.data_ptr(), None, None, None, None)),
    ]:  # no output at all; negative n; unclamped with bgra; unclamped neither 0 nor 1
        assert L.rt_shade_rays(r._ctx, ctypes.byref(q), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    out = r.shade_rays(do[:16], dd[:16])  # and the context still works
    assert r.shade_info()["rays"] == 16 and tuple(out.shape) == (16, 3)
    r.close()


# ------------------------------------------------------------------ handled overflow
def test_stack_overflow_fails_shade_info(dev, scenes):
    """the 41-triangle, 40-level handed-over tree of test_stack_overflow_fails_query_info: the walk's 34-entry stack
    overflows, which the kernel counts (the library's own error flag, not a device fault) and shade_info reports as
    RT_E_KERNEL (-8); a later query on another scene is unaffected"""
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
    r.shade_rays(do, dd, kernel="fast")
    with pytest.raises(dev.RtError, match="-8"):
        r.shade_info()
    r.upload(base)
    ref = np.load(os.path.join(GOLD, "car_only_64x36_strict.npz"))
    rgb = r.shade_rays(*[torch.from_numpy(x).cuda() for x in cam_rays(host.camera_array(host.camera(64, 36)), 64, 36)])
    assert r.shade_info()["stack_overflows"] == 0
    assert same_bits(rgb.cpu().numpy(), ref["rgb"].reshape(-1, 3))
    r.close()


# ------------------------------------------------------------------ generators
@pytest.mark.parametrize("kernel,regroup", FAST_FORMS)
def test_equirect_and_ortho_rays(grids, kernel, regroup):
    from prt import rays
    sh = grids["sh"]
    views = {"equirect": rays.equirect([0.3, -3.0, 2.0], 32, 16),
             "ortho": rays.ortho([0.0, -9.0, 3.0], [0.0, 1.0, 0.0], [0.4, 0.0, 0.0], [0.0, 0.0, 0.4], 32, 16)}
    for name, (o, d) in views.items():
        ref = sh.shade(o, d, "strict")
        assert (ref["hit"] >= 0).sum() > 100 and ref["info"]["shadow"] > 0, name  # (the view sees the scene)
        got = sh.shade(o, d, kernel, regroup)
        equal(got, ref, name)
        for a, _ in COUNTS:
            assert got["info"][a] == ref["info"][a], (name, a)
        assert got["info"]["strict_paths"] == 0, name


@pytest.mark.parametrize("kernel,regroup", FORMS)
def test_pinhole_rays_equal_the_render(dev, scenes, kernel, regroup):
    from prt import rays
    W, H = 64, 36
    cam = host.camera(W, H)
    sh = Shader(dev, scenes["car_boxed"])
    want = sh.render(cam, W, H, kernel="fast" if kernel == "fast" else "strict")
    g = np.load(os.path.join(GOLD, f"car_boxed_{W}x{H}_strict.npz"))
    assert same_bits(want["rgb"], g["rgb"].reshape(-1, 3))  # (the yardstick is the fixture's frame)
    got = sh.shade(*rays.pinhole(cam, W, H), kernel, regroup)
    equal(got, want)
    check_counters(got["info"], want["stats"])
    sh.r.close()
