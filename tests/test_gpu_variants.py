"""Every query on scenes of other magnitudes and shapes (tests/variants.py): one small generated mesh at its own size,
tiny, translated far from the origin, large, anisotropic, at sizes where products of coordinates and D itself
overflow, and cut down to one, two and nine triangles. Each of the nine geometry queries -- nearest, nearest_tris,
overlaps, sweep, sweep_contacts, cuts, clearance, proximity, trace_hits -- must give its numpy mirror's bits under
kernel="strict" and under kernel="fast", on the GPU-built and on the host-built views, and the fast kernel must have
walked the wide view to get them; trace_rays and occluded, which have no mirror, must agree between the kernels.

The mirrors' answers come from variants.expectations(), once per variant. test_the_variants_test_something holds the
counts that keep a variant from passing vacuously; it needs no renderer, only this module's mark."""
import numpy as np
import pytest

from tests import variants
from tests.nearest_ref import same_bits
from tests.variants import K, N

pytestmark = pytest.mark.gpu

KERNELS = ["strict", "fast"]
ACCELS = ["auto", "host"]


@pytest.fixture(scope="module")
def dev():
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    return device


@pytest.fixture(scope="module")
def renderers(dev):
    """one renderer per (variant, accel), made when first asked for; the four asked for last are kept"""
    made = {}

    def get(name, accel):
        if (name, accel) not in made:
            made[name, accel] = dev.Renderer(0).upload(variants.scene(name), accel=accel)
        r = made.pop((name, accel))
        made[name, accel] = r  # (the last asked for at the end)
        for key in list(made)[:-4]:
            made.pop(key).close()
        return r
    yield get
    for r in made.values():
        r.close()


def cuda(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()  # (a copy: the expectations are read-only)


def host_arrays(out, info=None):
    """the outputs on the host. info: the query's info call, made first -- it synchronises the renderer's stream, on
    which the query ran, and raises on an overflowed stack -> the arrays, with the info block when one was asked for"""
    block = info() if info is not None else None
    arrays = tuple(x.cpu().numpy() for x in out)
    return arrays if info is None else (arrays, block)


def equal(got, want, what):
    """bit for bit: array_equal on the integer arrays, same_bits on the float ones"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        if w.dtype == np.float32:
            assert same_bits(g, w), (what, j)
        else:
            np.testing.assert_array_equal(g, w, err_msg=str((what, j)))


def served(info, kernel, wide, walked, exhaustive, n=N, outside=0):
    """which loop served the n valid queries: under "fast" on a scene with a wide view the walk, but for the `outside`
    queries beyond the walk's stated domain; else the exhaustive loop"""
    assert info["stack_overflows"] == 0, info
    if kernel == "fast" and wide:
        assert info[walked] == n - outside and info[exhaustive] == outside, info
    else:
        assert info[exhaustive] == n and info[walked] == 0, info


def run_queries(r, e, kernel):
    """all nine queries of one renderer under one kernel against the expectations e"""
    import torch
    wide = r.scene_info()["wide_nodes"] > 0
    what = (e.name, kernel)
    # 1. nearest
    got, info = host_arrays(r.nearest(cuda(e.pts), kernel=kernel), r.nearest_info)
    equal(got, e.nearest[:3], what + ("nearest",))
    served(info, kernel, wide, "walked_points", "exhaustive_points")
    # 2. nearest_tris
    for ca in (False, True):
        (tri, d2, count, point), info = host_arrays(
            r.nearest_tris(cuda(e.pts), k=K, count_all=ca, points_out=True, kernel=kernel), r.neighbours_info)
        equal((tri, d2, point, count), e.neighbours[ca], what + ("nearest_tris", ca))
        served(info, kernel, wide, "walked_points", "exhaustive_points")
    # 3. overlaps
    for ca in (False, True):
        got, info = host_arrays(r.overlaps(cuda(e.lo), cuda(e.hi), k=K, count_all=ca, kernel=kernel), r.overlaps_info)
        equal(got, e.overlaps[ca], what + ("overlaps", ca))
        served(info, kernel, wide, "walked_boxes", "exhaustive_boxes")
    # 4. sweep
    c, d, rad = (cuda(x) for x in e.sweeps)
    out = N - e.sweep_walks
    got, info = host_arrays(r.sweep(c, d, rad, kernel=kernel), r.sweep_info)
    equal(got, e.sweep[:3], what + ("sweep",))
    served(info, kernel, wide, "walked_spheres", "exhaustive_spheres", outside=out)
    # 5. sweep_contacts
    for ca in (False, True):
        got, info = host_arrays(r.sweep_contacts(c, d, rad, k=K, count_all=ca, points_out=True, kernel=kernel),
                                r.contacts_info)
        equal(got, e.contacts[ca], what + ("sweep_contacts", ca))
        served(info, kernel, wide, "walked_spheres", "exhaustive_spheres", outside=out)
    # 6. cuts
    for ca in (False, True):
        got, info = host_arrays(r.cuts(cuda(e.cut_q), k=K, count_all=ca, kernel=kernel), r.cuts_info)
        equal(got, e.cuts[ca], what + ("cuts", ca))
        served(info, kernel, wide, "walked", "exhaustive")
    # 7. clearance
    q = cuda(e.clear_q)
    kind = torch.empty(N, dtype=torch.int32, device="cuda")
    tri, d2, oq, om = r.clearance(q, kernel=kernel, kind=kind)
    got, info = host_arrays((tri, d2, oq, om, kind), r.clearance_info)
    equal(got, e.clearance[:5], what + ("clearance",))
    served(info, kernel, wide, "walked", "exhaustive")
    # 8. proximity
    for ca in (False, True):
        kind = torch.empty((N, K), dtype=torch.int32, device="cuda")
        tri, d2, count, oq, om = r.proximity(q, k=K, count_all=ca, pairs_out=True, kernel=kernel, kind=kind)
        got, info = host_arrays((tri, d2, oq, om, kind, count), r.proximity_info)
        equal(got, e.proximity[ca][:6], what + ("proximity", ca))
        served(info, kernel, wide, "walked", "exhaustive")
    # 9. trace_hits: the rays as they are and with unit directions
    for rays, want, walks in ((e.rays, e.hits, e.ray_walks), (e.unit_rays, e.unit_hits, e.unit_ray_walks)):
        o, dr = cuda(rays[0]), cuda(rays[1])
        for ca in (False, True):
            got, info = host_arrays(r.trace_hits(o, dr, max_hits=K, count_all=ca, kernel=kernel), r.hits_info)
            equal(got, want[ca], what + ("trace_hits", ca, walks))
            assert info["stack_overflows"] == 0, info
            walked = info["unit_rays"] + info["short_rays"] + info["full_rays"]
            assert walked + info["exhaustive_rays"] == N, info
            if kernel == "fast" and wide:
                assert walked == walks, info
            elif kernel == "strict":
                assert info["exhaustive_rays"] == N, info


def rays_agree(r, e):
    """trace_rays and occluded have no numpy mirror: the fast kernel's answer is the strict one's"""
    for rays in (e.rays, e.unit_rays):
        o, d = cuda(rays[0]), cuda(rays[1])
        with np.errstate(over="ignore"):
            md = cuda((rays[1].astype(np.float64) ** 2).sum(1).astype(np.float32))  # up to the aimed-at centroid
        (hs, ts), _ = host_arrays(r.trace_rays(o, d, kernel="strict"), r.query_info)
        (hf, tf), info = host_arrays(r.trace_rays(o, d, kernel="fast"), r.query_info)
        assert info["stack_overflows"] == 0 and info["rays"] == N, info
        np.testing.assert_array_equal(hf, hs, err_msg=e.name)
        assert same_bits(tf, ts), e.name
        (os_,), _ = host_arrays((r.occluded(o, d, md, kernel="strict"),), r.query_info)
        (of,), info = host_arrays((r.occluded(o, d, md, kernel="fast"),), r.query_info)
        assert info["stack_overflows"] == 0 and info["rays"] == N, info
        np.testing.assert_array_equal(of, os_, err_msg=e.name)


# ------------------------------------------------------------------ 1. what makes the variants a test
def test_the_variants_test_something():
    """the mirrors' own counts, as tests/test_variants_host.py holds them on the CPU (no GPU work; the expectations
    are the ones the tests below use)"""
    for name in variants.MULTI:
        variants.check_figures(name)


# ------------------------------------------------------------------ 2. every variant, both builds, both kernels
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", variants.NAMES)
def test_queries_match_the_mirrors(renderers, name, accel, kernel):
    r = renderers(name, accel)
    info = r.scene_info()
    assert info["wide_nodes"] > 0 and info["n_triangles"] == len(variants.coords(name))
    if accel == "host":
        assert info["accel_built"] == "host"
    if name in variants.MULTI:
        assert info["wide_nodes"] > 34  # more than the triangles need at 32 a node: no view of nothing
    run_queries(r, variants.expectations(name), kernel)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", variants.NAMES)
def test_ray_queries_agree_between_the_kernels(renderers, name, accel):
    rays_agree(renderers(name, accel), variants.expectations(name))


# ------------------------------------------------------------------ 3. the full sets
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["moved", "aniso"])
def test_csr_sets(renderers, name, kernel):
    e = variants.expectations(name)
    r = renderers(name, "auto")
    off, tri = host_arrays(r.overlaps_csr(cuda(e.lo), cuda(e.hi), kernel=kernel))
    np.testing.assert_array_equal(off, e.overlap_sets[0])
    np.testing.assert_array_equal(tri, e.overlap_sets[1])
    assert r.overlaps_info()["stack_overflows"] == 0
    off, tri, seg = host_arrays(r.cuts_csr(cuda(e.cut_q), kernel=kernel))
    np.testing.assert_array_equal(off, e.cut_sets[0])
    np.testing.assert_array_equal(tri, e.cut_sets[1])
    assert same_bits(seg, e.cut_sets[2])
    assert r.cuts_info()["stack_overflows"] == 0
    assert len(e.overlap_sets[1]) > N and len(e.cut_sets[1]) > N


# ------------------------------------------------------------------ 4. a moving scene
def test_moving_scene(dev):
    """`plain` moved to `moved`'s coordinates: after update_vertices, after rebuild_views(mode="device") and after
    rebuild_views(mode="host") all nine queries give the moved mirror's bits"""
    e = variants.expectations("moved")
    r = dev.Renderer(0).upload(variants.scene("plain"))
    assert r.scene_info()["accel_built"] == "gpu"
    coords = cuda(e.coords)
    for step in ("update", "device", "host"):
        if step == "update":
            r.update_vertices(coords)
        else:
            r.rebuild_views(coords, mode=step)
            assert r.rebuild_info()["mode_used"] == step
        assert r.scene_info()["wide_nodes"] > 34
        for kernel in KERNELS:
            run_queries(r, e, kernel)
        rays_agree(r, e)
    r.close()


# ------------------------------------------------------------------ 5. the coordinate limit
def test_coordinates_beyond_the_limit_are_refused(dev):
    """RT_COORD_MAX = 2^123: an upload and an update beyond it are errors that change nothing"""
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="RT_COORD_MAX"):
        r.upload(variants.scene("edge"))
    e = variants.expectations("plain")
    r.upload(variants.scene("plain"))
    before, _ = host_arrays(r.nearest(cuda(e.pts), kernel="fast"), r.nearest_info)
    with pytest.raises(dev.RtError, match="RT_COORD_MAX"):
        r.update_vertices(cuda(variants.coords("edge")))
    equal(host_arrays(r.nearest(cuda(e.pts), kernel="fast"), r.nearest_info)[0], before, "after the refused update")
    equal(before, e.nearest[:3], "plain")
    r.close()
