"""One small generated mesh at other magnitudes and shapes, its query sets and the numpy mirrors' answers for them
(tests/test_variants_host.py on the CPU, tests/test_gpu_variants.py on the GPU).

The mesh M (float64, 1,088 triangles) is a bumpy UV sphere without poles -- 32 steps around, 16 from 0.15 to pi - 0.15,
radius 1 + 0.15 sin 3u sin 2v, z scaled by 0.8, two triangles per quad over shared vertices: 960 triangles with many
exact ties -- and a flat sheet of 8 x 8 quads exactly in the plane z = -1.25 over [-1.5, 1.5]^2: 128 triangles whose
boxes have no thickness on one axis. Every variant is formed in float64 and then rounded to float32; R (a fixed
rotation) keeps a variant from being a bit-shift of another:

  plain   M                                   mx at its floor of 16
  tiny    M * 3.1e-4                          extent about twice the inflation: every box overlaps every other
  moved   M R^T + (3000.25, -1999.6, 517.3)   mx about 1,500 x extent: D is dominated by rounding
  far     M + (70001.3, 65000.7, -81234.9)    ulp(mx) about 1/128 of the extent
  large   M R^T * 1.7e6                       ordinary arithmetic, large exponents
  aniso   M * (1000, 1, 0.001)                slivers, many contacts per sweep
  huge    M R^T * 2.9e17                      products of three coordinates overflow
  beyond  M * 1e20                            D itself overflows for most pairs; a box's area overflows float32
  few1, few2, few9                            the first 1, 2, 9 triangles of moved: root-only views

The query sets (N = 256 per kind and variant) come from the mirrors' own generators, every one of which scales with the
scene's box. expectations(name) runs every mirror once per process and variant; nothing in it touches the library."""
import functools
import warnings

import numpy as np

from tests import clearance_ref, contacts_ref, cut_ref, hits_ref, nearest_ref, neighbours_ref, overlap_ref, \
    proximity_ref, sweep_ref

F = np.float32
N = 256
K = 8
NAMES = ["plain", "tiny", "moved", "far", "large", "aniso", "huge", "beyond", "few1", "few2", "few9"]
MULTI = NAMES[:8]  # the variants of all 1,088 triangles


def mesh():
    """M: [1088, 3, 3] float64"""
    nu, nv = 32, 16
    u = 2 * np.pi * np.arange(nu) / nu
    v = np.linspace(0.15, np.pi - 0.15, nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    r = 1 + 0.15 * np.sin(3 * uu) * np.sin(2 * vv)
    P = np.stack([r * np.sin(vv) * np.cos(uu), r * np.sin(vv) * np.sin(uu), 0.8 * r * np.cos(vv)], axis=-1)
    tris = []
    for i in range(nu):
        j = (i + 1) % nu
        for k in range(nv - 1):
            a, b, c, d = P[i, k], P[j, k], P[j, k + 1], P[i, k + 1]
            tris += [[a, b, c], [a, c, d]]
    g = np.linspace(-1.5, 1.5, 9)
    for i in range(8):
        for k in range(8):
            a, b, c, d = ([g[i], g[k], -1.25], [g[i + 1], g[k], -1.25], [g[i + 1], g[k + 1], -1.25],
                          [g[i], g[k + 1], -1.25])
            tris += [[a, b, c], [a, c, d]]
    out = np.array(tris, np.float64)
    assert out.shape == (1088, 3, 3)
    return out


def rotation():
    return np.linalg.qr(np.random.default_rng(1).normal(size=(3, 3)))[0]


def coords64(name):
    """the variant's coordinates before rounding: [n, 3, 3] float64 (`edge`, M * 2e37, is the host tests' own case)"""
    M, R = mesh(), rotation()
    if name in ("few1", "few2", "few9"):
        return coords64("moved")[:int(name[3:])]
    return {"plain": lambda: M,
            "tiny": lambda: M * 3.1e-4,
            "moved": lambda: M @ R.T + np.array([3000.25, -1999.6, 517.3]),
            "far": lambda: M + np.array([70001.3, 65000.7, -81234.9]),
            "large": lambda: M @ R.T * 1.7e6,
            "aniso": lambda: M * np.array([1000.0, 1.0, 0.001]),
            "huge": lambda: M @ R.T * 2.9e17,
            "beyond": lambda: M * 1e20,
            "edge": lambda: M * 2e37}[name]()


@functools.lru_cache(maxsize=None)
def coords(name):
    """[n, 3, 3] float32, read-only"""
    c = np.ascontiguousarray(coords64(name).astype(F))
    c.setflags(write=False)
    return c


def triangles(c64):
    """TRI_DTYPE records of float64 coordinates: coords and centroid (the float64 mean) rounded, kd = 0.5, the two norm
    rows, as tests/test_gpu_nearest.py::test_degenerate_triangles makes them"""
    from prt import host
    t = np.zeros(len(c64), host.TRI_DTYPE)
    with np.errstate(over="ignore"):
        t["coords"] = c64
        t["centroid"] = np.asarray(c64, np.float64).mean(1)
    t["kd"] = 0.5
    t["norm"][:, 0] = [0, 0, 1]
    t["norm"][:, 1] = [0, 0, -1]
    return t


def scene(name, heuristic=3):
    """the variant as a host.Scene without lights, its BVH built"""
    from prt import host
    return host.Scene(triangles(coords64(name)), np.zeros(0, host.LIGHT_DTYPE)).build_bvh(heuristic)


def inflation(c):
    """the upload's own: 2^-16 of max(16, max|coordinate|), in float32"""
    return np.ldexp(F(max(16.0, float(np.abs(c).max()))), -16)


# ------------------------------------------------------------------ the query sets
def _box(c):
    v = np.asarray(c, np.float64).reshape(-1, 3)
    return v.min(0), v.max(0)


def _uniform(c, n, rng):
    lo, hi = _box(c)
    g = (hi - lo) / 4
    return rng.random((n, 3)) * (hi - lo + 2 * g) + (lo - g)


def _noisy_centroids(c, n, rng):
    ext = overlap_ref.scene_extent(c)
    return np.asarray(c, np.float64)[rng.integers(0, len(c), n)].mean(1) + rng.normal(0, 0.005 * ext, (n, 3))


def points(c, seed=31):
    """64 noisy centroids (noise 0.5 % of the extent), 64 exact vertices, 128 uniform in the box grown by a quarter"""
    rng = np.random.default_rng(seed)
    cen = _noisy_centroids(c, 64, rng)
    vert = np.asarray(c, np.float64)[rng.integers(0, len(c), 64), rng.integers(0, 3, 64)]
    return np.ascontiguousarray(np.concatenate([cen, vert, _uniform(c, 128, rng)]).astype(F))


def rays(c, seed=37):
    """N rays from uniform points of the grown box towards noisy centroids, not normalised"""
    rng = np.random.default_rng(seed)
    o = _uniform(c, N, rng)
    d = _noisy_centroids(c, N, rng) - o
    return np.ascontiguousarray(o.astype(F)), np.ascontiguousarray(d.astype(F))


def unit_rays(c, seed=37):
    """the same rays with directions of length 1: inside the ray walks' domain whatever the scene's size"""
    rng = np.random.default_rng(seed)
    o = _uniform(c, N, rng)
    d = _noisy_centroids(c, N, rng) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(o.astype(F)), np.ascontiguousarray(d.astype(F))


def ray_domain(o, d, mx):
    """the rays the fast ray walks serve (rt_query.hpp query_domain): finite, 2^-20 <= max|d_i| <= 2^20,
    max|o_i| <= 4 mx; the others run the exhaustive loop under either kernel"""
    dm = np.abs(d).max(1)
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (dm >= F(2.0 ** -20)) & (dm <= F(2.0 ** 20)) & \
        (np.abs(o).max(1) <= F(4) * mx)


def sweep_domain(c, d, r, mx):
    """the sweeps the walk serves (rt_sweep.hpp sweep_domain): every nonzero |d_i| in [2^-64, 2^64], max|c_i| and r at
    most 2^20 mx; the others run the exhaustive loop under either kernel"""
    ad = np.abs(d)
    ok = ((ad == 0) | ((ad >= F(2.0 ** -64)) & (ad <= F(2.0 ** 64)))).all(1)
    cm = np.ldexp(mx, 20)
    return ok & (np.abs(c).max(1) <= cm) & (r <= cm)


class Expectations:
    """one variant's queries and every mirror's answer for them (arrays are shared between tests: leave them alone)"""

    def __init__(self, name):
        c = coords(name)
        self.name, self.coords = name, c
        self.mx = F(max(16.0, float(np.abs(c).max())))
        self.pts = points(c)
        self.lo, self.hi = overlap_ref.surface_boxes(c, N, 41)
        self.sweeps = sweep_ref.fixture_sweeps(c, N, 43)
        self.cut_q = cut_ref.surface_tris(c, N, 47)
        self.clear_q = clearance_ref.fixture_tris(c, N, 53)
        self.rays = rays(c)
        self.ray_walks = int(ray_domain(*self.rays, self.mx).sum())
        self.sweep_walks = int(sweep_domain(*self.sweeps, self.mx).sum())
        for q in (self.pts, self.lo, self.hi, *self.sweeps, self.cut_q, self.clear_q, *self.rays):
            assert np.isfinite(q).all()
        # 1. nearest; 2. nearest_tris (k = 8, count_all both ways)
        self.nearest = nearest_ref.expected(self.pts, c, ties=True)
        tab = neighbours_ref.table(self.pts, c)
        self.neighbours = {ca: neighbours_ref.answer(tab, min(K, 16), count_all=ca) for ca in (False, True)}
        # 3. overlaps and its CSR sets
        self.overlap_sets = overlap_ref.sets(self.lo, self.hi, c)
        self.overlaps = {ca: overlap_ref.answer(self.overlap_sets, K, ca) for ca in (False, True)}
        # 4. sweep; 5. sweep_contacts
        self.sweep = sweep_ref.expected(*self.sweeps, c)
        self.members = contacts_ref.members(*self.sweeps, c)
        self.contacts = {ca: contacts_ref.lists(self.members, self.sweeps[0], self.sweeps[1], c, K, ca)
                         for ca in (False, True)}
        # 6. cuts and its CSR sets with the segments
        self.cut_sets = cut_ref.sets(self.cut_q, c)
        self.cuts = {ca: overlap_ref.answer(self.cut_sets[:2], K, ca) for ca in (False, True)}
        # 7. clearance (counts=True: pairs evaluated, pairs whose box bound exceeded their D); 8. proximity
        self.clearance = clearance_ref.expected(self.clear_q, c, counts=True)
        self.proximity = {ca: proximity_ref.lists(self.clear_q, c, K, count_all=ca) for ca in (False, True)}
        # 9. trace_hits
        self.unit_rays = unit_rays(c)
        self.unit_ray_walks = int(ray_domain(*self.unit_rays, self.mx).sum())
        self.hits, self.unit_hits = {}, {}
        for r, out in ((self.rays, self.hits), (self.unit_rays, self.unit_hits)):
            with warnings.catch_warnings():  # (n = e1 x e2 overflows on `beyond`; the mirror's threads warn of it)
                warnings.simplefilter("ignore", RuntimeWarning)
                tri, t, count, total = hits_ref.expected(hits_ref.hit_lists(*r, c), K)
            out[False], out[True] = (tri, t, count), (tri, t, total)

    def figures(self):
        """the counts that keep a variant from passing vacuously, read off the mirrors"""
        kind = self.clearance[4]
        return {"nearest found": int((self.nearest[0] >= 0).sum()),
                "nearest ties": int((self.nearest[3] >= 2).sum()),
                "sweep found": int((self.sweep[0] >= 0).sum()),
                "sweep ties": int((self.sweep[3] >= 2).sum()),
                "overlaps non-empty": int((self.overlaps[True][1] > 0).sum()),
                "cuts non-empty": int((self.cuts[True][1] > 0).sum()),
                "clearance found": int((self.clearance[0] >= 0).sum()),
                "kinds 0-5": int(((kind >= 0) & (kind <= 5)).sum()),
                "kinds 6-14": int(((kind >= 6) & (kind <= 14)).sum()),
                "kind 15": int((kind == 15).sum()),
                "bound above D": int(self.clearance[7]),
                "rays hit": int((self.hits[True][2] > 0).sum()),
                "unit rays hit": int((self.unit_hits[True][2] > 0).sum()),
                "rays walked": self.ray_walks, "unit rays walked": self.unit_ray_walks,
                "sweeps walked": self.sweep_walks}


@functools.lru_cache(maxsize=None)
def expectations(name):
    return Expectations(name)


def check_figures(name):
    """the conditions on the mirrors' output that keep a multi-triangle variant from passing vacuously -> its figures"""
    f = expectations(name).figures()
    print(name, f)
    if name in ("plain", "tiny", "moved", "far", "large"):
        assert f["nearest found"] == N and f["nearest ties"] >= 64
        assert f["sweep found"] >= 192 and f["overlaps non-empty"] >= 192 and f["cuts non-empty"] >= 192
        assert f["clearance found"] == N
        assert f["kinds 0-5"] >= 16 and f["kinds 6-14"] >= 16 and f["kind 15"] >= 16
        assert f["bound above D"] == 0  # no pair's record-box bound exceeds its D
    elif name == "aniso":
        assert f["sweep found"] >= 128 and f["overlaps non-empty"] >= 128 and f["cuts non-empty"] >= 128
        assert f["sweep ties"] >= 64  # several members at the winning toi
    else:  # huge, beyond: NaN, inf and the clamps decide
        assert f["sweep found"] <= 32 and f["cuts non-empty"] == 0 and f["kind 15"] == 0
        if name == "huge":
            assert f["nearest found"] == N
        else:
            assert 64 <= f["nearest found"] <= 224
    # the walks' stated domains: unit directions are inside the ray walks' on every scene that an |o| <= 4 mx allows,
    # `beyond`'s motions (above 2^64) are outside the sweep walk's
    assert f["unit rays walked"] == N
    assert f["sweeps walked"] == (0 if name == "beyond" else N)
    return f
