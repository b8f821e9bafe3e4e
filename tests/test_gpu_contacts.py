"""Contact queries (rt_sweep_contacts: Renderer.sweep_contacts / contacts_info) against tests/contacts_ref.py, the
yardstick built on tests/sweep_ref.py's numpy float32 restatement of toi, which tests/test_contacts_abi.py holds between
two float64 brute-force sets on the CPU. An answer is triangle indices, times, points and a count with defined bits, so
every comparison is array_equal / same_bits and no case is excluded; every check also checks the info counters' sums.
Per scene the sweeps are tests/test_gpu_sweep.py's 640 (512 from sweep_ref.fixture_sweeps plus 128 of the 64 x 36
camera's primary rays with radii from the fixture's set), rebuilt here; the members are computed once per module."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import contacts_ref, sweep_ref
from tests.contacts_ref import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
FMAX = sweep_ref.FMAX
KERNELS = ["strict", "fast"]
W, H = 64, 36
NS, NC = 512, 128
N = NS + NC
CHUNK = 256  # QUERY_CHUNK (rt_query.hpp)
KS = (1, 4, 8, 16)
# every (k, count_all) a request can make: the four capacities, a k inside one, and the pure count
VARIANTS = [(0, True)] + [(k, a) for k in KS for a in (False, True)]
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


def query(r, c, d, rad, k, kernel, t_max=None, count_all=False):
    """(tri, t, count, point, info)"""
    out = r.sweep_contacts(cuda(c), cuda(d), cuda(rad), k=k, t_max=None if t_max is None else cuda(t_max),
                           count_all=count_all, points_out=True, kernel=kernel)
    info = r.contacts_info()
    tri, t, count = (x.cpu().numpy() for x in out[:3])
    point = out[3].cpu().numpy() if len(out) > 3 else np.zeros((len(c), 0, 3), F)  # (k = 0 stores nothing)
    return tri, t, count, point, info


def check(got, want, total, what=""):
    """every output against the yardstick's (tri, t, count, point), and the info counters' sums; total: |S_i|"""
    tri, t, count, point, info = got
    k = want[0].shape[1]
    assert tri.shape == want[0].shape and t.shape == want[1].shape, what
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    bad = np.nonzero((t.view(np.int32) != want[1].view(np.int32)).any(axis=1))[0] if k else []
    assert len(bad) == 0, (what, bad[:8], t[bad[:8]], want[1][bad[:8]])
    np.testing.assert_array_equal(count, want[2], err_msg=str(what))
    if k:
        assert same_bits(point, want[3]), what
    n = len(tri)
    assert info["spheres"] == n and info["stack_overflows"] == 0, (what, info)
    assert info["found"] == int((total > 0).sum()) and info["found"] + info["empty_spheres"] == n, (what, info)
    assert info["tris_stored"] == int(np.minimum(total, k).sum()), (what, info)
    assert info["tris_counted"] == int(want[2].sum()), (what, info)


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
    """one fixture scene: a Renderer, the N sweeps and the yardstick's members for them, unbounded and with t_max = 1"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.c, self.d, self.rad = fixture_sweeps(self.coords, seed)
        self.one = np.ones(N, F)
        self.mem = {None: contacts_ref.members(self.c, self.d, self.rad, self.coords),
                    1: contacts_ref.members(self.c, self.d, self.rad, self.coords, self.one)}
        self.mx = max(16.0, float(np.abs(self.coords).max()))  # the scene's coordinate magnitude (rt_hip.hip)
        self._want = {}
        self.runs = {}

    def tm(self, bound):
        return None if bound is None else self.one

    def want(self, bound, k, count_all):
        """the yardstick's outputs for all N sweeps, computed once per variant and never changed"""
        key = (bound, k, count_all)
        if key not in self._want:
            w = contacts_ref.lists(self.mem[bound], self.c, self.d, self.coords, k, count_all)
            for x in w:
                x.setflags(write=False)
            self._want[key] = w
        return self._want[key]


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, 41 + k) for k, (name, s) in enumerate(scenes.items())}
    yield out
    for f in out.values():
        f.r.close()


def rows_of(want, rows):
    return tuple(x[rows] for x in want)


# ------------------------------------------------------------------ 0. the fixture's variety (CPU work)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_the_fixture_has_every_size_class_and_boundary_ties(fix, scene):
    """measured: |S_i| = 0 / 1..16 / above 16 without a bound car_boxed 46 / 330 / 264, car_only 177 / 185 / 278; with
    t_max = 1 156 / 242 / 242 and 209 / 169 / 262; the largest |S_i| 9,155 and 5,776; 57 and 31 sweeps touching at the
    start; sweeps whose k-th and (k+1)-th toi tie bit for bit, k = 1 / 4 / 8 / 16: 31 / 57 / 72 / 97 and 110 / 87 / 84 /
    89"""
    f = fix[scene]
    for bound in (None, 1):
        tot = f.mem[bound].total
        sizes = (int((tot == 0).sum()), int(((tot >= 1) & (tot <= 16)).sum()), int((tot > 16).sum()))
        print(f"{scene} t_max={bound}: |S_i| = 0 / 1..16 / above 16: {sizes}, largest {int(tot.max())}")
        assert min(sizes) >= 32, (scene, bound, sizes)
    mem = f.mem[None]
    rows, first = contacts_ref.kth_toi(mem, 1)
    ties = [int(contacts_ref.boundary_ties(mem, k).sum()) for k in KS]
    print(f"{scene}: {int((first == 0).sum())} touching at the start, boundary ties at k = 1 / 4 / 8 / 16: {ties}")
    assert (first == 0).sum() >= 16 and min(ties) >= 16, (scene, ties)
    assert (f.mem[1].total <= mem.total).all() and (f.mem[1].total < mem.total).sum() >= 32


# ------------------------------------------------------------------ 1. fixture sweeps, all variants
def run_in_order(f, kernel, bound, k, count_all):
    """the N fixture sweeps in their own order under one variant, run once per module and kept for the comparison of
    the two kernels"""
    key = (kernel, bound, k, count_all)
    if key not in f.runs:
        f.runs[key] = query(f.r, f.c, f.d, f.rad, k, kernel, f.tm(bound), count_all)
    return f.runs[key]


@pytest.mark.parametrize("order", ["in order", "permuted"])
@pytest.mark.parametrize("bound", [None, 1])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_sweeps_all_variants(fix, scene, kernel, bound, order):
    f = fix[scene]
    p = np.random.default_rng(11).permutation(N)
    ms = 0.0
    for k, count_all in VARIANTS:
        want = f.want(bound, k, count_all)
        what = (scene, kernel, bound, k, count_all, order)
        if order == "in order":
            got = run_in_order(f, kernel, bound, k, count_all)
            check(got, want, f.mem[bound].total, what=what)
        else:
            got = query(f.r, f.c[p], f.d[p], f.rad[p], k, kernel, None if bound is None else f.one[p], count_all)
            check(got, rows_of(want, p), f.mem[bound].total[p], what=what)
        check_path(got[4], kernel, N, len(f.coords))
        ms += got[4]["kernel_ms"]
    print(f"{scene} {kernel} t_max={bound} {order}: {ms:.1f} ms in {len(VARIANTS)} kernels")


# ------------------------------------------------------------------ 2. fast against strict
@pytest.mark.parametrize("bound", [None, 1])
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fast_against_strict(fix, scene, bound):
    """the two kernels on the same runs (case 1's, in order), output by output, and the counters that do not describe
    the path"""
    f = fix[scene]
    for k, count_all in VARIANTS:
        a = run_in_order(f, "strict", bound, k, count_all)
        b = run_in_order(f, "fast", bound, k, count_all)
        what = (scene, bound, k, count_all)
        np.testing.assert_array_equal(a[0], b[0], err_msg=str(what))
        assert same_bits(a[1], b[1]) and same_bits(a[3], b[3]), what
        np.testing.assert_array_equal(a[2], b[2], err_msg=str(what))
        for key in ("spheres", "found", "tris_stored", "tris_counted", "empty_spheres", "stack_overflows"):
            assert a[4][key] == b[4][key], (what, key)
        assert b[4]["tris_tested"] < a[4]["tris_tested"], what  # (the walk tests fewer triangles than the loop)


# ------------------------------------------------------------------ 3. k = 1 is the sweep query
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_k1_is_the_sweep_query_bit_for_bit(fix, scene):
    f = fix[scene]
    c, d, rad = cuda(f.c), cuda(f.d), cuda(f.rad)
    for bound in (None, 1):
        tm = None if bound is None else cuda(f.one)
        out1 = f.r.sweep(c, d, rad, t_max=tm, kernel="fast")
        found = f.r.sweep_info()["found"]  # (synchronises the renderer's stream)
        tri1, t1, p1 = (x.cpu().numpy() for x in out1)
        assert found >= N // 2
        for kernel in KERNELS:
            out = f.r.sweep_contacts(c, d, rad, k=1, t_max=tm, points_out=True, kernel=kernel)
            info = f.r.contacts_info()
            tri, t, count, point = (x.cpu().numpy() for x in out)
            np.testing.assert_array_equal(tri[:, 0], tri1)
            assert same_bits(t[:, 0], t1) and same_bits(point[:, 0], p1), (scene, bound, kernel)
            np.testing.assert_array_equal(count, (tri1 >= 0).astype(np.int32))
            assert info["found"] == found == info["tris_stored"]


# ------------------------------------------------------------------ 4. every triangle twice
def test_every_triangle_twice(dev, scenes, fix):
    """car_only with every triangle twice (copy j + m of triangle j, the same record): each contact ties with its copy
    and every count_all count is exactly doubled -- a record offered twice, or a copy lost at the list's boundary,
    cannot pass. The yardstick is the members with their copies (same toi, index + m) in key order. Where no two
    DIFFERENT triangles tie among a sweep's listed contacts, the list of 2k entries is the first k contacts each followed
    by its copy; where they do, the order by (toi, index) puts a tie group's originals before its copies, so that form
    is asserted on the sweeps it applies to and the yardstick's on all."""
    s = scenes["car_only"]
    f = fix["car_only"]
    m = len(f.coords)
    t = s.triangles
    coords2 = np.concatenate([f.coords, f.coords])
    twice = host.Scene(host.triangle_init(coords2, *(np.concatenate([t[k], t[k]]) for k in ("ks", "kd", "kr"))),
                       s.lights.copy())
    r = dev.Renderer(0).upload(twice.build_bvh(3))
    for bound in (None, 1):
        mem = f.mem[bound]
        mem2 = contacts_ref.Members(N, np.concatenate([mem.si, mem.si]), np.concatenate([mem.ti, mem.ti + m]),
                                    np.concatenate([mem.toi, mem.toi]))
        assert np.array_equal(mem2.total, 2 * mem.total)
        for k2 in (2, 8, 16):
            want = contacts_ref.lists(mem2, f.c, f.d, coords2, k2)
            tri1, t1, _, p1 = contacts_ref.lists(mem, f.c, f.d, f.coords, k2 // 2)
            pairs = np.repeat(tri1, 2, axis=1)
            pairs[:, 1::2] = np.where(tri1 >= 0, tri1 + m, -1)
            paired = (pairs == want[0]).all(axis=1)  # the sweeps whose list is (j, j + m) pairs
            assert paired.sum() >= N // 2 and (~paired).sum() >= 16, (bound, k2, int(paired.sum()))
            assert same_bits(np.repeat(t1, 2, axis=1)[paired], want[1][paired])
            assert same_bits(np.repeat(p1, 2, axis=1)[paired], want[3][paired])
            for kernel in KERNELS:
                got = query(r, f.c, f.d, f.rad, k2, kernel, f.tm(bound))
                check(got, want, mem2.total, what=("twice", bound, kernel, k2))
                short = 2 * mem.total <= k2  # a list that holds all of S_i: every entry with its copy, the same toi
                for i in np.nonzero(short)[0][:64]:
                    n = int(mem.total[i])
                    assert np.array_equal(np.sort(got[0][i, :2 * n]),
                                          np.sort(np.concatenate([mem.ti[mem.si == i], mem.ti[mem.si == i] + m])))
        for kernel in KERNELS:
            for k in (0, 8):
                got = query(r, f.c, f.d, f.rad, k, kernel, f.tm(bound), count_all=True)
                np.testing.assert_array_equal(got[2], 2 * mem.total, err_msg=str((bound, kernel, k)))
                assert got[4]["tris_counted"] == 2 * int(mem.total.sum())
    r.close()


# ------------------------------------------------------------------ 5. t_max around the k-th toi
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_t_max_around_the_kth_toi(fix, scene, k):
    """every second fixture sweep with t_max at its k-th toi, one float below it and one float above it (no bound for
    a sweep with fewer than k members): at and above keep the k-th entry and whatever ties it, below drops them"""
    f = fix[scene]
    sel = np.arange(0, N, 2)
    c, d, rad = f.c[sel], f.d[sel], f.rad[sel]
    at = np.full(N, np.inf, F)
    rows, kth = contacts_ref.kth_toi(f.mem[None], k)
    at[rows] = kth
    at = at[sel]
    has = np.isfinite(at)
    assert has.sum() >= 100
    below = np.where(has, np.nextafter(at, F(-1)), at)  # (a k-th toi of 0: a negative bound, the empty set)
    above = np.where(has, np.nextafter(at, F(np.inf)), at)
    for name, tm in (("at", at), ("below", below), ("above", above)):
        mem = contacts_ref.members(c, d, rad, f.coords, tm)
        if name == "below":
            assert (mem.total[has] < k).all()
        else:
            assert (mem.total[has] >= k).all()
            assert np.array_equal(contacts_ref.kth_toi(mem, k)[1].view(np.int32), at[has].view(np.int32))
        for K, count_all in ((k, False), (k, True), (8, False), (0, True)):
            want = contacts_ref.lists(mem, c, d, f.coords, K, count_all)
            for kernel in KERNELS:
                got = query(f.r, c, d, rad, K, kernel, tm, count_all)
                check(got, want, mem.total, what=(scene, k, name, K, count_all, kernel))


# ------------------------------------------------------------------ 6. special inputs
def special_sweeps(f):
    """(c, d, r, t_max, kind): invalid sweeps, d = 0, a radius that covers the scene, sweeps outside the walk's domain
    (max|c| or r above 2^20 mx, a nonzero |d.k| outside [2^-64, 2^64]) and at its edges"""
    mem = f.mem[None]
    rows1, toi1 = contacts_ref.kth_toi(mem, 1)
    first = np.full(N, FMAX, F)
    first[rows1] = toi1
    found = np.nonzero((mem.total > 0) & (first > 0) & (f.rad > 0) & (f.d != 0).all(axis=1))[0][:6]
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
        add(ci, di, NEG_SUB, np.inf, "invalid")
        add(ci, di, ri, np.nan, "invalid")
        add(ci, di, ri, -1.0, "invalid")
        add(ci, di, ri, NEG_TINY, "invalid")
        add(ci, di, ri, -0.0, "valid")  # (-0 is the bound 0)
        add(ci, di, ri, 0.0, "valid")
        add(ci, di, ri, np.inf, "valid")
        hit = ci + di * first[i]
        add(hit, [0, 0, 0], ri, np.inf, "still")           # d = 0 at the contact: within rounding of touching
        add(hit, [0, 0, 0], ri * F(1.01), np.inf, "still")  # ... and touching
        add(hit, [0, 0, 0], ri * F(2), 0.0, "still")        # ... with the bound 0 too
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
    mem = contacts_ref.members(c, d, r, f.coords, tm)
    inv = kind == "invalid"
    assert inv.sum() >= 100 and len(c) >= 300 and (mem.total[inv] == 0).all()
    assert (mem.total[kind == "valid"] > 0).any() and (mem.total[kind == "valid"] == 0).any()  # (the bound -0 is 0)
    assert (mem.total[kind == "huge"] == len(f.coords)).all()  # every triangle, all at toi 0
    assert (mem.total[kind == "still"] > 0).any() and (mem.total[kind == "still"] == 0).any()
    assert (mem.total[kind == "outside"] > 0).sum() >= 12 and (mem.total[kind == "edge"] > 0).sum() >= 12
    valid, outside = int((~inv).sum()), int((kind == "outside").sum())
    for k, count_all in ((4, False), (16, False), (8, True), (0, True)):
        want = contacts_ref.lists(mem, c, d, f.coords, k, count_all)
        if k:
            huge = kind == "huge"
            assert (want[0][huge] == np.arange(k)).all() and (want[1][huge] == 0).all()  # the lowest indices of the tie
            assert (want[0][inv] == -1).all() and (want[1][inv] == FMAX).all()
            assert same_bits(want[3][inv], np.repeat(c[inv][:, None], k, axis=1))  # c's own bits, NaNs included
        for kernel in KERNELS:
            got = query(f.r, c, d, r, k, kernel, tm, count_all)
            check(got, want, mem.total, what=(scene, kernel, k, count_all))
            check_path(got[4], kernel, valid, len(f.coords), outside=outside)
            assert (got[2][inv] == 0).all()


# ------------------------------------------------------------------ 7. sweep counts around QUERY_CHUNK
@pytest.mark.parametrize("kernel", KERNELS)
def test_sphere_count_edges(fix, kernel):
    import torch
    f = fix["car_boxed"]
    K = 4
    want = f.want(None, K, False)
    c, d, r = cuda(f.c[:CHUNK + 1]), cuda(f.d[:CHUNK + 1]), cuda(f.rad[:CHUNK + 1])
    for n in (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1):
        tri = torch.full((n * K + 3,), -77, dtype=torch.int32, device="cuda")
        t = torch.full((n * K + 3,), -77.0, dtype=torch.float32, device="cuda")
        count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        point = torch.full((3 * n * K + 3,), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the fills are torch's work; the query runs on the renderer's stream)
        f.r.sweep_contacts((c.data_ptr(), n), d.data_ptr(), r.data_ptr(), k=K, kernel=kernel, tri=tri.data_ptr(),
                           t=t.data_ptr(), count=count.data_ptr(), point=point.data_ptr())  # (the buffers are longer)
        info = f.r.contacts_info()
        assert info["spheres"] == n and info["tris_stored"] == int(want[2][:n].sum()) and info["stack_overflows"] == 0
        tri, t, count, point = tri.cpu().numpy(), t.cpu().numpy(), count.cpu().numpy(), point.cpu().numpy()
        np.testing.assert_array_equal(tri[:n * K].reshape(n, K), want[0][:n], err_msg=str(n))
        np.testing.assert_array_equal(count[:n], want[2][:n], err_msg=str(n))
        assert same_bits(t[:n * K].reshape(n, K), want[1][:n]), n
        assert same_bits(point[:3 * n * K].reshape(n, K, 3), want[3][:n]), n
        assert (tri[n * K:] == -77).all() and (t[n * K:] == -77).all() and (count[n:] == -77).all(), n
        assert (point[3 * n * K:] == -77).all(), n
    # a scalar radius, the default k, and no point output
    rows = np.nonzero(f.rad == f.rad[1])[0]
    out = f.r.sweep_contacts(cuda(f.c[rows]), cuda(f.d[rows]), float(f.rad[1]), kernel=kernel)
    f.r.sync()
    assert len(out) == 3
    w8 = f.want(None, 8, False)
    np.testing.assert_array_equal(out[0].cpu().numpy(), w8[0][rows])
    assert same_bits(out[1].cpu().numpy(), w8[1][rows]) and np.array_equal(out[2].cpu().numpy(), w8[2][rows])


# ------------------------------------------------------------------ 8. every structure
@pytest.mark.parametrize("accel,flags", [("auto", 0), ("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        for k, count_all in ((8, False), (16, True), (0, True)):
            got = query(r, f.c, f.d, f.rad, k, kernel, None, count_all)
            check(got, f.want(None, k, count_all), f.mem[None].total, what=(accel, flags, kernel, k))
            check_path(got[4], kernel, N, len(f.coords), wide=accel != "reference")
    r.close()


# ------------------------------------------------------------------ 9. a moved scene and a rebuilt scene
def test_moved_and_rebuilt_scene(dev, scenes, fix):
    """tests/test_gpu_nearest.py::test_moving_scene's car_boxed scaled by 1.3 and sheared: after update_vertices, and
    again after rebuild_views(mode="auto"), both kernels answer as the yardstick does on the moved coordinates and as a
    fresh upload of the moved scene does (every second fixture sweep; the point output goes through ref_inv, which no
    refit or rebuild may invalidate)"""
    s = scenes["car_boxed"]
    M = np.array([[1.3, 0.0, 0.0], [0.2, 1.3, 0.0], [0.0, -0.15, 1.3]], np.float32)
    coords = np.ascontiguousarray((s.triangles["coords"].reshape(-1, 3) @ M).reshape(-1, 3, 3), np.float32)
    f = fix["car_boxed"]
    rows = np.arange(0, N, 2)
    c, d, rad = f.c[rows], f.d[rows], f.rad[rows]
    mem = contacts_ref.members(c, d, rad, coords)
    want = {(k, a): contacts_ref.lists(mem, c, d, coords, k, a) for k, a in ((8, False), (0, True))}
    still = rows_of(f.want(None, 8, False), rows)
    assert (want[8, False][0] != still[0]).any(axis=1).sum() > 100 and (mem.total > 0).sum() > 100
    t = s.triangles
    moved = host.Scene(host.triangle_init(coords, t["ks"], t["kd"], t["kr"]), s.lights.copy()).build_bvh(3)
    fresh = dev.Renderer(0).upload(moved)
    fresh_out = {ka: query(fresh, c, d, rad, ka[0], "fast", None, ka[1]) for ka in want}
    fresh.close()
    r = dev.Renderer(0).upload(s)
    check(query(r, c, d, rad, 8, "fast"), still, f.mem[None].total[rows], what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="auto")
        for kernel in KERNELS:
            for (k, count_all), w in want.items():
                got = query(r, c, d, rad, k, kernel, None, count_all)
                check(got, w, mem.total, what=(step, kernel, k))
                for a, b in zip(got[:4], fresh_out[k, count_all][:4]):
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (step, kernel, k)
        assert got[4]["walked_spheres"] == len(rows)
    r.close()


# ------------------------------------------------------------------ 10. isolation
def test_a_contacts_query_leaves_renders_and_other_queries_alone(dev, scenes, fix):
    import torch
    from prt import rays
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    pts = cuda(f.coords[::97, 0])
    o, p = rays.pinhole(cam, W, H)
    lo, hi = (pts - 0.05).contiguous(), (pts + 0.05).contiguous()
    down = torch.zeros_like(pts)
    down[:, 1] = -1.0
    far = torch.full((o.shape[0],), 1e30, dtype=torch.float32, device="cuda")
    q = cuda(f.coords[::97] + F(0.01))
    c, d, rad = cuda(f.c), cuda(f.d), cuda(f.rad)
    torch.cuda.synchronize()  # (these tensors are torch's work; the queries run on the renderer's stream)

    def strip(info):
        return {k: v for k, v in info.items() if k != "kernel_ms"}

    def infos_of(r):
        return [r.query_info(), r.shade_info(), r.nearest_info(), r.neighbours_info(), r.overlaps_info(),
                r.hits_info(), r.sweep_info(), r.cuts_info()]

    def others(r):
        """the nine other queries"""
        occ = r.occluded(o, p, far)
        hit, t = r.trace_rays(o, p)
        rgb = r.shade_rays(o, p)
        near = r.nearest(pts)
        nb = r.nearest_tris(pts, k=4, points_out=True)  # (its points share ref_inv with the contacts query's)
        ov = r.overlaps(lo, hi, k=4)
        hits = r.trace_hits(o, p, max_hits=2)
        sw = r.sweep(pts, down, 0.01)
        cu = r.cuts(q, k=4)
        r.sync()
        out = [x.cpu().numpy() for x in (occ, hit, t, rgb, *near, *nb, *ov, *hits, *sw, *cu)]
        return out, infos_of(r)

    r = dev.Renderer(0).upload(scenes["car_boxed"])
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    frame0, stats0, launch0 = r.download(hit=True), r.stats(), r.launch_info()
    out0, infos0 = others(r)
    for kernel, k, count_all in (("fast", 16, False), ("strict", 4, True), ("fast", 0, True), ("fast", 8, False)):
        got = r.sweep_contacts(c, d, rad, k=k, kernel=kernel, count_all=count_all, points_out=True)
        ci = r.contacts_info()
        assert ci["spheres"] == N
    w8 = f.want(None, 8, False)
    assert np.array_equal(got[0].cpu().numpy(), w8[0]) and same_bits(got[3].cpu().numpy(), w8[3])
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
    cj = r.contacts_info()  # ... and none of them touched the contacts query's own counters
    assert strip(cj) == strip(ci) and abs(cj["kernel_ms"] - ci["kernel_ms"]) < 1e-4
    out = r.sweep_contacts(c, d, rad, k=8, points_out=True)
    r.sync()
    tri, t, count, point = (x.cpu().numpy() for x in out)
    assert np.array_equal(tri, w8[0]) and same_bits(t, w8[1]) and np.array_equal(count, w8[2])
    assert same_bits(point, w8[3])
    r.close()


# ------------------------------------------------------------------ 11. errors
def test_contacts_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    w4 = f.want(None, 4, False)
    c, d, rad = cuda(f.c), cuda(f.d), cuda(f.rad)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.sweep_contacts(c, d, rad)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no contacts query run yet
        r.contacts_info()
    r.sweep(c[:100], d[:100], rad[:100])
    with pytest.raises(dev.RtError, match="-5"):  # (a sweep query is not a contacts query)
        r.contacts_info()
    r.sweep_contacts(c[:100], d[:100], rad[:100], k=4)
    info = r.contacts_info()
    assert info["spheres"] == 100 and info["tris_stored"] == int(w4[2][:100].sum())
    with pytest.raises(dev.RtError, match="status -1"):
        r.sweep_contacts(c, d, rad, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.sweep_contacts((0, 16), d.data_ptr(), rad.data_ptr())  # null centre
    L = _lib.hip()
    tri = torch.empty(64, dtype=torch.int32, device="cuda")
    tt = torch.empty(64, dtype=torch.float32, device="cuda")
    pt = torch.empty(192, dtype=torch.float32, device="cuda")
    cnt = torch.empty(16, dtype=torch.int32, device="cuda")
    pc, pd, pr = c.data_ptr(), d.data_ptr(), rad.data_ptr()
    t, u, p, n = tri.data_ptr(), tt.data_ptr(), pt.data_ptr(), cnt.data_ptr()
    Q, R = _lib.SphereContacts, _lib.ContactResults
    for q, res in [
        (Q(None, pd, pr, None, 16, 4, 0, 0), R(t, u, p, n)),      # null centre, motion, radius
        (Q(pc, None, pr, None, 16, 4, 0, 0), R(t, u, p, n)),
        (Q(pc, pd, None, None, 16, 4, 0, 0), R(t, u, p, n)),
        (Q(pc, pd, pr, None, 16, -1, 0, 0), R(t, u, p, n)),       # max_tris out of range
        (Q(pc, pd, pr, None, 16, 17, 0, 0), R(t, u, p, n)),
        (Q(pc, pd, pr, None, 16, 4, 0, 0), R(None, None, None, n)),  # max_tris > 0 with tri, t and point all NULL
        (Q(pc, pd, pr, None, 16, 0, 0, 0), R(t, u, p, n)),        # max_tris = 0 without count_all
        (Q(pc, pd, pr, None, 16, 0, 1, 0), R(t, u, p, None)),     # ... and without count
        (Q(pc, pd, pr, None, 16, 4, 2, 0), R(t, u, p, n)),        # count_all not 0 / 1
        (Q(pc, pd, pr, None, 16, 4, -1, 0), R(t, u, p, n)),
        (Q(pc, pd, pr, None, 16, 4, 0, 3), R(t, u, p, n)),        # unknown kernel
        (Q(pc, pd, pr, None, 16, 4, 0, -1), R(t, u, p, n)),
        (Q(pc, pd, pr, None, -1, 4, 0, 0), R(t, u, p, n)),        # negative n
    ]:
        assert L.rt_sweep_contacts(r._ctx, ctypes.byref(q), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx)
    assert L.rt_sweep_contacts(r._ctx, None, None) == -1
    assert L.rt_sweep_contacts(r._ctx, ctypes.byref(Q(pc, pd, pr, None, 16, 4, 0, 0)), None) == -1
    assert L.rt_get_contacts_info(r._ctx, None) == -1
    after = r.contacts_info()  # a refused call leaves contacts_info() as it was
    assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in info.items() if k != "kernel_ms"}
    assert abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # one list output alone is enough, with or without count
    for res in (R(t, None, None, None), R(None, u, None, n), R(None, None, p, None)):
        assert L.rt_sweep_contacts(r._ctx, ctypes.byref(Q(pc, pd, pr, None, 16, 4, 0, 0)), ctypes.byref(res)) == 0
    r.sync()
    assert np.array_equal(tri.cpu().numpy().reshape(16, 4), w4[0][:16])
    assert same_bits(tt.cpu().numpy().reshape(16, 4), w4[1][:16]) and np.array_equal(cnt.cpu().numpy(), w4[2][:16])
    assert same_bits(pt.cpu().numpy().reshape(16, 4, 3), w4[3][:16])
    # the pure count needs count alone
    assert L.rt_sweep_contacts(r._ctx, ctypes.byref(Q(pc, pd, pr, None, 16, 0, 1, 0)),
                               ctypes.byref(R(None, None, None, n))) == 0
    r.sync()
    assert np.array_equal(cnt.cpu().numpy(), f.mem[None].total[:16])
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_sweep_contacts(r._ctx, ctypes.byref(Q(None, None, None, None, 0, 4, 0, 0)),
                               ctypes.byref(R(None, None, None, None))) == 0
    assert r.contacts_info()["spheres"] == 0
    r.close()
