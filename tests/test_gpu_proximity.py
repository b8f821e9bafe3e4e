"""Proximity queries (rt_proximity_triangles: Renderer.proximity / proximity_csr / proximity_info) against
tests/proximity_ref.py, the lists, counts and CSR sets over tests/clearance_ref.py's D, pair of points and kind. A
query's answer is the first k members of S_i by (D, original index), so every comparison is bit for bit and no case is
excluded. Per scene the queries are the 256 of clearance_ref.fixture_tris; the expectations are computed once per module,
with the mirror's pruned form: a list of 16 (the lists of 1, 4 and 8 are its heads) and the sets within the margin."""
import ctypes

import numpy as np
import pytest

from prt import host
from tests import clearance_ref as cr
from tests import cut_ref, overlap_ref
from tests import proximity_ref as pr
from tests.clearance_ref import same_bits

pytestmark = pytest.mark.gpu

FMAX = cr.FMAX
F = np.float32
KERNELS = ["strict", "fast"]
KERNEL_ID = {"auto": 0, "strict": 1, "fast": 2}
KS = [1, 4, 8, 16]
W, H = 64, 36
N = 256
SEED = {"car_only": 71, "car_boxed": 72}  # (tests/test_gpu_clearance.py's fixtures)


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


def query(r, q, k, kernel, md=None, count_all=False):
    """(tri, d2, on_query, on_mesh, kind, count, info)"""
    import torch
    kind = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
    tri, d2, count, oq, om = r.proximity(cuda(q), k=k, max_dist2=None if md is None else cuda(md), count_all=count_all,
                                         pairs_out=True, kernel=kernel, kind=kind)
    info = r.proximity_info()
    return tuple(x.cpu().numpy() for x in (tri, d2, oq, om, kind, count)) + (info,)


def check(got, want, what=""):
    """want: (tri, d2, on_query, on_mesh, kind, count) of the mirror, cut to the same k"""
    tri, d2, oq, om, kind, count, info = got
    np.testing.assert_array_equal(tri, want[0], err_msg=str(what))
    np.testing.assert_array_equal(kind, want[4], err_msg=str(what))
    np.testing.assert_array_equal(count, want[5], err_msg=str(what))
    assert same_bits(d2, want[1]), what
    assert same_bits(oq, want[2]) and same_bits(om, want[3]), what
    found = int((want[5] > 0).sum())
    assert info["triangles"] == len(tri) and info["found"] == found and info["empty"] == len(tri) - found, (what, info)
    assert info["stored"] == int((want[0] >= 0).sum()) and info["counted"] == int(want[5].sum()), (what, info)
    assert info["stack_overflows"] == 0 and info["listed"] == 0


def check_path(info, kernel, valid, n_tris, wide=True):
    """which loop served the queries: the walk under "fast" on a scene with a wide view, else the exhaustive loop"""
    assert info["walked"] + info["exhaustive"] == valid, info
    if kernel == "fast" and wide:
        assert info["walked"] == valid and info["exhaustive"] == 0, info
        assert (info["nodes_visited"] > 0) == (valid > 0), info
    else:
        assert info["exhaustive"] == valid and info["walked"] == 0, info
        assert info["pairs_tested"] == valid * n_tris and info["nodes_visited"] == 0 and info["pairs_gated"] == 0, info


def head(want, k, rows=slice(None)):
    """the list of k out of the mirror's list of 16 (no count_all: count = min(|S_i|, k))"""
    tri, d2, oq, om, kind, count = want[:6]
    return tri[rows, :k], d2[rows, :k], oq[rows, :k], om[rows, :k], kind[rows, :k], np.minimum(count[rows], k)


class Fix:
    """one fixture scene: a Renderer, its 256 queries, the mirror's list of 16 and its sets within the margin"""

    def __init__(self, dev, scene, seed):
        self.coords = scene.triangles["coords"]
        self.r = dev.Renderer(0).upload(scene)
        self.q = cr.fixture_tris(self.coords, N, seed)
        self.want = pr.lists(self.q, self.coords, 16, counts=True)
        assert self.want[8] == 0  # no evaluated pair's record-box bound exceeded its D
        self.tri, self.d2 = self.want[0], self.want[1]
        self.margin = F((0.005 * overlap_ref.scene_extent(self.coords)) ** 2)
        self.md = np.full(N, self.margin, F)
        self.csr = pr.csr(self.q, self.coords, self.md)
        self.size = np.diff(self.csr[0]).astype(np.int64)


@pytest.fixture(scope="module")
def fix(dev, scenes):
    out = {name: Fix(dev, s, SEED[name]) for name, s in scenes.items()}
    yield out
    for f in out.values():
        f.r.close()


# ------------------------------------------------------------------ 1. fixture queries: lists, both kernels, both orders
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_lists(fix, scene, k, kernel):
    f = fix[scene]
    p = np.random.default_rng(11).permutation(N)
    for order in (np.arange(N), p):
        got = query(f.r, f.q[order], k, kernel)
        check(got, head(f.want, k, order), what=(scene, k, kernel, order[0]))
        check_path(got[6], kernel, N, len(f.coords))


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fixture_conditions(fix, scene):
    """what makes the fixture a test: lists that overflow with crossings, ties across the list's end at D > 0, and at
    the margin empty sets, short sets and sets beyond any list. The floors are the issue's."""
    f = fix[scene]
    assert (f.want[5] == 16).all()  # without a bound every list is full
    crossings = np.array([int((f.csr[5][a:b] == 15).sum()) for a, b in zip(f.csr[0][:-1], f.csr[0][1:])])
    tied = {}
    for k in (4, 8):
        tied[k] = int(((f.d2[:, k - 1].view(np.int32) == f.d2[:, k].view(np.int32)) & (f.d2[:, k - 1] > 0)).sum())
    tied[16] = int((f.want[6] & (f.d2[:, 15] > 0)).sum())
    figures = {"crossings > 16": int((crossings > 16).sum()), "tied": tied, "empty": int((f.size == 0).sum()),
               "1..16": int(((f.size >= 1) & (f.size <= 16)).sum()), "> 16": int((f.size > 16).sum()),
               "total": int(f.size.sum())}
    print(scene, figures)
    assert figures["crossings > 16"] >= 32
    assert tied[4] >= 16 and tied[8] >= 16 and tied[16] >= 16
    assert figures["empty"] >= 64 and figures["1..16"] >= 16 and figures["> 16"] >= 64


# ------------------------------------------------------------------ 2. counts and bounds
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_counts_within_the_margin(fix, scene, kernel):
    import torch
    f = fix[scene]
    # k = 0: the pure count
    count = torch.full((N + 3,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = f.r.proximity(cuda(f.q), k=0, max_dist2=cuda(f.md), count_all=True, kernel=kernel, count=count)
    info = f.r.proximity_info()
    assert out[0].shape == (N, 0) and out[1].shape == (N, 0)
    count = count.cpu().numpy()
    np.testing.assert_array_equal(count[:N], f.size)
    assert (count[N:] == -77).all()
    assert info["counted"] == f.size.sum() and info["stored"] == 0 and info["found"] == (f.size > 0).sum(), info
    check_path(info, kernel, N, len(f.coords))
    # k = 8 with count_all: the list's head and every member counted
    off, tri, d2, pq, pm, kd = f.csr
    want = [np.full((N, 8), -1, np.int32), np.full((N, 8), FMAX, F), np.repeat(f.q[:, None, 0], 8, axis=1).copy(),
            np.repeat(f.q[:, None, 0], 8, axis=1).copy(), np.full((N, 8), -1, np.int32), f.size.astype(np.int32)]
    for i in range(N):
        c = min(int(f.size[i]), 8)
        s = slice(off[i], off[i] + c)
        want[0][i, :c], want[1][i, :c], want[2][i, :c], want[3][i, :c], want[4][i, :c] = tri[s], d2[s], pq[s], pm[s], kd[s]
    got = query(f.r, f.q, 8, kernel, f.md, count_all=True)
    tri_g, d2_g, oq_g, om_g, kind_g, count_g, info = got
    np.testing.assert_array_equal(tri_g, want[0])
    np.testing.assert_array_equal(count_g, want[5])
    np.testing.assert_array_equal(kind_g, want[4])
    assert same_bits(d2_g, want[1]) and same_bits(oq_g, want[2]) and same_bits(om_g, want[3])
    assert info["counted"] == f.size.sum() and info["stored"] == np.minimum(f.size, 8).sum(), info


@pytest.mark.parametrize("kernel", KERNELS)
def test_bounds(fix, kernel):
    f = fix["car_only"]
    k = 8
    kth = f.d2[:, k - 1]
    c = np.arange(N) % 7
    md = np.select([c == 0, c == 1, c == 2, c == 3, c == 4, c == 5],
                   [F(np.inf), kth, np.nextafter(kth, F(-np.inf)), F(0), F(-1.0), F(np.nan)], F(-0.0)).astype(F)
    want = pr.lists(f.q, f.coords, k, md)
    cnt = want[5]
    assert (cnt[c == 0] == k).all() and (cnt[c == 1] == k).all()  # the bound is inclusive, to the bit
    below = (c == 2) & (kth > 0)
    assert below.sum() > 10 and (cnt[below] < k).all()
    zero = (f.d2 == 0).sum(axis=1)
    assert np.array_equal(cnt[c == 3], np.minimum(zero[c == 3], k)) and np.array_equal(cnt[c == 6], np.minimum(zero[c == 6], k))
    assert (cnt[c == 3] > 0).any() and (cnt[c == 3] == 0).any()
    assert not cnt[c == 4].any() and not cnt[c == 5].any()
    got = query(f.r, f.q, k, kernel, md)
    check(got, want[:6], what="bounds")
    tri, d2, oq, om, kind, count, info = got
    unused = tri < 0
    assert (d2[unused] == FMAX).all() and (kind[unused] == -1).all()
    q0 = np.repeat(f.q[:, None, 0], k, axis=1)
    assert same_bits(oq[unused], q0[unused]) and same_bits(om[unused], q0[unused])
    valid = cr.valid_queries(f.q, md)
    assert not valid[(c == 4) | (c == 5)].any() and valid[c < 2].all()
    check_path(info, kernel, int(valid.sum()), len(f.coords))


def test_non_finite_corners_in_a_batch(fix):
    f = fix["car_boxed"]
    q = f.q[:162].copy()
    for i in range(27):  # every one of the nine numbers as NaN, +inf and -inf, five good queries between each
        q[6 * i].reshape(-1)[i % 9] = (np.nan, np.inf, -np.inf)[i // 9]
    bad = ~np.isfinite(q).all(axis=(1, 2))
    assert bad.sum() == 27
    want = list(head(f.want, 4, slice(0, 162)))
    want[0], want[1], want[4], want[5] = want[0].copy(), want[1].copy(), want[4].copy(), want[5].copy()
    want[0][bad], want[1][bad], want[4][bad], want[5][bad] = -1, FMAX, -1, 0
    q0 = np.repeat(q[:, None, 0], 4, axis=1)
    want[2], want[3] = np.where(bad[:, None, None], q0, want[2]), np.where(bad[:, None, None], q0, want[3])
    for kernel in KERNELS:
        got = query(f.r, q, 4, kernel)
        check(got, want, what=kernel)
        check_path(got[6], kernel, 162 - 27, len(f.coords))
        assert got[6]["empty"] == 27
        import torch
        count = f.r.proximity(cuda(q), k=0, count_all=True, max_dist2=cuda(f.md[:162]), kernel=kernel)[2]
        torch.cuda.synchronize()
        np.testing.assert_array_equal(count.cpu().numpy(), np.where(bad, 0, f.size[:162]))


# ------------------------------------------------------------------ 3. a list of one is the clearance query's answer
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_a_list_of_one_is_clearance_on_the_device(fix, scene, kernel):
    import torch
    f = fix[scene]
    md = np.where(np.arange(N) % 2 == 0, F(np.inf), f.margin).astype(F)
    q = cuda(f.q)
    ckind = torch.empty(N, dtype=torch.int32, device="cuda")
    want = f.r.clearance(q, max_dist2=cuda(md), kernel=kernel, kind=ckind)
    ci = f.r.clearance_info()
    want = [x.cpu().numpy() for x in (*want, ckind)]
    tri, d2, oq, om, kind, count, info = query(f.r, f.q, 1, kernel, md)
    for a, b in zip((tri, d2, oq, om, kind), want):
        assert np.array_equal(a.reshape(b.shape).view(np.int32), b.view(np.int32))
    assert np.array_equal(count, (want[0] >= 0).astype(np.int32)) and 0 < (want[0] < 0).sum() < N
    for name in ("triangles", "found", "walked", "exhaustive", "empty", "nodes_visited", "pairs_gated", "pairs_tested"):
        assert info[name] == ci[name], (name, info, ci)  # the same walk, pair for pair


# ------------------------------------------------------------------ 4. CSR
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_csr_sets(fix, scene, kernel):
    f = fix[scene]
    off, tri, d2, pair = f.r.proximity_csr(cuda(f.q), cuda(f.md), kernel=kernel)
    info = f.r.proximity_info()
    off, tri, d2, pair = (x.cpu().numpy() for x in (off, tri, d2, pair))
    woff, wtri, wd2, wpq, wpm, _ = f.csr
    assert len(wtri) > 5000
    np.testing.assert_array_equal(off, woff)
    np.testing.assert_array_equal(tri, wtri)
    assert same_bits(d2, wd2) and same_bits(pair[:, 0], wpq) and same_bits(pair[:, 1], wpm)
    assert info["listed"] == len(wtri) and info["counted"] == len(wtri) and info["stored"] == 0, info
    off2, tri2, d22, none = f.r.proximity_csr(cuda(f.q), cuda(f.md), pairs=False, kernel=kernel)
    assert none is None and np.array_equal(tri2.cpu().numpy(), wtri) and same_bits(d22.cpu().numpy(), wd2)


@pytest.mark.parametrize("kernel", KERNELS)
def test_short_segments_receive_members_only(fix, kernel):
    """the list form at the C ABI: segments as long as |S_i|, half of it, three longer and of no length, two guard words
    before the first and five after the last; every entry written is a member, once, with its own D, points and kind;
    the rest of a long segment and the guard words stay"""
    import torch
    from prt import _lib
    f = fix["car_only"]
    woff, wtri, wd2, wpq, wpm, wkd = f.csr
    size = f.size
    c = np.arange(N) % 4
    room = np.select([c == 0, c == 1, c == 2], [size, size // 2, size + 3], 0).astype(np.int64)
    offs = (2 + np.concatenate([[0], np.cumsum(room)])).astype(np.int32)
    total = int(offs[-1]) + 5
    lst = torch.full((total,), -77, dtype=torch.int32, device="cuda")
    ld2 = torch.full((total,), -77.0, dtype=torch.float32, device="cuda")
    lpt = torch.full((total, 2, 3), -77.0, dtype=torch.float32, device="cuda")
    lkd = torch.full((total,), -77, dtype=torch.int32, device="cuda")
    count = torch.empty(N, dtype=torch.int32, device="cuda")
    dq, dmd, doffs = cuda(f.q), cuda(f.md), cuda(offs, np.int32)
    torch.cuda.synchronize()
    t = _lib.ProxTris(dq.data_ptr(), dmd.data_ptr(), doffs.data_ptr(), N, 0, 1, KERNEL_ID[kernel])
    res = _lib.ProximityResults(None, None, None, None, None, count.data_ptr(), lst.data_ptr(), ld2.data_ptr(),
                                lpt.data_ptr(), lkd.data_ptr())
    assert _lib.hip().rt_proximity_triangles(f.r._ctx, ctypes.byref(t), ctypes.byref(res)) == 0
    info = f.r.proximity_info()
    lst, ld2, lpt, lkd, count = (x.cpu().numpy() for x in (lst, ld2, lpt, lkd, count))
    np.testing.assert_array_equal(count, size)
    written = np.zeros(total, bool)
    for i in range(N):
        a, w = int(offs[i]), min(int(size[i]), int(room[i]))
        written[a:a + w] = True
        mem = {int(t_): woff[i] + j for j, t_ in enumerate(wtri[woff[i]:woff[i + 1]])}
        assert len(set(lst[a:a + w].tolist())) == w  # no member twice
        for p_ in range(a, a + w):
            assert int(lst[p_]) in mem, (i, p_)
            j = mem[int(lst[p_])]
            assert ld2[p_].view(np.int32) == wd2[j].view(np.int32) and lkd[p_] == wkd[j], (i, p_)
            assert same_bits(lpt[p_, 0], wpq[j]) and same_bits(lpt[p_, 1], wpm[j]), (i, p_)
    assert info["listed"] == written.sum() and written.sum() > 1000 and (np.minimum(size, room) < size).sum() > 20
    assert (lst[~written] == -77).all() and (ld2[~written] == -77.0).all() and (lkd[~written] == -77).all()
    assert (lpt[~written] == -77.0).all() and (~written).sum() > 7


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_a_bound_of_zero_holds_the_cut_query_s_set(fix, scene):
    f = fix[scene]
    zero = np.zeros(N, F)
    coff, cidx, _ = f.r.cuts_csr(cuda(f.q), segments=False)
    coff, cidx = coff.cpu().numpy(), cidx.cpu().numpy()
    off, tri, d2, _ = f.r.proximity_csr(cuda(f.q), cuda(zero), pairs=False)
    off, tri, d2 = (x.cpu().numpy() for x in (off, tri, d2))
    assert (d2 == 0).all() and len(cidx) > 1000 and len(tri) >= len(cidx)
    for i in range(N):
        assert set(cidx[coff[i]:coff[i + 1]].tolist()) <= set(tri[off[i]:off[i + 1]].tolist()), i
        assert (np.diff(tri[off[i]:off[i + 1]]) > 0).all()  # all at D = 0: index order


# ------------------------------------------------------------------ 5. ties take the lower index
def test_ties_take_the_lower_index(dev, fix):
    base = host.Scene.named("car_only")
    t = base.triangles
    n = len(t)
    f = fix["car_only"]
    rows = np.arange(0, N, 4)
    q = f.q[rows]
    md = f.md[rows]
    doubled = host.Scene(np.concatenate([t, t]), base.lights).build_bvh(3)
    mirrored = host.Scene(np.concatenate([t[::-1], t]), base.lights).build_bvh(3)
    for name, s in (("doubled", doubled), ("copy first, reversed", mirrored)):
        want = pr.lists(q, s.triangles["coords"], 8)
        sizes = pr.sizes(q, s.triangles["coords"], md)
        assert np.array_equal(sizes, 2 * f.size[rows])  # the counts double
        # every D of the single scene's list twice; a triangle's two copies in index order wherever the list holds both
        # (it does unless a tie at one D runs across the list's end)
        assert same_bits(want[1][:, 0::2], f.d2[rows, :4]) and same_bits(want[1][:, 1::2], f.d2[rows, :4])
        orig = want[0] % n if name == "doubled" else np.where(want[0] < n, n - 1 - want[0], want[0] - n)
        both = 0
        for i in range(len(rows)):
            for o_ in np.unique(orig[i]):
                at = np.flatnonzero(orig[i] == o_)
                assert len(at) <= 2 and (len(at) == 1 or want[0][i, at[0]] < want[0][i, at[1]])
                assert len(at) == 1 or want[1][i, at[0]].view(np.int32) == want[1][i, at[1]].view(np.int32)
                both += len(at) == 2
        assert both >= 2 * len(rows)  # at least half of the entries have their copy beside them
        r = dev.Renderer(0).upload(s)
        for kernel in KERNELS:
            got = query(r, q, 8, kernel)
            check(got, want[:6], what=(name, kernel))
            count = r.proximity(cuda(q), k=0, count_all=True, max_dist2=cuda(md), kernel=kernel)[2]
            r.sync()
            np.testing.assert_array_equal(count.cpu().numpy(), sizes)
        r.close()


# ------------------------------------------------------------------ 6. shapes
@pytest.mark.parametrize("kernel", KERNELS)
def test_query_count_edges(fix, kernel):
    import torch
    from prt import _lib
    f = fix["car_boxed"]
    dq = cuda(f.q[:65])
    k = 4
    want = head(f.want, k)
    for n in (0, 1, 63, 65):
        tri = torch.full((n + 3, k), -77, dtype=torch.int32, device="cuda")
        kind = torch.full((n + 3, k), -77, dtype=torch.int32, device="cuda")
        d2 = torch.full((n + 3, k), -77.0, dtype=torch.float32, device="cuda")
        oq = torch.full((n + 3, k, 3), -77.0, dtype=torch.float32, device="cuda")
        om = torch.full((n + 3, k, 3), -77.0, dtype=torch.float32, device="cuda")
        count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.r.proximity(dq[:n], k=k, kernel=kernel, tri=tri, d2=d2, on_query=oq, on_mesh=om, kind=kind, count=count)
        assert f.r.proximity_info()["triangles"] == n
        tri, kind, d2, oq, om, count = (x.cpu().numpy() for x in (tri, kind, d2, oq, om, count))
        np.testing.assert_array_equal(tri[:n], want[0][:n], err_msg=str(n))
        np.testing.assert_array_equal(kind[:n], want[4][:n], err_msg=str(n))
        np.testing.assert_array_equal(count[:n], want[5][:n], err_msg=str(n))
        assert same_bits(d2[:n], want[1][:n]) and same_bits(oq[:n], want[2][:n]) and same_bits(om[:n], want[3][:n]), n
        assert (tri[n:] == -77).all() and (kind[n:] == -77).all() and (d2[n:] == -77.0).all(), n
        assert (oq[n:] == -77.0).all() and (om[n:] == -77.0).all() and (count[n:] == -77).all(), n
    # each single output alone
    L = _lib.hip()
    n = 65
    for only in range(5):
        bufs = [torch.full((n, k), -77, dtype=torch.int32, device="cuda"),
                torch.full((n, k), -77.0, dtype=torch.float32, device="cuda"),
                torch.full((n, k, 3), -77.0, dtype=torch.float32, device="cuda"),
                torch.full((n, k, 3), -77.0, dtype=torch.float32, device="cuda"),
                torch.full((n, k), -77, dtype=torch.int32, device="cuda")]
        torch.cuda.synchronize()
        ptrs = [b.data_ptr() if i == only else None for i, b in enumerate(bufs)]
        t = _lib.ProxTris(dq.data_ptr(), None, None, n, k, 0, KERNEL_ID[kernel])
        res = _lib.ProximityResults(*ptrs, None, None, None, None, None)
        assert L.rt_proximity_triangles(f.r._ctx, ctypes.byref(t), ctypes.byref(res)) == 0
        assert f.r.proximity_info()["triangles"] == n
        assert np.array_equal(bufs[only].cpu().numpy().view(np.int32), want[only][:n].view(np.int32)), only
    # k = 16 with only a count: the caller gives nothing else (at the C ABI a list query with none of its five list
    # outputs is RT_E_ARG, so the wrapper's own tri and d2 stand in)
    count = torch.full((n + 3,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f.r.proximity(dq[:n], k=16, max_dist2=cuda(f.md[:n]), kernel=kernel, count=count)
    info = f.r.proximity_info()
    count = count.cpu().numpy()
    np.testing.assert_array_equal(count[:n], np.minimum(f.size[:n], 16))
    assert (count[n:] == -77).all() and info["counted"] == info["stored"] == np.minimum(f.size[:n], 16).sum()
    f.r.proximity(dq[:n], k=16, max_dist2=cuda(f.md[:n]), count_all=True, kernel=kernel, count=count_all_out(n))
    assert f.r.proximity_info()["counted"] == f.size[:n].sum()


def count_all_out(n):
    import torch
    return torch.empty(n, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------ 7. every structure, moving scene
@pytest.mark.parametrize("accel,flags", [("host", 0), ("reference", 0), ("auto", 2 | 4)])
def test_every_acceleration_structure(dev, scenes, fix, accel, flags):
    """a scene uploaded with the reference accel has no wide view: the exhaustive loop under "fast" too"""
    f = fix["car_boxed"]
    r = dev.Renderer(0, flags=flags).upload(scenes["car_boxed"], accel=accel)
    for kernel in KERNELS:
        got = query(r, f.q, 8, kernel)
        check(got, head(f.want, 8), what=(accel, flags, kernel))
        check_path(got[6], kernel, N, len(f.coords), wide=accel != "reference")
    count = r.proximity(cuda(f.q), k=0, count_all=True, max_dist2=cuda(f.md))[2]
    r.sync()
    np.testing.assert_array_equal(count.cpu().numpy(), f.size)
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
    want = pr.lists(q, coords, 8)[:6]
    assert (want[0] != f.tri[rows, :8]).any(axis=1).sum() > 50 and not same_bits(want[1], f.d2[rows, :8])
    r = dev.Renderer(0).upload(s)
    assert r.scene_info()["accel_built"] == "gpu"
    check(query(r, q, 8, "fast"), head(f.want, 8, rows), what="before")
    for step in ("update", "rebuild"):
        if step == "update":
            r.update_vertices(cuda(coords))
        else:
            r.rebuild_views(cuda(coords), mode="device")
        for kernel in KERNELS:
            got = query(r, q, 8, kernel)
            check(got, want, what=(step, kernel))
        assert got[6]["walked"] == len(rows)
    r.close()


# ------------------------------------------------------------------ 8. the walk prunes
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_the_walk_prunes(fix, scene):
    f = fix[scene]
    info = query(f.r, f.q, 8, "fast")[6]
    wide = f.r.scene_info()["wide_nodes"]
    print(f"{scene}, {N} queries, k = 8: pairs_tested {info['pairs_tested']} ({info['pairs_tested'] / N:.1f} per query "
          f"of {len(f.coords)}), pairs_gated {info['pairs_gated']} ({info['pairs_gated'] / N:.1f}), nodes_visited "
          f"{info['nodes_visited']} ({info['nodes_visited'] / N:.1f} per query of {wide})")
    assert 0 < info["pairs_tested"] < N * len(f.coords) / 10
    assert 0 < info["nodes_visited"] < N * wide
    assert info["pairs_gated"] > 0 and info["stack_overflows"] == 0
    # the crossing-heavy rows alone: cut_ref.surface_tris, the fixture's first three sixteenths
    rows = slice(0, 3 * N // 16)
    info = query(f.r, f.q[rows], 8, "fast")[6]
    print(f"  the {3 * N // 16} surface queries: pairs_tested {info['pairs_tested']}, pairs_gated {info['pairs_gated']}")
    assert info["pairs_gated"] > 0


# ------------------------------------------------------------------ 9. isolation
def strip(info):
    return {k: v for k, v in info.items() if k != "kernel_ms"}


def same(a, b):
    return strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4


def test_a_proximity_query_shares_no_slot(dev, scenes, fix):
    """tests/test_gpu_query_slots.py with the eleventh family: a proximity query leaves the ten other infos and a
    rendered frame's bits as they were, and running the ten leaves its info alone"""
    import torch
    from prt import rays
    f = fix["car_boxed"]
    cam = host.camera(W, H)
    tris = cuda(f.q)
    pts = tris.mean(dim=1).contiguous()
    lo, hi = (pts - 0.05).contiguous(), (pts + 0.05).contiguous()
    down = torch.zeros_like(pts)
    down[:, 1] = -1.0
    o, d = rays.pinhole(cam, W, H)
    torch.cuda.synchronize()  # (these tensors are torch's work; the queries run on the renderer's stream)
    r = dev.Renderer(0).upload(scenes["car_boxed"])
    run = {
        "rays": lambda n: r.trace_rays(o[:n], d[:n]),
        "shade": lambda n: r.shade_rays(o[:n], d[:n]),
        "hits": lambda n: r.trace_hits(o[:n], d[:n], max_hits=2),
        "nearest": lambda n: r.nearest(pts[:n]),
        "neighbours": lambda n: r.nearest_tris(pts[:n], k=4, points_out=True),
        "overlaps": lambda n: r.overlaps(lo[:n], hi[:n], k=4),
        "sweep": lambda n: r.sweep(pts[:n], down[:n], 0.01),
        "contacts": lambda n: r.sweep_contacts(pts[:n], down[:n], 0.01, k=4),
        "cuts": lambda n: r.cuts(tris[:n], k=4),
        "clearance": lambda n: r.clearance(tris[:n]),
    }
    info = {"rays": r.query_info, "shade": r.shade_info, "hits": r.hits_info, "nearest": r.nearest_info,
            "neighbours": r.neighbours_info, "overlaps": r.overlaps_info, "sweep": r.sweep_info,
            "contacts": r.contacts_info, "cuts": r.cuts_info, "clearance": r.clearance_info}
    hit = torch.empty((H, W), dtype=torch.int32, device="cuda")
    r.render(cam, W, H, kernel="fast", hit=hit)
    r.sync()
    frame0, stats0, launch0 = r.download(hit=True), r.stats(), r.launch_info()
    outs0 = {}
    for j, name in enumerate(run):
        outs0[name] = run[name](65 + 16 * j)
    r.sync()
    outs0 = {name: [x.cpu().numpy() for x in (v if isinstance(v, tuple) else (v,))] for name, v in outs0.items()}
    held = {name: fn() for name, fn in info.items()}
    with pytest.raises(dev.RtError, match="status -5"):  # the ten ran; the eleventh has no info yet
        r.proximity_info()
    for kernel, k, n in (("fast", 8, 101), ("strict", 16, 67), ("fast", 0, 203)):
        r.proximity(tris[:n], k=k, count_all=k == 0, max_dist2=cuda(f.md[:n]), pairs_out=k > 0, kernel=kernel)
        pi = r.proximity_info()
        assert pi["triangles"] == n and pi["kernel_ms"] > 0
    for name in info:  # the ten other infos as they were
        assert same(info[name](), held[name]), (name, info[name](), held[name])
    frame1 = r.download(hit=True)
    assert same_bits(frame0[0], frame1[0]) and np.array_equal(frame0[1], frame1[1])
    assert r.stats() == stats0 and r.launch_info() == launch0
    for j, name in enumerate(run):  # the ten again: the same bits, and the proximity query's info stays
        out = run[name](65 + 16 * j)
        r.sync()
        out = [x.cpu().numpy() for x in (out if isinstance(out, tuple) else (out,))]
        for a, b in zip(out, outs0[name]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), name
        assert same(r.proximity_info(), pi), name
    r.render(cam, W, H, kernel="fast", hit=hit)
    assert r.sync() > 0
    frame2 = r.download(hit=True)
    assert same_bits(frame0[0], frame2[0]) and np.array_equal(frame0[1], frame2[1])
    assert same(r.proximity_info(), pi)
    with pytest.raises(dev.RtError, match="bad kernel"):  # a refused call leaves the family's info as it was
        r.proximity(tris[:50], kernel=7)
    assert same(r.proximity_info(), pi)
    r.proximity(tris[:0], k=4)  # an empty query: RT_OK, zero counters, no kernel time
    assert all(v == 0 for v in r.proximity_info().values())
    for name in info:  # (the ten ran again with the same counts)
        assert strip(info[name]()) == strip(held[name]), name
    r.close()


# ------------------------------------------------------------------ 10. fast against strict, no mirror
@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_fast_equals_strict_on_4096_queries(fix, scene):
    import torch
    f = fix[scene]
    q = cut_ref.surface_tris(f.coords, 4096, seed=97)
    a, b = (query(f.r, q, 8, kernel) for kernel in KERNELS)
    for x, y in zip(a[:6], b[:6]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    names = ("triangles", "found", "empty", "stored", "counted", "stack_overflows")
    assert {k: a[6][k] for k in names} == {k: b[6][k] for k in names} and a[6]["found"] == 4096
    assert a[6]["stored"] == 8 * 4096
    check_path(a[6], "strict", 4096, len(f.coords))
    check_path(b[6], "fast", 4096, len(f.coords))
    assert (a[4] == 15).sum() > 1000 and (a[4] < 15).sum() > 100
    md = cuda(np.full(4096, f.margin, F))
    counts = []
    for kernel in KERNELS:
        counts.append(f.r.proximity(cuda(q), k=0, count_all=True, max_dist2=md, kernel=kernel)[2])
        info = f.r.proximity_info()
        check_path(info, kernel, 4096, len(f.coords))
    torch.cuda.synchronize()
    c0, c1 = (c.cpu().numpy() for c in counts)
    assert np.array_equal(c0, c1) and c0.max() > 16 and info["counted"] == c0.sum()


# ------------------------------------------------------------------ 11. errors
def test_proximity_errors(dev, scenes, fix):
    import torch
    from prt import _lib
    f = fix["car_only"]
    q = cuda(f.q)
    r = dev.Renderer(0)
    with pytest.raises(dev.RtError, match="-5"):  # RT_E_STATE: nothing uploaded
        r.proximity(q)
    r.upload(scenes["car_only"])
    with pytest.raises(dev.RtError, match="-5"):  # no proximity query run yet
        r.proximity_info()
    r.proximity(q[:100], k=4)
    info = r.proximity_info()
    assert info["triangles"] == 100 and info["found"] == 100 and info["stored"] == 400
    with pytest.raises(dev.RtError, match="status -1"):
        r.proximity(q, kernel=7)
    with pytest.raises(dev.RtError, match="status -1"):
        r.proximity((0, 16))  # null tris
    L = _lib.hip()
    tri = torch.empty(16 * 16, dtype=torch.int32, device="cuda")
    cnt = torch.empty(16, dtype=torch.int32, device="cuda")
    offs = torch.zeros(17, dtype=torch.int32, device="cuda")
    p, t, c, o = q.data_ptr(), tri.data_ptr(), cnt.data_ptr(), offs.data_ptr()
    Q, R = _lib.ProxTris, _lib.ProximityResults
    nil = (None,) * 4
    for t_, res in [
        (Q(None, None, None, 16, 4, 0, 0), R(t, None, None, None, None, c, *nil)),   # null tris
        (Q(p, None, None, 16, 4, 0, 0), R(None, None, None, None, None, c, *nil)),   # max_tris > 0, all five null
        (Q(p, None, None, 16, 0, 0, 0), R(None, None, None, None, None, c, *nil)),   # max_tris = 0 without count_all
        (Q(p, None, None, 16, 0, 1, 0), R(None, None, None, None, None, None, *nil)),  # ... without count
        (Q(p, None, None, 16, 17, 0, 0), R(t, None, None, None, None, c, *nil)),     # max_tris out of range
        (Q(p, None, None, 16, -1, 0, 0), R(t, None, None, None, None, c, *nil)),
        (Q(p, None, None, 16, 4, 2, 0), R(t, None, None, None, None, c, *nil)),      # count_all not 0 / 1
        (Q(p, None, o, 16, 4, 0, 0), R(t, None, None, None, None, c, *nil)),         # offsets without list
        (Q(p, None, None, 16, 4, 0, 0), R(t, None, None, None, None, c, t, None, None, None)),  # list without offsets
        (Q(p, None, None, 16, 4, 0, 0), R(t, None, None, None, None, c, None, t, None, None)),  # list_d2 without list
        (Q(p, None, None, 16, 4, 0, 0), R(t, None, None, None, None, c, None, None, t, None)),  # list_points ...
        (Q(p, None, None, 16, 4, 0, 0), R(t, None, None, None, None, c, None, None, None, t)),  # list_kind ...
        (Q(p, None, None, 16, 4, 0, 3), R(t, None, None, None, None, c, *nil)),      # unknown kernel
        (Q(p, None, None, 16, 4, 0, -1), R(t, None, None, None, None, c, *nil)),
        (Q(p, None, None, -1, 4, 0, 0), R(t, None, None, None, None, c, *nil)),      # negative n
    ]:
        assert L.rt_proximity_triangles(r._ctx, ctypes.byref(t_), ctypes.byref(res)) == -1
        assert L.rt_last_error(r._ctx).startswith(b"rt_proximity_triangles: ")
    assert L.rt_proximity_triangles(r._ctx, None, None) == -1
    assert L.rt_proximity_triangles(r._ctx, ctypes.byref(Q(p, None, None, 16, 4, 0, 0)), None) == -1
    after = r.proximity_info()  # a refused call leaves proximity_info() as it was
    assert strip(after) == strip(info) and abs(after["kernel_ms"] - info["kernel_ms"]) < 1e-4
    # n = 0 is RT_OK with no pointers at all
    assert L.rt_proximity_triangles(r._ctx, ctypes.byref(Q(None, None, None, 0, 4, 0, 0)),
                                    ctypes.byref(R(*(None,) * 10))) == 0
    assert r.proximity_info()["triangles"] == 0
    r.close()
