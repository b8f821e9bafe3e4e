"""The clearance query's ABI (rt_clearance_triangles / rt_get_clearance_info, include/rt_hip.h) without a GPU: the symbols
are exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as tests/test_cut_abi.py
does), Renderer.clearance refuses bad arguments before any device call, and the yardstick of the GPU tests
(tests/clearance_ref.py) gives the stated answers on closed-form pairs, agrees with itself with and without its
pruning bit for bit, stays finite on degenerate triangles, and lies within a measured residual of the same fifteen
candidates and six exact edge-triangle crossing tests in float64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host
from tests import clearance_ref as cr
from tests.test_nearest_abi import degenerate_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")
F = np.float32
FMAX = cr.FMAX


def test_clearance_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_clearance_triangles", "rt_get_clearance_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_clearance_triangles, L.rt_get_clearance_info


def test_clearance_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_clear_tris": _lib.ClearTris, "rt_clearance_results": _lib.ClearanceResults,
               "rt_clearance_info": _lib.ClearanceInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layouts.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layouts"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in _lib.ClearTris._fields_] == ["tris", "max_dist2", "n", "kernel"]
    assert [f for f, _ in _lib.ClearanceResults._fields_] == ["tri", "d2", "on_query", "on_mesh", "kind"]
    assert [f for f, _ in _lib.ClearanceInfo._fields_] == [
        "triangles", "found", "walked", "exhaustive", "empty", "nodes_visited", "pairs_gated", "pairs_tested",
        "stack_overflows", "kernel_ms"]


def test_clearance_arguments_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, 3, dtype=torch.float32)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # a host tensor
        r.clearance(ok)
    with pytest.raises(device.RtError, match="tris: dtype"):
        r.clearance(ok.double())
    with pytest.raises(device.RtError, match=r"tris: shape .* expected \[n, 3, 3\]"):
        r.clearance(torch.zeros(8, 9))
    with pytest.raises(device.RtError, match=r"tris: shape .* expected \[n, 3, 3\]"):
        r.clearance(torch.zeros(8, 3, 4))
    with pytest.raises(device.RtError, match="contiguous"):
        r.clearance(torch.zeros(16, 3, 3)[::2])
    with pytest.raises(device.RtError, match="torch tensor"):
        r.clearance([[[0.0] * 3] * 3])
    for bad in ((1234, -1), (1234.0, 8), (1234, 8, 3)):
        with pytest.raises(device.RtError, match="raw pointer"):
            r.clearance(bad)
    raw = (1234, 8)
    with pytest.raises(device.RtError, match="max_dist2: shape"):
        r.clearance(raw, max_dist2=torch.zeros(8, 1))
    with pytest.raises(device.RtError, match="max_dist2: dtype"):
        r.clearance(raw, max_dist2=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(device.RtError, match="max_dist2: 7 elements"):
        r.clearance(raw, max_dist2=torch.zeros(7))
    with pytest.raises(device.RtError, match="max_dist2: expected a torch tensor"):
        r.clearance(raw, max_dist2=[1.0] * 8)
    # the optional outputs, before anything is allocated (an allocation would fail too: there is no device here)
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.clearance(raw, tri=torch.zeros(8))
    with pytest.raises(device.RtError, match="d2: 7 elements"):
        r.clearance(raw, d2=torch.zeros(7))
    with pytest.raises(device.RtError, match="on_query: shape"):
        r.clearance(raw, on_query=torch.zeros(24))
    with pytest.raises(device.RtError, match="on_mesh: 21 elements"):
        r.clearance(raw, on_mesh=torch.zeros(7, 3))
    with pytest.raises(device.RtError, match="kind: dtype"):
        r.clearance(raw, kind=torch.zeros(8))
    with pytest.raises(device.RtError, match="kind: 7 elements"):
        r.clearance(raw, kind=torch.zeros(7, dtype=torch.int32))
    r._ctx = None  # (nothing to destroy)


# ------------------------------------------------------------------ closed-form pairs
# mesh triangle 0 lies in z = 0, triangle 1 in z = 1, far apart in x
MESH = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[10, 0, 1], [14, 0, 1], [10, 4, 1]]], F)


def one(q, md=None, mesh=MESH):
    """the answer to one query -> (tri, d2, on_query, on_mesh, kind)"""
    tri, d2, oq, om, kind, _ = cr.expected(np.array([q], F), mesh, None if md is None else np.array([md], F))
    return int(tri[0]), d2[0], oq[0].tolist(), om[0].tolist(), int(kind[0])


def test_a_parallel_triangle_has_a_vertex_kind():
    h = F(0.5)
    assert one([[1, 1, h], [2, 1, h], [1, 2, h]]) == (0, F(0.25), [1, 1, 0.5], [1, 1, 0], 0)
    # below triangle 1, smaller than it: a query corner again, against the mesh triangle's interior
    assert one([[11, 1, 0.75], [11.5, 1, 0.75], [11, 1.5, 0.75]]) == (1, F(0.0625), [11, 1, 0.75], [11, 1, 1], 0)
    # larger than the mesh triangle, above it: the mesh corner a against the query's interior
    tri, d2, oq, om, kind = one([[-5, -5, 2], [8, -5, 2], [-5, 8, 2]])
    assert (tri, d2, om, kind) == (0, F(4), [0, 0, 0], 3) and oq == [0, 0, 2]


def test_two_skew_edges_have_an_edge_kind():
    """the query's first edge runs along z through (3, 3, .), the mesh triangle's third edge from (4, 0, 0) to
    (0, 4, 0): the closest points are (3, 3, 0) and (2, 2, 0); every corner candidate is farther (3, 18; 8 and more)"""
    assert one([[3, 3, -1], [3, 3, 1], [5, 5, 0]]) == (0, F(2), [3, 3, 0], [2, 2, 0], 6 + 3 * 0 + 2)
    # the same pair from the query's third edge (qb -> qc)
    assert one([[5, 5, 0], [3, 3, -1], [3, 3, 1]]) == (0, F(2), [3, 3, 0], [2, 2, 0], 6 + 3 * 2 + 2)


def test_crossing_and_touching_give_zero():
    # a piercing query: kind 15, both points the cut segment's first end
    assert one([[1, 1, -1], [2, 1, 1], [1, 1, 1]]) == (0, F(0), [1, 1, 0], [1, 1, 0], 15)
    # touching at a shared corner: rt_cut_triangles' closed intervals make that a crossing too
    tri, d2, oq, om, kind = one([[0, 0, 0], [-1, -1, 1], [-1, -1, 2]])
    assert (tri, d2, oq, om) == (0, F(0), [0, 0, 0], [0, 0, 0]) and kind == 15
    # the mesh triangle itself is coplanar with itself: no crossing, D = 0 through the first vertex candidate
    assert one(MESH[0]) == (0, F(0), [0, 0, 0], [0, 0, 0], 0)
    assert one(MESH[1]) == (1, F(0), [10, 0, 1], [10, 0, 1], 0)
    # coplanar and overlapping, no corner shared: a query corner inside the mesh triangle
    assert one([[1, 1, 0], [3, 1, 0], [1, 3, 0]])[1::3] == (F(0), 0)


def test_the_bound_is_inclusive_to_the_bit():
    q = [[1, 1, 0.5], [2, 1, 0.5], [1, 2, 0.5]]
    assert one(q, F(0.25))[:2] == (0, F(0.25)) and one(q, np.inf)[0] == 0
    below = np.nextafter(F(0.25), F(0))
    assert one(q, below) == (-1, FMAX, [1, 1, 0.5], [1, 1, 0.5], -1)  # one float beyond the bound: q0's bits twice
    assert one(q, F(0))[0] == -1 and one(MESH[0], F(0))[:2] == (0, F(0))  # 0 is a valid bound: what touches
    for bad in (np.nan, F(-1), F(-1e-45)):
        assert one(MESH[0], bad) == (-1, FMAX, [0, 0, 0], [0, 0, 0], -1)
    assert one(MESH[0], F(-0.0))[0] == 0


def test_a_non_finite_corner_gives_the_empty_set():
    good = np.array([[1, 1, -1], [2, 1, 1], [1, 1, 1]], F)
    q = []
    for pos in range(9):
        for bad in (np.nan, np.inf, -np.inf):
            t = good.copy()
            t.reshape(-1)[pos] = bad
            q.append(t)
    q = np.array(q)
    tri, d2, oq, om, kind, ties = cr.expected(q, MESH)
    assert len(q) == 27 and (tri == -1).all() and (d2 == FMAX).all() and (kind == -1).all() and (ties == 0).all()
    assert cr.same_bits(oq, q[:, 0]) and cr.same_bits(om, q[:, 0])


def test_degenerate_triangles_have_finite_answers():
    """test_nearest_abi.py's zero-area and repeated-vertex triangles as the mesh and as the queries: every pair's D
    and both points are finite, D >= 0, the points lie in the two boxes and the record-box bound does not exceed D"""
    deg = degenerate_triangles()
    rng = np.random.default_rng(13)
    plain = (rng.uniform(-2, 6, (64, 1, 3)) + rng.normal(0, 1, (64, 3, 3))).astype(F)
    for q, mesh in ((plain, deg), (deg, MESH), (deg, deg), (deg, plain)):
        Q, rec = cr.query_records(q), cr.records(mesh)
        qi, ti = (x.reshape(-1) for x in np.meshgrid(np.arange(len(q)), np.arange(len(mesh)), indexing="ij"))
        D, pq, pm, kind = cr.pair_eval(q, Q, rec, qi, ti)
        assert np.isfinite(D).all() and np.isfinite(pq).all() and np.isfinite(pm).all() and (D >= 0).all()
        assert (kind >= 0).all() and not np.signbit(D).any()
        free = kind < 15  # (a crossing's s0 is the cut query's point: on both triangles up to rounding)
        assert ((pq >= Q[5][qi]) & (pq <= Q[6][qi]))[free].all() and ((pm >= rec[5][ti]) & (pm <= rec[6][ti]))[free].all()
        assert (cr.box_bound(Q[5][qi], Q[6][qi], rec[5][ti], rec[6][ti]) <= D).all()
        tri = cr.expected(q, mesh)[0]
        assert (tri >= 0).all()


def test_a_needle_through_the_interior_reports_the_boundary():
    """the documented wart: a zero-area query is answered by the fifteen candidates alone, X excludes it as cuts does.
    This segment pierces triangle 0 at (1, 1, 0), a unit away from its two nearest edges: D = 1, not 0"""
    tri, d2, oq, om, kind = one([[1, 1, -1], [1, 1, 1], [1, 1, 1]])
    assert (tri, d2, kind) == (0, F(1), 0) and oq == [1, 1, -1] and om == [1, 1, 0]
    # ... while the same segment as one edge of a proper triangle crosses
    assert one([[1, 1, -1], [1, 1, 1], [1.5, 1, 1]])[1::3] == (F(0), 15)
    # a point query on the surface, and one off it
    assert one([[1, 1, 0]] * 3)[:2] == (0, F(0)) and one([[1, 1, 2]] * 3)[:2] == (0, F(4))


def test_pruned_and_unpruned_mirrors_agree():
    """64 queries x car_only: skipping the pairs whose record-box bound exceeds the best D so far changes no bit, and
    no evaluated pair's bound exceeds its D"""
    coords = host.Scene.named("car_only").triangles["coords"]
    q = cr.fixture_tris(coords, 256, seed=71)[::4]
    full = cr.expected(q, coords, prune=False, counts=True)
    fast = cr.expected(q, coords, prune=True, counts=True)
    print(f"car_only, 64 queries: {full[6]} pairs unpruned, {fast[6]} pruned; bound > D in {full[7]} pairs")
    assert full[6] == 64 * len(coords) and fast[6] < full[6] / 100 and full[7] == 0 and fast[7] == 0
    for a, b in zip(full[:6], fast[:6]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.itemsize == 4 else np.int64),
                                                     b.view(np.int32 if b.itemsize == 4 else np.int64))


# ------------------------------------------------------------------ the yardstick against float64
def _dot(u, v):
    return (u * v).sum(axis=-1)


def near64(p, tri):
    """float64 squared distance of points p [n, 3] to triangles tri [n, 3, 3] (Ericson's closest point)"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        den = va + vb + vc
        cases = [((d1 <= 0) & (d2 <= 0), a), ((d3 >= 0) & (d4 <= d3), b),
                 ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[:, None]),
                 ((d6 >= 0) & (d5 <= d6), c),
                 ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[:, None]),
                 ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0),
                  b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None])]
        P = a + ab * (vb / den)[:, None] + ac * (vc / den)[:, None]
    for cond, val in reversed(cases):
        P = np.where(cond[:, None], val, P)
    return _dot(p - P, p - P)


def segseg64(p1, d1, p2, d2):
    with np.errstate(all="ignore"):
        r = p1 - p2
        A, E, f, c, B = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
        den = A * E - B * B
        s = np.where(den > 0, np.clip((B * f - c * E) / den, 0, 1), 0.0)
        t = (B * s + f) / E
        s = np.where(t < 0, np.clip(-c / A, 0, 1), np.where(t > 1, np.clip((B - c) / A, 0, 1), s))
        t = np.clip(t, 0, 1)
        s, t = np.nan_to_num(s), np.nan_to_num(t)
    df = (p1 + d1 * s[:, None]) - (p2 + d2 * t[:, None])
    return _dot(df, df)


def seg_hits_tri64(p, d, tri):
    """does the segment p .. p + d meet the triangle (Moller-Trumbore, closed)"""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    h = np.cross(d, e2)
    det = _dot(e1, h)
    with np.errstate(all="ignore"):
        s = p - tri[:, 0]
        u = _dot(s, h) / det
        qv = np.cross(s, e1)
        v = _dot(d, qv) / det
        t = _dot(e2, qv) / det
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def dist2_64(q, m):
    """the fifteen candidates on the vertices v0, v1, v2 and the six edge-triangle crossing tests, in float64, for
    the pairs (q[p], m[p]) -> the squared distance [p]"""
    D = np.full(len(q), np.inf)
    for k in range(3):
        D = np.minimum(D, near64(q[:, k], m))
        D = np.minimum(D, near64(m[:, k], q))
    for i in range(3):
        for j in range(3):
            D = np.minimum(D, segseg64(q[:, i], q[:, (i + 1) % 3] - q[:, i], m[:, j], m[:, (j + 1) % 3] - m[:, j]))
    hit = np.zeros(len(q), bool)
    for i in range(3):
        hit |= seg_hits_tri64(q[:, i], q[:, (i + 1) % 3] - q[:, i], m)
        hit |= seg_hits_tri64(m[:, i], m[:, (i + 1) % 3] - m[:, i], q)
    return np.where(hit, 0.0, D)


def against_f64(coords, q, tri, d2):
    """the float64 distance of every query to the mesh -> (dist64 [n], the float64 answer's triangle [n]). Only the
    triangles whose float64 box distance does not exceed the float64 distance of the float32 answer's own pair can
    hold the minimum; those are evaluated."""
    c64, q64 = coords.astype(np.float64), q.astype(np.float64)
    top = dist2_64(q64, c64[tri])
    tlo, thi = c64.min(axis=1), c64.max(axis=1)
    qlo, qhi = q64.min(axis=1), q64.max(axis=1)
    dist, arg = np.zeros(len(q)), np.zeros(len(q), np.int64)
    for i in range(len(q)):
        e = np.maximum(np.maximum(tlo - qhi[i], qlo[i] - thi), 0.0)
        ti = np.flatnonzero((e * e).sum(axis=1) <= top[i])
        D = dist2_64(np.broadcast_to(q64[i], (len(ti), 3, 3)), c64[ti])
        dist[i], arg[i] = np.sqrt(D.min()), ti[np.argmin(D)]
    return dist, arg


# the measured residuals max |sqrt(D32) - dist64| (below), as fractions of the scene's extent
RESIDUAL = {"car_only": 2.93e-8, "car_boxed": 4.01e-8}
SEED = {"car_only": 71, "car_boxed": 72}


@pytest.mark.parametrize("scene", ["car_only", "car_boxed"])
def test_the_yardstick_agrees_with_float64(scene):
    """256 queries of clearance_ref.fixture_tris per scene (the GPU tests' own). Measured:
    car_only   kinds 15 / 0..2 / 3..5 / 6..14 = 113 / 52 / 45 / 46, 221 queries with a shared minimum, all 256 of proper
               area; max |sqrt(D32) - dist64| = 3.21e-7 = 2.93e-8 extent; float64 names another triangle for 12 queries
               (ties within rounding); the points lie within 2.9e-8 extent of their triangles;
    car_boxed  117 / 56 / 40 / 43, 185 shared minima; 8.16e-7 = 4.01e-8 extent; another triangle for 1 query; points
               within 4.0e-8 extent.
    No crossing is decided differently by the six float64 edge-triangle tests (such a query would show its whole
    distance as error). The points' own bounds are float32's: 2^-24 of a coordinate of up to one extent, over the
    ten or so roundings between the corners and a point, below 1e-6 extent.
    The bound is 4 x the measured residual, the margin of §3p and §3v; the conditions on the fixture are the
    issue's: at least 32 answers of kind 15, 32 of kinds 0..2, 32 of kinds 3..5 and 16 of kinds 6..14, at least 50
    queries whose minimal D two or more triangles share, and no query empty without a bound."""
    coords = host.Scene.named(scene).triangles["coords"]
    ext = cr.scene_extent(coords)
    q = cr.fixture_tris(coords, 256, seed=SEED[scene])
    tri, d2, oq, om, kind, ties = cr.expected(q, coords)
    groups = [int((kind == 15).sum()), int(((kind >= 0) & (kind <= 2)).sum()), int(((kind >= 3) & (kind <= 5)).sum()),
              int(((kind >= 6) & (kind <= 14)).sum())]
    assert (tri >= 0).all() and np.isfinite(oq).all() and np.isfinite(om).all()
    assert groups[0] >= 32 and groups[1] >= 32 and groups[2] >= 32 and groups[3] >= 16, groups
    assert int((ties >= 2).sum()) >= 50
    q64 = q.astype(np.float64)
    area = np.linalg.norm(np.cross(q64[:, 1] - q64[:, 0], q64[:, 2] - q64[:, 0]), axis=1)
    proper = area > 1e-12 * ext * ext
    dist, arg = against_f64(coords, q, tri, d2)
    err = np.abs(np.sqrt(d2.astype(np.float64)) - dist)
    # the reported points: each on its own triangle, and as far apart as D says
    on = max(np.sqrt(near64(oq.astype(np.float64), q64)).max(),
             np.sqrt(near64(om.astype(np.float64), coords[tri].astype(np.float64))).max())
    gap = np.abs(np.linalg.norm(oq.astype(np.float64) - om.astype(np.float64), axis=1) - np.sqrt(d2.astype(np.float64)))
    print(f"{scene}: kinds 15 / 0-2 / 3-5 / 6-14 = {groups}, {int((ties >= 2).sum())} queries with a shared minimum, "
          f"{int(proper.sum())} of proper area; max |sqrt(D32) - dist64| = {err[proper].max():.3e} = "
          f"{err[proper].max() / ext:.3e} extent (query {int(np.argmax(np.where(proper, err, -1)))}); the float64 answer is "
          f"another triangle for {int((arg != tri).sum())} queries; points off their triangles by at most "
          f"{on / ext:.3e} extent, |on_query - on_mesh| off sqrt(D) by at most {gap.max() / ext:.3e} extent")
    assert proper.sum() >= 250
    assert err[proper].max() <= 4 * RESIDUAL[scene] * ext
    assert on <= 1e-6 * ext and gap.max() <= 1e-6 * ext
