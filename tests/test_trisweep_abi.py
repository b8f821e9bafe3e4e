"""The triangle sweep query's ABI (rt_sweep_triangles / rt_get_trisweep_info, include/rt_hip.h) without a GPU: the
symbols are exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself), Renderer.sweep_tris
refuses bad arguments before any device call, the family's row of the query logic gives its messages, and the yardstick
of the GPU tests (tests/trisweep_ref.py) gives the stated answers on closed-form pairs and is sound against geometry in
float64 on the GPU tests' own fixture: every contact it reports is real, and none earlier was missed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host
from tests import trisweep_ref as tr
from tests.test_clearance_abi import dist2_64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")
F = np.float32
FMAX = tr.FMAX


def test_trisweep_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_sweep_triangles", "rt_get_trisweep_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_sweep_triangles, L.rt_get_trisweep_info


def test_trisweep_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_sweep_tris": _lib.SweepTris, "rt_trisweep_results": _lib.TrisweepResults,
               "rt_trisweep_info": _lib.TrisweepInfo}
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
    assert [f for f, _ in _lib.SweepTris._fields_] == ["tris", "motion", "t_max", "n", "kernel"]
    assert [f for f, _ in _lib.TrisweepResults._fields_] == ["tri", "t", "point", "kind"]
    assert [f for f, _ in _lib.TrisweepInfo._fields_] == [
        "triangles", "found", "empty", "walked", "exhaustive", "nodes_visited", "pairs_gated", "pairs_tested",
        "stack_overflows", "kernel_ms"]


def test_trisweep_arguments_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok, mv = torch.zeros(8, 3, 3, dtype=torch.float32), torch.zeros(8, 3, dtype=torch.float32)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # a host tensor
        r.sweep_tris(ok, mv)
    with pytest.raises(device.RtError, match="tris: dtype"):
        r.sweep_tris(ok.double(), mv)
    with pytest.raises(device.RtError, match=r"tris: shape .* expected \[n, 3, 3\]"):
        r.sweep_tris(torch.zeros(8, 9), mv)
    with pytest.raises(device.RtError, match=r"tris: shape .* expected \[n, 3, 3\]"):
        r.sweep_tris(torch.zeros(8, 3, 4), mv)
    with pytest.raises(device.RtError, match="contiguous"):
        r.sweep_tris(torch.zeros(16, 3, 3)[::2], mv)
    with pytest.raises(device.RtError, match="torch tensor"):
        r.sweep_tris([[[0.0] * 3] * 3], mv)
    for bad in ((1234, -1), (1234.0, 8), (1234, 8, 3)):
        with pytest.raises(device.RtError, match="raw pointer"):
            r.sweep_tris(bad, 5678)
    with pytest.raises(device.RtError, match=r"motions: shape .* expected \[n, 3\]"):
        r.sweep_tris(ok, torch.zeros(8, 4))
    with pytest.raises(device.RtError, match=r"motions: shape .* expected \[n, 3\]"):
        r.sweep_tris(ok, torch.zeros(24))
    with pytest.raises(device.RtError, match="motions: expected a torch tensor"):
        r.sweep_tris(ok, [[0.0] * 3] * 8)
    with pytest.raises(device.RtError, match="motions: a raw pointer"):
        r.sweep_tris((1234, 8), mv)
    raw = ((1234, 8), 5678)
    with pytest.raises(device.RtError, match="t_max: shape"):
        r.sweep_tris(*raw, t_max=torch.zeros(8, 1))
    with pytest.raises(device.RtError, match="t_max: dtype"):
        r.sweep_tris(*raw, t_max=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(device.RtError, match="t_max: 7 elements"):
        r.sweep_tris(*raw, t_max=torch.zeros(7))
    with pytest.raises(device.RtError, match="t_max: expected a torch tensor"):
        r.sweep_tris(*raw, t_max=[1.0] * 8)
    # the optional outputs, before anything is allocated (an allocation would fail too: there is no device here)
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.sweep_tris(*raw, tri=torch.zeros(8))
    with pytest.raises(device.RtError, match="t: 7 elements"):
        r.sweep_tris(*raw, t=torch.zeros(7))
    with pytest.raises(device.RtError, match="point: shape"):
        r.sweep_tris(*raw, point=torch.zeros(24))
    with pytest.raises(device.RtError, match="point: 21 elements"):
        r.sweep_tris(*raw, point=torch.zeros(7, 3))
    with pytest.raises(device.RtError, match="kind: dtype"):
        r.sweep_tris(*raw, kind=torch.zeros(8))
    with pytest.raises(device.RtError, match="kind: 7 elements"):
        r.sweep_tris(*raw, kind=torch.zeros(7, dtype=torch.int32))
    r._ctx = None  # (nothing to destroy)


def test_trisweep_row_of_the_query_logic(tmp_path):
    """tests/c/trisweep_logic_test.cpp: the family's messages against literal text, the earlier numbering as it was"""
    exe = tmp_path / "trisweep_logic_test"
    src = os.path.join(ROOT, "tests", "c", "trisweep_logic_test.cpp")
    inc = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc,
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


# ------------------------------------------------------------------ closed-form pairs
# mesh triangle 0 lies in z = 0, triangle 1 in z = 1, far apart in x
MESH = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[10, 0, 1], [14, 0, 1], [10, 4, 1]]], F)


def one(q, d, tm=None, mesh=MESH):
    """the answer to one query -> (tri, t, point, kind)"""
    tri, t, pt, kind, _ = tr.expected(np.array([q], F), np.array([d], F), mesh, None if tm is None else np.array([tm], F))
    return int(tri[0]), t[0], pt[0].tolist(), int(kind[0])


def test_a_plate_lands_on_its_first_corner():
    """a small plate parallel to triangle 0, one unit above it, moving down: the gate opens at 1/2 where the plate lies
    in the plane (coplanar: no crossing), and its three corners tie at u = 0; the first offered keeps the answer"""
    q = [[1, 1, 1], [2, 1, 1], [1, 2, 1]]
    assert one(q, [0, 0, -2]) == (0, F(0.5), [1, 1, 0], 0)
    assert one(q, [0, 0, -1]) == (0, F(1), [1, 1, 0], 0)
    assert one(q, [0, 0, 1]) == (-1, FMAX, [1, 1, 1], -1)  # moving away
    # a plate larger than the mesh triangle: the mesh corner a meets its interior (b and c tie later in the order)
    assert one([[-5, -5, 2], [8, -5, 2], [-5, 8, 2]], [0, 0, -1]) == (0, F(2), [0, 0, 0], 3)


def test_two_skew_edges_have_an_edge_kind():
    """the query's first edge runs along z through (5, 5, .) and moves along (-1, -1, 0) onto the mesh triangle's third
    edge from (4, 0, 0) to (0, 4, 0): the boxes meet at t0 = 1, the edges at (2, 2, 0) after 3. No corner candidate is
    valid: the motion lies in triangle 0's plane, and the mesh corners move along lines that miss the query's plane
    x = y"""
    assert one([[5, 5, -1], [5, 5, 1], [7, 7, 0]], [-1, -1, 0]) == (0, F(3), [2, 2, 0], 6 + 3 * 0 + 2)
    # the same pair from the query's third edge (qb -> qc)
    assert one([[7, 7, 0], [5, 5, -1], [5, 5, 1]], [-1, -1, 0]) == (0, F(3), [2, 2, 0], 6 + 3 * 2 + 2)


def test_a_start_in_contact_is_kind_15():
    q = [[1, 1, -1], [2, 1, 1], [1, 1, 1]]  # pierces triangle 0
    for d in ([0, 0, 0], [1, 2, 3], [0, 0, -5]):
        assert one(q, d) == (0, F(0), [1, 1, 0], 15)
    assert one(q, [1, 2, 3], F(0)) == (0, F(0), [1, 1, 0], 15)  # t_max = 0: does it touch now
    # d = 0 away from the mesh: nothing
    assert one([[1, 1, 2], [2, 1, 3], [1, 1, 3]], [0, 0, 0]) == (-1, FMAX, [1, 1, 2], -1)
    # a corner that arrives point first: the query's box and the triangle's meet where the triangles do, so the
    # crossing test holds at the gate's own t0 (the header's note on step 4)
    tri, t, pt, kind = one([[1, 1, 1], [2, 1, 3], [1, 1, 3]], [0, 0, -1])
    assert (tri, t, pt) == (0, F(1), [1, 1, 0]) and kind in (0, 15)


def test_the_bound_is_inclusive_to_the_bit():
    q, d = [[1, 1, 1], [2, 1, 1], [1, 2, 1]], [0, 0, -2]
    assert one(q, d, F(0.5))[:2] == (0, F(0.5)) and one(q, d, np.inf)[0] == 0
    below = np.nextafter(F(0.5), F(0))
    assert one(q, d, below) == (-1, FMAX, [1, 1, 1], -1)  # one float beyond the bound: q0's bits
    neg = np.array([0x80000001, 0x80011111], np.uint32).view(F)  # negative subnormals, from their bits
    for bad in (np.nan, F(-1), neg[0], neg[1]):
        assert one(MESH[0], [0, 0, 1], bad) == (-1, FMAX, [0, 0, 0], -1)
    assert one([[1, 1, -1], [2, 1, 1], [1, 1, 1]], d, F(-0.0))[0] == 0  # (-0 is the bound 0)


def test_a_non_finite_number_gives_the_empty_set():
    good = np.array([[1, 1, -1], [2, 1, 1], [1, 1, 1]], F)
    q, d = [], []
    for pos in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            t, m = good.copy(), np.array([0, 0, -1], F)
            if pos < 9:
                t.reshape(-1)[pos] = bad
            else:
                m[pos - 9] = bad
            q.append(t)
            d.append(m)
    q, d = np.array(q), np.array(d)
    tri, t, pt, kind, ties = tr.expected(q, d, MESH)
    assert len(q) == 36 and (tri == -1).all() and (t == FMAX).all() and (kind == -1).all() and (ties == 0).all()
    assert tr.same_bits(pt, q[:, 0])


def test_zero_area_queries_are_answered_by_the_candidates():
    """a segment and a point moving down onto triangle 0: X excludes them, the corner rays answer"""
    assert one([[1, 1, 2], [2, 1, 2], [2, 1, 2]], [0, 0, -1]) == (0, F(2), [1, 1, 0], 0)
    assert one([[1, 1, 2]] * 3, [0, 0, -4]) == (0, F(0.5), [1, 1, 0], 0)
    assert one([[1, 1, 0]] * 3, [0, 0, 0])[:2] == (-1, FMAX)  # a resting point has no motion to make a ray of


def test_a_shared_edge_goes_to_the_lower_index():
    """two mesh triangles that share the edge (0, 0, 0) - (0, 4, 0), met head on by a query edge: an exact tie (the
    query's lowest edge is its box's floor and the shared edge the mesh boxes' top, so the gate opens at the contact
    and the crossing test answers: kind 15)"""
    mesh = np.array([[[0, 0, 0], [4, 0, -1], [0, 4, 0]], [[0, 0, 0], [0, 4, 0], [-4, 0, -1]]], F)
    q = [[-1, 2, 3], [1, 2, 3], [0, 2, 5]]
    tri, t, pt, kind, ties = tr.expected(np.array([q], F), np.array([[0, 0, -1]], F), mesh)
    assert (tri[0], t[0], pt[0].tolist(), ties[0]) == (0, F(3), [0, 2, 0], 2) and kind[0] == 15
    tri, _, _, _, ties = tr.expected(np.array([q], F), np.array([[0, 0, -1]], F), mesh[::-1])
    assert (tri[0], ties[0]) == (0, 2)


# ------------------------------------------------------------------ the yardstick against geometry in float64
# The measured residuals over the 640 fixture queries per scene, as fractions of the scene's extent (the test prints them):
#   REAL   the largest float64 distance between a found answer's query, moved to toi, and its triangle;
#   EARLY  the largest (toi - the least float64 time of impact over every triangle) * |d|.
REAL = {"car_boxed": 4.66e-8, "car_only": 4.49e-8}
EARLY = {"car_boxed": 7.56e-8, "car_only": 7.92e-8}
CEILING = 2.0 ** -12  # of the extent: neither bound may exceed it


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for scene in ("car_boxed", "car_only"):
        coords = host.Scene.named(scene).triangles["coords"]
        q, d = tr.fixture(coords, tr.SEED[scene])
        out[scene] = coords, q, d, tr.expected(q, d, coords)
    return out


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_the_fixture_holds_what_it_must(fixtures, scene):
    coords, q, d, want = fixtures[scene]
    print(scene, tr.check_fixture(want))
    tri, t, pt, kind, _ = want
    none = tri < 0
    assert (t[none] == FMAX).all() and (kind[none] == -1).all() and tr.same_bits(pt[none], q[none, 0])
    rec = tr.records(coords)
    assert ((pt >= rec[5][tri]) & (pt <= rec[6][tri]))[~none].all()  # the point lies in the triangle's corner box


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_every_contact_is_real(fixtures, scene):
    """every found answer (j, toi): the float64 distance between the query moved to toi and triangle j, by
    tests/test_clearance_abi.py's dist2_64 (fifteen candidates and six edge-triangle crossings), within 8 x the
    measured residual; no query is excluded"""
    coords, q, d, (tri, t, pt, kind, _) = fixtures[scene]
    ext = tr.scene_extent(coords)
    found = tri >= 0
    moved = q.astype(np.float64) + (d.astype(np.float64) * t.astype(np.float64)[:, None])[:, None, :]
    dist = np.sqrt(dist2_64(moved[found], coords[tri[found]].astype(np.float64)))
    on = np.sqrt(dist2_64(np.repeat(pt[found].astype(np.float64)[:, None, :], 3, axis=1),
                          coords[tri[found]].astype(np.float64)))
    print(f"{scene}: {int(found.sum())} contacts, the largest distance {dist.max():.3e} = {dist.max() / ext:.3e} extent "
          f"(kind {int(kind[found][np.argmax(dist)])}); points off their triangles by at most {on.max() / ext:.3e} extent")
    assert 8 * REAL[scene] <= CEILING
    assert dist.max() <= 8 * REAL[scene] * ext
    assert on.max() <= 1e-6 * ext


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_nothing_earlier_was_missed(fixtures, scene):
    """no triangle's float64 time of impact lies below a found toi by more than the margin, and an empty answer has
    none at all (the fixture gives no t_max). tr.toi64 is evaluated for every pair whose float64 boxes meet before
    the query's toi (a contact needs that); the margin is a distance, (toi - toi64) * |d|, within 8 x the measured
    residual; no query is excluded"""
    coords, q, d, (tri, t, _, kind, _) = fixtures[scene]
    ext = tr.scene_extent(coords)
    found = tri >= 0
    until = np.where(found, t.astype(np.float64), np.inf)
    qi, ti = tr.gate64(q, d, coords, until)
    t64 = tr.toi64(q[qi], d[qi], coords[ti])
    first = np.full(len(q), np.inf)
    np.minimum.at(first, qi, t64)
    assert not np.isfinite(first[~found]).any(), np.flatnonzero(~found & np.isfinite(first))[:8]
    with np.errstate(invalid="ignore"):
        early = np.where(found, np.maximum(until - first, 0.0), 0.0) * np.linalg.norm(d.astype(np.float64), axis=1)
    w = int(np.argmax(early))
    print(f"{scene}: {len(qi)} float64 pairs; the earliest missed contact precedes toi by {early.max():.3e} = "
          f"{early.max() / ext:.3e} extent of travel (query {w}, kind {int(kind[w])})")
    assert 8 * EARLY[scene] <= CEILING
    assert early.max() <= 8 * EARLY[scene] * ext
