"""The triangle contact query's ABI (rt_sweep_tri_contacts / rt_get_tricontacts_info, include/rt_hip.h) without a GPU:
the symbols are exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself),
Renderer.sweep_tri_contacts refuses bad arguments before any device call, the family's row of the query logic gives its
messages, and the yardstick of the GPU tests (tests/tricontacts_ref.py) gives the stated lists on closed-form pairs and
is sound against geometry in float64 on the GPU tests' own fixture, over every member of every query: each member is a
real contact, and the set is geometry's but for grazing pairs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host
from tests import tricontacts_ref as tc
from tests import trisweep_ref as tr
from tests.test_clearance_abi import dist2_64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")
F = np.float32
FMAX = tc.FMAX


def test_tricontacts_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_sweep_tri_contacts", "rt_get_tricontacts_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_sweep_tri_contacts, L.rt_get_tricontacts_info
    # no context: refused before anything else is read
    assert L.rt_sweep_tri_contacts(None, None, None) == -1 and L.rt_get_tricontacts_info(None, None) == -1


def test_tricontacts_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_tri_contacts": _lib.TriContacts, "rt_tricontact_results": _lib.TricontactResults,
               "rt_tricontacts_info": _lib.TricontactsInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {",
             'printf("RT_TRICONTACTS_MAX %d\\n", RT_TRICONTACTS_MAX);']
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
    assert int(got["RT_TRICONTACTS_MAX"]) == _lib.TRICONTACTS_MAX == 16
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in _lib.TriContacts._fields_] == ["tris", "motion", "t_max", "n", "max_tris", "count_all",
                                                         "kernel"]
    assert [f for f, _ in _lib.TricontactResults._fields_] == ["tri", "t", "point", "kind", "count"]
    assert [f for f, _ in _lib.TricontactsInfo._fields_] == [
        "triangles", "found", "stored", "counted", "walked", "exhaustive", "empty", "nodes_visited", "pairs_gated",
        "pairs_tested", "stack_overflows", "kernel_ms"]


def test_tricontacts_arguments_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok, mv = torch.zeros(8, 3, 3, dtype=torch.float32), torch.zeros(8, 3, dtype=torch.float32)
    for bad in (-1, 17, 2.0, True, None):
        with pytest.raises(device.RtError, match="k: .* expected an int in 0..16"):
            r.sweep_tri_contacts(ok, mv, k=bad)
    with pytest.raises(device.RtError, match="k = 0 stores nothing"):
        r.sweep_tri_contacts(ok, mv, k=0)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # a host tensor
        r.sweep_tri_contacts(ok, mv)
    with pytest.raises(device.RtError, match="tris: dtype"):
        r.sweep_tri_contacts(ok.double(), mv)
    with pytest.raises(device.RtError, match=r"tris: shape .* expected \[n, 3, 3\]"):
        r.sweep_tri_contacts(torch.zeros(8, 9), mv)
    with pytest.raises(device.RtError, match="contiguous"):
        r.sweep_tri_contacts(torch.zeros(16, 3, 3)[::2], mv)
    with pytest.raises(device.RtError, match="torch tensor"):
        r.sweep_tri_contacts([[[0.0] * 3] * 3], mv)
    for bad in ((1234, -1), (1234.0, 8), (1234, 8, 3)):
        with pytest.raises(device.RtError, match="raw pointer"):
            r.sweep_tri_contacts(bad, 5678)
    with pytest.raises(device.RtError, match=r"motions: shape .* expected \[n, 3\]"):
        r.sweep_tri_contacts(ok, torch.zeros(8, 4))
    with pytest.raises(device.RtError, match="motions: expected a torch tensor"):
        r.sweep_tri_contacts(ok, [[0.0] * 3] * 8)
    with pytest.raises(device.RtError, match="motions: a raw pointer"):
        r.sweep_tri_contacts((1234, 8), mv)
    raw = ((1234, 8), 5678)
    with pytest.raises(device.RtError, match="t_max: shape"):
        r.sweep_tri_contacts(*raw, t_max=torch.zeros(8, 1))
    with pytest.raises(device.RtError, match="t_max: dtype"):
        r.sweep_tri_contacts(*raw, t_max=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(device.RtError, match="t_max: 7 elements"):
        r.sweep_tri_contacts(*raw, t_max=torch.zeros(7))
    with pytest.raises(device.RtError, match="t_max: expected a torch tensor"):
        r.sweep_tri_contacts(*raw, t_max=[1.0] * 8)
    # the optional outputs, before anything is allocated (an allocation would fail too: there is no device here)
    i32 = torch.int32
    with pytest.raises(device.RtError, match=r"tri: shape .* expected \[n, k\]"):
        r.sweep_tri_contacts(*raw, k=4, tri=torch.zeros(32, dtype=i32))
    with pytest.raises(device.RtError, match=r"tri: shape .* expected \[n, k\]"):
        r.sweep_tri_contacts(*raw, k=4, tri=torch.zeros(8, 5, dtype=i32))
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.sweep_tri_contacts(*raw, k=4, tri=torch.zeros(8, 4))
    with pytest.raises(device.RtError, match="t: 28 elements"):
        r.sweep_tri_contacts(*raw, k=4, t=torch.zeros(7, 4))
    with pytest.raises(device.RtError, match="count: 7 elements"):
        r.sweep_tri_contacts(*raw, k=4, count=torch.zeros(7, dtype=i32))
    with pytest.raises(device.RtError, match="count: dtype"):
        r.sweep_tri_contacts(*raw, k=4, count=torch.zeros(8))
    with pytest.raises(device.RtError, match=r"point: shape .* expected \[n, 4, 3\]"):
        r.sweep_tri_contacts(*raw, k=4, point=torch.zeros(8, 12))
    with pytest.raises(device.RtError, match="point: 84 elements"):
        r.sweep_tri_contacts(*raw, k=4, point=torch.zeros(7, 4, 3))
    with pytest.raises(device.RtError, match=r"kind: shape .* expected \[n, k\]"):
        r.sweep_tri_contacts(*raw, k=4, kind=torch.zeros(8, 3, dtype=i32))
    with pytest.raises(device.RtError, match="kind: dtype"):
        r.sweep_tri_contacts(*raw, k=4, kind=torch.zeros(8, 4))
    r._ctx = None  # (nothing to destroy)


def test_tricontacts_row_of_the_query_logic(tmp_path):
    """tests/c/tricontacts_logic_test.cpp: the family's number, its row and its messages against literal text"""
    exe = tmp_path / "tricontacts_logic_test"
    src = os.path.join(ROOT, "tests", "c", "tricontacts_logic_test.cpp")
    inc = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc,
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


# ------------------------------------------------------------------ closed-form lists
def lists(q, d, mesh, k, tm=None, count_all=False):
    """one query's lists -> (tri [k], t [k], point [k, 3], kind [k], count)"""
    out = tc.expected(np.array([q], F), np.array([d], F), np.asarray(mesh, F), k,
                      None if tm is None else np.array([tm], F), count_all)
    return out[0][0].tolist(), out[1][0].tolist(), out[2][0].tolist(), out[3][0].tolist(), int(out[4][0])


# two sheets, one under the other: triangle 0 in z = -1 (the lower), triangle 1 in z = 0
SHEETS = [[[0, 0, -1], [4, 0, -1], [0, 4, -1]], [[0, 0, 0], [4, 0, 0], [0, 4, 0]]]
PLATE = [[1, 1, 1], [2, 1, 1], [1, 2, 1]]


def test_a_plate_through_two_sheets_lists_both_in_time_order():
    tri, t, pt, kind, count = lists(PLATE, [0, 0, -4], SHEETS, 4)
    assert tri == [1, 0, -1, -1] and t == [0.25, 0.5, FMAX, FMAX] and count == 2
    assert pt == [[1, 1, 0], [1, 1, -1], [1, 1, 1], [1, 1, 1]]  # (unused slots: q0's own bits)
    assert kind == [0, 0, -1, -1]
    # k = 1 is the sweep's answer; the count is the list's, or the set's with count_all
    one = tr.expected(np.array([PLATE], F), np.array([[0, 0, -4]], F), np.array(SHEETS, F))
    tri, t, pt, kind, count = lists(PLATE, [0, 0, -4], SHEETS, 1)
    assert (tri, t, pt, kind, count) == ([int(one[0][0])], [one[1][0]], [one[2][0].tolist()], [int(one[3][0])], 1)
    assert lists(PLATE, [0, 0, -4], SHEETS, 1, count_all=True)[4] == 2
    assert lists(PLATE, [0, 0, -4], SHEETS, 0, count_all=True) == ([], [], [], [], 2)
    # the swept volume from q to q + d (t_max = 1): the prism reaches the upper sheet only
    assert lists(PLATE, [0, 0, -1.5], SHEETS, 0, tm=1, count_all=True)[4] == 1
    assert lists(PLATE, [0, 0, 1], SHEETS, 4)[4] == 0  # moving away


def test_a_shared_edge_lists_both_triangles_at_one_toi():
    """tests/test_trisweep_abi.py's pair of triangles that share the edge (0, 0, 0) - (0, 4, 0), met head on by a query
    edge: both at toi 3, the lower index first, whichever way round the mesh is stored"""
    mesh = np.array([[[0, 0, 0], [4, 0, -1], [0, 4, 0]], [[0, 0, 0], [0, 4, 0], [-4, 0, -1]]], F)
    q = [[-1, 2, 3], [1, 2, 3], [0, 2, 5]]
    for m in (mesh, mesh[::-1]):
        tri, t, pt, kind, count = lists(q, [0, 0, -1], m, 2)
        assert tri == [0, 1] and t == [3, 3] and count == 2 and pt == [[0, 2, 0], [0, 2, 0]]
    mem = tc.members(np.array([q], F), np.array([[0, 0, -1]], F), mesh)
    assert tc.boundary_ties(mem, 1).tolist() == [True] and tc.boundary_ties(mem, 2).tolist() == [False]


def test_a_start_in_contact_with_two_triangles():
    q = [[1, 1, -2], [2, 1, 1], [1, 1, 1]]  # pierces both sheets
    for d in ([0, 0, 0], [1, 2, 3]):
        tri, t, pt, kind, count = lists(q, d, SHEETS, 4)
        assert tri == [0, 1, -1, -1] and t == [0, 0, FMAX, FMAX] and kind == [15, 15, -1, -1] and count == 2
        assert pt[0][2] == -1 and pt[1][2] == 0
    assert lists(q, [1, 2, 3], SHEETS, 4, tm=0)[0] == [0, 1, -1, -1]  # t_max = 0: what it touches now


def test_the_bound_is_inclusive_to_the_bit():
    d = [0, 0, -4]
    mem = tc.members(np.array([PLATE], F), np.array([d], F), np.array(SHEETS, F))
    for k, want in ((1, 0.25), (2, 0.5)):
        rows, kth = tc.kth_toi(mem, k)
        assert rows.tolist() == [0] and kth[0] == F(want)
        assert lists(PLATE, d, SHEETS, 4, tm=kth[0], count_all=True)[4] == k  # T equal to the k-th toi keeps it
        assert lists(PLATE, d, SHEETS, 4, tm=np.nextafter(kth[0], F(0)), count_all=True)[4] == k - 1
        assert lists(PLATE, d, SHEETS, 4, tm=np.nextafter(kth[0], F(1)), count_all=True)[4] == k
    assert tc.kth_toi(mem, 3)[0].tolist() == []
    neg = np.array([0x80000001, 0x80011111], np.uint32).view(F)  # negative subnormals, from their bits
    for bad in (np.nan, F(-1), neg[0], neg[1]):
        assert lists(PLATE, d, SHEETS, 2, tm=bad) == ([-1, -1], [FMAX, FMAX], [[1, 1, 1]] * 2, [-1, -1], 0)


# ------------------------------------------------------------------ the yardstick against geometry in float64
# Measured over every member of the 640 fixture queries per scene (the tests print them):
#   REAL   the largest float64 distance between a member's query, moved to that member's toi, and its triangle, as a
#          fraction of the scene's extent (41,773 members on car_only, 43,307 on car_boxed; the first members alone give
#          tests/test_trisweep_abi.py's REAL);
#   SETS   (only in the float64 set, only in the float32 set): the pairs on which S_i and the set of pairs with a finite
#          float64 time of impact differ -- grazing pairs.
REAL = {"car_boxed": 1.01e-7, "car_only": 1.01e-7}
SETS = {"car_boxed": (2, 8), "car_only": (4, 21)}
CEILING = 2.0 ** -12  # of the extent: the bound may not exceed it (tests/test_trisweep_abi.py's)


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for scene in ("car_boxed", "car_only"):
        coords = host.Scene.named(scene).triangles["coords"]
        q, d = tr.fixture(coords, tr.SEED[scene])
        out[scene] = coords, q, d, tc.members(q, d, coords)
    return out


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_every_member_is_real(fixtures, scene):
    """every member (i, j, toi) of every fixture query: the float64 distance between query i moved to toi and triangle
    j, by tests/test_clearance_abi.py's dist2_64, within 8 x the measured residual; no query and no member is excluded"""
    coords, q, d, mem = fixtures[scene]
    ext = tr.scene_extent(coords)
    assert mem.total.sum() == len(mem.qi) > 40000
    moved = q.astype(np.float64)[mem.qi] + (d.astype(np.float64)[mem.qi] * mem.toi.astype(np.float64)[:, None])[:, None, :]
    dist = np.sqrt(dist2_64(moved, coords[mem.ti].astype(np.float64)))
    first = dist[mem.rank == 0]
    on = np.sqrt(dist2_64(np.repeat(mem.pt.astype(np.float64)[:, None, :], 3, axis=1), coords[mem.ti].astype(np.float64)))
    w = int(np.argmax(dist))
    print(f"{scene}: {len(dist)} members, the largest distance {dist.max() / ext:.3e} extent (query {int(mem.qi[w])}, "
          f"rank {int(mem.rank[w])}, kind {int(mem.kind[w])}); first members alone {first.max() / ext:.3e}; points off "
          f"their triangles by at most {on.max() / ext:.3e} extent")
    assert 8 * REAL[scene] <= CEILING
    assert dist.max() <= 8 * REAL[scene] * ext
    assert on.max() <= 1e-6 * ext


@pytest.mark.parametrize("scene", ["car_boxed", "car_only"])
def test_the_set_is_geometrys_but_for_grazing_pairs(fixtures, scene):
    """S_i against the pairs with a finite float64 time of impact (tr.gate64, then tr.toi64; the fixture gives no
    t_max): each difference is at most 1 per 1,000 members"""
    coords, q, d, mem = fixtures[scene]
    qi, ti = tr.gate64(q, d, coords, np.full(len(q), np.inf))
    fin = np.isfinite(tr.toi64(q[qi], d[qi], coords[ti]))
    n = len(coords)
    s64 = np.unique(qi[fin].astype(np.int64) * n + ti[fin])
    s32 = np.unique(mem.qi.astype(np.int64) * n + mem.ti)
    only64, only32 = len(np.setdiff1d(s64, s32)), len(np.setdiff1d(s32, s64))
    print(f"{scene}: {len(s32)} members in float32, {len(s64)} in float64; only in float64 {only64}, only in float32 "
          f"{only32} (measured: {SETS[scene]})")
    assert len(s32) == len(mem.qi)
    assert only64 * 1000 <= len(s32) and only32 * 1000 <= len(s32)
