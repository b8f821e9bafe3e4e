"""The overlap query's ABI (rt_overlap_boxes / rt_get_overlaps_info, include/rt_hip.h) without a GPU: the symbols are
exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as tests/test_neighbours_abi.py
does), Renderer.overlaps / overlaps_csr refuse bad arguments before any device call, prt.boxes.grid tiles its box, and
the yardstick of the GPU tests (tests/overlap_ref.py) agrees with a plain float64 separating-axis test wherever that
one is not within rounding of touching, and gives the stated answers on fixed cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host
from tests import overlap_ref
from tests.test_nearest_abi import degenerate_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")


def test_overlap_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_overlap_boxes", "rt_get_overlaps_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_overlap_boxes, L.rt_get_overlaps_info


def test_overlap_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_boxes": _lib.Boxes, "rt_overlap_results": _lib.OverlapResults, "rt_overlaps_info": _lib.OverlapsInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {",
             'printf("RT_OVERLAPS_MAX %d\\n", RT_OVERLAPS_MAX);']
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
    assert int(got["RT_OVERLAPS_MAX"]) == _lib.OVERLAPS_MAX == 16
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in _lib.OverlapsInfo._fields_] == [
        "boxes", "found", "tris_stored", "tris_counted", "tris_listed", "walked_boxes", "exhaustive_boxes",
        "empty_boxes", "nodes_visited", "tris_tested", "stack_overflows", "kernel_ms"]


def test_overlap_arguments_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, dtype=torch.float32)
    for call in (r.overlaps, r.overlaps_csr):
        with pytest.raises(device.RtError, match="expected cuda:0"):  # host tensors
            call(ok, ok)
        with pytest.raises(device.RtError, match="lo: dtype"):
            call(ok.double(), ok)
        with pytest.raises(device.RtError, match=r"lo: shape .* expected \[n, 3\]"):
            call(torch.zeros(8, 4), ok)
        with pytest.raises(device.RtError, match=r"hi: shape .* expected \[n, 3\]"):
            call(ok, torch.zeros(24))
        with pytest.raises(device.RtError, match="hi: 7 boxes, lo has 8"):
            call(ok, torch.zeros(7, 3))
        with pytest.raises(device.RtError, match="contiguous"):
            call(torch.zeros(16, 3)[::2], ok)
        with pytest.raises(device.RtError, match="torch tensor"):
            call([[0.0, 0.0, 0.0]], ok)
        with pytest.raises(device.RtError, match="raw pointers"):
            call((1234, 8), ok)
        with pytest.raises(device.RtError, match="raw pointers"):
            call((1234, -1), 5678)
    for k in (-1, 17, 2.0, True, None):
        with pytest.raises(device.RtError, match="k: "):
            r.overlaps(ok, ok, k=k)
    with pytest.raises(device.RtError, match="needs count_all"):
        r.overlaps(ok, ok, k=0)
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.overlaps((1234, 8), 5678, k=4, tri=torch.zeros(32))
    with pytest.raises(device.RtError, match="tri: 31 elements"):
        r.overlaps((1234, 8), 5678, k=4, tri=torch.zeros(31, dtype=torch.int32))
    with pytest.raises(device.RtError, match="count: 7 elements"):
        r.overlaps((1234, 8), 5678, k=4, count=torch.zeros(7, dtype=torch.int32))
    r._ctx = None  # (nothing to destroy)


def test_grid_tiles_its_box():
    from prt import boxes
    lo, hi = boxes.grid([-1.0, 0.5, 2.0], [3.0, 0.75, 2.0], (4, 3, 2), device="cpu")
    assert lo.shape == hi.shape == (24, 3) and lo.dtype == hi.dtype == torch.float32
    assert lo.is_contiguous() and hi.is_contiguous()
    lo, hi = lo.numpy().reshape(2, 3, 4, 3), hi.numpy().reshape(2, 3, 4, 3)  # [iz, iy, ix]: x fastest
    assert (lo <= hi).all()
    assert np.array_equal(lo[:, :, 0, 0], np.full((2, 3), -1, np.float32)) and (hi[:, :, -1, 0] == 3.0).all()
    assert (lo[:, 0, :, 1] == 0.5).all() and (hi[:, -1, :, 1] == 0.75).all()
    assert (lo[..., 2] == 2.0).all() and (hi[..., 2] == 2.0).all()  # (a flat axis: plane boxes)
    assert np.array_equal(hi[:, :, :-1, 0], lo[:, :, 1:, 0])  # adjacent cells share their face bit for bit
    assert np.array_equal(hi[:, :-1, :, 1], lo[:, 1:, :, 1])
    assert np.array_equal(lo[0, 0, :, 0], np.float32(-1.0) + np.arange(4, dtype=np.float32) * np.float32(1.0))
    for bad in ((0, 1, 1), (1, 1), (1, 1, -2)):
        with pytest.raises(ValueError):
            boxes.grid([0, 0, 0], [1, 1, 1], bad, device="cpu")
    with pytest.raises(ValueError):
        boxes.grid([0, 0, 0], [1, -1, 1], (1, 1, 1), device="cpu")


# ------------------------------------------------------------------ the yardstick against float64
def gap_f64(lo, hi, tri):
    """a plain 13-axis separating-axis test of boxes [p, 3] against triangles [p, 3, 3] (their vertices) in float64 ->
    the normalised gap [p]: the largest, over the axes, of the distance between the two projections along the unit
    axis; positive: separated by that much, negative: they overlap by at least that much on every axis"""
    lo, hi, tri = lo.astype(np.float64), hi.astype(np.float64), tri.astype(np.float64)
    ctr, h = (lo + hi) / 2, (hi - lo) / 2
    v = tri - ctr[:, None, :]
    e = [v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]]
    eye = np.eye(3)
    axes = [np.broadcast_to(eye[k], ctr.shape) for k in range(3)] + [np.cross(e[0], e[1])]
    axes += [np.cross(f, np.broadcast_to(eye[k], ctr.shape)) for f in e for k in range(3)]
    scale = np.maximum(np.abs(e[0]).max(1), np.abs(e[1]).max(1))
    gap = np.full(len(ctr), -np.inf)
    with np.errstate(all="ignore"):
        for i, L in enumerate(axes):
            ln = np.linalg.norm(L, axis=1)
            ok = ln > 1e-9 * (scale * scale if i == 3 else scale)  # (a vanishing cross product is no axis)
            L = L / np.where(ok, ln, 1.0)[:, None]
            p = np.einsum("pmk,pk->pm", v, L)
            r = (h * np.abs(L)).sum(1)
            g = np.maximum(p.min(1) - r, -p.max(1) - r)
            gap = np.where(ok, np.maximum(gap, g), gap)
    return gap


def against_f64(coords, lo, hi):
    """(step-1 pairs, accepted, disagreements outside the band, pairs inside the band, box sizes)"""
    ext = overlap_ref.scene_extent(coords)
    bi, ti, t = overlap_ref.pairs(lo, hi, coords)
    gap = gap_f64(lo[bi], hi[bi], coords[ti])
    band = np.abs(gap) <= 2.0 ** -20 * ext
    wrong = ~band & (t != (gap <= 0))
    return len(bi), int(t.sum()), int(wrong.sum()), int(band.sum()), np.bincount(bi[t], minlength=len(lo))


def test_the_yardstick_agrees_with_float64():
    """256 boxes at car_only's surface (overlap_ref.surface_boxes: the issue's generator). Measured: 22,550 step-1
    pairs, 20,629 accepted, 0 disagreements with float64 outside the band |gap| <= 2^-20 extent, 5 pairs (0.022 %)
    inside it; median |S_i| 35, maximum 943, 166 of 256 boxes above 16. The bounds are the issue's:
    agreement outside the band, at most 0.1 % of the step-1 pairs inside it."""
    coords = host.Scene.named("car_only").triangles["coords"]
    lo, hi = overlap_ref.surface_boxes(coords, 256, seed=31)
    pairs, accepted, wrong, band, size = against_f64(coords, lo, hi)
    print(f"car_only: {pairs} step-1 pairs, {accepted} accepted, {wrong} disagreements outside the band, {band} pairs "
          f"({100.0 * band / pairs:.3f} %) inside it; |S_i| median {int(np.median(size))}, max {int(size.max())}, "
          f"{int((size > 16).sum())} of {len(size)} boxes above 16")
    assert wrong == 0
    assert band <= 0.001 * pairs
    assert pairs > 10000 and (size > 16).sum() >= 100 and (size <= 16).sum() >= 50  # the cut at k and the CSR form


# ------------------------------------------------------------------ the yardstick on fixed cases
@pytest.fixture(scope="module")
def car():
    return host.Scene.named("car_only").triangles["coords"]


def test_a_point_box_at_v0_reports_every_triangle_with_that_v0(car):
    rows = np.arange(0, len(car), 257)
    p = car[rows, 0]
    csr = overlap_ref.sets(p, p, car)
    v0 = car[:, 0]
    for i, s in enumerate(overlap_ref.segments(csr)):
        same = np.nonzero((v0.view(np.int32) == p[i].view(np.int32)).all(axis=1))[0]
        assert rows[i] in s and np.isin(same, s).all(), rows[i]
        assert (np.diff(s) > 0).all()  # index order, no duplicates


def test_a_box_over_the_scene_reports_every_triangle(car):
    rec = overlap_ref.records(car)
    tight = rec[5].min(0), rec[6].max(0)  # (closed boxes: the corner boxes' own extent is enough)
    v = car.reshape(-1, 3)
    loose = v.min(0) - np.float32(1), v.max(0) + np.float32(1)
    lo, hi = np.stack([tight[0], loose[0]]), np.stack([tight[1], loose[1]])
    offsets, tris = overlap_ref.sets(lo, hi, car)
    assert np.array_equal(np.diff(offsets), [len(car)] * 2)
    assert np.array_equal(tris.reshape(2, -1), np.tile(np.arange(len(car), dtype=np.int32), (2, 1)))
    tri, count = overlap_ref.answer((offsets, tris), 16, count_all=True)
    assert np.array_equal(tri, np.tile(np.arange(16, dtype=np.int32), (2, 1))) and (count == len(car)).all()


def invalid_boxes(p):
    """boxes around p [3] that hold a NaN, an infinity or lo > hi on one axis -> (lo, hi)"""
    lo, hi = [], []
    for k in range(3):
        for bad_lo, bad_hi in ((np.nan, 0), (0, np.nan), (-np.inf, 0), (0, np.inf), (np.inf, np.inf), (1, 0.5)):
            l, h = p - np.float32(1), p + np.float32(1)
            l[k] = p[k] + np.float32(bad_lo) if bad_lo else l[k]
            h[k] = p[k] + np.float32(bad_hi) if bad_hi else h[k]
            lo.append(l)
            hi.append(h)
    return np.array(lo, np.float32), np.array(hi, np.float32)


def test_invalid_boxes_report_nothing(car):
    lo, hi = invalid_boxes(car[100, 0].copy())
    assert len(lo) == 18 and not overlap_ref.valid_boxes(lo, hi).any()
    offsets, tris = overlap_ref.sets(lo, hi, car)
    assert (offsets == 0).all() and len(tris) == 0
    tri, count = overlap_ref.answer((offsets, tris), 4, count_all=True)
    assert (tri == -1).all() and (count == 0).all() and tri.shape == (18, 4)
    good = overlap_ref.sets(car[100, 0][None] - np.float32(1), car[100, 0][None] + np.float32(1), car)
    assert good[0][1] > 0  # (the same box without the bad number is not empty)


def test_degenerate_triangles_have_defined_answers():
    """test_nearest_abi.py's zero-area and repeated-vertex triangles: T is a defined bool for every box, a point box at
    v0 and a box around the triangle report it, a box away from it does not, and the float64 test agrees outside the
    band"""
    coords = degenerate_triangles()
    n = len(coords)
    v = coords.reshape(-1, 3)
    rng = np.random.default_rng(13)
    far = (np.array([[50, 50, 50]], np.float32), np.array([[51, 51, 51]], np.float32))
    around = coords.min(1) - np.float32(0.25), coords.max(1) + np.float32(0.25)
    ctr = rng.uniform(v.min(0), v.max(0), (64, 3))
    half = 10.0 ** rng.uniform(-2, 0, (64, 3))
    lo = np.concatenate([coords[:, 0], around[0], far[0], (ctr - half)]).astype(np.float32)
    hi = np.concatenate([coords[:, 0], around[1], far[1], (ctr + half)]).astype(np.float32)
    segs = overlap_ref.segments(overlap_ref.sets(lo, hi, coords))
    for j in range(n):
        assert j in segs[j], j          # the point box at its v0
        assert j in segs[n + j], j      # the box around it (step 2)
    assert len(segs[2 * n]) == 0
    pairs, accepted, wrong, band, size = against_f64(coords, lo, hi)
    print(f"degenerate triangles: {pairs} step-1 pairs, {accepted} accepted, {wrong} disagreements, {band} in the band")
    assert wrong == 0 and accepted >= 2 * n and pairs > accepted  # (both verdicts occur beyond the 2 n built in)
