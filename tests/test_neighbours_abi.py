"""The neighbour query's ABI (rt_nearest_tris / rt_get_neighbours_info, include/rt_hip.h) without a GPU: the symbols
are exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as
tests/test_nearest_abi.py does), Renderer.nearest_tris refuses bad arguments before any device call, and the yardstick
of the GPU tests (tests/neighbours_ref.py) equals tests/nearest_ref.py at k = 1, counts what a plain comparison counts,
and has the order statistics of an independent float64 brute force."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host
from tests import nearest_ref, neighbours_ref
from tests.nearest_ref import same_bits
from tests.test_nearest_abi import _dist_f64, fixed_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")
FMAX = np.float32(3.402823466e+38)


def test_neighbours_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_nearest_tris", "rt_get_neighbours_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_nearest_tris, L.rt_get_neighbours_info


def test_neighbours_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_neighbours": _lib.Neighbours, "rt_neighbour_results": _lib.NeighbourResults,
               "rt_neighbours_info": _lib.NeighboursInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {",
             'printf("RT_NEIGHBOURS_MAX %d\\n", RT_NEIGHBOURS_MAX);']
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
    assert int(got["RT_NEIGHBOURS_MAX"]) == _lib.NEIGHBOURS_MAX == 16
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_neighbours_arguments_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, dtype=torch.float32)
    for k in (-1, 17, 2.0, True, None):
        with pytest.raises(device.RtError, match="k: "):
            r.nearest_tris(ok, k=k)
    with pytest.raises(device.RtError, match="needs count_all"):
        r.nearest_tris(ok, k=0)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # host tensors
        r.nearest_tris(ok)
    with pytest.raises(device.RtError, match="points: dtype"):
        r.nearest_tris(ok.double())
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.nearest_tris(torch.zeros(8, 4))
    with pytest.raises(device.RtError, match="contiguous"):
        r.nearest_tris(torch.zeros(16, 3)[::2])
    with pytest.raises(device.RtError, match="torch tensor"):
        r.nearest_tris([[0.0, 0.0, 0.0]])
    with pytest.raises(device.RtError, match=r"max_dist2: shape"):
        r.nearest_tris(ok, max_dist2=torch.zeros(8, 1))
    with pytest.raises(device.RtError, match=r"point: shape"):
        r.nearest_tris(ok, k=4, point=torch.zeros(8, 3, 4))
    with pytest.raises(device.RtError, match="max_dist2: dtype"):
        r.nearest_tris((1234, 8), max_dist2=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(device.RtError, match="max_dist2: 7 elements"):
        r.nearest_tris((1234, 8), max_dist2=torch.zeros(7))
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.nearest_tris((1234, 8), k=4, tri=torch.zeros(32))
    with pytest.raises(device.RtError, match="d2: 31 elements"):
        r.nearest_tris((1234, 8), k=4, d2=torch.zeros(31))
    with pytest.raises(device.RtError, match="count: 7 elements"):
        r.nearest_tris((1234, 8), k=4, count=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(device.RtError, match="point: 84 elements"):
        r.nearest_tris((1234, 8), k=4, point=torch.zeros(7, 4, 3))
    r._ctx = None  # (nothing to destroy)


# ------------------------------------------------------------------ the yardstick
@pytest.fixture(scope="module")
def car():
    coords = host.Scene.named("car_only").triangles["coords"]
    return coords, fixed_points(coords)


def mixed_bounds(n, d2):
    """every kind of bound: none, the nearest D itself, just below it, 0, negative, NaN, -0.0, a radius"""
    k = np.arange(n) % 8
    return np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6],
                     [np.float32(np.inf), d2, np.nextafter(d2, np.float32(-np.inf)), np.float32(0), np.float32(-1.0),
                      np.float32(np.nan), np.float32(-0.0)], np.float32(0.05)).astype(np.float32)


def test_k1_equals_the_nearest_yardstick(car):
    coords, pts = car
    pts = np.concatenate([pts, coords[::97, 1], [[np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0]]]).astype(np.float32)
    base = nearest_ref.expected(pts, coords)
    for md in (None, mixed_bounds(len(pts), base[1])):
        want = nearest_ref.expected(pts, coords, md)
        tri, d2, point, count = neighbours_ref.expected(pts, coords, 1, md)
        assert np.array_equal(tri[:, 0], want[0]) and same_bits(d2[:, 0], want[1]) and same_bits(point[:, 0], want[2])
        assert np.array_equal(count, (want[0] >= 0).astype(np.int32))
    assert (want[0] >= 0).sum() > 10 and (want[0] < 0).sum() > 10


def test_count_all_is_a_plain_comparison(car):
    coords, pts = car
    D, _ = nearest_ref.dist(pts, coords)
    near = D.min(axis=1)  # bounds around each point's own nearest D: 4 x, the D itself, just below it, 1.5 x
    j = np.arange(len(pts)) % 4
    md = np.select([j == 0, j == 1, j == 2], [near * np.float32(4), near, np.nextafter(near, np.float32(-np.inf))],
                   near * np.float32(1.5)).astype(np.float32)
    plain = (D <= md[:, None]).sum(axis=1)
    assert (plain > 16).sum() >= 5 and (plain[j == 2] == 0).all() and (plain[j == 1] >= 1).all()
    for k in (0, 4, 16):
        tri, d2, point, count, size, cut = neighbours_ref.expected(pts, coords, k, md, count_all=True, stats=True)
        assert np.array_equal(count, plain) and np.array_equal(size, plain)
        capped = neighbours_ref.expected(pts, coords, k, md)[3]
        assert np.array_equal(capped, np.minimum(plain, k))
        assert np.array_equal((tri >= 0).sum(axis=1), np.minimum(plain, k))
        assert ((d2 == FMAX) == (tri < 0)).all() and same_bits(point[tri < 0], np.repeat(pts[:, None], k, 1)[tri < 0])
        assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()  # sorted by D


# the worst |sqrt(D32 of rank r) - the r-th smallest float64 distance|, r = 1..16, over car_only's triangles and
# test_nearest_abi.fixed_points' 64 points, as measured
MEASURED_WORST_RANKED = 2.877e-7


def test_the_order_statistics_agree_with_float64_brute_force(car):
    """sqrt(D) of the yardstick's rank-r entry against the r-th smallest distance of an independent float64 brute force
    (plain Ericson on the vertices), r = 1..16, on test_nearest_abi.py's own 64 points of car_only. Measured worst
    difference: MEASURED_WORST_RANKED; asserted at four times it -- the margin test_nearest_abi.py takes, for the
    same reason: another numpy or libm, fixed inputs."""
    coords, pts = car
    c64 = coords.astype(np.float64)
    tri, d2, point, count = neighbours_ref.expected(pts, coords, 16)
    assert (count == 16).all() and (tri >= 0).all()
    worst = 0.0
    for i in range(len(pts)):
        ref = np.sort(_dist_f64(pts[i].astype(np.float64), c64))[:16]
        worst = max(worst, float(np.abs(np.sqrt(d2[i].astype(np.float64)) - ref).max()))
    print(f"worst |sqrt(D32 rank r) - dist64 rank r|, r = 1..16: {worst:.3e}")
    assert worst <= 4 * MEASURED_WORST_RANKED, worst
