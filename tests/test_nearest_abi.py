"""The nearest-surface query's ABI (rt_nearest_points / rt_get_nearest_info, include/rt_hip.h) without a GPU: the
symbols are exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as
tests/test_hits_abi.py does), Renderer.nearest refuses a mistyped, misshapen, strided or host tensor before any device
call, and the yardstick of the GPU tests (tests/nearest_ref.py) agrees with an independent float64 brute force and
stays finite on degenerate triangles."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host
from tests import nearest_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")


def test_nearest_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_nearest_points", "rt_get_nearest_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_nearest_points, L.rt_get_nearest_info


def test_nearest_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_points": _lib.Points, "rt_nearest_results": _lib.NearestResults,
               "rt_nearest_info": _lib.NearestInfo}
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


def test_nearest_tensors_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called (a call would fail
    on the null context with another message)"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, dtype=torch.float32)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # host tensors
        r.nearest(ok)
    with pytest.raises(device.RtError, match="points: dtype"):
        r.nearest(ok.double())
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.nearest(torch.zeros(8, 4))
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.nearest(torch.zeros(24))
    with pytest.raises(device.RtError, match="contiguous"):
        r.nearest(torch.zeros(16, 3)[::2])
    with pytest.raises(device.RtError, match="torch tensor"):
        r.nearest([[0.0, 0.0, 0.0]])
    with pytest.raises(device.RtError, match=r"max_dist2: shape"):  # (checked before the points' device)
        r.nearest(ok, max_dist2=torch.zeros(8, 1))
    with pytest.raises(device.RtError, match=r"point: shape"):
        r.nearest(ok, point=torch.zeros(24))
    with pytest.raises(device.RtError, match="max_dist2: dtype"):
        r.nearest((1234, 8), max_dist2=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(device.RtError, match="max_dist2: 7 elements"):
        r.nearest((1234, 8), max_dist2=torch.zeros(7))
    with pytest.raises(device.RtError, match="max_dist2: expected a torch tensor"):
        r.nearest((1234, 8), max_dist2=[1.0] * 8)
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.nearest((1234, 8), tri=torch.zeros(8))
    with pytest.raises(device.RtError, match="d2: 7 elements"):
        r.nearest((1234, 8), d2=torch.zeros(7))
    with pytest.raises(device.RtError, match="point: 21 elements"):
        r.nearest((1234, 8), point=torch.zeros(7, 3))
    r._ctx = None  # (nothing to destroy)


# ------------------------------------------------------------------ the yardstick against float64
def _dist_f64(p, c):
    """plain Ericson 5.1.5 on the vertices v0, v1, v2 in float64: the distance of point p [3] to every triangle of
    c [m, 3, 3]"""
    a, b, cc = c[:, 0], c[:, 1], c[:, 2]
    ab, ac, ap = b - a, cc - a, p - a
    dot = lambda u, v: (u * v).sum(-1)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - cc
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    x, y = d4 - d3, d5 - d6
    with np.errstate(all="ignore"):
        den = 1.0 / (va + vb + vc)
        cands = [a, b, a + ab * (d1 / (d1 - d3))[:, None], cc, a + ac * (d2 / (d2 - d6))[:, None],
                 b + (cc - b) * (x / (x + y))[:, None]]
        inner = a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (x >= 0) & (y >= 0)]
    q = np.select([k[:, None] for k in conds], cands, inner)
    return np.linalg.norm(p - q, axis=1)


def fixed_points(coords, n=64, seed=5):
    """n fixed points in the scene's box grown by a quarter"""
    rng = np.random.default_rng(seed)
    lo, hi = coords.reshape(-1, 3).min(0).astype(np.float64), coords.reshape(-1, 3).max(0).astype(np.float64)
    g = (hi - lo) / 4
    return (rng.random((n, 3)) * (hi - lo + 2 * g) + (lo - g)).astype(np.float32)


# the worst |sqrt(D32) - dist64| over car_only's triangles and fixed_points' 64 points, as measured
MEASURED_WORST = 1.361e-6


def test_the_yardstick_agrees_with_float64_brute_force():
    coords = host.Scene.named("car_only").triangles["coords"]
    pts = fixed_points(coords)
    c64 = coords.astype(np.float64)
    worst = 0.0
    for i in range(0, len(pts), 16):
        D, _ = nearest_ref.dist(pts[i:i + 16], coords)
        assert D.dtype == np.float32 and np.isfinite(D).all()
        for r in range(D.shape[0]):
            p = pts[i + r].astype(np.float64)
            ref = _dist_f64(p, c64)
            worst = max(worst, float(np.abs(np.sqrt(D[r].astype(np.float64)) - ref).max()))
    print(f"worst |sqrt(D32) - dist64| = {worst:.3e}")
    assert worst <= 4 * MEASURED_WORST, worst


def degenerate_triangles():
    """three equal vertices, two equal vertices (each pair), three collinear vertices (each middle one)"""
    a, b, c = [1.0, 2.0, 3.0], [2.5, 2.0, 3.5], [4.0, 2.0, 4.0]  # (collinear: b = (a + c) / 2)
    return np.array([[a, a, a], [a, a, b], [a, b, a], [b, a, a], [a, b, c], [b, a, c], [a, c, b],
                     [[0.1, 0.2, 0.3], [0.3, 0.6, 0.9], [0.7, 1.4, 2.1]]], np.float32)


def test_the_yardstick_is_finite_on_degenerate_triangles():
    coords = degenerate_triangles()
    rng = np.random.default_rng(9)
    pts = np.concatenate([rng.uniform(-2, 6, (64, 3)), coords.reshape(-1, 3), coords.mean(1)]).astype(np.float32)
    D, P = nearest_ref.dist(pts, coords)
    assert np.isfinite(D).all() and np.isfinite(P).all() and (D >= 0).all()
    b1 = coords[:, 0] + (coords[:, 1] - coords[:, 0])
    b2 = coords[:, 0] + (coords[:, 2] - coords[:, 0])
    lo = np.minimum(np.minimum(coords[:, 0], b1), b2)
    hi = np.maximum(np.maximum(coords[:, 0], b1), b2)
    assert (P >= lo[None]).all() and (P <= hi[None]).all()
    tri, d2, point = nearest_ref.expected(pts, coords)
    assert (tri >= 0).all() and np.isfinite(d2).all() and np.isfinite(point).all()
    v = coords[:7].reshape(-1, 3)  # (vertices whose a + (v - a) is exact)
    on = nearest_ref.expected(v, coords)
    assert (on[1] == 0).all() and nearest_ref.same_bits(on[2], v)  # a vertex is at distance 0
