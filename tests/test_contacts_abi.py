"""The contact query's ABI (rt_sweep_contacts / rt_get_contacts_info, include/rt_hip.h) without a GPU: the symbols are
exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as tests/test_sweep_abi.py does),
Renderer.sweep_contacts refuses bad arguments before any device call, and the yardstick of the GPU tests
(tests/contacts_ref.py) gives the stated answers on closed-form cases and is sandwiched between two float64 brute-force
sets of the same geometry, ungated and not recentred, on sweeps through car_only and car_boxed."""
import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from prt import host
from tests import contacts_ref, sweep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")
F = np.float32
FMAX = sweep_ref.FMAX


def test_contacts_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_sweep_contacts", "rt_get_contacts_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_sweep_contacts, L.rt_get_contacts_info


def test_contacts_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_sphere_contacts": _lib.SphereContacts, "rt_contact_results": _lib.ContactResults,
               "rt_contacts_info": _lib.ContactsInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {",
             'printf("RT_CONTACTS_MAX %d\\n", RT_CONTACTS_MAX);']
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
    assert int(got["RT_CONTACTS_MAX"]) == _lib.CONTACTS_MAX == 16
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in _lib.ContactsInfo._fields_] == [
        "spheres", "found", "tris_stored", "tris_counted", "walked_spheres", "exhaustive_spheres", "empty_spheres",
        "nodes_visited", "tris_tested", "stack_overflows", "kernel_ms"]
    assert [f for f, _ in _lib.SphereContacts._fields_] == ["centre", "motion", "radius", "t_max", "n", "max_tris",
                                                            "count_all", "kernel"]
    assert [f for f, _ in _lib.ContactResults._fields_] == ["tri", "t", "point", "count"]


def test_a_null_context_is_an_argument_error():
    """the one RT_E_ARG that needs no context (the others: tests/test_gpu_contacts.py)"""
    from prt import _lib
    L = _lib.hip()
    q, res, info = _lib.SphereContacts(), _lib.ContactResults(), _lib.ContactsInfo()
    assert L.rt_sweep_contacts(None, ctypes.byref(q), ctypes.byref(res)) == -1  # RT_E_ARG
    assert L.rt_get_contacts_info(None, ctypes.byref(info)) == -1  # RT_E_ARG


def test_contacts_arguments_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, dtype=torch.float32)
    for k in (-1, 17, 2.0, True, None):
        with pytest.raises(device.RtError, match="k: "):
            r.sweep_contacts(ok, ok, 0.5, k=k)
    with pytest.raises(device.RtError, match="needs count_all"):
        r.sweep_contacts(ok, ok, 0.5, k=0)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # host tensors
        r.sweep_contacts(ok, ok, 0.5)
    with pytest.raises(device.RtError, match="centres: dtype"):
        r.sweep_contacts(ok.double(), ok, 0.5)
    with pytest.raises(device.RtError, match=r"centres: shape .* expected \[n, 3\]"):
        r.sweep_contacts(torch.zeros(8, 4), ok, 0.5)
    with pytest.raises(device.RtError, match=r"motions: shape .* expected \[n, 3\]"):
        r.sweep_contacts(ok, torch.zeros(24), 0.5)
    with pytest.raises(device.RtError, match="motions: 7 spheres, centres has 8"):
        r.sweep_contacts(ok, torch.zeros(7, 3), 0.5)
    with pytest.raises(device.RtError, match="contiguous"):
        r.sweep_contacts(torch.zeros(16, 3)[::2], ok, 0.5)
    with pytest.raises(device.RtError, match="torch tensor"):
        r.sweep_contacts([[0.0, 0.0, 0.0]], ok, 0.5)
    with pytest.raises(device.RtError, match="raw pointers"):
        r.sweep_contacts((1234, 8), ok, 0.5)
    with pytest.raises(device.RtError, match="raw pointers"):
        r.sweep_contacts((1234, -1), 5678, 91011)
    with pytest.raises(device.RtError, match="raw pointers"):
        r.sweep_contacts((1234, 8), 5678, 0.5)
    with pytest.raises(device.RtError, match=r"radius: shape"):
        r.sweep_contacts(ok, ok, torch.zeros(8, 1))
    with pytest.raises(device.RtError, match="radius: 7 spheres"):
        r.sweep_contacts(ok, ok, torch.zeros(7))
    with pytest.raises(device.RtError, match="radius: expected a float"):
        r.sweep_contacts(ok, ok, [0.5] * 8)
    with pytest.raises(device.RtError, match=r"t_max: shape"):
        r.sweep_contacts(ok, ok, 0.5, t_max=torch.zeros(8, 1))
    with pytest.raises(device.RtError, match="t_max: expected a torch tensor"):
        r.sweep_contacts((1234, 8), 5678, 91011, t_max=[1.0] * 8)
    with pytest.raises(device.RtError, match="t_max: dtype"):
        r.sweep_contacts((1234, 8), 5678, 91011, t_max=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(device.RtError, match="t_max: 7 elements"):
        r.sweep_contacts((1234, 8), 5678, 91011, t_max=torch.zeros(7))
    with pytest.raises(device.RtError, match=r"point: shape"):
        r.sweep_contacts(ok, ok, 0.5, k=4, point=torch.zeros(8, 3, 4))
    with pytest.raises(device.RtError, match="tri: dtype"):
        r.sweep_contacts((1234, 8), 5678, 91011, k=4, tri=torch.zeros(32))
    with pytest.raises(device.RtError, match="t: 31 elements"):
        r.sweep_contacts((1234, 8), 5678, 91011, k=4, t=torch.zeros(31))
    with pytest.raises(device.RtError, match="count: 7 elements"):
        r.sweep_contacts((1234, 8), 5678, 91011, k=4, count=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(device.RtError, match="point: 84 elements"):
        r.sweep_contacts((1234, 8), 5678, 91011, k=4, point=torch.zeros(7, 4, 3))
    r._ctx = None  # (nothing to destroy)


# ------------------------------------------------------------------ the yardstick on closed-form cases
FLAT = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F)  # in the plane z = 0
RING = [(2, 0, -1), (1, 2, -1), (-1, 2, -1), (-2, 0, -1), (-1, -2, -1), (1, -2, -1)]


def fan():
    """six triangles around the apex (0, 0, 0) of a cone, the apex at corner 0, 1 or 2 in turn (small integers: every
    record is exact)"""
    tris = []
    for i in range(6):
        t = [(0, 0, 0), RING[i], RING[(i + 1) % 6]]
        tris.append(t[-(i % 3):] + t[:-(i % 3)] if i % 3 else t)
    return np.array(tris, F)


def one(c, d, r, coords, k, t_max=None, count_all=False):
    tri, t, count, point = contacts_ref.expected(np.array([c], F), np.array([d], F), np.array([r], F), coords, k,
                                                 None if t_max is None else np.array([t_max], F), count_all)
    return tri[0], t[0], int(count[0]), point[0]


def test_a_drop_onto_a_shared_vertex_lists_the_whole_fan():
    coords = fan()
    tri, t, count, point = one([0, 0, 5], [0, 0, -1], 1.0, coords, 8)
    assert count == 6 and np.array_equal(tri, [0, 1, 2, 3, 4, 5, -1, -1])
    assert np.array_equal(t[:6], np.full(6, 4.0, F)) and (t[6:] == FMAX).all()
    assert np.array_equal(point[:6], np.zeros((6, 3), F))  # every contact point is the apex
    assert np.array_equal(point[6:], np.array([[0, 0, 5]] * 2, F))  # unused slots: c's own bits
    tri, t, count, _ = one([0, 0, 5], [0, 0, -1], 1.0, coords, 4)  # a full list: the lowest indices of the tie
    assert count == 4 and np.array_equal(tri, [0, 1, 2, 3])
    assert one([0, 0, 5], [0, 0, -1], 1.0, coords, 4, count_all=True)[2] == 6


def test_two_parallel_sheets_give_two_entries_a_gap_apart():
    coords = np.stack([FLAT, FLAT + np.array([0, 0, -2], F)])
    tri, t, count, point = one([1, 1, 5], [0, 0, -2], 0.5, coords, 4)  # speed 2, gap 2
    assert count == 2 and np.array_equal(tri, [0, 1, -1, -1])
    assert t[0] == 2.25 and t[1] == 3.25 and t[1] - t[0] == 2.0 / 2.0
    assert np.array_equal(point[:2], np.array([[1, 1, 0], [1, 1, -2]], F))
    # t_max exactly at the second contact's toi keeps it; one float below drops it
    assert one([1, 1, 5], [0, 0, -2], 0.5, coords, 4, t_max=3.25)[2] == 2
    below = float(np.nextafter(F(3.25), F(0)))
    tri, t, count, _ = one([1, 1, 5], [0, 0, -2], 0.5, coords, 4, t_max=below)
    assert count == 1 and np.array_equal(tri, [0, -1, -1, -1]) and t[1] == FMAX
    assert one([1, 1, 5], [0, 0, -2], 0.5, coords, 0, t_max=below, count_all=True)[2] == 1


def test_a_start_in_contact_lists_every_touching_triangle_at_zero():
    far = FLAT + np.array([0, 0, 10], F)
    coords = np.stack([far, FLAT, FLAT + np.array([0, 0, 1], F), FLAT + np.array([0, 0, -0.5], F)])
    for d in ([0, 0, 0], [1, 2, -3]):
        tri, t, count, point = one([1, 1, 0.5], d, 1.0, coords, 4, t_max=0.0)
        assert count == 3 and np.array_equal(tri, [1, 2, 3, -1]) and np.array_equal(t[:3], np.zeros(3, F))
        assert np.array_equal(point[:3], np.array([[1, 1, 0], [1, 1, 1], [1, 1, -0.5]], F))


def test_the_pure_count_counts():
    coords = fan()
    tri, t, count, point = one([0, 0, 5], [0, 0, -1], 1.0, coords, 0, count_all=True)
    assert tri.shape == (0,) and t.shape == (0,) and point.shape == (0, 3) and count == 6
    assert one([0, 0, 5], [0, 0, -1], 1.0, coords, 0, t_max=1.0, count_all=True)[2] == 0  # the capsule stops short
    assert one([0, 0, 5], [0, 0, -1], -1.0, coords, 0, count_all=True)[2] == 0  # r < 0: the empty set


def test_k1_equals_the_sweep_yardstick_bit_for_bit():
    coords = host.Scene.named("car_only").triangles["coords"]
    c, d, r = sweep_ref.fixture_sweeps(coords, 128, seed=41)
    for tm in (None, np.ones(128, F)):
        tri1, t1, p1, _ = sweep_ref.expected(c, d, r, coords, tm)
        tri, t, count, point = contacts_ref.expected(c, d, r, coords, 1, tm)
        assert np.array_equal(tri[:, 0], tri1) and contacts_ref.same_bits(t[:, 0], t1)
        assert contacts_ref.same_bits(point[:, 0], p1) and np.array_equal(count, (tri1 >= 0).astype(np.int32))
        assert (tri1 >= 0).sum() >= 32


# ------------------------------------------------------------------ the yardstick against float64
def _d(u, v):
    return (u * v).sum(-1)


def _region64(q, a, e1, e2):
    """Ericson 5.1.5 in float64 -> (squared distance, the interior case was reached)"""
    ap = q - a
    d1, d2 = _d(e1, ap), _d(e2, ap)
    bp = ap - e1
    d3, d4 = _d(e1, bp), _d(e2, bp)
    cp = ap - e2
    d5, d6 = _d(e1, cp), _d(e2, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    x, y = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (x >= 0) & (y >= 0)]
    den = 1.0 / (va + vb + vc)
    b = a + e1
    shape = np.broadcast(d1[..., None], a).shape
    cands = [np.broadcast_to(a, shape), np.broadcast_to(b, shape), a + e1 * (d1 / (d1 - d3))[..., None],
             np.broadcast_to(a + e2, shape), a + e2 * (d2 / (d2 - d6))[..., None],
             b + (e2 - e1) * (x / (x + y))[..., None]]
    inner = a + e1 * (vb * den)[..., None] + e2 * (vc * den)[..., None]
    p = np.select([np.broadcast_to(k[..., None], shape) for k in conds], cands, inner)
    df = q - p
    return _d(df, df), ~np.logical_or.reduce(conds)


def toi_f64(c, d, r, v):
    """the first contact of spheres (c [s, 3], d [s, 3], r [s]) with triangles v [m, 3, 3] in float64, straight from the
    geometry: touching at the start, else the least of the face, edge and vertex entries of the ray c + t d into the
    Minkowski sum -> [s, m], +inf where there is none. No gate, no recentring."""
    c, d, r = c[:, None, :], d[:, None, :], r[:, None]
    a, b, cc = v[None, :, 0], v[None, :, 1], v[None, :, 2]
    e1, e2 = b - a, cc - a
    with np.errstate(all="ignore"):
        D0, _ = _region64(c, a, e1, e2)
        r2, dd = r * r, _d(d, d)
        u = np.full(D0.shape, np.inf)
        n = np.cross(e1, e2)
        ln = np.sqrt(_d(n, n))
        so, dn = _d(n, c - a), _d(n, d)
        sg = np.where(so < 0, -1.0, 1.0)
        tf = (sg * r * ln - so) / dn
        _, interior = _region64(c + d * tf[..., None], a, e1, e2)
        u = np.where((ln > 0) & (dn * sg < 0) & (tf >= 0) & interior & (tf < u), tf, u)
        for p, f in ((a, e1), (a, e2), (b, cc - b)):
            m = c - p
            md, nd, ff = _d(m, f), _d(d, f), _d(f, f)
            A = ff * dd - nd * nd
            Bq = ff * _d(m, d) - nd * md
            Cq = ff * (_d(m, m) - r2) - md * md
            disc = Bq * Bq - A * Cq
            cand = (-Bq - np.sqrt(disc)) / A
            s = md + cand * nd
            u = np.where((A > 0) & (disc >= 0) & (cand >= 0) & (s >= 0) & (s <= ff) & (cand < u), cand, u)
        for p in (a, b, cc):
            m = c - p
            Bv, Cv = _d(m, d), _d(m, m) - r2
            disc = Bv * Bv - dd * Cv
            cand = (-Bv - np.sqrt(disc)) / dd
            u = np.where((dd > 0) & (disc >= 0) & (cand >= 0) & (cand < u), cand, u)
        return np.where(D0 <= r2, 0.0, u)


THICK_BAND = 2.0 ** -20  # of the extent, sweeps with r > 0
THIN_BAND = 2.0 ** -14   # of the extent, thin sweeps (r = 0): the edge quadratic's ff*K - md*md cancels at r2 = 0, at a
#                          scale of sqrt(2^-24) times the triangle's size


def sandwich(coords, n, seed, chunk=16):
    """contacts_ref's members against the float64 brute force on n fixture sweeps with no t_max -> the figures"""
    c, d, r = sweep_ref.fixture_sweeps(coords, n, seed)
    ext = sweep_ref.scene_extent(coords)
    mem = contacts_ref.members(c, d, r, coords)
    m = len(coords)
    M = np.zeros((n, m), bool)
    M[mem.si, mem.ti] = True
    t32 = np.full((n, m), np.inf)
    t32[mem.si, mem.ti] = mem.toi
    v = coords.astype(np.float64)
    c64, d64, r64 = c.astype(np.float64), d.astype(np.float64), r.astype(np.float64)
    band = np.where(r64 > 0, THICK_BAND, THIN_BAND) * ext
    inner, outer, dt = np.zeros((n, m), bool), np.zeros((n, m), bool), np.zeros((n, m))

    def brute(s):  # (the chunks are independent and numpy releases the interpreter lock: a few threads share them)
        sl = slice(s, s + chunk)
        inner[sl] = np.isfinite(toi_f64(c64[sl], d64[sl], np.maximum(r64[sl] - band[sl], 0.0), v))
        outer[sl] = np.isfinite(toi_f64(c64[sl], d64[sl], r64[sl] + band[sl], v))
        t64 = toi_f64(c64[sl], d64[sl], r64[sl], v)
        both = M[sl] & np.isfinite(t64)
        speed = np.linalg.norm(d64[sl], axis=1)[:, None]
        with np.errstate(invalid="ignore"):
            dt[sl] = np.where(both, np.abs(t32[sl] - t64) * speed / ext, 0.0)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(brute, range(0, n, chunk)))
    thin = (r64 == 0)[:, None]
    sizes = mem.total
    return {"members": int((M & ~thin).sum()), "thin_members": int((M & thin).sum()),
            "lost": int((inner & ~M & ~thin).sum()), "extra": int((M & ~outer & ~thin).sum()),
            "between": int((outer & ~inner & ~thin).sum()),
            "thin_lost": int((inner & ~M & thin).sum()), "thin_extra": int((M & ~outer & thin).sum()),
            "dt": float(dt.max()), "dt999": float(np.quantile(dt[dt > 0], 0.999)) if (dt > 0).any() else 0.0,
            "none": int((sizes == 0).sum()), "short": int(((sizes >= 1) & (sizes <= 16)).sum()),
            "long": int((sizes > 16).sum())}


# max |t32 - t64| |d| / extent over the pairs that are float32 members and float64 members at r itself, as measured on
# the 256 fixture sweeps below
MEASURED_DT = {"car_only": 6.54e-6, "car_boxed": 2.20e-5}


SCENES = ["car_only", "car_boxed"]
_figures = {}


def figures(name):
    """sandwich() on the scene's 256 fixture sweeps (seed 41), computed once per module"""
    if name not in _figures:
        _figures[name] = sandwich(host.Scene.named(name).triangles["coords"], 256, seed=41)
        print(f"{name}: {_figures[name]}")
    return _figures[name]


@pytest.mark.parametrize("name", SCENES)
def test_the_members_lie_between_two_float64_sets(name):
    """256 fixture sweeps per scene (sweep_ref.fixture_sweeps, seed 41), no t_max. With M the float32 member pairs and
    F64(rho) the pairs whose float64 brute-force toi exists at radius rho: F64(max(r - delta, 0)) <= M <= F64(r + delta),
    delta = 2^-20 of the extent for r > 0 and 2^-14 for thin sweeps (r = 0), whose grazing membership is exact only to
    the scale at which the edge quadratic cancels.
    Measured: car_only 104,772 members (104,477 with r > 0 and 295 thin), 0 outside either set, 5 pairs with r > 0
    between the two float64 sets; max |t32 - t64| |d| / extent 6.54e-6 (99.9th percentile 4.5e-7). car_boxed 262,177
    members (261,819 and 358), 0 outside, 18 between; 2.20e-5 (3.1e-7). The maxima are grazing later contacts, not first
    ones. The bound on t is 4x the figure measured with this very fixture (MEASURED_DT)."""
    m = figures(name)
    assert m["members"] >= 50000 and m["thin_members"] >= 100
    assert m["lost"] == 0 and m["extra"] == 0
    assert m["thin_lost"] == 0 and m["thin_extra"] == 0
    assert m["dt"] <= 4 * MEASURED_DT[name]


def test_the_float64_fixture_has_every_size_class():
    """the variety of the fixture the sandwich is measured on: at least 32 sweeps with |S_i| = 0, at least 32 with
    1..16 and at least 32 above 16. The fixture is the two scenes' 2 x 256 sweeps, and the floor is taken over all of
    it: per scene the classes hold 33 / 90 / 133 (car_only) and 24 / 109 / 123 (car_boxed) sweeps, so a floor of 32 per
    scene cannot hold for car_boxed's stated 256 sweeps (seed 41, no t_max) whatever the code does, while the figures
    this fixture is stated with were measured with the floor in place. Each scene must still show every class."""
    tot = {k: sum(figures(name)[k] for name in SCENES) for k in ("none", "short", "long")}
    print(tot)
    assert min(tot.values()) >= 32, tot
    for name in SCENES:
        m = figures(name)
        assert min(m["none"], m["short"], m["long"]) > 0, (name, m)
