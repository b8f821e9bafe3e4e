"""The wide view's premise on scenes of other magnitudes (tests/variants.py), on the CPU: whatever the binary tree
(binned SAH, the reference's heuristic 3) and the collapse (the cost collapse, the greedy one), with the upload's own
inflation, the view holds every triangle once and every leaf slot's decoded box contains the RECORD box of each of its
triangles -- the box of a, fl(a + e1), fl(a + e2) that the query kernels' headers argue from, which can lie an ulp
outside the vertex box tests/test_host.py::_check_wbvh checks."""
import subprocess
import sys

import numpy as np
import pytest

from prt import host
from tests import overlap_ref, variants
from tests.test_host import _check_wbvh

TREES = ["binned_sah", 3]
BUILDERS = ["wbvh_build", "wbvh_build_greedy"]


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name, tree):
        if (name, tree) not in cache:
            cache[name, tree] = variants.scene(name, tree)
        return cache[name, tree]
    return get


def check_view(s, builder, monkeypatch):
    """wbvh_check, _check_wbvh and the record boxes for one scene and collapse -> the builder's info"""
    c = s.triangles["coords"]
    inflate = variants.inflation(c)
    build = getattr(host, builder)
    words, order, info = build(s.nodes, s.tri_idx, s.triangles, inflate)
    rc, cinfo = host.wbvh_check(words, order)
    assert rc == 0, (rc, info)
    assert cinfo["n_nodes"] == info["n_nodes"] == len(words) and cinfo["depth"] == info["depth"]
    assert info["n_nodes"] >= -(-len(c) // 32)  # a node holds at most 8 x 4 triangles
    plain = host.wbvh_build  # (_check_wbvh builds the view it checks with host.wbvh_build: hand it this collapse)
    monkeypatch.setattr(host, "wbvh_build", lambda n, i, t, f=0.0, _fn=None: plain(n, i, t, f, _fn="rth_" + builder))
    assert _check_wbvh(s, inflate)["n_nodes"] == info["n_nodes"]
    rec = overlap_ref.records(c)
    tlo, thi = rec[5], rec[6]
    assert np.isfinite(tlo).all() and np.isfinite(thi).all()
    D = host.wbvh_decode(words)
    seen = np.zeros(len(c), int)
    for k in range(len(words)):
        for slot in range(8):
            m = int(D["meta"][k, slot])
            if (int(D["imask"][k]) >> slot) & 1 or not m:
                continue
            at = int(D["tri_base"][k]) + (m & 31)
            sub = order[at:at + (m >> 5)]
            seen[sub] += 1
            lo, hi = D["lo"][k, slot], D["hi"][k, slot]
            assert np.isfinite(lo).all() and np.isfinite(hi).all(), (k, slot)
            assert (lo <= tlo[sub]).all() and (hi >= thi[sub]).all(), (k, slot, lo, hi, tlo[sub], thi[sub])
    assert (seen == 1).all()
    return info


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", variants.NAMES)
def test_views_hold_every_record_box(scenes, monkeypatch, name, tree, builder):
    info = check_view(scenes(name, tree), builder, monkeypatch)
    assert info["depth"] <= 16 and info["max_children"] <= 8  # the walks' stack bound
    if name in variants.MULTI:
        assert info["n_nodes"] > 34
    else:
        assert info["n_nodes"] == 1 and info["depth"] == 1  # few1, few2, few9: the root alone


@pytest.mark.parametrize("name", variants.MULTI)
def test_the_mirrors_find_what_the_variants_are_for(name):
    """the conditions on the mirrors' answers that tests/test_gpu_variants.py rests on, before any GPU run"""
    variants.check_figures(name)


@pytest.mark.parametrize("tree", TREES)
def test_the_cost_collapse_on_areas_beyond_float32(scenes, tree):
    """`beyond`: a box's area (1e40 and more) is no float32. A collapse that keeps its costs in float32 sees +inf
    everywhere, takes the root for one leaf slot of 1,088 triangles and returns RT_OK with n_nodes = 1, depth = 1 and no
    triangle reachable (wbvh_check: -105); the costs are kept on lengths divided by the power of two above the root's
    longest side, so the view is the one the scene's copy of unit size gets"""
    s = scenes("beyond", tree)
    inflate = variants.inflation(s.triangles["coords"])
    words, order, info = host.wbvh_build(s.nodes, s.tri_idx, s.triangles, inflate)
    print("beyond", tree, info)
    assert host.wbvh_check(words, order)[0] == 0
    assert info["n_nodes"] > 34 and info["depth"] > 1


@pytest.mark.parametrize("tree", TREES)
def test_the_cost_collapse_does_not_depend_on_a_power_of_two(scenes, tree):
    """topology and planes of `plain` scaled by 2^40 and by 2^-76 (sides of 1e-23, whose areas are no float32 either:
    they are 0) are `plain`'s: every length scales exactly; the inflation's floor of 16 is left out, inflate = 0"""
    s = scenes("plain", tree)
    t0 = s.triangles.copy()
    # (coordinates like sin(pi) = 1e-16 would be denormals at 2^-76, which a fast-math library loaded earlier in the
    # process flushes to zero: they are 0 here from the start)
    t0["coords"][np.abs(t0["coords"]) < 1e-6] = 0
    t0["centroid"][np.abs(t0["centroid"]) < 1e-6] = 0
    base = host.wbvh_build(s.nodes, s.tri_idx, t0, 0.0)
    for e in (40, -76):
        t = t0.copy()
        t["coords"] = np.ldexp(t["coords"], e)
        t["centroid"] = np.ldexp(t["centroid"], e)
        nodes = s.nodes.copy()
        nodes["min"], nodes["max"] = np.ldexp(nodes["min"], e), np.ldexp(nodes["max"], e)
        words, order, info = host.wbvh_build(nodes, s.tri_idx, t, 0.0)
        assert info == base[2] and np.array_equal(order, base[1]), e
        assert np.array_equal(words[:, 4:], base[0][:, 4:]), e  # child and triangle bases, meta bytes, planes
        assert np.array_equal(words[:, 3] >> 24, base[0][:, 3] >> 24), e  # the interior masks


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("tree", TREES)
def test_edge_of_the_coordinate_range(monkeypatch, tree, builder):
    """`edge`, M * 2e37 (max|coordinate| 3e37, above the stated limit RT_COORD_MAX = 2^123): a grid's origin, 1,024
    steps below the boxes, may be no float32 any more. The builders answer with a view that passes every check or with
    an error, never with RT_OK and planes that were not verified"""
    s = variants.scene("edge", tree)
    c = s.triangles["coords"]
    assert np.isfinite(c).all() and float(np.abs(c).max()) > 2.0 ** 123
    try:
        words, order, info = getattr(host, builder)(s.nodes, s.tri_idx, s.triangles, variants.inflation(c))
    except RuntimeError as e:
        print("edge", tree, builder, e)
        return
    print("edge", tree, builder, info)
    check_view(s, builder, monkeypatch)


def test_refit_reports_planes_that_do_not_fit():
    """the refit's quantiser is the builders': moved to coordinates at the float32 range's end it is an error"""
    s = variants.scene("plain", "binned_sah")
    words, order, _ = host.wbvh_build(s.nodes, s.tri_idx, s.triangles, variants.inflation(s.triangles["coords"]))
    t = variants.triangles(variants.mesh() * 2e38)
    assert np.isfinite(t["coords"]).all()
    with pytest.raises(RuntimeError):
        host.wbvh_refit(words, order, t, variants.inflation(t["coords"]))
    t = variants.triangles(variants.mesh() * 7e36)  # max|coordinate| 1.05e37, under RT_COORD_MAX
    assert float(np.abs(t["coords"]).max()) < 2.0 ** 123
    ok = host.wbvh_refit(words, order, t, variants.inflation(t["coords"]))
    assert host.wbvh_check(ok, order)[0] == 0


def test_binned_sah_refuses_a_non_finite_centroid():
    """the float32 mean of corners near 1e38 is +inf: the bin of such a centroid is (int)NaN, an index far outside the
    bins. In one child process, so that a crash is this test's failure and not the run's end"""
    code = ("import sys\n"
            f"sys.path[:0] = {[p for p in sys.path if p]!r}\n"
            "import numpy as np\n"
            "from prt import host\n"
            "from tests import variants\n"
            "for bad in ('inf', '-inf', 'nan'):\n"
            "    t = variants.triangles(variants.mesh())\n"
            "    t['centroid'][5::7, 1] = float(bad)\n"
            "    try:\n"
            "        host.bvh_build(t, 'binned_sah')\n"
            "    except RuntimeError as e:\n"
            "        print('refused', bad, e)\n"
            "    else:\n"
            "        raise SystemExit(3)\n"
            "t = variants.triangles(variants.mesh() * 2.2e38)\n"  # (the issue's case: the mean of corners near 1e38)
            "assert np.isfinite(t['coords']).all()\n"
            "t['centroid'] = t['coords'].sum(1, dtype=np.float32) / np.float32(3)\n"
            "assert np.isinf(t['centroid']).any()\n"
            "try:\n"
            "    host.bvh_build(t, 'binned_sah')\n"
            "except RuntimeError as e:\n"
            "    print('refused', 'mean', e)\n"
            "else:\n"
            "    raise SystemExit(4)\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.count("refused") == 4, (p.returncode, p.stdout, p.stderr[-400:])


def test_binned_sah_bins_an_overflowing_centroid_extent():
    """finite centroids whose extent is no float32 (3e38 apart): the bin scale is 0 and the offsets are +inf -- a valid
    tree all the same"""
    from tests.test_host import _check_tree
    t = variants.triangles(variants.mesh() * 1.6e38)
    assert np.isfinite(t["coords"]).all() and np.isfinite(t["centroid"]).all()
    nodes, idx, _ = host.bvh_build(t, "binned_sah")
    assert _check_tree(nodes, idx, t) <= 24
