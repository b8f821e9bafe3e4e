"""The wide BVH's refit on the CPU (rth_wbvh_refit, host.wbvh_refit) and the quantiser it shares with the device refit
(csrc/hip/rt_quant.hpp): with unmoved triangles the refit reproduces the collapse's words bit for bit; after a rigid
move of half the triangles, and after a far move that also shrinks some of them to points' size, every decoded child
box contains its whole subtree's inflated vertices, every topology word is what it was and every triangle is reached
exactly once. The quantiser alone runs over random and adversarial box sets under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

from prt import host
from tests.test_host import _wbvh_subtree_tris

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inflation(coords):
    """the library's: 2^-16 of max(16, max |coordinate|) (rt_upload_scene)"""
    return float(np.ldexp(np.float32(max(np.float32(16.0), np.abs(coords).max())), -16))


def regrow(nodes, tri_idx, coords):
    """the reference tree with the same child / tr_len / tri_idx and every box regrown as bvh.c grows it: min / max
    over the node's triangles' vertices from +-1e10 (children follow their parent in the reference layout)"""
    out = nodes.copy()
    c = np.asarray(coords, np.float32)
    tlo, thi = c.min(1), c.max(1)
    seed_lo, seed_hi = np.full(3, 1e10, np.float32), np.full(3, -1e10, np.float32)
    for i in range(len(out) - 1, -1, -1):
        ln, ch = int(out["tr_len"][i]), int(out["child"][i])
        if ln > 0:
            t = tri_idx[ch:ch + ln]
            out["min"][i] = np.minimum(seed_lo, tlo[t].min(0))
            out["max"][i] = np.maximum(seed_hi, thi[t].max(0))
        elif ch != 0:
            assert ch > i
            out["min"][i] = np.minimum(out["min"][ch], out["min"][ch + 1])
            out["max"][i] = np.maximum(out["max"][ch], out["max"][ch + 1])
        else:
            out["min"][i], out["max"][i] = seed_lo, seed_hi
    return out


def test_regrown_boxes_of_unmoved_triangles_are_the_builders():
    """the premise of a vertex update's S' (rt_hip.h): bvh.c's node boxes are pure folds of the vertices from +-1e10,
    so regrowing them over the kept topology changes no bit of bvh_build's output"""
    for s in (host.Scene.named("car_only").build_bvh(3), host.Scene.random(2000).build_bvh(3)):
        again = regrow(s.nodes, s.tri_idx, s.triangles["coords"])
        assert again.tobytes() == s.nodes.tobytes()


@pytest.fixture(scope="module")
def trees():
    """(scene, words, order, inflate) for car_only, car_boxed and Scene.random(2000), reference-layout (h3) and
    binned-SAH trees"""
    out = {}
    for name, make in (("car_only", lambda: host.Scene.named("car_only")), ("car_boxed", lambda: host.Scene.named("car_boxed")),
                       ("random2000", lambda: host.Scene.random(2000))):
        for heur in (3, "binned_sah"):
            s = make().build_bvh(heur)
            infl = inflation(s.triangles["coords"])
            words, order, _ = host.wbvh_build(s.nodes, s.tri_idx, s.triangles, infl)
            words.setflags(write=False)
            out[f"{name}-{heur}"] = (s, words, order, infl)
    return out


KEYS = ["car_only-3", "car_only-binned_sah", "car_boxed-3", "car_boxed-binned_sah", "random2000-3",
        "random2000-binned_sah"]


def moved_half(tris, far=False):
    """S': the triangles with centroid x above the median moved rigidly -- a rotation about z and a translation; far:
    50 units away instead, and every tenth of them scaled by 1e-3 about its first vertex (other exponents, and axes of
    zero extent once the float rounding swallows the scaled edges)"""
    c = tris["coords"].astype(np.float64)
    sel = np.nonzero(tris["centroid"][:, 0] > np.median(tris["centroid"][:, 0]))[0]
    assert 0 < len(sel) < len(tris)
    a = 0.3
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    m = c[sel] @ R.T + (np.array([50.0, -50.0, 50.0]) if far else np.array([0.7, -0.4, 0.25]))
    if far:
        small = np.arange(0, len(sel), 10)
        m[small] = m[small, :1] + (m[small] - m[small, :1]) * 1e-3
    c[sel] = m
    c = c.astype(np.float32)
    return host.triangle_init(c, tris["ks"], tris["kd"], tris["kr"]), sel


def check_refit(words0, order, tris1, infl):
    words1 = host.wbvh_refit(words0, order, tris1, infl)
    # every topology word: imask, child_base, tri_base, meta
    np.testing.assert_array_equal(words1[:, 3] >> 24, words0[:, 3] >> 24)
    np.testing.assert_array_equal(words1[:, 4:8], words0[:, 4:8])
    D = host.wbvh_decode(words1)
    v = tris1["coords"]
    tlo, thi = v.min(1) - np.float32(infl), v.max(1) + np.float32(infl)  # (float32, as the refit grows them)
    n = len(tris1)
    seen_tri = np.zeros(n, int)
    seen_node = np.zeros(len(words1), int)
    memo = {}
    stack = [0]
    while stack:
        k = stack.pop()
        seen_node[k] += 1
        internal = [s for s in range(8) if (D["imask"][k] >> s) & 1]
        for s in range(8):
            m = int(D["meta"][k, s])
            if s in internal:
                c = int(D["child_base"][k]) + sum(1 for j in internal if j < s)
                stack.append(c)
                sub = _wbvh_subtree_tris(D, c, order, memo)
            elif m:
                cnt, off = m >> 5, m & 31
                sub = order[int(D["tri_base"][k]) + off: int(D["tri_base"][k]) + off + cnt]
                seen_tri[sub] += 1
            else:
                assert (D["qlo"][k, :, s] == 255).all() and (D["qhi"][k, :, s] == 0).all()  # still an inverted box
                continue
            assert (D["lo"][k, s] <= tlo[sub]).all() and (D["hi"][k, s] >= thi[sub]).all(), (k, s)
    assert (seen_node == 1).all() and (seen_tri == 1).all()
    return words1


@pytest.mark.parametrize("key", KEYS)
def test_refit_of_unmoved_triangles_reproduces_the_build(trees, key):
    s, words, order, infl = trees[key]
    again = host.wbvh_refit(words, order, s.triangles, infl)
    assert again.dtype == np.uint32 and again.shape == words.shape
    np.testing.assert_array_equal(again, words)
    np.testing.assert_array_equal(host.wbvh_refit(words, order, s.triangles, 0.0),
                                  host.wbvh_build(s.nodes, s.tri_idx, s.triangles, 0.0)[0])


@pytest.mark.parametrize("key", KEYS)
def test_refit_after_a_rigid_move(trees, key):
    s, words, order, _ = trees[key]
    tris1, sel = moved_half(s.triangles)
    assert not np.array_equal(tris1["coords"][sel], s.triangles["coords"][sel])
    w1 = check_refit(words, order, tris1, inflation(tris1["coords"]))
    assert not np.array_equal(w1, words)


@pytest.mark.parametrize("key", KEYS)
def test_refit_after_a_far_move_with_shrunk_triangles(trees, key):
    s, words, order, infl0 = trees[key]
    tris1, sel = moved_half(s.triangles, far=True)
    infl1 = inflation(tris1["coords"])
    assert infl1 > infl0  # the magnitude, hence the inflation, changed
    w1 = check_refit(words, order, tris1, infl1)
    e0 = (words[:, 3] & 0xFFFFFF)
    assert (w1[:, 3] & 0xFFFFFF != e0).any()  # other exponents
    ext = tris1["coords"][sel[::10]].max(1) - tris1["coords"][sel[::10]].min(1)
    if key.startswith("car_only"):  # (its small triangles; the random scene's unit-sized ones keep some extent)
        assert (ext == 0).any()  # zero-extent axes among the shrunk triangles
    # and back: the original coordinates give the original words again
    np.testing.assert_array_equal(host.wbvh_refit(w1, order, s.triangles, infl0), words)


def test_refit_refuses_bad_arguments(trees):
    s, words, order, infl = trees["random2000-binned_sah"]
    with pytest.raises(RuntimeError):
        host.wbvh_refit(words, order, s.triangles, -1.0)
    bad = order.copy()
    bad[0] = len(order)
    with pytest.raises(RuntimeError):
        host.wbvh_refit(words, bad, s.triangles, infl)


def test_triangle_init_equals_the_loaders_triangles():
    t = host.Scene.named("car_only").triangles
    again = host.triangle_init(t["coords"], t["ks"], t["kd"], t["kr"])
    assert again.tobytes() == t.tobytes()


def test_shared_quantiser_under_sanitizers(tmp_path):
    exe = tmp_path / "refit_quant_test"
    src = os.path.join(ROOT, "tests", "c", "refit_quant_test.cpp")
    inc = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", inc, "-o", str(exe), src],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refit_quant: ok" in r.stdout
