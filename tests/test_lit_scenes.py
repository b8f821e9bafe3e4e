"""tests/lit_scenes.py is worth testing with: on the oracle and the host library alone (no GPU), the generator is
deterministic, both loaders read its files alike, and the oracle's 64x40 frames reach what tests/test_gpu_lights.py
relies on -- every material, every kind of light, paths to the last level, lit but not saturated frames, and a last
light whose loss would show. The conditions are fixed; the generator is what gets tuned."""
import hashlib

import numpy as np
import pytest

from prt import host
from tests import lit_scenes as ls

W, H = 64, 40
COUNTS = ls.LIGHT_COUNTS
# md5 of the .obj, .mtl and 40-light file of each form
MD5 = {"open": ("858f1e34f66ffac4d9b3a45afe070b96", "bab4c1b832a1970628f435d092e1d68f",
                "b3a3f75817eab97a4e876f291d16b007"),
       "hall": ("45e1182c5b00a113e47f676d4879c51a", "bab4c1b832a1970628f435d092e1d68f",
                "8c839b7abeb3d3975fc99a3c383ccbc2")}


@pytest.fixture(scope="module")
def lit(tmp_path_factory):
    return ls.Lit(tmp_path_factory.mktemp("lit"))


def differing(a, b):
    """pixels with any channel different"""
    return (a["rgb"].view(np.int32) != b["rgb"].view(np.int32)).any(-1)


def test_slots():
    """the docstring's slots: which light is of which kind, prefix-stable, the 8 / L scaling"""
    for form in ls.FORMS:
        a = ls.lights(40, form=form).astype(np.float64)
        for L in COUNTS:
            b = ls.lights(L, form=form).astype(np.float64)
            assert b.shape == (L, 6)
            np.testing.assert_array_equal(b[:, :3], a[:L, :3])
            if L:
                np.testing.assert_allclose(b[:, 3:] * L, a[:L, 3:] * 40, rtol=1e-6)
        pos, kl = a[:, :3], a[:, 3:]
        for j in range(40):
            special = j in (ls.IN_PLANE, ls.TWIN) or (j == ls.FAR and form == "open")
            if special:
                continue
            inside = abs(pos[j, 0]) <= 6 and -9 <= pos[j, 1] <= 7
            if j % 5 == 4:
                assert inside and -6 <= pos[j, 2] <= -3, j
            elif j % 5 == 0 and j >= 5:
                assert np.abs(pos[j]).max() <= 0.5, j
            else:
                assert inside and 3 <= pos[j, 2] <= 7.5, j
            assert (kl[j] > 0).all() or j == ls.BLACK
        for j in ls.ORDINARY_LAST:
            assert j % 5 not in (0, 4) and j not in (ls.BLACK, ls.IN_PLANE, ls.FAR, ls.TWIN)
        assert (kl[ls.BLACK] == 0).all()
        assert np.float32(pos[ls.IN_PLANE, 2]) == ls.FLOOR_Z and abs(pos[ls.IN_PLANE, 0]) < 7
        assert (pos[ls.TWIN] == pos[ls.TWIN - 1]).all()
    far = ls.lights(40, form="open")[ls.FAR].astype(np.float64)
    d2 = float((far[:3] ** 2).sum())
    assert d2 > 2.0 ** 40 and 2e6 < d2 ** 0.5 < 3e6
    assert abs(far[3:].max() * 40 / 8 - 1e13) < 1e7 and 2 * 1e13 * 8 < 2.0 ** 50  # (|cr| <= kd + ks < 2; L >= 1)
    assert len(ls.MATERIALS) >= 12


def test_generator_is_deterministic(lit, tmp_path):
    for form in ls.FORMS:
        a = lit.paths(form, 40)
        b = ls.write(tmp_path, form, 40)
        got = tuple(hashlib.md5(open(p, "rb").read()).hexdigest() for p in a)
        assert got == tuple(hashlib.md5(open(p, "rb").read()).hexdigest() for p in b)
        assert got == MD5[form], (form, got)


def test_both_loaders_read_the_same_scene(lit):
    for form in ls.FORMS:
        coords, mats = ls.triangles(form)
        assert len(coords) == (1088 if form == "open" else 1152)
        for L in COUNTS:
            o, s = lit.oracle(form, L), lit.scene(form, L)
            assert s.triangles.tobytes() == o.triangles_bytes(), (form, L)
            assert s.lights.tobytes() == o.lights_bytes(), (form, L)
            # and what was written is what was read, bit for bit
            assert np.array_equal(s.lights.view(np.float32).reshape(-1, 6).view(np.int32),
                                  ls.lights(L, form=form).view(np.int32))
        assert np.array_equal(s.triangles["coords"].view(np.int32), coords.view(np.int32))
        for k, col in (("kd", 1), ("ks", 2), ("kr", 3)):
            want = np.array([ls.MATERIALS[m][col] for m in mats], np.float32)
            assert np.array_equal(s.triangles[k], want), (form, k)


def test_frames_see_the_scene(lit):
    for form in ls.FORMS:
        _, mats = ls.triangles(form)
        f = lit.frame(form, 40, W, H)
        hit = f["hit"]
        assert (hit >= 0).mean() >= 0.95, form
        seen = set(mats[hit[hit >= 0]].tolist())
        assert seen == set(range(len(ls.MATERIALS))), (form, sorted(set(range(len(ls.MATERIALS))) - seen))
    f = lit.frame("hall", 40, W, H, bounces=8)
    assert f["counters"]["reflection"] >= 5 * W * H, f["counters"]


def test_frames_are_lit_and_not_saturated(lit):
    for form in ls.FORMS:
        for L in COUNTS:
            if L == 0:
                continue
            for bounces in ((4, 8) if form == "hall" else (4,)):
                f = lit.frame(form, L, W, H, bounces)
                c, rgb = f["counters"], f["rgb"]
                what = (form, L, bounces)
                assert c["shadow"] > 0 and c["shadow_skipped"] > 0, what
                clamped = float((rgb >= 1).mean())
                inside = float(((rgb > 0.02) & (rgb < 0.98)).mean())
                print(what, f"clamped {clamped:.3f} inside {inside:.3f}")
                assert 0.01 <= clamped <= 0.5, (what, clamped)
                assert inside >= 0.5, (what, inside)


def test_the_last_light_shows(lit):
    """L = 8 against 9 and 32 against 33 (as the issue states it: the kl scale differs too), and the stricter form:
    the L-light file without its last line, every other kl as it is"""
    for form in ls.FORMS:
        for L in (8, 9, 32, 33):
            full = lit.frame(form, L, W, H)
            cut = lit.frame(form, (f"{L}_cut", ls.lights(L, form=form)[:-1]), W, H)
            assert differing(full, cut).mean() >= 0.05, (form, L)
        for a, b in ((8, 9), (32, 33)):
            assert differing(lit.frame(form, a, W, H), lit.frame(form, b, W, H)).mean() >= 0.05, (form, a, b)


def test_the_edge_lights_show(lit):
    """removing the in-plane light alone, the far light alone (open) or one of the twins changes pixels; the black one
    changes none but is walked; the in-plane light's shadow rays are partly skipped and partly cast"""
    for form in ls.FORMS:
        for L in (7, 40):
            arr = ls.lights(L, form=form)
            full = lit.frame(form, L, W, H)

            def without(j):
                return lit.frame(form, (f"{L}_no{j}", np.delete(arr, j, axis=0)), W, H)

            assert differing(full, without(ls.IN_PLANE)).sum() >= 1, (form, L)
            if L == 7:
                continue
            assert differing(full, without(ls.TWIN)).sum() >= 1, form
            if form == "open":
                assert differing(full, without(ls.FAR)).sum() >= 1
            nb = without(ls.BLACK)
            assert differing(full, nb).sum() == 0
            assert nb["counters"]["shadow"] + nb["counters"]["shadow_skipped"] < \
                full["counters"]["shadow"] + full["counters"]["shadow_skipped"]
    one = lit.frame("open", ("in_plane_only", ls.lights(7)[ls.IN_PLANE:ls.IN_PLANE + 1]), W, H)["counters"]
    assert one["shadow"] > 0 and one["shadow_skipped"] > 0, one


def test_the_centre_column_holds_the_culled_edge(lit, tmp_path):
    """what the scene turned up on the GPU: the centre column's primary rays have d.x = 0 exactly and
    run in the plane x = 0, 1e-16 beside the sphere's seam between two strips of longitude. hit_triangle accepts the
    triangle across the seam at a smaller t; the reference's slab test, dividing by that zero, culls its box exactly,
    so the BVH walk never tests it. The oracle's exhaustive loop does, and differs in the hit there with a nearer t: a
    fast walk that takes the minimum over every triangle its padded boxes reach is wrong on these pixels."""
    from tests.oracle_bind import OracleScene, camera
    for W, H in ((64, 40), (36, 20)):
        cam = camera(W, H)
        assert ((cam[1] - cam[0]) + cam[2] * np.float32(W // 2))[0] == 0
        ref = lit.frame("open", 0, W, H)
        o = OracleScene.load(*ls.write(tmp_path, "open", 0))
        o.build_bvh(3)
        o.set_use_bvh(False)
        every = o.render(W, H)
        ys, xs = np.nonzero((ref["hit"] != every["hit"]) & (ref["hit"] >= 0) & (ref["hit"] < 960))
        assert len(ys) >= 1 and (xs == W // 2).all(), (W, H, xs, ys)
        nearer = every["t"][ys, xs] < ref["t"][ys, xs]
        assert nearer.any(), (W, H)
        assert (every["hit"][ys, xs] < 960).all()


def test_moved_lights(lit):
    """moved(): every light moves, light 0 goes from above the floor to below it"""
    for L in (2, 8, 9, 33):
        a = ls.lights(L, form="hall")
        b = ls.moved(a)
        assert (a[:, :3] != b[:, :3]).any(1).all() and np.array_equal(a[:, 3:], b[:, 3:])
        assert a[0, 2] > ls.FLOOR_Z > b[0, 2]
        s = host.Scene.load(*lit.paths("hall", (f"{L}_moved", b)))
        assert np.array_equal(s.lights.view(np.float32).reshape(-1, 6).view(np.int32), b.view(np.int32))
