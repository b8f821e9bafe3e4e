"""One small generated scene with materials and any number of lights, written as the three text files the loaders read
(tests/test_lit_scenes.py on the CPU, tests/test_gpu_lights.py on the GPU). The oracle and host.Scene.load read the
same bytes; nothing of it is committed as data.

Geometry (coordinates formed in float64, rounded to float32, printed with nine digits so that they read back exactly;
seen from host.camera's pose at (0, -9, 3)):
  * the 960-triangle bumpy sphere of tests/variants.py::mesh(), scaled by 2 about the origin (exact ties on its shared
    edges and vertices);
  * a room around it and the camera, every face a 4 x 4 grid of quads (32 triangles): the floor z = -2.5 over
    x in [-7, 7], y in [-10, 8], the walls x = -7, x = 7 and y = 8 up to z = 8.
  `open` is that (1,088 triangles, sky above and behind the camera); `hall` adds the ceiling z = 8 and the wall y = -10
  (1,152 triangles) and makes the floor, the ceiling and the walls x = -7, x = 7 mirrors, so that paths run to the last
  level.

Materials: MATERIALS, every one on the sphere in runs of RUN triangles (one strip of longitude, so a wave's lanes see
several), the room's faces reuse them. Among them kr = (1, 1, 1) with ks = kd = 0 (`mirror`), kr = (0.9, 0, 0.3)
(`tint`), kr = (1e-3, 0, 0) (`faint`), kr = 0 (`dull`), ks = kd = kr = 0 (`black`), `glossy` and `matte`.

Lights: lights(L, seed, form) gives L lights for any L >= 0; light j (counted from 0) has the same position and the
same colour before scaling for every L > j, and every kl is scaled by 8 / L. Positions come from a hash of (seed, j),
not from a library's generator. The slots:
  j % 5 == 4          (every fifth light) under the floor: back-facing for the floor, shadow_skipped > 0
  j % 5 == 0, j >= 5  (every fifth plus one) inside the sphere
  j == 2   BLACK      kl = 0
  j == 6   IN_PLANE   z exactly the floor's float32 z, inside the room: dot(L - p, n) is +-0 or tiny for the floor's
                      points, which is not raytrace()'s early-out, so shadow rays run along the surface
  j == 11  FAR        `open` only: at distance 2.5e6 with kl = 1e13 * 8 / L, so dist^2 > 2^40 (rtx::div3's IEEE
                      fallback) and kl * cr < 2^50
  j == 13  TWIN       at light 12's position exactly
  every other j       inside the room at z in [3, 7.5]; the 8th, 9th, 32nd and 33rd lights (j = 7, 8, 31, 32) are
                      of this kind, so a kernel that drops the last light of 8, 9, 32 or 33 changes pixels
"""
import os

import numpy as np

F = np.float32
FORMS = ("open", "hall")
RUN = 30
SEED = 7
FLOOR_Z = F(-2.5)
BLACK, IN_PLANE, FAR, TWIN = 2, 6, 11, 13
ORDINARY_LAST = (7, 8, 31, 32)  # the last light of L = 8, 9, 32, 33

# name, kd, ks, kr
MATERIALS = [
    ("mirror", (0, 0, 0), (0, 0, 0), (1, 1, 1)),
    ("tint", (0.3, 0.3, 0.3), (0.2, 0.2, 0.2), (0.9, 0, 0.3)),
    ("faint", (0.5, 0.4, 0.3), (0.2, 0.2, 0.2), (1e-3, 0, 0)),
    ("dull", (0.6, 0.5, 0.2), (0.3, 0.3, 0.3), (0, 0, 0)),
    ("black", (0, 0, 0), (0, 0, 0), (0, 0, 0)),
    ("glossy", (0.2, 0.2, 0.2), (0.8, 0.8, 0.8), (0.2, 0.2, 0.2)),
    ("matte", (0.7, 0.7, 0.7), (0, 0, 0), (0, 0, 0)),
    ("red", (0.8, 0.1, 0.1), (0.1, 0.1, 0.1), (0.2, 0.2, 0.2)),
    ("green", (0.1, 0.7, 0.2), (0.3, 0.3, 0.3), (0.1, 0.3, 0.1)),
    ("blue", (0.1, 0.2, 0.8), (0.5, 0.5, 0.5), (0, 0, 0.5)),
    ("chrome", (0.05, 0.05, 0.05), (0.9, 0.9, 0.9), (0.8, 0.8, 0.8)),
    ("ground", (0.5, 0.5, 0.5), (0.1, 0.1, 0.1), (0.2, 0.2, 0.2)),
    ("wall", (0.6, 0.6, 0.5), (0, 0, 0), (0.1, 0.1, 0.1)),
    ("glass", (0.1, 0.1, 0.1), (0.1, 0.1, 0.1), (0.85, 0.85, 0.85)),
]
MAT = {m[0]: i for i, m in enumerate(MATERIALS)}


def _grid(p, eu, ev):
    """a 4 x 4 grid of quads over p + s eu + t ev (s, t in [0, 1]): 32 triangles [32, 3, 3] float64"""
    p, eu, ev = (np.asarray(a, np.float64) for a in (p, eu, ev))
    out = []
    for i in range(4):
        for k in range(4):
            a, b = p + eu * (i / 4) + ev * (k / 4), p + eu * ((i + 1) / 4) + ev * (k / 4)
            c, d = p + eu * ((i + 1) / 4) + ev * ((k + 1) / 4), p + eu * (i / 4) + ev * ((k + 1) / 4)
            out += [[a, b, c], [a, c, d]]
    return np.array(out)


def triangles(form):
    """-> (coords [n, 3, 3] float32, material index [n]) of `open` (n = 1,088) or `hall` (n = 1,152)"""
    from tests import variants
    assert form in FORMS
    hall = form == "hall"
    sphere = variants.mesh()[:960] * 2.0
    mats = [(np.arange(960) // RUN) % len(MATERIALS)]
    z0, z1 = float(FLOOR_Z), 8.0
    faces = [(_grid([-7, -10, z0], [14, 0, 0], [0, 18, 0]), "mirror" if hall else "ground"),     # floor
             (_grid([-7, -10, z0], [0, 18, 0], [0, 0, z1 - z0]), "glass" if hall else "wall"),    # x = -7
             (_grid([7, -10, z0], [0, 18, 0], [0, 0, z1 - z0]), "mirror" if hall else "matte"),   # x = 7
             (_grid([-7, 8, z0], [14, 0, 0], [0, 0, z1 - z0]), "wall")]                           # y = 8
    if hall:
        faces += [(_grid([-7, -10, z1], [14, 0, 0], [0, 18, 0]), "chrome"),                       # ceiling
                  (_grid([-7, -10, z0], [14, 0, 0], [0, 0, z1 - z0]), "ground")]                  # y = -10
    parts = [sphere] + [f for f, _ in faces]
    mats += [np.full(32, MAT[m]) for _, m in faces]
    return np.concatenate(parts).astype(F), np.concatenate(mats)


def _unit(seed, j, k):
    """a number in [0, 1) from (seed, j, k): a 64-bit mix (splitmix64's finaliser), its top 24 bits"""
    M = (1 << 64) - 1
    x = (seed * 0x9E3779B97F4A7C15 + j * 0xBF58476D1CE4E5B9 + k * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & M
    for _ in range(2):
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & M
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & M
        x ^= x >> 31
    return (x >> 40) / float(1 << 24)


def _between(lo, hi, u):
    return lo + (hi - lo) * u


def light(j, seed=SEED, form="open"):
    """light j before the 8 / L scaling: (x, y, z, r, g, b) float64"""
    u = [_unit(seed, j, k) for k in range(6)]
    kl = [_between(5.0, 14.0, v) for v in u[3:]]
    if j == FAR and form == "open":
        return [0.4e6, -1.5e6, 1.96e6, 1e13, 8e12, 6e12]  # |p| = 2.5e6
    if j == TWIN:
        return light(TWIN - 1, seed, form)[:3] + kl
    if j == IN_PLANE:
        return [3.0, -2.0, float(FLOOR_Z)] + kl
    if j == BLACK:
        kl = [0.0, 0.0, 0.0]
    if j % 5 == 4:  # under the floor
        pos = [_between(-6, 6, u[0]), _between(-9, 7, u[1]), _between(-6, -3, u[2])]
    elif j % 5 == 0 and j >= 5:  # inside the sphere
        pos = [_between(-0.5, 0.5, u[0]), _between(-0.5, 0.5, u[1]), _between(-0.4, 0.4, u[2])]
    else:
        pos = [_between(-6, 6, u[0]), _between(-9, 7, u[1]), _between(3, 7.5, u[2])]
    return pos + kl


def lights(L, seed=SEED, form="open"):
    """-> [L, 6] float32: position and kl * 8 / L of lights 0 .. L - 1"""
    out = np.array([light(j, seed, form) for j in range(L)], np.float64).reshape(L, 6)
    if L:
        out[:, 3:] *= 8.0 / L
    return out.astype(F)


def moved(arr):
    """every light of [L, 6] moved: by (0.375, -0.25, 0.5), and every third (0, 3, ...) mirrored to the other side of
    the floor's plane, which carries light 0 (above it for every L >= 1) below it"""
    out = np.array(arr, np.float64)
    out[:, :3] += [0.375, -0.25, 0.5]
    out[::3, 2] = 2 * float(FLOOR_Z) - out[::3, 2]
    return out.astype(F)


def _num(v):
    return format(float(F(v)), ".9g")


def write_lights(path, arr):
    """one 'x y z r g b' line per light, nine digits: the float32 values read back exactly"""
    with open(path, "w") as f:
        for row in np.asarray(arr, F).reshape(-1, 6):
            f.write(" ".join(_num(v) for v in row) + "\n")
    return str(path)


def write_geometry(dirpath, form):
    """-> (obj, mtl): `form`'s triangles, three 'v' lines and one 'f' per triangle, a 'usemtl' where the material
    changes; Kd / Ks / Kr on the three lines after 'newmtl'"""
    obj, mtl = os.path.join(str(dirpath), f"{form}.obj"), os.path.join(str(dirpath), f"{form}.mtl")
    with open(mtl, "w") as f:
        for name, kd, ks, kr in MATERIALS:
            f.write(f"newmtl {name}\n")
            for key, v in (("Kd", kd), ("Ks", ks), ("Kr", kr)):
                f.write(f"{key} " + " ".join(_num(c) for c in v) + "\n")
            f.write("\n")
    coords, mats = triangles(form)
    with open(obj, "w") as f:
        for v in coords.reshape(-1, 3):
            f.write("v " + " ".join(_num(c) for c in v) + "\n")
        last = -1
        for i, m in enumerate(mats):
            if m != last:
                f.write(f"usemtl {MATERIALS[m][0]}\n")
                last = m
            f.write(f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}\n")
    return obj, mtl


def write(dirpath, form, L, seed=SEED):
    """-> (obj, mtl, lights) paths of `form` with L lights under dirpath (the geometry is written once per form)"""
    d = str(dirpath)
    obj, mtl = os.path.join(d, f"{form}.obj"), os.path.join(d, f"{form}.mtl")
    if not (os.path.exists(obj) and os.path.exists(mtl)):
        write_geometry(d, form)
    return obj, mtl, write_lights(os.path.join(d, f"{form}_{L}_{seed}.lights"), lights(L, seed, form))


LIGHT_COUNTS = (0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 40)


class Lit:
    """the files, loaded scenes and oracle frames of one directory, each made once (shared between tests: leave the
    arrays alone). A light set is a count L (lights(L, SEED, form)) or a (tag, [n, 6] array) pair of the caller's."""

    def __init__(self, dirpath):
        self.dir = str(dirpath)
        self._paths, self._oracle, self._frames, self._host = {}, {}, {}, {}

    def paths(self, form, lset):
        tag = lset if isinstance(lset, int) else lset[0]
        if (form, tag) not in self._paths:
            if isinstance(lset, int):
                self._paths[form, tag] = write(self.dir, form, lset)
            else:
                obj, mtl, _ = write(self.dir, form, 0)
                self._paths[form, tag] = (obj, mtl, write_lights(os.path.join(self.dir, f"{form}_{tag}.lights"),
                                                                 lset[1]))
        return self._paths[form, tag]

    def oracle(self, form, lset):
        from tests.oracle_bind import OracleScene
        p = self.paths(form, lset)
        if p not in self._oracle:
            self._oracle[p] = OracleScene.load(*p)
            self._oracle[p].build_bvh(3)
        return self._oracle[p]

    def frame(self, form, lset, W, H, bounces=4):
        """the oracle's frame: hit, t, rgb, bounce_hit [H, W, 4], counters"""
        key = (self.paths(form, lset), W, H, bounces)
        if key not in self._frames:
            o = self.oracle(form, lset)
            o.set_bounces(bounces)
            out = o.render(W, H, bounce_hits=True)
            for k in ("hit", "t", "rgb", "bounce_hit"):
                out[k].setflags(write=False)
            self._frames[key] = out
        return self._frames[key]

    def frame_spp(self, form, lset, W, H, spp, bounces=4):
        """the oracle's supersampled frame: (rgb, counters)"""
        key = (self.paths(form, lset), W, H, bounces, spp)
        if key not in self._frames:
            o = self.oracle(form, lset)
            o.set_bounces(bounces)
            self._frames[key] = o.render_spp(W, H, spp)
        return self._frames[key]

    def scene(self, form, lset):
        """host.Scene.load of the same three files, its BVH built"""
        from prt import host
        p = self.paths(form, lset)
        if p not in self._host:
            self._host[p] = host.Scene.load(*p).build_bvh(3)
        return self._host[p]
