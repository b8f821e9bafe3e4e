"""The multi-hit query's yardstick: a numpy float32 restatement of the reference's hit_triangle
(cpu/src/raytracer.c:35-59) over [rays, triangles], in chunks of rays -- its brute-force path (USE_BVH 0,
raytracer.c:115-129) without the minimum. Every operation is one float32 operation in vec.c's operand order
(dot = x*x + y*y + z*z evaluated left to right, cross as vec_cross writes it, 1.0f / det and then the products), so
each t carries the reference's bits. A ray's hit set is every triangle with t < FLT_MAX and t <= t_max, ordered by
(t, original index)."""
import numpy as np

F = np.float32
EPS = F(1e-3)  # const float EPSILON = 1e-3
FMAX = F(3.402823466e+38)


def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz  # (float32 arrays: each product and each sum rounds once, left to right)


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def hit_t(o, d, coords):
    """t [rays, triangles] float32: hit_triangle's return value (FLT_MAX on a miss) for every pair"""
    o, d, c = np.asarray(o, F), np.asarray(d, F), np.asarray(coords, F)
    v0 = c[:, 0]
    e1 = c[:, 1] - c[:, 0]
    e2 = c[:, 2] - c[:, 0]
    n = _cross(e1[:, 0], e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1], e2[:, 2])
    ox, oy, oz = (o[:, k, None] for k in range(3))
    dx, dy, dz = (d[:, k, None] for k in range(3))
    with np.errstate(all="ignore"):
        det = -_dot(dx, dy, dz, n[0][None], n[1][None], n[2][None])
        inv = F(1.0) / det
        ax, ay, az = ox - v0[None, :, 0], oy - v0[None, :, 1], oz - v0[None, :, 2]
        t = _dot(ax, ay, az, n[0][None], n[1][None], n[2][None]) * inv
        qx, qy, qz = _cross(ax, ay, az, dx, dy, dz)
        u = _dot(e2[None, :, 0], e2[None, :, 1], e2[None, :, 2], qx, qy, qz) * inv
        v = -_dot(e1[None, :, 0], e1[None, :, 1], e1[None, :, 2], qx, qy, qz) * inv
        ok = ~(np.abs(det) < EPS) & (t > EPS) & (u >= F(0)) & (v >= F(0)) & ((u + v) <= F(1))
    assert t.dtype == F and u.dtype == F and det.dtype == F
    return np.where(ok, t, FMAX)


def hit_lists(o, d, coords, t_max=None, chunk=16, threads=8):
    """per ray: (tri int32 [k], t float32 [k]) of its whole hit set, sorted by (t, original index). The chunks of
    rays are independent; numpy's loops release the interpreter lock, so a few threads share them."""
    from concurrent.futures import ThreadPoolExecutor
    o, d = np.asarray(o, F), np.asarray(d, F)

    def one(a):
        t = hit_t(o[a:a + chunk], d[a:a + chunk], coords)
        with np.errstate(invalid="ignore"):
            m = t < FMAX
            if t_max is not None:
                m &= t <= np.asarray(t_max, F)[a:a + chunk, None]  # (a NaN bound: nothing; +inf: everything)
        part = []
        for r in range(t.shape[0]):
            idx = np.flatnonzero(m[r]).astype(np.int32)
            tt = t[r, idx]
            order = np.lexsort((idx, tt))
            part.append((idx[order], tt[order]))
        return part

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(0, len(o), chunk)))
    return [x for p in parts for x in p]


def expected(lists, max_hits):
    """(tri [n, max_hits], t [n, max_hits], count [n] = min(|S|, max_hits), total [n] = |S|) as rt_trace_hits fills them"""
    n = len(lists)
    tri = np.full((n, max_hits), -1, np.int32)
    t = np.full((n, max_hits), FMAX, np.float32)
    total = np.array([len(i) for i, _ in lists], np.int32).reshape(n)
    for r, (i, tt) in enumerate(lists):
        k = min(len(i), max_hits)
        tri[r, :k] = i[:k]
        t[r, :k] = tt[:k]
    return tri, t, np.minimum(total, max_hits).astype(np.int32), total


def bounded(lists, t_max):
    """the lists of the same rays under per-ray bounds t_max (t <= t_max; NaN or non-positive: empty)"""
    out = []
    for (i, tt), b in zip(lists, np.asarray(t_max, F)):
        with np.errstate(invalid="ignore"):
            k = (tt <= b) if b > 0 else np.zeros(len(tt), bool)
        out.append((i[k], tt[k]))
    return out
