"""The nearest-surface query's yardstick: a numpy float32 restatement of D and P as include/rt_hip.h states them
(rt_nearest_points) over [points, triangles], in chunks of points. Every operation is one float32 operation in the
stated order (dot = x*x + y*y + z*z evaluated left to right, nothing fused), on what a triangle record holds:
a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0). The clamp into the triangle's own box uses np.fmax / np.fmin (C's fmaxf /
fminf: a NaN operand loses). A point's answer is the first triangle by (D, original index) among those with
D <= min(max_dist2, FLT_MAX)."""
import numpy as np

F = np.float32
FMAX = F(3.402823466e+38)


def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz  # (float32 arrays: each product and each sum rounds once, left to right)


def dist(points, coords):
    """(D [points, triangles] float32, P [points, triangles, 3] float32) for every pair"""
    q, c = np.asarray(points, F), np.asarray(coords, F)
    assert q.dtype == F and c.dtype == F
    a = [c[None, :, 0, k] for k in range(3)]
    e1 = [(c[:, 1, k] - c[:, 0, k])[None, :] for k in range(3)]
    e2 = [(c[:, 2, k] - c[:, 0, k])[None, :] for k in range(3)]
    qq = [q[:, k, None] for k in range(3)]
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        ap = [qq[k] - a[k] for k in range(3)]
        d1, d2 = _dot(*e1, *ap), _dot(*e2, *ap)
        bp = [ap[k] - e1[k] for k in range(3)]
        d3, d4 = _dot(*e1, *bp), _dot(*e2, *bp)
        cp = [ap[k] - e2[k] for k in range(3)]
        d5, d6 = _dot(*e1, *cp), _dot(*e2, *cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        x, y = d4 - d3, d5 - d6
        b = [a[k] + e1[k] for k in range(3)]
        cc = [a[k] + e2[k] for k in range(3)]
        # the first condition that holds, in the stated order (np.select takes the first true one)
        conds = [(d1 <= zero) & (d2 <= zero),
                 (d3 >= zero) & (d4 <= d3),
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),
                 (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero),
                 (va <= zero) & (x >= zero) & (y >= zero)]
        s_ab = d1 / (d1 - d3)
        s_ac = d2 / (d2 - d6)
        s_bc = x / (x + y)
        den = one / ((va + vb) + vc)
        v, w = vb * den, vc * den
        P = []
        for k in range(3):
            shape = np.broadcast(d1, a[k]).shape
            p = np.select(conds, [np.broadcast_to(a[k], shape), np.broadcast_to(b[k], shape), a[k] + e1[k] * s_ab,
                                  np.broadcast_to(cc[k], shape), a[k] + e2[k] * s_ac,
                                  b[k] + (e2[k] - e1[k]) * s_bc],
                          (a[k] + e1[k] * v) + e2[k] * w)
            lo = np.fmin(np.fmin(a[k], b[k]), cc[k])
            hi = np.fmax(np.fmax(a[k], b[k]), cc[k])
            p = np.fmin(np.fmax(p, lo), hi)
            assert p.dtype == F
            P.append(p)
        df = [qq[k] - P[k] for k in range(3)]
        D = _dot(*df, *df)
    assert D.dtype == F and d1.dtype == F and va.dtype == F and den.dtype == F
    return D, np.stack(P, axis=-1)


def expected(points, coords, max_dist2=None, chunk=16, threads=8, ties=False):
    """(tri [n] int32, d2 [n] float32, point [n, 3] float32) as rt_nearest_points fills them: the first triangle by
    (D, index) with D <= min(max_dist2, FLT_MAX); -1 / FLT_MAX / the query point's bits for the empty set (nothing
    within the bound, a NaN or negative bound, a non-finite point). ties=True adds, per point, the number of triangles
    whose D equals the minimum over ALL triangles (0 for a non-finite point). The chunks of points are independent;
    numpy's loops release the interpreter lock, so a few threads share them."""
    from concurrent.futures import ThreadPoolExecutor
    q = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(q)
    md = np.full(n, FMAX, F) if max_dist2 is None else np.asarray(max_dist2, F).reshape(n)
    tri = np.full(n, -1, np.int32)
    d2 = np.full(n, FMAX, F)
    out = q.copy()
    nt = np.zeros(n, np.int64)

    def one(a):
        sl = slice(a, min(a + chunk, n))
        D, P = dist(q[sl], coords)
        with np.errstate(invalid="ignore"):
            # (a NaN or negative bound, read from the bits: a negative subnormal stays negative whatever the process'
            # flush-to-zero state, which a fast-math library loaded earlier may have set)
            bits = md[sl].view(np.int32)
            mag = bits & 0x7FFFFFFF
            valid = ~(mag > 0x7F800000) & ~((bits < 0) & (mag != 0)) & np.isfinite(q[sl]).all(axis=1)
            bound = np.fmin(md[sl], FMAX)
            inside = (D <= bound[:, None]) & valid[:, None]
            Dm = np.where(inside, D, F(np.inf))
            j = np.argmin(Dm, axis=1)  # (the first occurrence: the lowest index of an exact tie)
            rows = np.arange(D.shape[0])
            got = inside[rows, j]
            dmin = np.min(np.where(np.isnan(D), F(np.inf), D), axis=1)
            nt[sl] = np.where(np.isfinite(q[sl]).all(axis=1), (D == dmin[:, None]).sum(axis=1), 0)
        tri[sl] = np.where(got, j, -1)
        d2[sl] = np.where(got, D[rows, j], FMAX)
        out[sl] = np.where(got[:, None], P[rows, j], q[sl])

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(0, n, chunk)))
    return (tri, d2, out, nt) if ties else (tri, d2, out)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
