"""The sweep query's yardstick (rt_sweep_spheres, include/rt_hip.h): a numpy float32 restatement of toi(sweep, record)
as the header states it. Every operation is one float32 operation in the stated order (dot = x*x + y*y + z*z left to
right, nothing fused), on what a triangle record holds: a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0). fminf / fmaxf are
np.fmin / np.fmax (a NaN operand loses); a comparison with a NaN operand is false, in numpy as in C.

Step 1 (the gate) is evaluated for every (sweep, triangle) pair, in chunks of sweeps; steps 2 and 3 only for the pairs
that pass it, as flat arrays (tests/overlap_ref.py's scheme). D, P and the region case of steps 2 and 3 are
tests/nearest_ref.py's dist() restated pair by pair -- a sweep's recentred centre differs from triangle to triangle, so
dist()'s [points, triangles] product does not apply; near() below is checked against dist() bit for bit by
tests/test_sweep_abi.py. A sweep's answer is the first triangle by (toi, original index)."""
import numpy as np

from tests import nearest_ref, overlap_ref

F = np.float32
FMAX = nearest_ref.FMAX
same_bits = nearest_ref.same_bits
records = overlap_ref.records
scene_extent = overlap_ref.scene_extent


def _dot(u, v):
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]  # (float32: each product and sum rounds once)


def near(q, a, e1, e2):
    """rt_nearest_points' D, P and "the last case (the interior) was reached" for the pairs (q[p], record p):
    ([p] float32, [p, 3] float32, [p] bool)"""
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        ap = q - a
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        bp = ap - e1
        d3, d4 = _dot(e1, bp), _dot(e2, bp)
        cp = ap - e2
        d5, d6 = _dot(e1, cp), _dot(e2, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        x, y = d4 - d3, d5 - d6
        b, cc = a + e1, a + e2
        conds = [(d1 <= zero) & (d2 <= zero),
                 (d3 >= zero) & (d4 <= d3),
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),
                 (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero),
                 (va <= zero) & (x >= zero) & (y >= zero)]
        s_ab = (d1 / (d1 - d3))[:, None]
        s_ac = (d2 / (d2 - d6))[:, None]
        s_bc = (x / (x + y))[:, None]
        den = one / ((va + vb) + vc)
        v, w = (vb * den)[:, None], (vc * den)[:, None]
        c3 = [np.broadcast_to(k[:, None], a.shape) for k in conds]
        p = np.select(c3, [a, b, a + e1 * s_ab, cc, a + e2 * s_ac, b + (e2 - e1) * s_bc], (a + e1 * v) + e2 * w)
        lo = np.fmin(np.fmin(a, b), cc)
        hi = np.fmax(np.fmax(a, b), cc)
        P = np.fmin(np.fmax(p, lo), hi)
        df = q - P
        D = _dot(df, df)
        interior = ~np.logical_or.reduce(conds)
    assert D.dtype == F and P.dtype == F and va.dtype == F
    return D, P, interior


def valid_sweeps(c, d, r, tm):
    """not (a non-finite c, d or r; r < 0; a NaN or negative t_max). The signs are read from the bits: a negative
    subnormal stays negative whatever the process' flush-to-zero state."""
    def neg(x):
        bits = x.view(np.int32)
        return (bits < 0) & ((bits & 0x7FFFFFFF) != 0)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(c).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(r) & ~neg(r) & ~np.isnan(tm) &
                ~neg(tm))


def gate(c, d, r, T, tlo, thi):
    """step 1 for every pair -> (open [sweeps, triangles] bool, t0 [sweeps, triangles] float32)"""
    n, m = len(c), len(tlo)
    t0 = np.zeros((n, m), F)
    t1 = np.broadcast_to(T[:, None], (n, m)).astype(F)
    ok = np.ones((n, m), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            glo = tlo[None, :, k] - r[:, None]
            ghi = thi[None, :, k] + r[:, None]
            ck, dk = c[:, k, None], d[:, k, None]
            z = (dk.view(np.int32) & 0x7FFFFFFF) == 0  # (d.k == 0, read from the bits: a subnormal is not zero
            #                                             whatever the process' flush-to-zero state)
            inv = F(1) / dk
            ta = (glo - ck) * inv
            tb = (ghi - ck) * inv
            assert ta.dtype == F and glo.dtype == F
            t0 = np.where(z, t0, np.fmax(t0, np.fmin(ta, tb)))
            t1 = np.where(z, t1, np.fmin(t1, np.fmax(ta, tb)))
            ok &= ~z | ((glo <= ck) & (ck <= ghi))
        ok &= t0 <= t1
    assert t0.dtype == F and t1.dtype == F
    return ok, t0


def steps23(c, d, r, rec, t0):
    """toi for the pairs (sweep p with c[p], d[p], r[p]; record rec[.][p]) that passed the gate at t0[p] -> [pairs]
    float32, +inf where no candidate is valid (membership toi <= T is the caller's)"""
    a, e1, e2, b, cc = rec[:5]
    zero = F(0)
    with np.errstate(all="ignore"):
        r2 = r * r
        dd = _dot(d, d)
        c0 = c + d * t0[:, None]
        D0, _, _ = near(c0, a, e1, e2)
        touching = D0 <= r2
        u = np.full(len(c), np.inf, F)

        def take(u, cand, ok):
            return np.where(ok & (cand < u), cand, u)
        # the face, from the original centre
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        nn = _dot(n, n)
        ln = np.sqrt(nn)
        so = _dot(n, c - a)
        dn = _dot(n, d)
        sg = np.where(so < zero, F(-1), F(1))
        tf = (sg * (r * ln) - so) / dn
        assert n.dtype == F and ln.dtype == F and tf.dtype == F
        _, _, interior = near(c + d * tf[:, None], a, e1, e2)
        u = take(u, np.fmax(tf - t0, zero), (nn > zero) & (dn * sg < zero) & (tf >= zero) & interior)
        for p, f in ((a, e1), (a, e2), (b, e2 - e1)):
            m = c0 - p
            md, nd, ff = _dot(m, f), _dot(d, f), _dot(f, f)
            A = ff * dd - nd * nd
            K = _dot(m, m) - r2
            Cq = ff * K - md * md
            Bq = ff * _dot(m, d) - nd * md
            disc = Bq * Bq - A * Cq
            cand = (-Bq - np.sqrt(disc)) / A
            s = md + cand * nd
            assert cand.dtype == F and s.dtype == F and disc.dtype == F
            u = take(u, cand, (A > zero) & (disc >= zero) & (cand >= zero) & (zero <= s) & (s <= ff))
        for v in (a, b, cc):
            m = c0 - v
            Bv = _dot(m, d)
            Cv = _dot(m, m) - r2
            disc = Bv * Bv - dd * Cv
            cand = (-Bv - np.sqrt(disc)) / dd
            assert cand.dtype == F
            u = take(u, cand, (dd > zero) & (disc >= zero) & (cand >= zero))
        toi = np.where(touching, t0, t0 + u)
    assert toi.dtype == F
    return toi


def _inputs(centre, motion, radius, t_max):
    c = np.ascontiguousarray(centre, F).reshape(-1, 3)
    d = np.ascontiguousarray(motion, F).reshape(-1, 3)
    n = len(c)
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, F), (n,)))
    tm = np.full(n, np.inf, F) if t_max is None else np.ascontiguousarray(t_max, F).reshape(n)
    assert len(d) == n
    return c, d, r, tm


def pairs(centre, motion, radius, coords, t_max=None, chunk=64):
    """(si, ti, toi): the pairs that pass the gate in (sweep, triangle) order and toi for each (+inf: no candidate);
    invalid sweeps have none. Membership of S_i is toi <= fminf(t_max, FLT_MAX)."""
    c, d, r, tm = _inputs(centre, motion, radius, t_max)
    rec = records(coords)
    ok = valid_sweeps(c, d, r, tm)
    T = np.fmin(tm, FMAX)
    sis, tis, ts = [], [], []
    for s in range(0, len(c), chunk):
        sl = slice(s, s + chunk)
        g, t0 = gate(c[sl], d[sl], r[sl], T[sl], rec[5], rec[6])
        g &= ok[sl, None]
        si, ti = np.nonzero(g)
        t0 = t0[si, ti]
        si += s
        sis.append(si)
        tis.append(ti)
        ts.append(steps23(c[si], d[si], r[si], [x[ti] for x in rec], t0))
    if not sis:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F)
    return np.concatenate(sis), np.concatenate(tis), np.concatenate(ts)


def expected(centre, motion, radius, coords, t_max=None, chunk=64):
    """(tri [n] int32, t [n] float32, point [n, 3] float32, ties [n] int64) as rt_sweep_spheres fills them: the first
    triangle by (toi, index) with toi <= fminf(t_max, FLT_MAX); -1 / FLT_MAX / c's bits for the empty set. ties: the
    number of members of S_i whose toi equals the answer's (0 for the empty set)."""
    c, d, r, tm = _inputs(centre, motion, radius, t_max)
    n = len(c)
    si, ti, toi = pairs(c, d, r, coords, tm, chunk)
    T = np.fmin(tm, FMAX)
    with np.errstate(invalid="ignore"):
        member = toi <= T[si]
    si, ti, toi = si[member], ti[member], toi[member]
    tri = np.full(n, -1, np.int32)
    t = np.full(n, FMAX, F)
    point = c.copy()
    ties = np.zeros(n, np.int64)
    if len(si):
        # toi >= +0, so its bits order as the floats do: one key per pair, the least per sweep
        key = (toi.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64)
        first = np.nonzero(np.diff(si, prepend=-1))[0]
        best = np.minimum.reduceat(key, first)
        rows = si[first]
        tri[rows] = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
        t[rows] = (best >> np.uint64(32)).astype(np.uint32).view(F)
        np.add.at(ties, si[toi.view(np.uint32) == t[si].view(np.uint32)], 1)
        rec = records(coords)
        with np.errstate(all="ignore"):
            C = c[rows] + d[rows] * t[rows, None]
        _, P, _ = near(C, rec[0][tri[rows]], rec[1][tri[rows]], rec[2][tri[rows]])
        point[rows] = P
    return tri, t, point, ties


# ------------------------------------------------------------------ the fixture's generator
def scene_box(coords):
    v = np.asarray(coords, np.float64).reshape(-1, 3)
    return v.min(0), v.max(0)


def fixture_sweeps(coords, n, seed):
    """n sweeps: centres uniform in the scene box grown by a quarter, motions towards noisy triangle centroids at 1.5x
    the distance (so the centroid is reached at t = 2/3), every fourth motion axis-aligned (two zero components), radii
    from {0, 0.1 %, 1 %, 5 %} of the extent -> (centre [n, 3], motion [n, 3], radius [n]) float32"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(coords)
    ext = scene_extent(coords)
    grow = 0.25 * (hi - lo)
    c = rng.uniform(lo - grow, hi + grow, (n, 3))
    cen = np.asarray(coords, np.float64).mean(axis=1)[rng.integers(0, len(coords), n)]
    d = 1.5 * (cen + rng.normal(0, 0.01 * ext, (n, 3)) - c)
    ax = np.arange(n) % 4 == 3
    k = np.abs(d).argmax(axis=1)
    keep = np.zeros((n, 3), bool)
    keep[np.arange(n), k] = True
    d = np.where(ax[:, None] & ~keep, 0.0, d)
    r = ext * np.array([0.0, 1e-3, 1e-2, 5e-2])[rng.integers(0, 4, n)]
    return c.astype(F), d.astype(F), r.astype(F)
