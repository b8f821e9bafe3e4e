"""The cut query's yardstick (rt_cut_triangles, include/rt_hip.h): a numpy float32 restatement of X(q, record) and of the
cut segment as the header states them. Every operation is one float32 operation in the stated order (nothing fused), on
what a triangle record holds: a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0). fminf / fmaxf are np.fmin / np.fmax (a NaN
operand loses); a comparison with a NaN operand is false, in numpy as in C.

Step 1 (the corner boxes against the queries' corner boxes, comparisons only) is evaluated for every (query, triangle)
pair, in chunks of queries; steps 2..6 only for the pairs that pass it, as flat arrays. sets() returns every query's
full S_i in CSR form with the segments (np.nonzero walks row-major, so each list is in index order); overlap_ref's
answer() and segments() read any k and count_all off it. A query with a non-finite number has the empty set."""
import numpy as np

from tests import overlap_ref
from tests.overlap_ref import answer, records, scene_extent, segments  # noqa: F401  (the same CSR helpers)

F = np.float32


def tris(q):
    q = np.ascontiguousarray(q, F).reshape(-1, 3, 3)
    assert q.dtype == F
    return q


def valid_tris(q):
    return np.isfinite(tris(q)).all(axis=(1, 2))


def corner_boxes(q):
    """(qlo, qhi) [n, 3]: fminf(fminf(q0, q1), q2), fmaxf(fmaxf(q0, q1), q2)"""
    q = tris(q)
    return np.fmin(np.fmin(q[:, 0], q[:, 1]), q[:, 2]), np.fmax(np.fmax(q[:, 0], q[:, 1]), q[:, 2])


def cross(u, v):
    """rt_overlap_boxes' nrm"""
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def apart(d):
    """d [p, 3]: all three > 0, all three < 0 or all three == 0"""
    return (d > 0).all(axis=1) | (d < 0).all(axis=1) | (d == 0).all(axis=1)


def line_axis(D):
    """step 4: 0, then 1 if |D.y| > |D.x|, then 2 if |D.z| > |D.k|"""
    A = np.abs(D)
    k = np.where(A[:, 1] > A[:, 0], 1, 0)
    best = np.where(k == 1, A[:, 1], A[:, 0])
    return np.where(A[:, 2] > best, 2, k)


def interval(V, d, k):
    """step 5 for corners V [p, 3 corners, 3] with distances d [p, 3] on axis k [p] -> (start [p, 3], end [p, 3],
    lo [p], hi [p])"""
    ar = np.arange(len(d))
    s = (d > 0).astype(np.int8) - (d < 0).astype(np.int8)
    s0, s1, s2 = s[:, 0], s[:, 1], s[:, 2]
    al = np.select([(s0 == s1) & (s0 != 0), (s0 == s2) & (s0 != 0), ((s1 == s2) & (s1 != 0)) | (s0 != 0), s1 != 0],
                   [2, 1, 0, 1], default=2)
    x, y = (al + 1) % 3, (al + 2) % 3
    va, da = V[ar, al], d[ar, al]
    out = []
    for o in (x, y):
        lam = da / (da - d[ar, o])
        P = va + (V[ar, o] - va) * lam[:, None]
        assert lam.dtype == F and P.dtype == F
        out.append((P, P[ar, k]))
    (px, tx), (py, ty) = out
    fwd = (tx <= ty)[:, None]
    return np.where(fwd, px, py), np.where(fwd, py, px), np.fmin(tx, ty), np.fmax(tx, ty)


def gate(qlo, qhi, rec):
    """[queries, triangles] bool: tlo.k <= qhi.k && thi.k >= qlo.k on all three axes (overlap_ref.step1)"""
    return overlap_ref.step1(qlo, qhi, rec)


def steps26(q, rec, qi, ti):
    """X and the cut segment for the pairs (query qi[p], triangle ti[p]) that passed the gate ->
    (X [pairs] bool, s0 [pairs, 3], s1 [pairs, 3]); the segment of a pair that is no member is not meaningful"""
    a, e1, e2, b, c = (x[ti] for x in rec[:5])
    q0, q1, q2 = q[qi, 0], q[qi, 1], q[qi, 2]
    with np.errstate(all="ignore"):
        nq = cross(q1 - q0, q2 - q0)
        dm = np.stack([dot(nq, m - q0) for m in (a, b, c)], axis=1)
        nm = cross(e1, e2)
        dq = np.stack([dot(nm, m - a) for m in (q0, q1, q2)], axis=1)
        assert nq.dtype == F and dm.dtype == F and dq.dtype == F
        out = apart(dm) | apart(dq)
        k = line_axis(cross(nq, nm))
        ms, me, mlo, mhi = interval(np.stack([a, b, c], axis=1), dm, k)
        qs, qe, qlo, qhi = interval(q[qi], dq, k)
        X = ~out & (mlo <= qhi) & (qlo <= mhi)
        s0 = np.where((qlo > mlo)[:, None], qs, ms)
        s1 = np.where((qhi < mhi)[:, None], qe, me)
    assert s0.dtype == F and s1.dtype == F
    return X, s0, s1


def pairs(q, coords, chunk=64):
    """(qi, ti, X, s0, s1): the gate pairs in (query, triangle) order, X and the segment for each"""
    q = tris(q)
    rec = records(coords)
    ok = valid_tris(q)
    with np.errstate(invalid="ignore"):
        qlo, qhi = corner_boxes(q)
    qis, tis, xs, s0s, s1s = [], [], [], [], []
    for s in range(0, len(q), chunk):
        m = gate(qlo[s:s + chunk], qhi[s:s + chunk], rec) & ok[s:s + chunk, None]
        qi, ti = np.nonzero(m)
        qi += s
        X, s0, s1 = steps26(q, rec, qi, ti)
        qis.append(qi)
        tis.append(ti)
        xs.append(X)
        s0s.append(s0)
        s1s.append(s1)
    if not qis:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, bool), np.zeros((0, 3), F), np.zeros((0, 3), F)
    return tuple(np.concatenate(x) for x in (qis, tis, xs, s0s, s1s))


def sets(q, coords, chunk=64):
    """every query's S_i -> (offsets [n + 1] int64, tris [offsets[n]] int32, seg [offsets[n], 2, 3] float32), each
    list in index order"""
    n = len(tris(q))
    qi, ti, X, s0, s1 = pairs(q, coords, chunk)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(qi[X], minlength=n), out=offsets[1:])
    return offsets, ti[X].astype(np.int32), np.stack([s0[X], s1[X]], axis=1)


def expected(q, coords, k, count_all=False):
    return answer(sets(q, coords)[:2], k, count_all)


def surface_tris(coords, n, seed):
    """n query triangles at the surface: each centre a uniform point on a random triangle plus N(0, 1e-3 extent) per
    axis, the corners the centre plus size * (N(0, 1)^{3 x 3} with the corner mean removed), size = extent *
    10^U(-3, -1.3) -> [n, 3, 3] float32"""
    rng = np.random.default_rng(seed)
    c = np.asarray(coords, np.float64)
    ext = scene_extent(coords)
    t = rng.integers(0, len(c), n)
    u, w = rng.random(n), rng.random(n)
    flip = u + w > 1
    u, w = np.where(flip, 1 - u, u), np.where(flip, 1 - w, w)
    ctr = c[t, 0] + u[:, None] * (c[t, 1] - c[t, 0]) + w[:, None] * (c[t, 2] - c[t, 0])
    ctr = ctr + rng.normal(0, 1e-3 * ext, (n, 3))
    off = rng.normal(0, 1, (n, 3, 3))
    off = off - off.mean(axis=1, keepdims=True)
    size = ext * 10.0 ** rng.uniform(-3, -1.3, n)
    return (ctr[:, None, :] + size[:, None, None] * off).astype(F)
