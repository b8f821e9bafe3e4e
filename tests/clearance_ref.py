"""The clearance query's yardstick (rt_clearance_triangles, include/rt_hip.h): a numpy float32 restatement of D(q, record),
the pair of points and the winning candidate as the header states them. Every operation is one float32 operation in the
stated order (dot = x*x + y*y + z*z left to right, nothing fused), on what a triangle record holds: a = v0,
e1 = fl(v1 - v0), e2 = fl(v2 - v0), and on the query made a record the same way. fminf / fmaxf are np.fmin / np.fmax (a
NaN operand loses); a comparison with a NaN operand is false, in numpy as in C.

Candidates 0..5 are tests/sweep_ref.py's near() (rt_nearest_points' D and P, pair by pair), the crossing is
tests/cut_ref.py's gate and steps26 (rt_cut_triangles' X and its segment): both called, not restated. New here are the
segment-segment closest pair of candidates 6..14 and the box-to-box lower bound.

A query's answer is the first triangle by (D, original index). expected() evaluates the pairs of a query in the order
of their record-box bounds and, with prune=True, skips a pair whose bound exceeds the smallest D already found for that
query (or the query's own bound); prune=False evaluates every pair. tests/test_clearance_abi.py holds the two against
each other bit for bit."""
import numpy as np

from tests import cut_ref, nearest_ref, overlap_ref, sweep_ref

F = np.float32
FMAX = nearest_ref.FMAX
same_bits = nearest_ref.same_bits
records = overlap_ref.records
scene_extent = overlap_ref.scene_extent
tris = cut_ref.tris
valid_tris = cut_ref.valid_tris
_dot = sweep_ref._dot


def clamp01(x):
    return np.fmin(np.fmax(x, F(0)), F(1))


def query_records(q):
    """(q0, f1, f2, qb, qc, qlo, qhi), each [n, 3] float32: the query as a record, its corners and the box of the five
    points q0, q1, q2, qb, qc"""
    q = tris(q)
    with np.errstate(all="ignore"):
        q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
        f1, f2 = q1 - q0, q2 - q0
        qb, qc = q0 + f1, q0 + f2
        qlo = np.fmin(np.fmin(np.fmin(np.fmin(q0, q1), q2), qb), qc)
        qhi = np.fmax(np.fmax(np.fmax(np.fmax(q0, q1), q2), qb), qc)
    assert f1.dtype == F and qb.dtype == F and qlo.dtype == F
    return q0, f1, f2, qb, qc, qlo, qhi


def box_bound(qlo, qhi, lo, hi):
    """e = fmaxf(fmaxf(lo - qhi, qlo - hi), 0) per axis; e.x*e.x + e.y*e.y + e.z*e.z (any broadcastable shapes [..., 3])"""
    with np.errstate(all="ignore"):
        e = np.fmax(np.fmax(lo - qhi, qlo - hi), F(0))
        b = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]
    assert b.dtype == F
    return b


def edge_pair(p1, d1, p2, d2, qlo, qhi, tlo, thi):
    """the closest pair of the segments (p1, d1), (p2, d2), clamped into the two boxes -> (D [p], c1 [p, 3], c2 [p, 3])"""
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        r = p1 - p2
        A, E, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
        c, B = _dot(d1, r), _dot(d1, d2)
        den = A * E - B * B
        s = np.where(den > zero, clamp01((B * f - c * E) / den), zero)
        t = (B * s + f) / E
        s = np.where(t < zero, clamp01(-c / A), np.where(t > one, clamp01((B - c) / A), s))
        t = clamp01(t)
        assert s.dtype == F and t.dtype == F and den.dtype == F
        c1 = p1 + d1 * s[:, None]
        c2 = p2 + d2 * t[:, None]
        c1 = np.fmin(np.fmax(c1, qlo), qhi)
        c2 = np.fmin(np.fmax(c2, tlo), thi)
        df = c1 - c2
        D = _dot(df, df)
    assert D.dtype == F and c1.dtype == F and c2.dtype == F
    return D, c1, c2


def pair_eval(q, Q, rec, qi, ti):
    """D, the pair of points and the kind for the pairs (query qi[p], triangle ti[p]) ->
    (D [p] float32, on_query [p, 3], on_mesh [p, 3], kind [p] int32)"""
    a, e1, e2, b, c, tlo, thi = (x[ti] for x in rec)
    q0, f1, f2, qb, qc, qlo, qhi = (x[qi] for x in Q)
    n = len(qi)
    D = np.full(n, np.inf, F)
    pq, pm = q0.copy(), a.copy()
    kind = np.full(n, -1, np.int32)

    def offer(d, cq, cm, k):
        nonlocal D, pq, pm, kind
        with np.errstate(invalid="ignore"):
            w = d < D
        D = np.where(w, d, D)
        pq = np.where(w[:, None], cq, pq)
        pm = np.where(w[:, None], cm, pm)
        kind = np.where(w, np.int32(k), kind)

    for k, v in enumerate((q0, qb, qc)):
        d, P, _ = sweep_ref.near(v, a, e1, e2)
        offer(d, v, P, k)
    for k, v in enumerate((a, b, c)):
        d, P, _ = sweep_ref.near(v, q0, f1, f2)
        offer(d, P, v, 3 + k)
    with np.errstate(all="ignore"):
        f3, e3 = f2 - f1, e2 - e1
    for i, (p1, d1) in enumerate(((q0, f1), (q0, f2), (qb, f3))):
        for j, (p2, d2) in enumerate(((a, e1), (a, e2), (b, e3))):
            d, c1, c2 = edge_pair(p1, d1, p2, d2, qlo, qhi, tlo, thi)
            offer(d, c1, c2, 6 + 3 * i + j)
    # the crossing: rt_cut_triangles' X on the raw corners (its gate on the raw corner box, then steps 2..6)
    rlo, rhi = cut_ref.corner_boxes(q[qi])
    with np.errstate(invalid="ignore"):
        g = ((tlo <= rhi) & (thi >= rlo)).all(axis=1)
    gi = np.flatnonzero(g)
    if len(gi):
        X, s0, _ = cut_ref.steps26(q, rec, qi[gi], ti[gi])
        gi, s0 = gi[X], s0[X]
        D[gi] = F(0)
        pq[gi] = s0
        pm[gi] = s0
        kind[gi] = 15
    assert D.dtype == F and pq.dtype == F and pm.dtype == F
    return D, pq, pm, kind


def _neg(x):
    bits = x.view(np.int32)
    return (bits < 0) & ((bits & 0x7FFFFFFF) != 0)


def valid_queries(q, md):
    """not (a non-finite corner; a NaN or negative bound). The sign is read from the bits, as sweep_ref does."""
    return valid_tris(q) & ~np.isnan(md) & ~_neg(md)


def expected(q, coords, max_dist2=None, prune=True, chunk=32, counts=False):
    """(tri [n] int32, d2 [n] float32, on_query [n, 3], on_mesh [n, 3] float32, kind [n] int32, ties [n] int64) as
    rt_clearance_triangles fills them: the first triangle by (D, index) with D <= fminf(max_dist2, FLT_MAX); -1 /
    FLT_MAX / q0's bits twice / -1 for the empty set. ties: the number of members of S_i whose D equals the answer's.
    prune: skip a pair whose record-box bound exceeds the smallest D found so far for its query (pairs are taken in
    rounds of the 8, 64, 512 smallest bounds, then all). counts=True appends the number of pairs evaluated and of
    pairs whose bound exceeded their D (which must be 0)."""
    q = tris(q)
    n, m = len(q), len(coords)
    md = np.full(n, np.inf, F) if max_dist2 is None else np.ascontiguousarray(max_dist2, F).reshape(n)
    rec = records(coords)
    Q = query_records(q)
    ok = valid_queries(q, md)
    bound = np.fmin(md, FMAX)
    tri = np.full(n, -1, np.int32)
    d2 = np.full(n, FMAX, F)
    on_q, on_m = q[:, 0].copy(), q[:, 0].copy()
    kind = np.full(n, -1, np.int32)
    ties = np.zeros(n, np.int64)
    evaluated = above = 0
    empty_key = np.uint64(0xFFFFFFFFFFFFFFFF)
    for s in range(0, n, chunk):
        rows = np.flatnonzero(ok[s:s + chunk]) + s
        if not len(rows):
            continue
        k = len(rows)
        B = box_bound(Q[5][rows, None, :], Q[6][rows, None, :], rec[5][None], rec[6][None])  # [k, m]
        order = np.argsort(B, axis=1, kind="stable") if prune else None
        key = np.full(k, empty_key, np.uint64)
        bq, bm = on_q[rows].copy(), on_m[rows].copy()
        bk = np.full(k, -1, np.int32)
        lim = bound[rows].copy()
        done = np.zeros((k, m), bool)
        allD = np.full((k, m), np.nan, F)
        for width in ((8, 64, 512, m) if prune else (m,)):
            width = min(width, m)
            take = np.zeros((k, m), bool)
            if prune:
                np.put_along_axis(take, order[:, :width], True, axis=1)
                with np.errstate(invalid="ignore"):
                    take &= ~(B > lim[:, None])
            else:
                take[:] = True
            take &= ~done
            done |= take
            ri, ti = np.nonzero(take)
            if not len(ri):
                continue
            D, pq, pm, kd = pair_eval(q, Q, rec, rows[ri], ti)
            evaluated += len(ri)
            with np.errstate(invalid="ignore"):
                above += int((B[ri, ti] > D).sum())
                member = D <= bound[rows[ri]]
            allD[ri, ti] = D
            pk = np.where(member, (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64),
                          empty_key)
            first = np.nonzero(np.diff(ri, prepend=-1))[0]
            best = np.minimum.reduceat(pk, first)
            at = first + np.array([np.argmin(pk[a:b]) for a, b in zip(first, list(first[1:]) + [len(pk)])])
            r = ri[first]
            better = best < key[r]
            r, at, best = r[better], at[better], best[better]
            key[r] = best
            bq[r], bm[r], bk[r] = pq[at], pm[at], kd[at]
            lim[r] = (best >> np.uint64(32)).astype(np.uint32).view(F)
            if width == m:
                break
        got = key != empty_key
        g = rows[got]
        tri[g] = (key[got] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        d2[g] = (key[got] >> np.uint64(32)).astype(np.uint32).view(F)
        on_q[g], on_m[g], kind[g] = bq[got], bm[got], bk[got]
        ties[g] = (allD[got].view(np.uint32) == d2[g].view(np.uint32)[:, None]).sum(axis=1)
    out = tri, d2, on_q, on_m, kind, ties
    return out + (evaluated, above) if counts else out


# ------------------------------------------------------------------ the fixture's generator
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _hull_queries(c, ext, k_plates, k_edges, rng):
    """queries outside the mesh's convex hull, so that none crosses it and the closest pair is known by construction.
    For a random direction d the vertex v that is extreme along d has nothing of the mesh beyond it:
      plates  a triangle in the plane through v + h d perpendicular to d, centred over v: the closest pair is (the
              plate's interior, the mesh corner v): kinds 3..5;
      edges   with v2 the neighbour of v (a corner of a triangle that holds v) that is highest along d, d is turned
              perpendicular to the edge v v2; the query has one edge crossing over the middle of v v2 at height h, at
              right angles to it, and its third corner further out: where v v2 is an edge of the hull the closest pair
              is the two edges' interiors: kinds 6..14.
    h is 0.1 .. 2 % of the extent, the sizes 1 .. 5 %."""
    v = c.reshape(-1, 3)
    out = []
    for k, edges in ((k_plates, False), (k_edges, True)):
        d = _unit(rng.normal(0, 1, (k, 3)))
        top = np.argmax(d @ v.T, axis=1)
        p = v[top]
        h = ext * rng.uniform(0.001, 0.02, k)
        s = ext * rng.uniform(0.01, 0.05, k)
        if edges:
            mid = p.copy()
            for i in range(k):
                nb = c[top[i] // 3]
                nb = nb[np.any(nb != p[i], axis=1)]
                if not len(nb):
                    continue
                p2 = nb[np.argmax(nb @ d[i])]
                e = _unit(p2 - p[i])
                d[i] = _unit(d[i] - (d[i] @ e) * e)
                mid[i] = 0.5 * (p[i] + p2)
                p[i] = e  # (the edge's direction, below)
            w = _unit(np.cross(p, d))
            at = mid + h[:, None] * d
            jit = rng.uniform(-0.2, 0.2, (k, 1)) * s[:, None]
            q = np.stack([at - (s[:, None] + jit) * w, at + (s[:, None] - jit) * w,
                          at + s[:, None] * d + rng.normal(0, 0.3, (k, 3)) * s[:, None]], axis=1)
        else:
            ax = np.where(np.abs(d[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
            u = _unit(np.cross(d, ax))
            w = np.cross(d, u)
            th = rng.uniform(0, 2 * np.pi, (k, 1)) + np.array([0, 2, 4]) * np.pi / 3 + rng.normal(0, 0.2, (k, 3))
            ctr = p + h[:, None] * d
            q = ctr[:, None, :] + s[:, None, None] * (np.cos(th)[:, :, None] * u[:, None, :] +
                                                      np.sin(th)[:, :, None] * w[:, None, :])
        out.append(q)
    return out


def fixture_tris(coords, n, seed):
    """n query triangles (n a multiple of 16) -> [n, 3, 3] float32. The issue's four kinds, three sixteenths of n each
    but the last with two:
      1. cut_ref.surface_tris: at the surface, most of them crossing it;
      2. the same lifted along a random direction by 0.1 .. 5 % of the extent;
      3. centres uniform in the scene's box grown by a quarter, sizes 1 .. 10 % of the extent;
      4. mesh triangles themselves (every other one) and triangles that share one mesh vertex;
    and, because on these meshes those four give a mesh corner or an edge pair as the closest feature in only 3 .. 12 %
    of the queries (a car's surface is in layers: nearly everything near it crosses something),
      5. _hull_queries: plates over the hull's vertices and queries across the hull's edges, five sixteenths of n."""
    assert n % 16 == 0
    rng = np.random.default_rng(seed)
    c = np.asarray(coords, np.float64)
    ext = scene_extent(coords)
    k = 3 * n // 16
    a = cut_ref.surface_tris(coords, k, seed + 1).astype(np.float64)
    b = cut_ref.surface_tris(coords, k, seed + 2).astype(np.float64)
    d = _unit(rng.normal(0, 1, (k, 3)))
    b = b + (d * (ext * 10.0 ** rng.uniform(-3, np.log10(0.05), k))[:, None])[:, None, :]
    v = c.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    grow = 0.25 * (hi - lo)
    ctr = rng.uniform(lo - grow, hi + grow, (k, 3))
    off = rng.normal(0, 1, (k, 3, 3))
    off -= off.mean(axis=1, keepdims=True)
    u = ctr[:, None, :] + (ext * 10.0 ** rng.uniform(-2, -1, k))[:, None, None] * off
    last = n // 8
    t = rng.integers(0, len(c), last)
    own = c[t].copy()
    shared = np.arange(last) % 2 == 1  # one mesh vertex kept, the other two corners random around it
    apex = own[np.arange(last), rng.integers(0, 3, last)]
    away = apex[:, None, :] + (ext * 10.0 ** rng.uniform(-2.5, -1.3, last))[:, None, None] * rng.normal(0, 1, (last, 3, 3))
    away[:, 0] = apex
    own = np.where(shared[:, None, None], away, own)
    hull = n - 3 * k - last
    plates, edges = _hull_queries(c, ext, hull // 2, hull - hull // 2, rng)
    return np.ascontiguousarray(np.concatenate([a, b, u, own, plates, edges]).astype(F))
