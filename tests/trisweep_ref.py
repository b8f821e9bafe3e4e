"""The triangle sweep query's yardstick (rt_sweep_triangles, include/rt_hip.h): a numpy float32 restatement of
toi(query, record), the contact point and the winning candidate as the header states them. Every operation is one
float32 operation in the stated order (dot = x*x + y*y + z*z left to right, nothing fused), on what a triangle record
holds: a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0), and on the query made a record the same way. fminf / fmaxf are
np.fmin / np.fmax (a NaN operand loses); a comparison with a NaN operand is false, in numpy as in C.

The records are tests/overlap_ref.py's, the query records and the five-point box tests/clearance_ref.py's, the start in
contact is tests/cut_ref.py's gate and steps26 (rt_cut_triangles' X and its segment): all called, not restated. New here are the box-against-box slab gate, the
ray-triangle function of candidates 0..5 and the edge-edge time of candidates 6..14.

The gate is evaluated for every (query, triangle) pair, in chunks of queries; the rest only for the pairs that pass
it, as flat arrays (tests/sweep_ref.py's scheme). A query's answer is the first triangle by (toi, original index).

toi64 is geometry's answer: the same fifteen candidates and the same crossing test in float64 on the vertices
themselves, measured from t = 0, with no gate."""
import numpy as np

from tests import clearance_ref, cut_ref, nearest_ref, overlap_ref, sweep_ref

F = np.float32
FMAX = nearest_ref.FMAX
same_bits = nearest_ref.same_bits
records = overlap_ref.records
scene_extent = overlap_ref.scene_extent
tris = cut_ref.tris
query_records = clearance_ref.query_records
X = cut_ref.steps26
_dot = sweep_ref._dot
_cross = cut_ref.cross


def _neg(x):
    bits = x.view(np.int32)
    return (bits < 0) & ((bits & 0x7FFFFFFF) != 0)


def valid_queries(q, d, tm):
    """not (a non-finite corner or motion; a NaN or negative t_max). The sign is read from the bits, as sweep_ref does."""
    return cut_ref.valid_tris(q) & np.isfinite(d).all(axis=1) & ~np.isnan(tm) & ~_neg(tm)


def gate(qlo, qhi, d, T, tlo, thi):
    """step 2 for every pair -> (open [queries, triangles] bool, t0 [queries, triangles] float32)"""
    n, m = len(qlo), len(tlo)
    t0 = np.zeros((n, m), F)
    t1 = np.broadcast_to(T[:, None], (n, m)).astype(F)
    ok = np.ones((n, m), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            lo, hi = tlo[None, :, k], thi[None, :, k]
            ql, qh, dk = qlo[:, k, None], qhi[:, k, None], d[:, k, None]
            z = (dk.view(np.int32) & 0x7FFFFFFF) == 0  # (d.k == 0 read from the bits: a subnormal is not zero)
            inv = F(1) / dk
            ta = (lo - qh) * inv
            tb = (hi - ql) * inv
            assert ta.dtype == F and tb.dtype == F
            t0 = np.where(z, t0, np.fmax(t0, np.fmin(ta, tb)))
            t1 = np.where(z, t1, np.fmin(t1, np.fmax(ta, tb)))
            ok &= ~z | ((ql <= hi) & (lo <= qh))
        ok &= t0 <= t1
    assert t0.dtype == F and t1.dtype == F
    return ok, t0


def ray_tri(o, dr, a, e1, e2):
    """the ray o + u dr against the record (a, e1, e2): closed barycentric bounds, det != 0, u >= 0, no EPSILON culls
    -> (u [p] float32, valid [p] bool)"""
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        h = _cross(dr, e2)
        det = _dot(e1, h)
        inv = one / det
        s = o - a
        bu = _dot(s, h) * inv
        qv = _cross(s, e1)
        bv = _dot(dr, qv) * inv
        u = _dot(e2, qv) * inv
        valid = (det != zero) & (bu >= zero) & (bv >= zero) & (bu + bv <= one) & (u >= zero)
    assert u.dtype == F and bu.dtype == F and bv.dtype == F
    return u, valid


def edge_time(p, f, m, e, d):
    """query edge (p, f) moving along d against mesh edge (m, e) -> (u [p], the mesh-side point [p, 3], valid [p])"""
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        n = _cross(f, e)
        nn = _dot(n, n)
        dn = _dot(d, n)
        w0 = m - p
        u = _dot(w0, n) / dn
        rn = one / nn
        w = w0 - d * u[:, None]
        s = _dot(_cross(w, e), n) * rn
        t = _dot(_cross(w, f), n) * rn
        valid = (nn > zero) & (dn != zero) & (u >= zero) & (s >= zero) & (s <= one) & (t >= zero) & (t <= one)
        c2 = m + e * t[:, None]
    assert u.dtype == F and s.dtype == F and t.dtype == F and c2.dtype == F
    return u, c2, valid


def pair_eval(q, d, Q, rec, qi, ti, t0):
    """toi, the contact point and the kind for the pairs (query qi[p], triangle ti[p]) that passed the gate at t0[p]
    -> (toi [p] float32 (+inf: no candidate), point [p, 3], kind [p] int32)"""
    a, e1, e2, b, c, tlo, thi = (x[ti] for x in rec)
    q0, f1, f2, qb, qc, qlo, qhi = (x[qi] for x in Q)
    dq = d[qi]
    n = len(qi)
    with np.errstate(all="ignore"):
        sh = dq * t0[:, None]  # 3. recentre
        r0, rb, rc = q0 + sh, qb + sh, qc + sh
        raw = np.stack([r0, q[qi, 1] + sh, q[qi, 2] + sh], axis=1)
        nd = -dq
    assert r0.dtype == F and raw.dtype == F
    u = np.full(n, np.inf, F)
    pt = a.copy()
    kind = np.full(n, -1, np.int32)

    def offer(cu, valid, cp, k):
        nonlocal u, pt, kind
        with np.errstate(invalid="ignore"):
            w = valid & (cu < u)
        u = np.where(w, cu, u)
        pt = np.where(w[:, None], cp, pt)
        kind = np.where(w, np.int32(k), kind)

    for k, o in enumerate((r0, rb, rc)):  # 0..2
        cu, valid = ray_tri(o, dq, a, e1, e2)
        with np.errstate(all="ignore"):
            offer(cu, valid, o + dq * cu[:, None], k)
    for k, v in enumerate((a, b, c)):  # 3..5
        cu, valid = ray_tri(v, nd, r0, f1, f2)
        offer(cu, valid, v, 3 + k)
    with np.errstate(all="ignore"):
        f3, e3 = f2 - f1, e2 - e1
    for i, (p1, d1) in enumerate(((r0, f1), (r0, f2), (rb, f3))):  # 6..14
        for j, (p2, d2) in enumerate(((a, e1), (a, e2), (b, e3))):
            cu, cp, valid = edge_time(p1, d1, p2, d2, dq)
            offer(cu, valid, cp, 6 + 3 * i + j)
    with np.errstate(all="ignore"):
        toi = t0 + u
    # 4. a start in contact: rt_cut_triangles' X on the recentred raw corners (its gate on their box, then steps 2..6)
    clo, chi = cut_ref.corner_boxes(raw)
    with np.errstate(invalid="ignore"):
        g = ((tlo <= chi) & (thi >= clo)).all(axis=1)
    gi = np.flatnonzero(g)
    if len(gi):
        ar = np.arange(len(gi))
        hit, s0, _ = X(raw[gi], [x[gi] for x in (a, e1, e2, b, c)], ar, ar)
        gi, s0 = gi[hit], s0[hit]
        toi[gi] = t0[gi]
        pt[gi] = s0
        kind[gi] = 15
    with np.errstate(invalid="ignore"):
        pt = np.fmin(np.fmax(pt, tlo), thi)
    assert toi.dtype == F and pt.dtype == F
    return toi, pt, kind


def _inputs(q, motion, t_max):
    q = tris(q)
    n = len(q)
    d = np.ascontiguousarray(motion, F).reshape(-1, 3)
    tm = np.full(n, np.inf, F) if t_max is None else np.ascontiguousarray(t_max, F).reshape(n)
    assert len(d) == n
    return q, d, tm


def pairs(q, motion, coords, t_max=None, chunk=64):
    """(qi, ti, toi, point, kind): the pairs that pass the gate in (query, triangle) order; invalid queries have
    none. Membership of S_i is toi <= fminf(t_max, FLT_MAX)."""
    q, d, tm = _inputs(q, motion, t_max)
    rec = records(coords)
    Q = query_records(q)
    ok = valid_queries(q, d, tm)
    T = np.fmin(tm, FMAX)
    out = [[] for _ in range(5)]
    for s in range(0, len(q), chunk):
        sl = slice(s, s + chunk)
        g, t0 = gate(Q[5][sl], Q[6][sl], d[sl], T[sl], rec[5], rec[6])
        g &= ok[sl, None]
        qi, ti = np.nonzero(g)
        t0 = t0[qi, ti]
        qi += s
        toi, pt, kind = pair_eval(q, d, Q, rec, qi, ti, t0)
        for o, x in zip(out, (qi, ti, toi, pt, kind)):
            o.append(x)
    if not out[0]:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, F), np.zeros((0, 3), F), np.zeros(0, np.int32)
    return tuple(np.concatenate(x) for x in out)


def expected(q, motion, coords, t_max=None, chunk=64):
    """(tri [n] int32, t [n] float32, point [n, 3] float32, kind [n] int32, ties [n] int64) as rt_sweep_triangles fills
    them: the first triangle by (toi, index) with toi <= fminf(t_max, FLT_MAX); -1 / FLT_MAX / q0's bits / -1 for the
    empty set. ties: the number of members of S_i whose toi equals the answer's (0 for the empty set)."""
    q, d, tm = _inputs(q, motion, t_max)
    n = len(q)
    qi, ti, toi, pt, kd = pairs(q, d, coords, tm, chunk)
    T = np.fmin(tm, FMAX)
    with np.errstate(invalid="ignore"):
        member = toi <= T[qi]
    qi, ti, toi, pt, kd = qi[member], ti[member], toi[member], pt[member], kd[member]
    tri = np.full(n, -1, np.int32)
    t = np.full(n, FMAX, F)
    point = q[:, 0].copy()
    kind = np.full(n, -1, np.int32)
    ties = np.zeros(n, np.int64)
    if len(qi):
        # toi >= +0, so its bits order as the floats do: one key per pair, the least per query
        key = (toi.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64)
        first = np.nonzero(np.diff(qi, prepend=-1))[0]
        best = np.minimum.reduceat(key, first)
        at = np.flatnonzero(key == np.repeat(best, np.diff(np.append(first, len(key)))))  # (keys of a query are unique)
        rows = qi[first]
        assert len(at) == len(rows)
        tri[rows] = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
        t[rows] = (best >> np.uint64(32)).astype(np.uint32).view(F)
        point[rows] = pt[at]
        kind[rows] = kd[at]
        np.add.at(ties, qi[toi.view(np.uint32) == t[qi].view(np.uint32)], 1)
    return tri, t, point, kind, ties


# ------------------------------------------------------------------ geometry's answer, in float64
def _dot64(u, v):
    return (u * v).sum(axis=-1)


def _ray_tri64(o, dr, a, e1, e2):
    with np.errstate(all="ignore"):
        h = np.cross(dr, e2)
        det = _dot64(e1, h)
        s = o - a
        bu = _dot64(s, h) / det
        qv = np.cross(s, e1)
        bv = _dot64(dr, qv) / det
        u = _dot64(e2, qv) / det
        ok = (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (u >= 0)
    return np.where(ok, u, np.inf)


def _edge64(p, f, m, e, d):
    with np.errstate(all="ignore"):
        n = np.cross(f, e)
        nn = _dot64(n, n)
        dn = _dot64(d, n)
        w0 = m - p
        u = _dot64(w0, n) / dn
        w = w0 - d * u[:, None]
        s = _dot64(np.cross(w, e), n) / nn
        t = _dot64(np.cross(w, f), n) / nn
        ok = (nn > 0) & (dn != 0) & (u >= 0) & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    return np.where(ok, u, np.inf)


def _seg_hits_tri64(p, d, tri):
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(all="ignore"):
        h = np.cross(d, e2)
        det = _dot64(e1, h)
        s = p - tri[:, 0]
        u = _dot64(s, h) / det
        qv = np.cross(s, e1)
        v = _dot64(d, qv) / det
        t = _dot64(e2, qv) / det
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= 1)


def toi64(q, d, m):
    """the float64 time of impact of the pairs (query q[p] [p, 3, 3] moving along d[p], triangle m[p] [p, 3, 3]) from
    t = 0 -> [p] float64, +inf where there is none: 0 when an edge of one crosses the other now, else the least of the
    fifteen candidates. No gate."""
    q, d, m = (np.asarray(x, np.float64) for x in (q, d, m))
    u = np.full(len(q), np.inf)
    e1, e2 = m[:, 1] - m[:, 0], m[:, 2] - m[:, 0]
    f1, f2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
    for k in range(3):
        u = np.minimum(u, _ray_tri64(q[:, k], d, m[:, 0], e1, e2))
        u = np.minimum(u, _ray_tri64(m[:, k], -d, q[:, 0], f1, f2))
    for i in range(3):
        for j in range(3):
            u = np.minimum(u, _edge64(q[:, i], q[:, (i + 1) % 3] - q[:, i], m[:, j], m[:, (j + 1) % 3] - m[:, j], d))
    hit = np.zeros(len(q), bool)
    for i in range(3):
        hit |= _seg_hits_tri64(q[:, i], q[:, (i + 1) % 3] - q[:, i], m)
        hit |= _seg_hits_tri64(m[:, i], m[:, (i + 1) % 3] - m[:, i], q)
    return np.where(hit, 0.0, u)


def gate64(q, d, coords, until):
    """the (query, triangle) pairs whose float64 boxes meet at some time in [0, until[query]] (a contact needs that),
    with a relative slack of 1e-9 -> (qi, ti)"""
    q, d, c = (np.asarray(x, np.float64) for x in (q, d, coords))
    tlo, thi = c.min(axis=1), c.max(axis=1)
    qlo, qhi = q.min(axis=1), q.max(axis=1)
    slack = 1e-9 * max(np.abs(c).max(), np.abs(q[np.isfinite(q)]).max() if np.isfinite(q).any() else 0.0)
    qis, tis = [], []
    for i in range(len(q)):
        t0, t1 = np.zeros(len(c)), np.full(len(c), float(until[i]))
        ok = np.ones(len(c), bool)
        with np.errstate(all="ignore"):
            for k in range(3):
                lo, hi = tlo[:, k] - qhi[i, k] - slack, thi[:, k] - qlo[i, k] + slack
                if d[i, k] == 0:
                    ok &= (lo <= 0) & (hi >= 0)
                else:
                    ta, tb = lo / d[i, k], hi / d[i, k]
                    t0 = np.maximum(t0, np.minimum(ta, tb))
                    t1 = np.minimum(t1, np.maximum(ta, tb))
            ok &= t0 <= t1
        ti = np.flatnonzero(ok)
        qis.append(np.full(len(ti), i))
        tis.append(ti)
    return np.concatenate(qis), np.concatenate(tis)


# ------------------------------------------------------------------ the fixture's generator
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _hull_aimed(c, ext, k, rng):
    """k queries that meet the mesh's convex hull from outside -> (tris [k, 3, 3], motion [k, 3]) float64. For a
    random direction w the vertex v that is extreme along w has nothing of the mesh beyond it. Even rows: a plate in
    the plane through v perpendicular to w, centred over v, so that the mesh corner v meets the plate's interior
    (kinds 3..5). Odd rows: with v2 the neighbour of v that is highest along w, w is turned perpendicular to the edge
    v v2 and the query's first edge crosses over the middle of v v2 at right angles, its third corner further out
    (kinds 6..14 where v v2 is an edge of the hull). Both are lifted along w by 0.1 .. 1 extent and move back along
    -w, touching at t = 1/2 .. 1."""
    v = c.reshape(-1, 3)
    w = _unit(rng.normal(0, 1, (k, 3)))
    top = np.argmax(w @ v.T, axis=1)
    p = v[top].copy()
    s = ext * rng.uniform(0.01, 0.05, k)
    q = np.zeros((k, 3, 3))
    for i in range(k):
        if i % 2:
            nb = c[top[i] // 3]
            nb = nb[np.any(nb != p[i], axis=1)]
            p2 = nb[np.argmax(nb @ w[i])] if len(nb) else p[i] + [ext * 1e-3, 0, 0]
            e = _unit(p2 - p[i])
            w[i] = _unit(w[i] - (w[i] @ e) * e)
            mid, x = 0.5 * (p[i] + p2), np.cross(e, w[i])
            j = rng.uniform(-0.2, 0.2) * s[i]
            q[i] = [mid - (s[i] + j) * x, mid + (s[i] - j) * x, mid + s[i] * w[i] + rng.normal(0, 0.3, 3) * s[i]]
        else:
            ax = np.array([1.0, 0, 0]) if abs(w[i, 0]) < 0.9 else np.array([0, 1.0, 0])
            x = _unit(np.cross(w[i], ax))
            y = np.cross(w[i], x)
            th = rng.uniform(0, 2 * np.pi) + np.array([0, 2, 4]) * np.pi / 3 + rng.normal(0, 0.2, 3)
            q[i] = p[i] + s[i] * (np.cos(th)[:, None] * x + np.sin(th)[:, None] * y)
    lift = (ext * rng.uniform(0.1, 1.0, k))[:, None] * w
    return q + lift[:, None, :], -lift / rng.uniform(0.5, 1.0, k)[:, None]


def fixture_seeded(coords, n, seed):
    """n seeded query triangles (n a multiple of 8) of 0.05 .. 5 % of the extent with motions of 0.1 .. 2 extents ->
    (tris [n, 3, 3], motion [n, 3]) float32.
      the first eighth   _hull_aimed: mesh corners against plates, edges across hull edges;
      the second eighth  aimed: the motion carries one of the query's own features (its centroid, an edge midpoint, a
                         corner) onto a feature of a random mesh triangle (the same seven) at t = 1/2 .. 1;
      the rest           centres uniform in the scene's box grown by a quarter, motions towards noisy triangle centroids
                         at 1.5 x the distance (clipped to 0.1 .. 2 extents), every fourth motion axis-aligned (two zero
                         components), every eighth query starting at the surface (cut_ref.surface_tris)."""
    assert n % 8 == 0
    rng = np.random.default_rng(seed)
    c = np.asarray(coords, np.float64)
    ext = scene_extent(coords)
    v = c.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    grow = 0.25 * (hi - lo)
    ctr = rng.uniform(lo - grow, hi + grow, (n, 3))
    off = rng.normal(0, 1, (n, 3, 3))
    off -= off.mean(axis=1, keepdims=True)
    size = ext * 10.0 ** rng.uniform(np.log10(5e-4), np.log10(5e-2), n) / 2.0
    q = ctr[:, None, :] + size[:, None, None] * off
    cen = c.mean(axis=1)[rng.integers(0, len(c), n)]
    d = 1.5 * (cen + rng.normal(0, 0.02 * ext, (n, 3)) - ctr)
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    d = d / ln * np.clip(ln, 0.1 * ext, 2.0 * ext)
    ax = np.arange(n) % 4 == 3
    keep = np.zeros((n, 3), bool)
    keep[np.arange(n), np.abs(d).argmax(axis=1)] = True
    d = np.where(ax[:, None] & ~keep, 0.0, d)
    at = np.arange(n)[::8]
    q[at] = cut_ref.surface_tris(coords, len(at), seed + 1)
    k = n // 8
    q[:k], d[:k] = _hull_aimed(c, ext, k, rng)
    t = c[rng.integers(0, len(c), k)]

    def feats(x):
        return np.stack([x.mean(axis=1), 0.5 * (x[:, 0] + x[:, 1]), 0.5 * (x[:, 1] + x[:, 2]),
                         0.5 * (x[:, 2] + x[:, 0]), x[:, 0], x[:, 1], x[:, 2]], axis=1)
    target = feats(t)[np.arange(k), rng.integers(0, 7, k)]
    source = feats(q[k:2 * k])[np.arange(k), rng.integers(0, 7, k)]
    d[k:2 * k] = (target - source) / rng.uniform(0.5, 1.0, k)[:, None]
    return np.ascontiguousarray(q.astype(F)), np.ascontiguousarray(d.astype(F))


def fixture_camera(coords, o, p):
    """one query triangle at every ray (o, p): centred 2 % of the extent down the ray, 0.2 .. 2 % of the extent in
    size, across the ray, moving along it -> (tris [n, 3, 3], motion [n, 3]) float32"""
    n = len(o)
    o, p = np.asarray(o, np.float64), np.asarray(p, np.float64)
    ext = scene_extent(coords)
    w = _unit(p)
    ax = np.where(np.abs(w[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    u = _unit(np.cross(w, ax))
    v = np.cross(w, u)
    size = ext * 10.0 ** np.linspace(np.log10(2e-3), np.log10(2e-2), n)
    th = (np.arange(n) * 0.37)[:, None] + np.array([0, 2, 4]) * np.pi / 3
    ctr = o + 0.02 * ext * w
    q = ctr[:, None, :] + size[:, None, None] * (np.cos(th)[:, :, None] * u[:, None, :] +
                                                  np.sin(th)[:, :, None] * v[:, None, :])
    return np.ascontiguousarray(q.astype(F)), np.ascontiguousarray(p.astype(F))


NS, NC = 512, 128  # the fixture's seeded and camera queries
CAM_W, CAM_H = 64, 36
SEED = {"car_boxed": 41, "car_only": 42}  # chosen on the CPU: the yardstick alone meets check_fixture below


def fixture(coords, seed):
    """the NS + NC fixture queries of a scene -> (tris [N, 3, 3], motion [N, 3]) float32: fixture_seeded, then
    fixture_camera on NC rays of the CAM_W x CAM_H reference camera"""
    from prt import host, rays
    q, d = fixture_seeded(coords, NS, seed)
    o, p = rays.pinhole(host.camera(CAM_W, CAM_H), CAM_W, CAM_H, device="cpu")
    rows = np.arange(NC) * ((CAM_W * CAM_H) // NC) + 7
    cq, cd = fixture_camera(coords, o.numpy()[rows], p.numpy()[rows])
    return np.concatenate([q, cq]), np.concatenate([d, cd])


def check_fixture(want):
    """what the fixture must hold, from the yardstick's answers -> the figures, for printing"""
    tri, t, _, kind, ties = want
    n = len(tri)
    found = tri >= 0
    groups = [int(((kind >= a) & (kind <= b)).sum()) for a, b in ((0, 2), (3, 5), (6, 14), (15, 15))]
    fig = dict(found=int(found.sum()), empty=int((~found).sum()), ties=int((ties > 1).sum()), kinds=groups)
    assert fig["found"] >= n // 2 and fig["empty"] >= 16 and fig["ties"] >= 8, fig
    assert min(groups) >= 8, fig
    return fig


def domain(q, d, mx):
    """the queries the walk serves (rt_trisweep.hpp tsw_domain): every nonzero |d.k| in [2^-64, 2^64] and every |q.k| at
    most 2^20 mx; the others run the exhaustive loop under either kernel"""
    ad = np.abs(d)
    ok = ((ad == 0) | ((ad >= F(2.0 ** -64)) & (ad <= F(2.0 ** 64)))).all(axis=1)
    return ok & (np.abs(tris(q)).reshape(-1, 9).max(axis=1) <= np.ldexp(F(mx), 20))
