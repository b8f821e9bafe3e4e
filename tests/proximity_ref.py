"""The proximity query's yardstick (rt_proximity_triangles, include/rt_hip.h): lists, counts and CSR sets over
tests/clearance_ref.py's D, pair of points and kind. Nothing of the pair function is restated here: pair_eval,
box_bound, records, query_records and valid_queries are clearance_ref's own.

Query i's candidate set is S_i = { j : D(q_i, j) <= fminf(max_dist2[i], FLT_MAX) } in (D, index) order. members() finds,
per query, every member that can matter: all of S_i (k=None: counts and CSR sets), or with a list of k the members up
to and including every tie at the k-th D. With prune=True it evaluates a pair only when its record-box bound does not
exceed the query's current limit -- its bound, then the k-th smallest D found so far -- in rounds of the 64, 512, 4096
smallest bounds, then all, as clearance_ref.expected does; prune=False evaluates every pair. It counts the pairs
evaluated and those whose bound exceeded their D, which must be 0: that is what makes the pruned form complete.
tests/test_proximity_abi.py holds the two forms against each other bit for bit."""
import numpy as np

from tests import clearance_ref as cr

F = np.float32
FMAX = cr.FMAX
same_bits = cr.same_bits
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def key_d2(key):
    return (key >> np.uint64(32)).astype(np.uint32).view(F)


def key_tri(key):
    return (key & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)


def members(q, coords, max_dist2=None, k=None, prune=True, chunk=32):
    """(keys, evaluated, above): keys[i] is a sorted uint64 array of D_bits << 32 | index over the members of S_i found
    (all of them with k=None; with a list of k at least the first k and every tie at the k-th D). evaluated: pairs
    evaluated; above: those whose record-box bound exceeded their D."""
    q = cr.tris(q)
    n, m = len(q), len(coords)
    md = np.full(n, np.inf, F) if max_dist2 is None else np.ascontiguousarray(max_dist2, F).reshape(n)
    rec = cr.records(coords)
    Q = cr.query_records(q)
    ok = cr.valid_queries(q, md)
    bound = np.fmin(md, FMAX)
    keys = [np.zeros(0, np.uint64)] * n
    evaluated = above = 0
    for s in range(0, n, chunk):
        rows = np.flatnonzero(ok[s:s + chunk]) + s
        if not len(rows):
            continue
        r = len(rows)
        B = cr.box_bound(Q[5][rows, None, :], Q[6][rows, None, :], rec[5][None], rec[6][None])  # [r, m]
        order = np.argsort(B, axis=1, kind="stable") if prune else None
        K = np.full((r, m), EMPTY, np.uint64)
        lim = bound[rows].copy()
        done = np.zeros((r, m), bool)
        for width in ((64, 512, 4096, m) if prune else (m,)):
            width = min(width, m)
            take = np.zeros((r, m), bool)
            if prune:
                np.put_along_axis(take, order[:, :width], True, axis=1)
                with np.errstate(invalid="ignore"):
                    take &= ~(B > lim[:, None])
            else:
                take[:] = True
            take &= ~done
            done |= take
            ri, ti = np.nonzero(take)
            if len(ri):
                D = cr.pair_eval(q, Q, rec, rows[ri], ti)[0]
                evaluated += len(ri)
                with np.errstate(invalid="ignore"):
                    above += int((B[ri, ti] > D).sum())
                    member = D <= bound[rows[ri]]
                K[ri[member], ti[member]] = (D[member].view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
                    ti[member].astype(np.uint64)
                if k is not None and k > 0 and k <= m:  # the list's limit: the k-th smallest key's D once there are k
                    kth = np.partition(K, k - 1, axis=1)[:, k - 1]
                    full = kth != EMPTY
                    lim[full] = np.fmin(lim[full], key_d2(kth[full]))
            if width == m:
                break
        for j, row in enumerate(rows):
            kk = K[j][K[j] != EMPTY]
            kk.sort()
            keys[row] = kk
    return keys, evaluated, above


def lists(q, coords, k, max_dist2=None, prune=True, count_all=False, counts=False):
    """(tri [n, k] int32, d2 [n, k] float32, on_query [n, k, 3], on_mesh [n, k, 3] float32, kind [n, k] int32, count [n]
    int32, tied [n] bool) as rt_proximity_triangles fills them: the first k of S_i; -1 / FLT_MAX / q0's bits twice / -1
    in the unused slots; count = min(|S_i|, k), or |S_i| with count_all (every member is then found: the limit is the
    bound alone). tied: the k-th and the (k+1)-th member share their D's bits. counts=True appends (evaluated, above)."""
    q = cr.tris(q)
    n = len(q)
    keys, evaluated, above = members(q, coords, max_dist2, None if count_all else k, prune)
    tri = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), FMAX, F)
    on_q = np.repeat(q[:, None, 0, :], k, axis=1).copy()
    on_m = on_q.copy()
    kind = np.full((n, k), -1, np.int32)
    count = np.zeros(n, np.int32)
    tied = np.zeros(n, bool)
    for i, kk in enumerate(keys):
        c = min(len(kk), k)
        tri[i, :c] = key_tri(kk[:c])
        d2[i, :c] = key_d2(kk[:c])
        count[i] = len(kk) if count_all else c
        tied[i] = k > 0 and len(kk) > k and (kk[k] >> np.uint64(32)) == (kk[k - 1] >> np.uint64(32))
    qi, slot = np.nonzero(tri >= 0)
    if len(qi):  # the stored pairs' points and kinds: the pair function again (D depends on no limit)
        D, pq, pm, kd = cr.pair_eval(q, cr.query_records(q), cr.records(coords), qi, tri[qi, slot].astype(np.int64))
        assert same_bits(D, d2[qi, slot])
        on_q[qi, slot], on_m[qi, slot], kind[qi, slot] = pq, pm, kd
    out = tri, d2, on_q, on_m, kind, count, tied
    return out + (evaluated, above) if counts else out


def sizes(q, coords, max_dist2, prune=True):
    """|S_i| [n] int64 (a count_all query's count)"""
    return np.array([len(kk) for kk in members(q, coords, max_dist2, None, prune)[0]], np.int64)


def csr(q, coords, max_dist2, prune=True):
    """(offsets [n + 1] int32, tri, d2, on_query, on_mesh, kind over the total): every S_i in (D, index) order, as
    Renderer.proximity_csr returns it"""
    q = cr.tris(q)
    keys = members(q, coords, max_dist2, None, prune)[0]
    offsets = np.zeros(len(q) + 1, np.int32)
    offsets[1:] = np.cumsum([len(kk) for kk in keys])
    allk = np.concatenate(keys) if len(keys) else np.zeros(0, np.uint64)
    tri, d2 = key_tri(allk), key_d2(allk)
    qi = np.repeat(np.arange(len(q)), np.diff(offsets))
    if len(qi):
        D, pq, pm, kd = cr.pair_eval(q, cr.query_records(q), cr.records(coords), qi, tri.astype(np.int64))
        assert same_bits(D, d2)
    else:
        pq = pm = np.zeros((0, 3), F)
        kd = np.zeros(0, np.int32)
    return offsets, tri, d2, pq, pm, kd
