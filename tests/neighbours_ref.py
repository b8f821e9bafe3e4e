"""The neighbour query's yardstick (rt_nearest_tris, include/rt_hip.h): tests/nearest_ref.py's D and P over [points,
triangles], in chunks of points; per point a STABLE argsort of D over the triangles -- which is the (D, original index)
order --, of which the triangles inside a bound are a prefix (D <= bound is monotone in D); its first k entries and the
count. The validity rules are nearest_ref.expected's: a NaN or negative bound (read from the bits) and a non-finite
point have the empty set.

table() does the expensive part once per point set (every D, and the order and P of the first KEEP = 17 entries: no
list is longer than 16, and the 17th decides a tie across the cut at k = 16); answer() reads any k, bound and count_all
off it; expected() is the two together."""
import numpy as np

from tests import nearest_ref
from tests.nearest_ref import F, FMAX

KEEP = 17


def table(points, coords, chunk=16, threads=8):
    """(q [n, 3], D [n, triangles] float32, order [n, KEEP] int32: the first KEEP triangles by (D, index) among those
    with a D that is no NaN, -1 beyond them; P [n, KEEP, 3]: their closest points)"""
    from concurrent.futures import ThreadPoolExecutor
    q = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, m = len(q), len(coords)
    keep = min(KEEP, m)
    Dall = np.empty((n, m), F)
    order = np.full((n, KEEP), -1, np.int32)
    Ptop = np.zeros((n, KEEP, 3), F)

    def one(a):
        sl = slice(a, min(a + chunk, n))
        D, P = nearest_ref.dist(q[sl], coords)
        Dall[sl] = D
        o = np.argsort(D, axis=1, kind="stable")[:, :keep]  # (equal D keep the lower index first; NaN sorts last)
        rows = np.arange(D.shape[0])[:, None]
        ok = ~np.isnan(D[rows, o])
        order[sl, :keep] = np.where(ok, o, -1)
        Ptop[sl, :keep] = P[rows, o]

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(0, n, chunk)))
    return q, Dall, order, Ptop


def answer(tab, k, max_dist2=None, count_all=False, stats=False, rows=None):
    """(tri [n, k] int32, d2 [n, k] float32, point [n, k, 3] float32, count [n] int32) as rt_nearest_tris fills them:
    the first k triangles by (D, index) with D <= min(max_dist2, FLT_MAX); -1 / FLT_MAX / the query point's bits in
    unused slots; count = min(|S_i|, k), or |S_i| with count_all. stats=True adds, per point, |S_i| [n] int64 and
    whether D[k - 1] == D[k] in S_i's order, a tie across the cut [n] bool (False where |S_i| <= k or k = 0).
    rows: the points to answer for (indices into the table; default all, in order)."""
    assert 0 <= k < KEEP
    q, Dall, order, Ptop = tab
    if rows is not None:
        q, Dall, order, Ptop = q[rows], Dall[rows], order[rows], Ptop[rows]
    n = len(q)
    md = np.full(n, FMAX, F) if max_dist2 is None else np.asarray(max_dist2, F).reshape(n)
    with np.errstate(invalid="ignore"):
        bits = md.view(np.int32)
        mag = bits & 0x7FFFFFFF
        valid = ~(mag > 0x7F800000) & ~((bits < 0) & (mag != 0)) & np.isfinite(q).all(axis=1)
        bound = np.fmin(md, FMAX)
        size = np.where(valid, (Dall <= bound[:, None]).sum(axis=1), 0).astype(np.int64)
    r = np.arange(n)[:, None]
    Dtop = np.where(order >= 0, Dall[r, np.maximum(order, 0)], F(np.nan))
    used = np.arange(k)[None, :] < size[:, None]
    assert (order[:, :k][used] >= 0).all()
    tri = np.where(used, order[:, :k], -1).astype(np.int32)
    d2 = np.where(used, Dtop[:, :k], FMAX).astype(F)
    point = np.where(used[:, :, None], Ptop[:, :k], q[:, None, :]).astype(F)
    count = (size if count_all else np.minimum(size, k)).astype(np.int32)
    if not stats:
        return tri, d2, point, count
    with np.errstate(invalid="ignore"):
        cut = (size > k) & (Dtop[:, k - 1] == Dtop[:, k]) if k > 0 else np.zeros(n, bool)
    return tri, d2, point, count, size, cut


def expected(points, coords, k, max_dist2=None, count_all=False, stats=False, chunk=16, threads=8):
    return answer(table(points, coords, chunk, threads), k, max_dist2, count_all, stats)
