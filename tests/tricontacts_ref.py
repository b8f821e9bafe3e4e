"""The triangle contact query's yardstick (rt_sweep_tri_contacts, include/rt_hip.h), built on the triangle sweep query's
(tests/trisweep_ref.py) as tests/contacts_ref.py is on tests/sweep_ref.py: the members of S_i are trisweep_ref.pairs()
with toi <= fminf(t_max, FLT_MAX), ordered by the key toi_bits << 32 | original index (toi >= +0, so the bits order as
the floats do); a query's list is its first k keys, its count the number of its members, and each entry's point and
kind are that pair's own, straight from pairs()."""
import numpy as np

from tests import trisweep_ref

F = np.float32
FMAX = trisweep_ref.FMAX
same_bits = trisweep_ref.same_bits


class Members:
    """S_i of n queries, flat and sorted by (query, key): start[i] .. start[i + 1] are query i's members"""

    def __init__(self, n, qi, ti, toi, pt, kind):
        key = (toi.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64)
        order = np.lexsort((key, qi))
        self.n = n
        self.qi, self.ti, self.toi, self.key = qi[order], ti[order].astype(np.int32), toi[order], key[order]
        self.pt, self.kind = pt[order], kind[order].astype(np.int32)
        self.total = np.bincount(qi, minlength=n).astype(np.int64)  # |S_i|
        self.start = np.concatenate([[0], np.cumsum(self.total)])
        self.rank = np.arange(len(qi)) - self.start[self.qi]  # each member's position in its query's order


def members(q, motion, coords, t_max=None, chunk=64):
    q, d, tm = trisweep_ref._inputs(q, motion, t_max)
    qi, ti, toi, pt, kind = trisweep_ref.pairs(q, d, coords, tm, chunk)
    T = np.fmin(tm, FMAX)
    with np.errstate(invalid="ignore"):
        keep = toi <= T[qi]
    return Members(len(q), qi[keep], ti[keep], toi[keep], pt[keep], kind[keep])


def lists(mem, q, k, count_all=False):
    """(tri [n, k] int32, t [n, k] float32, point [n, k, 3] float32, kind [n, k] int32, count [n] int32) as
    rt_sweep_tri_contacts fills them: -1 / FLT_MAX / q0's own bits / -1 in unused slots; count = min(|S_i|, k), or |S_i|
    with count_all"""
    q = trisweep_ref.tris(q)
    n = mem.n
    assert len(q) == n
    tri = np.full((n, k), -1, np.int32)
    t = np.full((n, k), FMAX, F)
    point = np.repeat(q[:, :1, :], k, axis=1).copy()
    kind = np.full((n, k), -1, np.int32)
    sel = mem.rank < k
    qi, j = mem.qi[sel], mem.rank[sel]
    tri[qi, j] = mem.ti[sel]
    t[qi, j] = mem.toi[sel]
    point[qi, j] = mem.pt[sel]
    kind[qi, j] = mem.kind[sel]
    count = (mem.total if count_all else np.minimum(mem.total, k)).astype(np.int32)
    return tri, t, point, kind, count


def expected(q, motion, coords, k, t_max=None, count_all=False):
    return lists(members(q, motion, coords, t_max), q, k, count_all)


def boundary_ties(mem, k):
    """the queries whose k-th and (k+1)-th toi tie bit for bit -> [n] bool"""
    out = np.zeros(mem.n, bool)
    rows = np.nonzero(mem.total > k)[0]
    at = mem.start[rows] + k
    out[rows] = mem.toi[at - 1].view(np.uint32) == mem.toi[at].view(np.uint32)
    return out


def kth_toi(mem, k):
    """the k-th toi of every query with at least k members -> (rows, toi)"""
    rows = np.nonzero(mem.total >= k)[0]
    return rows, mem.toi[mem.start[rows] + k - 1]
