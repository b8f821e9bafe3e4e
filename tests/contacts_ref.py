"""The contact query's yardstick (rt_sweep_contacts, include/rt_hip.h), built on the sweep query's (tests/sweep_ref.py):
the members of S_i are sweep_ref.pairs() with toi <= fminf(t_max, FLT_MAX), ordered by the key toi_bits << 32 | original
index (toi >= +0, so the bits order as the floats do); a sweep's list is its first k keys, its count the number of its
members, and each entry's point is sweep_ref.near() at the centre c + d*toi_j on that entry's own triangle."""
import numpy as np

from tests import sweep_ref

F = np.float32
FMAX = sweep_ref.FMAX
same_bits = sweep_ref.same_bits


class Members:
    """S_i of n sweeps, flat and sorted by (sweep, key): start[i] .. start[i + 1] are sweep i's members"""

    def __init__(self, n, si, ti, toi):
        key = (toi.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ti.astype(np.uint64)
        order = np.lexsort((key, si))
        self.n = n
        self.si, self.ti, self.toi, self.key = si[order], ti[order].astype(np.int32), toi[order], key[order]
        self.total = np.bincount(si, minlength=n).astype(np.int64)  # |S_i|
        self.start = np.concatenate([[0], np.cumsum(self.total)])
        self.rank = np.arange(len(si)) - self.start[self.si]  # each member's position in its sweep's order


def members(centre, motion, radius, coords, t_max=None, chunk=64):
    c, d, r, tm = sweep_ref._inputs(centre, motion, radius, t_max)
    si, ti, toi = sweep_ref.pairs(c, d, r, coords, tm, chunk)
    T = np.fmin(tm, FMAX)
    with np.errstate(invalid="ignore"):
        keep = toi <= T[si]
    return Members(len(c), si[keep], ti[keep], toi[keep])


def lists(mem, centre, motion, coords, k, count_all=False):
    """(tri [n, k] int32, t [n, k] float32, count [n] int32, point [n, k, 3] float32) as rt_sweep_contacts fills them:
    -1 / FLT_MAX / c's own bits in unused slots; count = min(|S_i|, k), or |S_i| with count_all"""
    c = np.ascontiguousarray(centre, F).reshape(-1, 3)
    d = np.ascontiguousarray(motion, F).reshape(-1, 3)
    n = mem.n
    tri = np.full((n, k), -1, np.int32)
    t = np.full((n, k), FMAX, F)
    point = np.repeat(c[:, None, :], k, axis=1).copy()
    sel = mem.rank < k
    si, j = mem.si[sel], mem.rank[sel]
    tri[si, j] = mem.ti[sel]
    t[si, j] = mem.toi[sel]
    if sel.any():
        rec = sweep_ref.records(coords)
        with np.errstate(all="ignore"):
            C = c[si] + d[si] * mem.toi[sel][:, None]
        _, P, _ = sweep_ref.near(C, rec[0][mem.ti[sel]], rec[1][mem.ti[sel]], rec[2][mem.ti[sel]])
        point[si, j] = P
    count = (mem.total if count_all else np.minimum(mem.total, k)).astype(np.int32)
    return tri, t, count, point


def expected(centre, motion, radius, coords, k, t_max=None, count_all=False):
    mem = members(centre, motion, radius, coords, t_max)
    return lists(mem, centre, motion, coords, k, count_all)


def boundary_ties(mem, k):
    """the sweeps whose k-th and (k+1)-th toi tie bit for bit -> [n] bool"""
    out = np.zeros(mem.n, bool)
    rows = np.nonzero(mem.total > k)[0]
    at = mem.start[rows] + k
    out[rows] = mem.toi[at - 1].view(np.uint32) == mem.toi[at].view(np.uint32)
    return out


def kth_toi(mem, k):
    """the k-th toi of every sweep with at least k members -> (rows, toi)"""
    rows = np.nonzero(mem.total >= k)[0]
    return rows, mem.toi[mem.start[rows] + k - 1]
