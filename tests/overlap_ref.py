"""The overlap query's yardstick (rt_overlap_boxes, include/rt_hip.h): a numpy float32 restatement of T(lo, hi, record)
as the header states it. Every operation is one float32 operation in the stated order (nothing fused), on what a
triangle record holds: a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0). fminf / fmaxf are np.fmin / np.fmax (a NaN operand
loses); a comparison with a NaN operand is false, in numpy as in C.

Step 1 (the corner boxes against the query boxes, comparisons only) is evaluated for every (box, triangle) pair, in
chunks of boxes; steps 2 and 3 only for the pairs that pass it, as flat arrays. sets() returns every box's full S_i in
CSR form (np.nonzero walks row-major, so each segment is in index order); answer() reads any k and count_all off it.
The boxes that are invalid (a non-finite number, lo > hi on an axis) have the empty set."""
import numpy as np

F = np.float32


def records(coords):
    """(a, e1, e2, b, c, tlo, thi), each [m, 3] float32: the record, its corners and their box"""
    c = np.asarray(coords, F)
    assert c.dtype == F
    with np.errstate(all="ignore"):
        a = c[:, 0]
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        b, cc = a + e1, a + e2
        tlo = np.fmin(np.fmin(a, b), cc)
        thi = np.fmax(np.fmax(a, b), cc)
    assert e1.dtype == F and b.dtype == F and tlo.dtype == F
    return a, e1, e2, b, cc, tlo, thi


def valid_boxes(lo, hi):
    with np.errstate(invalid="ignore"):
        return np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)


def step1(lo, hi, rec):
    """[boxes, triangles] bool: tlo.k <= hi.k && thi.k >= lo.k on all three axes"""
    tlo, thi = rec[5], rec[6]
    with np.errstate(invalid="ignore"):
        m = np.ones((len(lo), len(tlo)), bool)
        for k in range(3):
            m &= (tlo[None, :, k] <= hi[:, None, k]) & (thi[None, :, k] >= lo[:, None, k])
    return m


def steps23(lo, hi, rec, bi, ti):
    """T for the pairs (box bi[p], triangle ti[p]) that passed step 1 -> [pairs] bool"""
    a, e1, e2, b, c, tlo, thi = (x[ti] for x in rec)
    lo, hi = lo[bi], hi[bi]
    half = F(0.5)
    with np.errstate(all="ignore"):
        inside = ((tlo >= lo) & (thi <= hi)).all(axis=1)  # 2.
        l2, h2 = half * lo, half * hi
        ctr, h = l2 + h2, h2 - l2
        v = [a - ctr, b - ctr, c - ctr]
        sep = np.zeros(len(ti), bool)
        for f in (e1, e2 - e1, e2):
            for k in range(3):
                i, j = (k + 1) % 3, (k + 2) % 3
                p = [v[m][:, j] * f[:, i] - v[m][:, i] * f[:, j] for m in range(3)]
                rad = h[:, i] * np.abs(f[:, j]) + h[:, j] * np.abs(f[:, i])
                assert p[0].dtype == F and rad.dtype == F
                sep |= (np.fmin(np.fmin(p[0], p[1]), p[2]) > rad) | (np.fmax(np.fmax(p[0], p[1]), p[2]) < -rad)
        nrm = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
               e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
        d = (nrm[0] * v[0][:, 0] + nrm[1] * v[0][:, 1]) + nrm[2] * v[0][:, 2]
        r = (h[:, 0] * np.abs(nrm[0]) + h[:, 1] * np.abs(nrm[1])) + h[:, 2] * np.abs(nrm[2])
        assert d.dtype == F and r.dtype == F
        sep |= np.abs(d) > r
    return inside | ~sep


def pairs(lo, hi, coords, chunk=64):
    """(bi, ti, T): the step-1 pairs in (box, triangle) order and T for each"""
    lo = np.ascontiguousarray(lo, F).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, F).reshape(-1, 3)
    rec = records(coords)
    ok = valid_boxes(lo, hi)
    bis, tis, ts = [], [], []
    for s in range(0, len(lo), chunk):
        m = step1(lo[s:s + chunk], hi[s:s + chunk], rec) & ok[s:s + chunk, None]
        bi, ti = np.nonzero(m)
        bi += s
        bis.append(bi)
        tis.append(ti)
        ts.append(steps23(lo, hi, rec, bi, ti))
    if not bis:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
    return np.concatenate(bis), np.concatenate(tis), np.concatenate(ts)


def sets(lo, hi, coords, chunk=64):
    """every box's S_i -> (offsets [n + 1] int64, tris [offsets[n]] int32), each segment in index order"""
    n = len(np.asarray(lo).reshape(-1, 3))
    bi, ti, t = pairs(lo, hi, coords, chunk)
    bi, ti = bi[t], ti[t]
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(bi, minlength=n), out=offsets[1:])
    return offsets, ti.astype(np.int32)


def answer(csr, k, count_all=False, rows=None):
    """(tri [n, k] int32, count [n] int32) as rt_overlap_boxes fills them: the first k members of S_i by index, -1 in
    unused slots; count = min(|S_i|, k), or |S_i| with count_all. rows: the boxes to answer for (default all, in
    order)."""
    offsets, tris = csr
    starts, size = offsets[:-1], np.diff(offsets)
    if rows is not None:
        starts, size = starts[rows], size[rows]
    n = len(starts)
    j = np.arange(k)[None, :]
    used = j < size[:, None]
    at = np.minimum(starts[:, None] + j, max(len(tris) - 1, 0))
    tri = np.where(used, tris[at] if len(tris) else -1, -1).astype(np.int32).reshape(n, k)
    count = (size if count_all else np.minimum(size, k)).astype(np.int32)
    return tri, count


def segments(csr, rows=None):
    """the boxes' sets as a list of int32 arrays"""
    offsets, tris = csr
    rows = range(len(offsets) - 1) if rows is None else rows
    return [tris[offsets[i]:offsets[i + 1]] for i in rows]


def expected(lo, hi, coords, k, count_all=False):
    return answer(sets(lo, hi, coords), k, count_all)


def scene_extent(coords):
    """the longest side of the scene's box"""
    v = np.asarray(coords, np.float64).reshape(-1, 3)
    return float((v.max(0) - v.min(0)).max())


def surface_boxes(coords, n, seed):
    """n boxes at the surface: each centre a random point on a random triangle plus N(0, 1e-3 extent) per axis, each
    per-axis half-width extent * 10^U(-3.5, -1) -> (lo, hi) float32"""
    rng = np.random.default_rng(seed)
    c = np.asarray(coords, np.float64)
    ext = scene_extent(coords)
    t = rng.integers(0, len(c), n)
    u, w = rng.random(n), rng.random(n)
    flip = u + w > 1
    u, w = np.where(flip, 1 - u, u), np.where(flip, 1 - w, w)
    ctr = c[t, 0] + u[:, None] * (c[t, 1] - c[t, 0]) + w[:, None] * (c[t, 2] - c[t, 0])
    ctr = ctr + rng.normal(0, 1e-3 * ext, (n, 3))
    half = ext * 10.0 ** rng.uniform(-3.5, -1, (n, 3))
    return (ctr - half).astype(F), (ctr + half).astype(F)
