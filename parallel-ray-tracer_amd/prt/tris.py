"""Triangle generators for Renderer.cuts / cuts_csr: each returns one contiguous [n, 3, 3] float32 torch tensor on
`device` (default "cuda"; "cpu" for inspection), as prt.boxes makes box sets.

Every value is formed in float32 by separate multiplies and adds (no fused multiply-add), on the GPU and on the CPU
alike."""
import numpy as np


def _vec(v):
    a = np.asarray(v, np.float32)
    if a.shape != (3,):
        raise ValueError(f"expected 3 components, got shape {a.shape}")
    return a


def sheet(origin, u, v, dims, device="cuda"):
    """the 2 * dims[0] * dims[1] triangles that tile the parallelogram origin + s u + t v, 0 <= s, t <= 1: dims =
    (nu, nv) cells, u fastest -- cell (i, j) is triangles 2 c and 2 c + 1 with c = i + nu * j, split along its diagonal
    from corner (i, j) to corner (i + 1, j + 1):
      2 c      P(i, j), P(i + 1, j), P(i + 1, j + 1)
      2 c + 1  P(i, j), P(i + 1, j + 1), P(i, j + 1)
    with the grid point P(i, j) = (origin + u * (i / nu)) + v * (j / nv), computed once, so neighbouring triangles
    share their corners bit for bit and the far corners are origin + u, (origin + u) + v and origin + v themselves.
    This is how a large cut is spread over the GPU's lanes: one query per tile instead of one query for the whole
    sheet. A mesh triangle that crosses several tiles appears in each of those tiles' lists, each time with its piece
    of the segment; the pieces of one mesh triangle lie on one line and chain end to end (up to rounding). A mesh
    triangle that meets the sheet exactly on a shared tile edge can be reported by both tiles (closed intervals)."""
    import torch
    o, u, v = _vec(origin), _vec(u), _vec(v)
    d = tuple(int(x) for x in dims)
    if len(d) != 2 or min(d) < 1:
        raise ValueError(f"dims: {dims!r}, expected two positive cell counts")
    if not (np.isfinite(o).all() and np.isfinite(u).all() and np.isfinite(v).all()):
        raise ValueError("sheet: origin, u and v must be finite")
    nu, nv = d
    f32 = dict(dtype=torch.float32, device=device)
    fu = torch.arange(nu + 1, **f32) / float(nu)  # (the last fraction is 1 exactly)
    fv = torch.arange(nv + 1, **f32) / float(nv)
    to, tu, tv = (torch.tensor(x, **f32) for x in (o, u, v))
    pu = to[None, :] + tu[None, :] * fu[:, None]               # [nu + 1, 3]
    p = pu[None, :, :] + (tv[None, :] * fv[:, None])[:, None, :]  # [nv + 1, nu + 1, 3]: P(i, j) = p[j, i]
    p00, p10, p11, p01 = p[:-1, :-1], p[:-1, 1:], p[1:, 1:], p[1:, :-1]
    lower = torch.stack([p00, p10, p11], dim=2)  # [nv, nu, 3 corners, 3]
    upper = torch.stack([p00, p11, p01], dim=2)
    return torch.stack([lower, upper], dim=2).reshape(2 * nu * nv, 3, 3).contiguous()
