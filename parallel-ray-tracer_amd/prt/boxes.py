"""Box generators for Renderer.overlaps / overlaps_csr: each returns (lo, hi), two contiguous [n, 3] float32 torch
tensors on `device` (default "cuda"; "cpu" for inspection), as prt.rays makes ray sets.

Every value is formed in float32 by separate multiplies and adds (no fused multiply-add), on the GPU and on the CPU
alike."""
import numpy as np


def _vec(v):
    a = np.asarray(v, np.float32)
    if a.shape != (3,):
        raise ValueError(f"expected 3 components, got shape {a.shape}")
    return a


def grid(lo, hi, dims, device="cuda"):
    """the cells of a regular voxel grid over the box [lo, hi]: dims = (nx, ny, nz) cells, x fastest -- cell
    (ix, iy, iz) is box ix + nx * (iy + ny * iz). With the cell size c = (hi - lo) / dims, a cell spans
    [lo + c * i, lo + c * (i + 1)] per axis; its upper plane is computed exactly as its neighbour's lower one, so
    adjacent cells share a face bit for bit (closed boxes: a triangle on the face is in both), and the last plane of
    each axis is hi itself."""
    import torch
    lo, hi = _vec(lo), _vec(hi)
    d = tuple(int(x) for x in dims)
    if len(d) != 3 or min(d) < 1:
        raise ValueError(f"dims: {dims!r}, expected three positive cell counts")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError("grid: lo and hi must be finite with lo <= hi")
    planes = []
    for k in range(3):
        c = torch.tensor((hi[k] - lo[k]) / np.float32(d[k]), dtype=torch.float32, device=device)
        p = torch.arange(d[k] + 1, dtype=torch.float32, device=device) * c + float(lo[k])
        p[-1] = float(hi[k])
        planes.append(p)
    iz, iy, ix = torch.meshgrid(*(torch.arange(n, device=device) for n in d[::-1]), indexing="ij")
    idx = (ix.reshape(-1), iy.reshape(-1), iz.reshape(-1))
    blo = torch.stack([planes[k][idx[k]] for k in range(3)], dim=1)
    bhi = torch.stack([planes[k][idx[k] + 1] for k in range(3)], dim=1)
    return blo.contiguous(), bhi.contiguous()
