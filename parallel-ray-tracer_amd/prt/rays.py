"""Ray generators for Renderer.shade_rays / trace_rays: each returns (origins, dirs), two contiguous [W * H, 3] float32
torch tensors in row-major pixel order on `device` (default "cuda"; "cpu" for inspection).

pinhole reproduces a frame's primary rays bit for bit, so shade_rays(*pinhole(cam, W, H)) equals render(cam, W, H);
equirect and ortho are projections rt_camera cannot express. Every value is formed in float32 by separate multiplies
and adds (no fused multiply-add), on the GPU and on the CPU alike."""
import math

import numpy as np


def _torch():
    import torch
    return torch


def _cam_rows(cam):
    """[pos, ul, inc_x, inc_y] as a [4, 3] float32 array from an rt_camera (prt._lib.Camera) or an array"""
    if hasattr(cam, "inc_x"):
        return np.array([[v.x, v.y, v.z] for v in (cam.pos, cam.ul, cam.inc_x, cam.inc_y)], np.float32)
    a = np.asarray(cam, np.float32)
    if a.shape != (4, 3):
        raise ValueError(f"camera: shape {a.shape}, expected [4, 3] (pos, ul, inc_x, inc_y)")
    return a


def _grid(W, H, device):
    """pixel coordinates (x, y) as [W * H, 1] float32 columns, row-major"""
    torch = _torch()
    if W < 1 or H < 1:
        raise ValueError(f"a {W} x {H} grid has no rays")
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device),
                            torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    return xs.reshape(-1, 1), ys.reshape(-1, 1)


def _vec(v, device):
    torch = _torch()
    a = np.asarray(v, np.float32)
    if a.shape != (3,):
        raise ValueError(f"expected 3 components, got shape {a.shape}")
    return torch.from_numpy(a.copy()).to(device)[None, :]


def pinhole(cam, W, H, device="cuda"):
    """the primary rays of rt_camera `cam` on a W x H frame (main.c:229-233): o = pos,
    d = ((ul - pos) + inc_x * x) + inc_y * y, in that order"""
    torch = _torch()
    a = torch.from_numpy(_cam_rows(cam)).to(device)
    xs, ys = _grid(W, H, device)
    d = (a[1] - a[0])[None, :]
    d = d + a[2][None, :] * xs
    d = d + a[3][None, :] * ys
    o = a[0][None, :].expand(W * H, 3)
    return o.contiguous(), d.contiguous()


def equirect(pos, W, H, device="cuda"):
    """a 360 x 180 degree panorama from `pos`, z up: pixel (x, y) looks along azimuth (x + 0.5) / W * 360 - 180 degrees
    (from +x towards +y) and polar angle (y + 0.5) / H * 180 degrees from +z (row 0 next to the zenith); unit
    directions, normalised in float32"""
    torch = _torch()
    xs, ys = _grid(W, H, device)
    phi = (xs + 0.5) * (2.0 * math.pi / W) - math.pi
    theta = (ys + 0.5) * (math.pi / H)
    st = torch.sin(theta)
    d = torch.cat([st * torch.cos(phi), st * torch.sin(phi), torch.cos(theta)], dim=1)
    n = torch.sqrt((d * d).sum(dim=1, keepdim=True))
    d = d / n
    o = _vec(pos, device).expand(W * H, 3)
    return o.contiguous(), d.contiguous()


def ortho(pos, forward, right, up, W, H, device="cuda"):
    """parallel rays along `forward` (as given: not normalised) from a W x H window centred on `pos`: pixel (x, y)
    starts at pos + right * (x + 0.5 - W / 2) + up * (H / 2 - 0.5 - y), so |right| and |up| are the pixel pitch"""
    xs, ys = _grid(W, H, device)
    o = _vec(pos, device)
    o = o + _vec(right, device) * (xs + (0.5 - W / 2))
    o = o + _vec(up, device) * ((H / 2 - 0.5) - ys)
    d = _vec(forward, device).expand(W * H, 3)
    return o.contiguous(), d.contiguous()
