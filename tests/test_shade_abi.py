"""The radiance-query ABI (rt_shade_rays / rt_get_shade_info, include/rt_hip.h) without a GPU: the symbols are
exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as tests/test_query_abi.py
does), Renderer.shade_rays refuses a mistyped, misshapen, strided or host tensor before any device call, and
prt.rays.pinhole forms a frame's primary directions bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from prt import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")


def test_shade_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_shade_rays", "rt_get_shade_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_shade_rays, L.rt_get_shade_info


def test_shade_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_shade": _lib.Shade, "rt_shade_results": _lib.ShadeResults, "rt_shade_info": _lib.ShadeInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layouts.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layouts"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    # the query structs next to them are what they were (tests/test_query_abi.py pins their layouts)
    assert ctypes.sizeof(_lib.Rays) == 40 and ctypes.sizeof(_lib.RayResults) == 24 and ctypes.sizeof(_lib.QueryInfo) == 72


def test_shade_tensors_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called (a call would fail
    on the null context with another message)"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, dtype=torch.float32)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # host tensors
        r.shade_rays(ok, ok)
    with pytest.raises(device.RtError, match="dtype"):
        r.shade_rays(ok.double(), ok)
    with pytest.raises(device.RtError):  # (on a machine without a GPU the origins are refused first: a host tensor)
        r.shade_rays(ok, ok.double())
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.shade_rays(torch.zeros(8, 4), torch.zeros(8, 4))
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.shade_rays(torch.zeros(24), torch.zeros(24))
    with pytest.raises(device.RtError, match="contiguous"):
        r.shade_rays(torch.zeros(16, 3)[::2], ok)
    with pytest.raises(device.RtError, match="contiguous"):
        r.shade_rays(torch.zeros(3, 8).t(), ok)
    with pytest.raises(device.RtError, match="origins has 8"):
        r.shade_rays(ok, torch.zeros(7, 3))
    with pytest.raises(device.RtError, match="torch tensor"):
        r.shade_rays([[0.0, 0.0, 0.0]], ok)
    with pytest.raises(device.RtError, match="raw pointers"):
        r.shade_rays((1234, 8), ok)
    with pytest.raises(device.RtError, match="unclamped has no bgra"):
        r.shade_rays((1234, 8), 5678, unclamped=True, bgra=91011)
    # the outputs, with raw ray pointers (which pass): a host, a mistyped and a short tensor
    with pytest.raises(device.RtError, match="expected cuda:0"):
        r.shade_rays((1234, 8), 5678, rgb=torch.zeros(8, 3))
    with pytest.raises(device.RtError, match="dtype"):
        r.shade_rays((1234, 8), 5678, hit=torch.zeros(8))
    with pytest.raises(device.RtError, match="elements"):
        r.shade_rays((1234, 8), 5678, bounces=4, bounce_hit=torch.zeros(8 * 3, dtype=torch.int32))
    r._ctx = None  # (nothing to destroy)


def cam_rays(a, W, H):
    """tests/test_gpu_query.py cam_rays: the primary rays of camera a = [pos, ul, inc_x, inc_y] in numpy float32, in
    the kernels' order ((ul - pos) + inc_x * x) + inc_y * y"""
    a = np.asarray(a, np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    xs, ys = xs.reshape(-1, 1), ys.reshape(-1, 1)
    d = (a[1] - a[0])[None, :].astype(np.float32)
    d = d + a[2][None, :] * xs
    d = d + a[3][None, :] * ys
    o = np.broadcast_to(a[0], d.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def test_pinhole_equals_the_frame_kernels_formula():
    from prt import rays
    W, H = 64, 36
    ref_cam = host.camera(W, H)
    hand = np.array([[0.3, -9.1, 3.7], [-0.1234567, -7.000001, 3.3333333], [0.0501, 1e-3, -3e-5],
                     [1e-7, -0.0123, -0.04999]], np.float32)
    for cam, arr in ((ref_cam, host.camera_array(ref_cam)), (hand, hand)):
        o, d = rays.pinhole(cam, W, H, device="cpu")
        wo, wd = cam_rays(arr, W, H)
        assert o.dtype == torch.float32 and d.dtype == torch.float32 and o.is_contiguous() and d.is_contiguous()
        assert tuple(o.shape) == (W * H, 3) and tuple(d.shape) == (W * H, 3)
        assert same_bits(o.numpy(), wo) and same_bits(d.numpy(), wd)
    with pytest.raises(ValueError):
        rays.pinhole(hand[:3], W, H, device="cpu")


def test_equirect_and_ortho_shapes():
    from prt import rays
    o, d = rays.equirect([1.0, 2.0, 3.0], 32, 16, device="cpu")
    assert tuple(o.shape) == (512, 3) and tuple(d.shape) == (512, 3) and d.dtype == torch.float32
    assert same_bits(o.numpy(), np.tile(np.array([1, 2, 3], np.float32), (512, 1)))
    l2 = (d.double() ** 2).sum(1)
    assert float((l2 - 1).abs().max()) < 4e-7  # normalised in float32
    assert d[0, 2] > 0.99 and d[-1, 2] < -0.99 and d[0, 0] < 0 < d[16, 0]  # zenith first; azimuth -180 .. 180 degrees
    o, d = rays.ortho([0.0, -20.0, 3.0], [0.0, 2.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.25], 4, 2, device="cpu")
    assert same_bits(d.numpy(), np.tile(np.array([0, 2, 0], np.float32), (8, 1)))
    want = np.array([[-0.75 + 0.5 * x, -20.0, 3.0 + 0.25 * (0.5 - y)] for y in range(2) for x in range(4)], np.float32)
    assert same_bits(o.numpy(), want)
