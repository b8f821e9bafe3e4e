"""The vertex-update ABI (rt_update_vertices / rt_get_update_info / rt_update_lights, include/rt_hip.h; rth_wbvh_refit,
include/rt_host.h) without a GPU: the symbols are exported, prt/_lib.py's ctypes mirrors equal the C layouts (from the
C compiler itself, as tests/test_shade_abi.py does), rt_scene_info's layout is what it was, and
Renderer.update_vertices refuses a mistyped, misshapen, strided or host tensor before any device call."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, lib)], capture_output=True, text=True,
                         check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_update_symbols_are_exported():
    assert {"rt_update_vertices", "rt_get_update_info", "rt_update_lights", "rt_debug_read_wide"} <= exported("librt_hip.so")
    assert {"rth_wbvh_refit", "rth_triangle_init"} <= exported("librt_host.so")


def test_update_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_vertex_update": _lib.VertexUpdate, "rt_update_info": _lib.UpdateInfo, "rt_scene_info": _lib.SceneInfo}
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
    assert ctypes.sizeof(_lib.VertexUpdate) == 16 and ctypes.sizeof(_lib.UpdateInfo) == 28
    assert ctypes.sizeof(_lib.SceneInfo) == 60  # unchanged by the update calls


def test_update_tensors_are_checked_before_any_call():
    """a Renderer that owns no context: every refusal below happens before the library is called"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, 3, dtype=torch.float32)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # a host tensor
        r.update_vertices(ok)
    with pytest.raises(device.RtError, match="dtype"):
        r.update_vertices(ok.double())
    with pytest.raises(device.RtError, match=r"expected \[n, 3, 3\]"):
        r.update_vertices(torch.zeros(8, 9))
    with pytest.raises(device.RtError, match=r"expected \[n, 3, 3\]"):
        r.update_vertices(torch.zeros(8, 3, 4))
    with pytest.raises(device.RtError, match="contiguous"):
        r.update_vertices(torch.zeros(16, 3, 3)[::2])
    with pytest.raises(device.RtError, match="torch tensor"):
        r.update_vertices([[[0.0] * 3] * 3])
    r._ctx = None  # (nothing to destroy)
