"""The ray-query ABI (rt_trace_rays / rt_get_query_info, include/rt_hip.h) without a GPU: the symbols are exported,
prt/_lib.py's ctypes mirrors equal the C layouts (from the C compiler itself, as tests/test_abi.py does), and
Renderer.trace_rays / occluded refuse a mistyped, misshapen, strided or host tensor before any device call."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "parallel-ray-tracer_amd", "lib")


def test_query_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "librt_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"rt_trace_rays", "rt_get_query_info"} <= names
    L = ctypes.CDLL(os.path.join(LIB, "librt_hip.so"))
    L.rt_trace_rays, L.rt_get_query_info


def test_query_structs_match_the_c_layouts(tmp_path):
    from prt import _lib
    structs = {"rt_rays": _lib.Rays, "rt_ray_results": _lib.RayResults, "rt_query_info": _lib.QueryInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_hip.h"', "int main(void) {",
             'printf("closest %d\\n", (int)RT_QUERY_CLOSEST);', 'printf("occluded %d\\n", (int)RT_QUERY_OCCLUDED);']
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
    assert int(got["closest"]) == 0 and int(got["occluded"]) == 1  # the kinds Renderer.trace_rays / occluded pass
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_ray_tensors_are_checked_before_any_launch():
    """a Renderer that owns no context: every refusal below happens before the library is called (a call would fail
    on the null context with another message)"""
    from prt import device
    r = device.Renderer.__new__(device.Renderer)
    r.device, r._ctx = 0, ctypes.c_void_p()
    ok = torch.zeros(8, 3, dtype=torch.float32)
    with pytest.raises(device.RtError, match="expected cuda:0"):  # host tensors
        r.trace_rays(ok, ok)
    with pytest.raises(device.RtError, match="dtype"):
        r.trace_rays(ok.double(), ok)
    with pytest.raises(device.RtError):  # (on a machine without a GPU the origins are refused first: a host tensor)
        r.trace_rays(ok, ok.double())
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.trace_rays(torch.zeros(8, 4), torch.zeros(8, 4))
    with pytest.raises(device.RtError, match=r"expected \[n, 3\]"):
        r.trace_rays(torch.zeros(24), torch.zeros(24))
    with pytest.raises(device.RtError, match="contiguous"):
        r.trace_rays(torch.zeros(16, 3)[::2], ok)
    with pytest.raises(device.RtError, match="contiguous"):
        r.occluded(torch.zeros(3, 8).t(), ok, torch.zeros(8))
    with pytest.raises(device.RtError, match="origins has 8"):
        r.trace_rays(ok, torch.zeros(7, 3))
    with pytest.raises(device.RtError, match="torch tensor"):
        r.trace_rays([[0.0, 0.0, 0.0]], ok)
    with pytest.raises(device.RtError, match="raw pointers"):
        r.trace_rays((1234, 8), ok)
    r._ctx = None  # (nothing to destroy)
