"""The compiled walk step's loads and waits, read from the assembly: no GPU.

The bench instantiation of k_persist (the all-levels pool with the job list), its cursor form and the per-level pool are
compiled alone with tools/isa_one.sh's flags plus line tables (about 3 s each) and read by tools/step_waits.py:
  (a) no scalar load (a kernel-argument re-read with its lgkmcnt wait) in the parts "stack", "node test" and "triangle
      tests", and none on the lines of any walk's step loop;
  (b) in the pool's step, no s_waitcnt naming vmcnt on a path from the next-node loads to the first triangle-record loads
      of the packed or of the sequential path, and no s_waitcnt vmcnt(0) directly before a triangle-record load group;
  (c) the budget the step lives in: at most 128 VGPRs, no scratch, 64 B of static LDS.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc not installed")

BENCH = "4,false,false,true,4,false,true,2,true,true,2,true"
FORMS = {"list": BENCH, "cursor": "4,false,false,true,4,false,true,2,true,true,2,false",
         "per-level": "4,false,false,true,4,false,true,2,true,true,1,true"}
_DONE = {}


def compiled(form, tmp):
    """(assembly path, the kernel's resource numbers) of one instantiation, compiled once"""
    if form not in _DONE:
        d = tmp / form
        d.mkdir()
        src, asm = d / "one.hip", d / "one.s"
        src.write_text('#include "rt_kernels.hpp"\n#include "rt_shpool.hpp"\n'
                       f"template __global__ void rtd::k_persist<{FORMS[form]}>(rtd::KArgs);\n")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                        "-fno-slp-vectorize", "-fhip-fp32-correctly-rounded-divide-sqrt", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip"), "-gline-tables-only",
                        "--cuda-device-only", "-S", "-o", str(asm), str(src)], check=True, cwd=ROOT,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        s = asm.read_text()
        desc = s.split(".amdhsa_kernel ")[1]
        num = {k: int(re.search(k + r"\s+(\d+)", desc).group(1))
               for k in (".amdhsa_next_free_vgpr", ".amdhsa_private_segment_fixed_size", ".amdhsa_group_segment_fixed_size")}
        num["scratch_ops"] = len(re.findall(r"^\s*scratch_(?:load|store)", s, re.M))
        _DONE[form] = (str(asm), num)
    return _DONE[form]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("walk_step_isa")


@pytest.fixture(scope="module")
def step_waits():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import step_waits as sw
    finally:
        sys.path.pop(0)
    return sw


@pytest.mark.parametrize("form", list(FORMS))
def test_no_scalar_loads_in_the_step(form, workdir, step_waits):
    asm, _ = compiled(form, workdir)
    _, bad = step_waits.check(asm, "k_persist")
    assert not bad["smem_parts"], bad["smem_parts"]
    assert not bad["smem_step"], bad["smem_step"]


@pytest.mark.parametrize("form", list(FORMS))
def test_no_wait_between_node_and_triangle_loads(form, workdir, step_waits):
    asm, _ = compiled(form, workdir)
    _, bad = step_waits.check(asm, "k_persist")
    assert bad["tri_paths"] == 2, f"the pool step's packed and sequential triangle loads were not both found: {bad}"
    assert not bad["wait_before_tris"], bad["wait_before_tris"]
    assert not bad["drain_before_tris"], bad["drain_before_tris"]


@pytest.mark.parametrize("form", list(FORMS))
def test_budget(form, workdir):
    _, num = compiled(form, workdir)
    assert num[".amdhsa_next_free_vgpr"] <= 128, num
    assert num[".amdhsa_private_segment_fixed_size"] == 0 and num["scratch_ops"] == 0, num
    assert num[".amdhsa_group_segment_fixed_size"] == 64, num
