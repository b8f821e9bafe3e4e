"""What the ten query entry points decide alike (rt_query_logic.hpp), compiled with g++ and run on the CPU: the shared
argument checks with every family's messages verbatim, the list families' capacity rule, the grid rule. No GPU: the
GPU tests pin what the queries compute and that the families keep apart (tests/test_gpu_query_slots.py); this pins the
shared decisions themselves, edge by edge."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_logic(tmp_path):
    exe = tmp_path / "query_logic_test"
    src = os.path.join(ROOT, "tests", "c", "query_logic_test.cpp")
    inc = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc,
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), src], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
