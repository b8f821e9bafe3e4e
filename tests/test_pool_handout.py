"""The shadow pool's job-list hand-out (rt_pool_list.hpp: the group bases, an owner's slot, a refill's take), compiled
with g++ and run on the CPU against a transcription of the cursor hand-out it replaces (tests/c/pool_handout_test.cpp):
the same (lane -> job) map round by round and every job handed out exactly once -- all masks empty, one job, a group of
64 then empty groups then a group of 1, more requesters than jobs, exactly as many, 1 / 2 / 8 lights x 1 / 4 / 8
levels, 3,600 seeded random mask sets, regroup 1 / 16 / 63 / 64. No GPU: tests/test_gpu_pool_handout.py checks the
kernels that call this header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_handout(tmp_path):
    exe = tmp_path / "pool_handout_test"
    src = os.path.join(ROOT, "tests", "c", "pool_handout_test.cpp")
    inc = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, "-o", str(exe), src],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
